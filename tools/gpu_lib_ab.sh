#!/bin/bash
# Engine-library A/B on one box: bench.py config lines with each library (MTGPU_LIB), alternating.
# usage: CFGS="config2" ROUNDS=2 tools/gpu_lib_ab.sh <outdir> <lib.so>...
set -o pipefail
O=gpurun_out/${1:-libab}; shift; mkdir -p $O
export PYTHONUNBUFFERED=1
for r in $(seq 1 ${ROUNDS:-2}); do
  for lib in "$@"; do
    for c in ${CFGS:-config2}; do
      n=$(basename $lib .so)_${c}_$r
      MTGPU_LIB=$lib timeout -k 10 300 python -u bench.py --full --config $c --steps ${STEPS:-5} --warmup 2 --no-cpu-baseline --no-ingest > $O/$n.json 2> $O/$n.err || { echo FAIL $n; tail -20 $O/$n.err; exit 1; }
      python -c "import json;d=json.load(open('$O/$n.json'));print('$n', round(d['value']/1e6,2), 'M ops/s', round(d['ms_per_step'],1), 'ms', d['parity'][-22:])"
    done
  done
done
