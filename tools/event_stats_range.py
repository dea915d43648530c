"""Diagnostic: how many range ops of a bench stream the fused leaf step applies (MT_RANGE_LEAF,
csrc/mt_core.h rangeLeaf), counted on the host emulation (-DMT_EVRANGE), with the same generator
and seed as tools/event_stats_c2.py on a subset of documents.  Not the product.

usage: python tools/event_stats_range.py [config2] [docs=16] [residency=blk]
"""
import ctypes as C, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from fluidframework_amd.engine import Engine
from fluidframework_amd.batch import MtGenParams
import bench
lib = "/tmp/libmtemu_mt_evrange.so"
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DMT_EVRANGE",
                       "-o", lib, os.path.join(ROOT, "tests", "emu", "mt_emu.cpp")])
cfg = sys.argv[1] if len(sys.argv) > 1 else "config2"
docs = int(sys.argv[2]) if len(sys.argv) > 2 else 16
res = sys.argv[3] if len(sys.argv) > 3 else "blk"
c = dict(bench.CONFIGS[cfg]); c["docs"] = docs
eng = Engine(docs, lib_path=lib, prefix="emu_", **bench.caps_for(c))
eng.set_residency(bench.RESIDENCY[res])
eng.upload_props(bench.ann_props()); eng.upload_names(['"c%d"' % i for i in range(64)])
p = MtGenParams(7, docs, c["ops"], c["clients"], c["lag"], c["ins"], c["rem"], c["ins_len"], c["rem_len"], c["ann_sets"],
                c["rewrite"])
eng.generate(p); eng.sync(); eng.generated_to_resident(); eng.open_docs(0, docs)
fn = eng.lib.emu_prof_get; fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
base = np.zeros((docs, 8), np.uint64); fn(eng.h, docs, base.ctypes.data)
eng.replay_resident(); eng.sync()
raw = np.zeros((docs, 8), np.uint64); fn(eng.h, docs, raw.ctypes.data)
msgs = float(docs * c["ops"]); t = (raw - base).sum(axis=0).astype(float)
names = ["range ops", "fused", "both boundaries in one leaf", "no room for the splits", "refused otherwise", "rows split by the fused step"]
print(f"{cfg} docs={docs} res={res}, per message: " + "  ".join(f"{nm} {t[i]/msgs:.3f}" for i, nm in enumerate(names)))
print("share of range ops: " + "  ".join(f"{nm} {100*t[i]/max(t[0],1):.1f}%" for i, nm in enumerate(names) if 0 < i < 5))
# MT_LEAF_SPLIT: the "no room" range ops that rangeLeaf applies all the same (slot 7; slot 1 counts none of them).
# MT_INSERT_LEAF (slot 6, low / high 32 bits): each paired insert saves one visit to its leaf block
# (insertAtPath); one whose block of 7 splits under the half also saves the computeU and the root walk
# that the two-visit path needs after that split (a block of 6 splits under the new row: nothing follows).
pair = float((raw - base)[:, 6].astype(np.uint64).__and__(np.uint64(0xFFFFFFFF)).sum())
psplit = float(((raw - base)[:, 6] >> np.uint64(32)).sum())
print(f"range ops applied across a block split {t[7]/msgs:.4f} per message ({100*t[7]/max(t[0],1):.1f}% of range ops)")
print(f"inserts per message: right half and new row linked together {pair/msgs:.4f}  of those splitting their block "
      f"{psplit/msgs:.4f}")
