"""Range ops applied across a leaf block's split (MT_LEAF_SPLIT, on by default) on the device, in
the engine instantiations that tests/test_gpu_leaf_split.py does not reach: LDS residency, the
long-document kernel, block residency with 40 LDS blocks that every document outgrows mid-run
(finished by the all-HBM rest kernel, or in the same wave by the continuation kernel) and the wide
kernel of a partitioned launch.  The hand-built cases of tests/leaf_split_cases.py in both modes
and a generated stream, each against the oracle.
"""
import functools

import pytest

from oracle_lib import gen_params, generate
from test_emu_parity import CONFIGS, ann_props, compare
from test_gpu_parity import gpu_engine
import leaf_split_cases as LS

pytestmark = pytest.mark.gpu

# name -> (residency, continuation threshold or None, partition (min_ops, cus) for the hand-built
# cases and for the stream, or None)
KERNELS = {
    "lds": ((1, 0, 0, 0), None, None),
    "big": ((3, 0, 0, 0), None, None),
    "blk40_rest": ((2, 0, 40, 12), None, None),
    "blk40_cont": ((2, 0, 40, 12), 0, None),
    # the hand-built documents have 8 to 34 messages: from 10 up in the wide kernel, the others in
    # the block kernel beside it; every run of the stream (1,500 messages) in the wide kernel
    "wide": (None, None, ((10, 32), (1000, 32))),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name in ("remove", "annotate"):
        batch, props, hits = LS.build_ranges(name)
        return batch, props, len(hits)
    props = ann_props()
    p = gen_params(seed=19, n_docs=8, **CONFIGS["cfg2"])     # 1,500 messages per document
    batch, st, _ = generate(p, props)
    assert st == [0] * 8
    return batch, props, 8


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", ["remove", "annotate", "cfg2"])
def test_gpu_leaf_split_in_every_replay_kernel(name, kernel):
    batch, props, n = inputs(name)
    res, cont, part = KERNELS[kernel]
    cap = {}
    if res is not None:
        cap["residency"] = res
    if cont is not None:
        cap["cont"] = cont
    made = []

    def factory(k, **kw):
        eng = gpu_engine(k, **kw)
        if part is not None:
            eng.set_partition(*part[name == "cfg2"])
        made.append(eng)
        return eng

    compare(batch, props, n, factory=factory, **cap)
    if part is not None:                                     # the launch was partitioned: the wide kernel ran
        assert made[0].partition_info() == {"min_msgs": part[name == "cfg2"][0], "cus": 32}
