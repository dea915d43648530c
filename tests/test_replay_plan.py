"""The replay plan (csrc/mt_plan.h mt_plan_replay): which kernels a resident batch gets, on which
lanes and over which runs, asserted launch by launch.  The HIP backend issues exactly these
launches and the host emulation runs exactly these, so the table below is what both do."""
import ctypes

import numpy as np
import pytest

from emu_lib import emu_engine
from oracle_lib import gen_params
from test_emu_parity import NAMES, ann_props
from test_long_docs import size_class_batch

HBM, REST, LDS, BLK, BLK_CONT, BLKW, BIG = range(7)          # mt_plan.h MT_PK_*
MAIN, SIDE, A, B = range(4)                                  # mt_plan.h MT_LANE_*
COUNTS = [300, 2500, 80, 1200, 40, 3000]                     # three runs of at least 1,000 ops
PAD = 27 << 10


def L(kernel, lane, n, runs=False, pad=0):
    return (kernel, lane, n, pad, int(runs))


def plan(eng, full):
    f = eng.lib.emu_test_plan
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    out = np.zeros(4 * 5, np.int32)
    n = f(eng.h, int(full), out.ctypes.data)
    assert n >= 0, n
    return [tuple(int(x) for x in out[5 * i:5 * i + 5]) for i in range(n)]


def engine(counts=COUNTS, upload=True):
    eng = emu_engine(len(counts), rows_per_doc=3 * max(counts) + 64, window_per_doc=8192,
                     propsets_per_doc=2 * max(counts) + 64, text_per_doc=8 * max(counts) + 4096)
    eng.upload_props(ann_props())
    eng.upload_names(NAMES)
    eng.open_docs(0, len(counts))
    if upload:
        eng.upload(size_class_batch(tuple(counts))[0])
    return eng


def classes(eng, kind, min_ops=1000):
    if kind == "size":
        eng.set_size_class(min_ops)
    elif kind == "partition":
        eng.set_partition(min_ops, 8)


HAND_OVER = [L(BLK, MAIN, 6), L(REST, MAIN, 6)]
IN_WAVE = [L(BLK_CONT, MAIN, 6)]


@pytest.mark.parametrize("cont", [None, 0])
@pytest.mark.parametrize("kind", [None, "size", "partition"])
@pytest.mark.parametrize("full", [False, True])
def test_plan_of_every_residency(full, kind, cont):
    eng = engine()
    classes(eng, kind)
    if cont is not None:
        eng.set_continuation(cont)
    want = {0: [L(HBM, MAIN, 6)], 1: [L(LDS, MAIN, 6), L(REST, MAIN, 6)], 3: [L(BIG, MAIN, 6)]}
    if kind == "partition":        # (A) the long runs on lane A's CUs, the rest on lane B's
        want[2] = ([L(BLK_CONT, A, 3, runs=True, pad=PAD), L(BLK_CONT, B, 3, runs=True)] if full else
                   [L(BLKW, A, 3, runs=True), L(BLK, B, 3, runs=True), L(REST, MAIN, 6)])
    elif kind == "size":           # (B) the long runs on the second stream, first
        want[2] = ([L(BIG, SIDE, 3, runs=True), L(BLK_CONT, MAIN, 3, runs=True)] if full else
                   [L(BLKW, SIDE, 3, runs=True), L(BLK, MAIN, 3, runs=True), L(REST, MAIN, 6)])
    else:                          # (D) no run reaches the default threshold of 16,384 ops; every run reaches 0
        want[2] = IN_WAVE if full or cont == 0 else HAND_OVER
    for res in (0, 1, 2, 3):
        eng.set_residency(res)
        assert plan(eng, full) == want[res], res


@pytest.mark.parametrize("full", [False, True])
def test_plan_of_a_continuation_threshold_one_run_reaches(full):
    eng = engine()
    eng.set_residency(2)
    eng.set_continuation(3000)
    assert plan(eng, full) == IN_WAVE
    eng.set_continuation(3001)
    assert plan(eng, full) == (IN_WAVE if full else HAND_OVER)


@pytest.mark.parametrize("kind", ["size", "partition"])
@pytest.mark.parametrize("full", [False, True])
def test_plan_of_a_size_class_without_long_or_short_runs(full, kind):
    eng = engine()
    eng.set_residency(2)
    classes(eng, kind, 10**6)      # no long run: the plan of block residency alone
    assert plan(eng, full) == (IN_WAVE if full else HAND_OVER)
    eng.set_continuation(0)
    assert plan(eng, full) == IN_WAVE
    classes(eng, kind, 10)         # no short run: one launch, nothing to hand over
    lane = A if kind == "partition" else SIDE
    if not full:
        assert plan(eng, full) == [L(BLKW, lane, 6, runs=True)]
    elif kind == "partition":
        assert plan(eng, full) == [L(BLK_CONT, A, 6, runs=True, pad=PAD)]
    else:
        assert plan(eng, full) == [L(BIG, SIDE, 6, runs=True)]


def test_plan_of_a_device_built_batch():
    eng = engine(upload=False)
    p = gen_params(seed=77, n_docs=len(COUNTS), ops=8, clients=5, lag=48, ins=60, rem=30, ins_len=8, rem_len=8,
                   ann_sets=24, rewrite=5)
    eng.generate(p, ops_per_doc=COUNTS, clients_per_doc=[5] * len(COUNTS))
    eng.sync()
    eng.generated_to_resident()
    eng.set_residency(2)
    assert plan(eng, False) == HAND_OVER
    assert plan(eng, True) == IN_WAVE
    eng.set_continuation(3000)
    assert plan(eng, False) == IN_WAVE
    eng.set_size_class(1000)
    assert plan(eng, False) == [L(BLKW, SIDE, 3, runs=True), L(BLK, MAIN, 3, runs=True), L(REST, MAIN, 6)]
    assert plan(eng, True) == [L(BIG, SIDE, 3, runs=True), L(BLK_CONT, MAIN, 3, runs=True)]


def test_plan_does_not_keep_an_earlier_batchs_continuation_class():
    """Under a size class that no run of the batch reaches, the choice between the in-wave
    continuation and the hand-over is made from this batch's run lengths, not from the count an
    earlier batch left behind."""
    eng = engine(upload=False)
    eng.set_residency(2)
    eng.set_continuation(0)
    batch = size_class_batch(tuple(COUNTS))[0]
    eng.apply(batch)
    eng.sync()
    assert plan(eng, False) == IN_WAVE
    eng.set_size_class(10**6)
    eng.open_docs(0, len(COUNTS))
    eng.upload(batch)
    assert plan(eng, False) == IN_WAVE           # every run still reaches a threshold of 0
    eng.set_continuation(2000)
    eng.upload(batch)
    assert plan(eng, False) == IN_WAVE           # the runs of 2,500 and 3,000 ops reach 2,000
    short = (300, 80, 40)
    eng.upload(size_class_batch(short)[0])
    assert plan(eng, False) == [L(BLK, MAIN, 3), L(REST, MAIN, 3)]
    eng.replay_resident()
    eng.sync()
    assert (eng.status(range(len(short))) == 0).all()
