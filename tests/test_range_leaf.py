"""Range ops applied in one visit to their leaf block (MT_RANGE_LEAF, csrc/mt_core.h rangeLeaf)
on the host emulation: hand-built cases against the oracle, and the fused build against a
-DMT_RANGE_LEAF=0 build of the same sources, which must leave every document in the same
state pool for pool.  Both builds carry the range-op event counters (-DMT_EVRANGE), so each
case also proves which path it took.
"""
import ctypes as C
import os

import numpy as np
import pytest

from fluidframework_amd.engine import Engine
from oracle_lib import gen_params, generate
from emu_lib import DEPS, ROOT, SRC, _atomic_build
from test_emu_parity import CONFIGS, NAMES, ann_props, compare
import range_leaf_cases as RL

EV_OPS, EV_FUSED, EV_SAME_LEAF, EV_NO_ROOM, EV_REFUSED, EV_SPLITS = range(6)


def variant(fused):
    """The emulation with the range-op counters, fused step on or off, under its own file name."""
    lib = os.path.join(ROOT, "tests", "emu", "libmtemu_range%d.so" % fused)
    if not os.path.exists(lib) or any(os.path.getmtime(lib) < os.path.getmtime(d) for d in DEPS):
        _atomic_build(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DMT_G_MWMIN=64",
                       "-DMT_BPC_CHECK=1", "-DMT_EVRANGE", "-DMT_RANGE_LEAF=%d" % fused, "-o", None, SRC], lib)
    return lib


def factory(fused):
    lib = variant(fused)
    return lambda n, **kw: Engine(n, lib_path=lib, prefix="emu_", **kw)


def events(eng, n):
    fn = eng.lib.emu_prof_get
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros((n, 8), np.uint64)
    fn(eng.h, n, out.ctypes.data)
    return out.astype(np.int64)


def state(eng, n, msn, seq):
    """Everything the two builds must agree on, per document."""
    cnt = eng.counters(range(n))
    return dict(status=eng.status(range(n)), pools=eng.pools(range(n)), text=eng.get_text(range(n)),
                digests=eng.snapshot_digests(range(n), msn, seq, threads=2), dumps=[eng.dump(d) for d in range(n)],
                **{"cnt_" + k: v for k, v in cnt.items()})


def assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "dumps":
            for d, (x, y) in enumerate(zip(a[k], b[k])):
                assert x.shape == y.shape and (x == y).all(), f"doc {d}: segment dump differs"
        elif k == "text":
            assert a[k] == b[k]
        else:
            assert np.array_equal(a[k], b[k]), f"{k}: {a[k]} vs {b[k]}"


def run_both(batch, props, n, **cap):
    """Fused and unfused builds on one batch, each checked against the oracle (compare); returns
    the fused build's events, the unfused build's, after checking that the states agree."""
    last = batch.op_offsets[1:] - 1
    msn, seq = batch.arrays["msn"][last], batch.arrays["seq"][last]
    got = []
    for fused in (1, 0):
        eng = compare(batch, props, n, factory=factory(fused), **cap)
        got.append((state(eng, n, msn, seq), events(eng, n)))
        eng.close()
    assert_same_state(got[0][0], got[1][0])
    return got[0][1], got[1][1]


# block residency (the default), every pool in HBM, LDS residency, long-document residency
RESIDENCIES = [None, (0, 0, 0, 0), (1, 0, 0, 0), (3, 0, 0, 0)]


@pytest.mark.parametrize("res", RESIDENCIES, ids=lambda r: "default" if r is None else "res%d" % r[0])
@pytest.mark.parametrize("mode", RL.MODES)
def test_hand_built_cases_match_oracle_and_unfused_build(mode, res):
    batch, props, hits = RL.build(mode)
    n = len(hits)
    cap = {} if res is None else {"residency": res}
    ev1, ev0 = run_both(batch, props, n, **cap)
    assert (ev0[:, EV_FUSED] == 0).all()
    for d, name in enumerate(RL.CASES):
        assert ev1[d, EV_FUSED] == hits[d], f"{name}: {ev1[d, EV_FUSED]} fused range ops, expected {hits[d]}"
        assert ev1[d, EV_OPS] == ev0[d, EV_OPS] >= max(hits[d], 1), name


def test_delta_capture_takes_the_unfused_path():
    """With delta capture armed every range op falls back, and the records equal the oracle's."""
    from test_message_surface import check_delta_records
    made = []

    def f(n, **kw):
        made.append(factory(1)(n, **kw))
        return made[-1]

    kinds = check_delta_records(f, "mixed", n_docs=2, n_msgs=400)
    assert {1, 2} <= kinds                                   # REMOVE and ANNOTATE records were compared
    ev = events(made[0], 2)
    assert (ev[:, EV_OPS] > 0).all() and (ev[:, EV_FUSED] == 0).all(), ev


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_generated_streams_fused_equals_unfused(cfg):
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS[cfg])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    ev1, ev0 = run_both(batch, props, 4)
    assert (ev0[:, EV_FUSED] == 0).all()
    # not vacuous: every document took the fused step
    print(cfg, "range ops, fused, same leaf, no room, refused, splits per document:\n", ev1[:, :6])
    assert (ev1[:, EV_FUSED] > 0).all(), ev1[:, :6]
    assert (ev1[:, EV_FUSED] + ev1[:, EV_NO_ROOM] + ev1[:, EV_REFUSED] == ev1[:, EV_SAME_LEAF]).all()
