"""Leaf blocks that split under an op applied in one visit, on the host emulation: inserts whose
split row's right half and new row enter their leaf block together (MT_INSERT_LEAF, csrc/mt_core.h
opInsert / insertAtPath<true>), and range ops whose right halves split the block (MT_LEAF_SPLIT,
rangeLeaf).  Hand-built cases against the oracle, and the build with both switches on against a
-DMT_LEAF_SPLIT=0 -DMT_INSERT_LEAF=0 build of the same sources, which must leave every document in
the same state pool for pool (row ids included: the halves and the new row are allocated in the
old order).  The builds carry the -DMT_EVRANGE counters, so each case also proves which path it took.
"""
import os

import numpy as np
import pytest

from fluidframework_amd.engine import Engine
from oracle_lib import gen_params, generate
from emu_lib import DEPS, ROOT, SRC, _atomic_build
from test_emu_parity import CONFIGS, ann_props, compare
from test_range_leaf import RESIDENCIES, assert_same_state, state
from test_range_leaf import events as RL_events
import leaf_split_cases as LS

EV_FUSED, EV_NO_ROOM = 1, 3
EV_PAIRED, EV_PAIR_SPLIT, EV_RANGE_SPLIT = 6, 7, 8      # columns of events() below


def variant(leaf_split, insert_leaf):
    lib = os.path.join(ROOT, "tests", "emu", "libmtemu_leafsplit%d%d.so" % (leaf_split, insert_leaf))
    if not os.path.exists(lib) or any(os.path.getmtime(lib) < os.path.getmtime(d) for d in DEPS):
        _atomic_build(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DMT_G_MWMIN=64",
                       "-DMT_BPC_CHECK=1", "-DMT_EVRANGE", "-DMT_LEAF_SPLIT=%d" % leaf_split,
                       "-DMT_INSERT_LEAF=%d" % insert_leaf, "-o", None, SRC], lib)
    return lib


def factory(leaf_split, insert_leaf):
    lib = variant(leaf_split, insert_leaf)
    return lambda n, **kw: Engine(n, lib_path=lib, prefix="emu_", **kw)


def events(eng, n):
    """The eight -DMT_EVRANGE slots with slot 6 unpacked: columns 0..5 as they are, 6 paired
    inserts, 7 of those splitting their block, 8 range ops applied across a block split."""
    ev = RL_events(eng, n)
    return np.concatenate([ev[:, :6], ev[:, 6:7] & 0xFFFFFFFF, ev[:, 6:7] >> 32, ev[:, 7:8]], axis=1)


def run_both(batch, props, n, arm=(1, 1), **cap):
    """The build with the switches at `arm` and the build with both off on one batch, each checked
    against the oracle (compare); returns the first one's events, the other's and the first one's
    state, after checking that the states agree."""
    last = batch.op_offsets[1:] - 1
    msn, seq = batch.arrays["msn"][last], batch.arrays["seq"][last]
    got = []
    for sw in (arm, (0, 0)):
        eng = compare(batch, props, n, factory=factory(*sw), **cap)
        got.append((state(eng, n, msn, seq), events(eng, n)))
        eng.close()
    assert_same_state(got[0][0], got[1][0])
    return got[0][1], got[1][1], got[0][0]


@pytest.mark.parametrize("res", RESIDENCIES, ids=lambda r: "default" if r is None else "res%d" % r[0])
def test_hand_built_cases_match_oracle_and_two_visit_build(res):
    batch, props, paired, split = LS.build()
    n = len(paired)
    cap = {} if res is None else {"residency": res}
    ev1, ev0, _ = run_both(batch, props, n, **cap)
    assert (ev0[:, EV_PAIRED] == 0).all() and (ev0[:, EV_PAIR_SPLIT] == 0).all()
    for d, name in enumerate(LS.CASES):
        assert ev1[d, EV_PAIRED] == paired[d], f"{name}: {ev1[d, EV_PAIRED]} paired inserts, expected {paired[d]}"
        assert ev1[d, EV_PAIR_SPLIT] == split[d], f"{name}: {ev1[d, EV_PAIR_SPLIT]} block splits, expected {split[d]}"


@pytest.mark.parametrize("res", RESIDENCIES, ids=lambda r: "default" if r is None else "res%d" % r[0])
@pytest.mark.parametrize("mode", ["remove", "annotate"])
def test_hand_built_range_cases_match_oracle_and_three_visit_build(mode, res):
    batch, props, hits = LS.build_ranges(mode)
    n = len(hits)
    cap = {} if res is None else {"residency": res}
    ev1, ev0, _ = run_both(batch, props, n, **cap)
    assert (ev0[:, EV_RANGE_SPLIT] == 0).all()
    for d, name in enumerate(LS.RANGE_CASES):
        assert ev1[d, EV_RANGE_SPLIT] == hits[d], f"{name}: {ev1[d, EV_RANGE_SPLIT]} range ops across a split, expected {hits[d]}"
        # the old slots keep their meaning: no room is counted either way, fused only without a split
        assert ev1[d, EV_NO_ROOM] == ev0[d, EV_NO_ROOM] >= hits[d] and ev1[d, EV_FUSED] == ev0[d, EV_FUSED], name


@pytest.mark.parametrize("res", [None, (0, 0, 0, 0)], ids=["default", "res0"])
def test_compaction_between_the_cut_and_the_linking(res):
    """A text arena of 2,048 units for documents that insert some 3,900: it compacts several times
    per document, and an insert's own allocation is what sets a compaction off while its row's
    right half is cut but not yet among its block's children.  A half or a new row that the
    compaction missed would lose its text.  (A hand-built document cannot show this with the
    MSN at 0: nothing is ever reclaimed, so a full arena stays full.)"""
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS["cfg2"])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    cap = {"text": 2048} if res is None else {"text": 2048, "residency": res}
    ev1, ev0, s1 = run_both(batch, props, 4, **cap)
    assert (ev1[:, EV_PAIRED] > 0).all() and (ev0[:, EV_PAIRED] == 0).all()
    assert (s1["cnt_ins_units"] > 2048).all(), s1["cnt_ins_units"]      # more text than the arena holds: it compacted


def test_delta_capture_takes_the_two_visit_path():
    """With delta capture armed every insert takes the old path, and the records equal the oracle's."""
    from test_message_surface import check_delta_records
    made = []

    def f(n, **kw):
        made.append(factory(1, 1)(n, **kw))
        return made[-1]

    kinds = check_delta_records(f, "mixed", n_docs=2, n_msgs=400)
    assert {0, 1, 2, -2} <= kinds                            # INSERT, REMOVE, ANNOTATE and SPLIT records were compared
    ev = events(made[0], 2)
    assert (ev[:, 0] > 0).all() and (ev[:, [EV_FUSED, EV_PAIRED, EV_PAIR_SPLIT, EV_RANGE_SPLIT]] == 0).all(), ev


@pytest.mark.parametrize("res", RESIDENCIES, ids=lambda r: "default" if r is None else "res%d" % r[0])
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_generated_streams_one_visit_equals_two_visits(cfg, res):
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS[cfg])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    cap = {} if res is None else {"residency": res}
    ev1, ev0, _ = run_both(batch, props, 4, **cap)
    assert (ev0[:, EV_PAIRED] == 0).all() and (ev0[:, EV_RANGE_SPLIT] == 0).all()
    # not vacuous: every document took each new path, with and without a block split
    print(cfg, "paired inserts, of those splitting their block, range ops across a split, per document:\n", ev1[:, 6:9])
    assert (ev1[:, EV_PAIR_SPLIT] > 0).all() and (ev1[:, EV_PAIRED] > ev1[:, EV_PAIR_SPLIT]).all(), ev1[:, 6:9]
    assert (ev1[:, EV_RANGE_SPLIT] > 0).all() and (ev1[:, EV_RANGE_SPLIT] <= ev1[:, EV_NO_ROOM]).all(), ev1[:, :9]
    assert (ev1[:, EV_FUSED] == ev0[:, EV_FUSED]).all() and (ev1[:, EV_NO_ROOM] == ev0[:, EV_NO_ROOM]).all()


@pytest.mark.parametrize("arm", [(1, 0), (0, 1)], ids=["leaf_split_only", "insert_leaf_only"])
def test_generated_stream_each_switch_alone(arm):
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS["cfg2"])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    ev1, _, _ = run_both(batch, props, 4, arm=arm)
    assert ((ev1[:, EV_RANGE_SPLIT] > 0) == bool(arm[0])).all() and ((ev1[:, EV_PAIRED] > 0) == bool(arm[1])).all(), ev1[:, 6:9]
