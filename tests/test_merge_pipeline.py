"""The zamboni's merge runs (mt_core.h scourLeaves: decideRun, commitRun, gatherText through
global-typed text accesses): the state after every scour is the oracle's.

Hand-built streams of one client: a first phase inserts the segments with the MSN at 0, so nothing
is scoured; then the MSN follows the sequence number and one scour meets all the runs of the leaf
block.  Segments that are adjacent in the document but were inserted in reverse order lie apart in
the text arena, so the run that merges them copies its text (a "gather"); a property map of its
own separates two runs.  A generated stream (tests/batch_cut_cases.py cfg2) adds packParent's
scours over several leaf blocks.  The shapes: two and three copied runs in one scour, a run
extended in place between two copied ones, a run into the head's slack before one into a new
region, runs of exactly and of one more than MT_GT_CH * 64 units, a compaction by the second
run's plan, the last-unit load of the trailing-newline test, a head that loses MT_M_NONL.

Every stream runs under block and HBM residency, as one batch and one message per batch
(batch_cut_cases.cut_batch), and with delta capture armed (the FULL kernels), against the oracle:
statuses, text, the dump, both snapshot formats, the scoured / rows_rw counters.  The emulation
variant runs on a -DMT_EVGATHER build and asserts from its counters (tools/event_stats_gather.py)
that each stream reaches the shape it was built for.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine's library loads the HIP runtime, as tests/test_batch_cuts.py)

import batch_cut_cases as bc
from emu_lib import ROOT, _atomic_build
from fluidframework_amd.batch import BatchBuilder, ClientNames, PropTable
from fluidframework_amd.engine import Engine
from oracle_lib import OracleDoc
from test_batch_cuts import host_oracle_state, host_state
from test_combine_known_answers import ins, msg

sys.path.insert(0, os.path.join(ROOT, "tools"))
from event_stats_gather import AFTER, counts  # noqa: E402

CH_UNITS = 4 * 64                      # MT_GT_CH * MT_WAVE: the units gatherText loads before it stores any
CAPS = dict(rows_per_doc=512, window_per_doc=256, propsets_per_doc=256, text_per_doc=1 << 14)
EV_LIB = os.path.join(ROOT, "tests", "emu", "libmtemu_evgather.so")
EV_DEPS = [os.path.join(ROOT, "tests", "emu", "mt_emu.cpp"), os.path.join(ROOT, "include", "mtgpu.h")] + \
          [os.path.join(ROOT, "fluidframework_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "fluidframework_amd", "csrc"))]
RESIDENCIES = {"blk": 2, "hbm": 0}
SEP = {"text": "|", "props": {"s": 1}}


def build_ev_lib():
    if not os.path.exists(EV_LIB) or any(os.path.getmtime(EV_LIB) < os.path.getmtime(d) for d in EV_DEPS):
        _atomic_build(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DMT_EVGATHER",
                       "-DMT_G_MWMIN=64", "-DMT_BPC_CHECK=1", "-o", None, EV_DEPS[0]], EV_LIB)
    return EV_LIB


FACTORIES = {"emu": lambda n, **kw: Engine(n, lib_path=build_ev_lib(), prefix="emu_", **kw),
             "gpu": lambda n, **kw: Engine(n, device=0, **kw)}


# ---- the streams ---------------------------------------------------------------------------
def t(ch, n):
    return ch * n


def P(ch, n):
    """A text segment with the separator's property map."""
    return {"text": ch * n, "props": {"s": 1}}


def reversed_inserts(segs):
    """Inserts that leave `segs` in document order and in reverse order in the text arena."""
    return [ins(0, s) for s in reversed(segs)]


def one_more(msgs, op=None, msn=None):
    """One more message after `msgs` (MSN: its reference sequence number unless given); without
    an op, a message that only moves the sequence numbers (the leaf blocks stay as they are)."""
    k = len(msgs)
    m = msg(k + 1, k, k if msn is None else msn, op)
    if op is None:
        m["type"] = "noop"
    return msgs + [m]


def settle(ops, n=3):
    """`ops` with the MSN at 0, then n messages whose MSN follows the sequence number."""
    msgs = [msg(i + 1, i, 0, op) for i, op in enumerate(ops)]
    for _ in range(n):
        msgs = one_more(msgs)
    return msgs


def slack_then_region():
    """A scour merges A1 A2 into a region of twice their size; then A3 arrives behind them (it fits
    the head's slack) and B1 B2 behind a separator (a new region): both runs in the next scour."""
    msgs = settle(reversed_inserts([t("a", 10), t("b", 10)]), n=2)          # merged: one segment of 20 units
    k = len(msgs)
    held = msgs[-1]["minimumSequenceNumber"]
    for op in [ins(20, t("d", 9)), ins(20, t("c", 9)), ins(20, SEP), ins(20, t("e", 5))]:   # a b e | c d
        msgs = one_more(msgs, op, msn=held)
    assert len(msgs) == k + 4
    for _ in range(3):
        msgs = one_more(msgs)
    return msgs


# name -> (messages, text_per_doc or None, the counters the emulation must show)
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out["two_runs"] = (settle(reversed_inserts([t("a", 7), t("b", 9), SEP, t("c", 70), t("d", 5)])), None,
                       {AFTER: 1})
    # (a leaf block holds seven children at most: the middle run is set apart by its property map)
    out["three_runs"] = (settle(reversed_inserts([t("a", 7), t("b", 9), P("c", 70), P("d", 5), t("e", 3), t("f", 130)])),
                         None, {AFTER: 2, "calls with >= 3 gathers": 1})
    # c d are inserted one after the other: adjacent in the arena, extended in place
    ops = reversed_inserts([t("e", 3), t("f", 13)]) + [ins(0, P("c", 6)), ins(6, P("d", 4))] + \
        reversed_inserts([t("a", 7), t("b", 9)])
    out["in_place_between"] = (settle(ops), None, {"gathers after a gather and a run extended in place": 1})
    out["slack_then_region"] = (slack_then_region(), None, {"new-region gathers right after a slack gather": 1})
    out["exact_and_one_more"] = (settle(reversed_inserts([t("a", 100), t("b", CH_UNITS - 100), SEP, t("c", 100), t("d", CH_UNITS - 99)])),
                                 None, {"gathers of exactly MT_GT_CH chunks": 1, "gathers of more than MT_GT_CH chunks": 1, AFTER: 1})
    out["newlines"] = (settle(reversed_inserts(["ab", "x\n", "yy", "zz", SEP, "p\nq", "rr"])), None,
                       {"calls that load a last unit (lastNL)": 1, "heads that lose MT_M_NONL": 1, AFTER: 2})
    return out


GC_TEXT = 300        # text_per_doc of the compaction stream: 141 units inserted, 120 more for the first run, 160 for the second


@functools.lru_cache(maxsize=None)
def gc_case():
    """The second run's new region no longer fits the arena's live half: its plan compacts, with
    the first run's move made before it."""
    segs = [t("a", 30), t("b", 30), SEP, t("c", 40), t("d", 40)]
    return settle(reversed_inserts(segs)), GC_TEXT, {"compactions by a run's plan after a gather in the call": 1}


# ---- the harness -----------------------------------------------------------------------------
class Harness:
    """One document per stream on one engine, beside one oracle document each."""

    def __init__(self, kind, streams, res, text=None, capture=False):
        self.n = len(streams)
        self.eng = FACTORIES[kind](self.n, **{**CAPS, **({"text_per_doc": text} if text else {})})
        self.eng.set_residency(RESIDENCIES[res])
        self.props = PropTable()
        self.eng.props = self.props
        self.names = [ClientNames() for _ in range(self.n)]
        self.eng.open_docs(0, self.n)
        if capture:
            self.eng.delta_capture(1 << 16)
        self.ora = [OracleDoc(True) for _ in range(self.n)]
        self.ora_counting = [OracleDoc(True) for _ in range(self.n)]    # never read (the oracle's reads count rows too)
        self.msn, self.seq = [0] * self.n, [0] * self.n
        self.streams = streams
        bb = BatchBuilder(self.props, None)
        for d, msgs in enumerate(streams):
            bb.names = self.names[d]
            bb.begin_doc(d)
            for m in msgs:
                bb.add_message(m)
            self.eng.upload_doc_names(d, self.names[d].json_literals())
        self.batch = bb.build()
        if kind == "emu":
            self.prof = self.eng.lib.emu_prof_get
            import ctypes as C
            self.prof.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]

    def oracle_to(self, upto):
        """The oracle's documents brought to message upto[d] of each stream."""
        for d, msgs in enumerate(self.streams):
            for m in msgs[self.seq[d]:upto[d]]:
                assert self.ora[d].apply_msg(m) == 0 and self.ora_counting[d].apply_msg(m) == 0
                self.msn[d], self.seq[d] = m["minimumSequenceNumber"], m["sequenceNumber"]

    def check(self, where):
        bc.assert_same_state(host_state(self.eng, self.n, self.msn, self.seq), host_oracle_state(self.ora, self.msn, self.seq), where)
        got = self.eng.counters(range(self.n))
        for d, od in enumerate(self.ora_counting):
            want = od.counters()
            assert {k: int(got[k][d]) for k in ("scoured", "rows_rw")} == {k: want[k] for k in ("scoured", "rows_rw")}, (where, d)

    def counts(self):
        raw = np.zeros((self.n, 8), np.uint64)
        self.prof(self.eng.h, self.n, raw.ctypes.data)
        return [counts(raw[d:d + 1]) for d in range(self.n)]


def run_streams(kind, names, streams, wants, res, cutting, text=None, capture=False):
    h = Harness(kind, streams, res, text, capture)
    if cutting == "one_batch":
        h.eng.apply(h.batch)
        h.eng.sync()
        h.oracle_to([len(s) for s in streams])
        h.check("one batch")
    else:
        done = [0] * h.n
        for j, (b, runs) in enumerate(bc.cut_batch(h.batch, bc.plan_per_message(bc.n_messages(h.batch)))):
            h.eng.apply(b)
            h.eng.sync()
            for r in runs:
                done[r] += 1
            h.oracle_to(done)
            h.check(f"after message {j}")
        assert done == [len(s) for s in streams]
    if kind == "emu":
        for name, got, want in zip(names, h.counts(), wants):
            for key, least in want.items():
                assert got[key] >= least, f"{name}: {key} = {got[key]}, the stream does not reach its shape ({got})"
    h.eng.close()


def run_cases(kind, res, cutting, capture=False):
    cs = cases()
    run_streams(kind, list(cs), [c[0] for c in cs.values()], [c[2] for c in cs.values()], res, cutting, capture=capture)
    msgs, text, want = gc_case()
    run_streams(kind, ["compaction"], [msgs], [want], res, cutting, text=text, capture=capture)


def run_generated(kind, res, n_docs=2):
    """cfg2 of the batch-cut streams: packParent scours several leaf blocks in one visit."""
    batch, props = bc.generated("cfg2", n_docs)
    eng = bc.new_engine(FACTORIES[kind], n_docs, props, (RESIDENCIES[res], 0, 0, 0))
    ora = bc.Oracle(n_docs, props)
    eng.apply(batch)
    eng.sync()
    ora.apply(batch, list(range(n_docs)))
    wants = [od.counters() for od in ora.docs]            # before the oracle's reads, which count rows too
    bc.assert_same_state(bc.engine_state(eng, n_docs, ora.msn, ora.seq), ora.state(), "generated cfg2")
    got = eng.counters(range(n_docs))
    for d, want in enumerate(wants):
        assert {k: int(got[k][d]) for k in ("scoured", "rows_rw")} == {k: want[k] for k in ("scoured", "rows_rw")}, d
    if kind == "emu":
        import ctypes as C
        fn = eng.lib.emu_prof_get
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        raw = np.zeros((n_docs, 8), np.uint64)
        fn(eng.h, n_docs, raw.ctypes.data)
        c = counts(raw)
        assert c["gathers after a gather, call over >= 3 leaves (packParent)"] >= 10 and c["calls with >= 3 gathers"] >= 10, c
        assert c["gathers"] > c[AFTER] > 0 and c["64-unit chunks"] >= c["gathers"], c
    eng.close()


RES = pytest.mark.parametrize("res", list(RESIDENCIES))
CUT = pytest.mark.parametrize("cutting", ["one_batch", "per_message"])


@RES
@CUT
def test_merge_runs_on_emulation(res, cutting):
    run_cases("emu", res, cutting)


@RES
def test_merge_runs_with_capture_armed_on_emulation(res):
    run_cases("emu", res, "one_batch", capture=True)


@RES
def test_generated_stream_on_emulation(res):
    run_generated("emu", res)


@pytest.mark.gpu
@RES
@CUT
def test_merge_runs_on_gpu(res, cutting):
    run_cases("gpu", res, cutting)


@pytest.mark.gpu
@RES
def test_merge_runs_with_capture_armed_on_gpu(res):
    run_cases("gpu", res, "one_batch", capture=True)


@pytest.mark.gpu
@RES
def test_generated_stream_on_gpu(res):
    run_generated("gpu", res)
