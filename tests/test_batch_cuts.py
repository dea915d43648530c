"""A stream's result does not depend on how it is cut into batches.

1. Device level (tests/batch_cut_cases.py): generated OpBatch streams through Engine.apply under
   three cuttings and every residency, with the property table arriving late, a checkpoint
   between two cuttings, documents that grow, and reads between the batches.
2. Host level: message streams (tests/msg_gen.py) through ClientGroup and the Node Client with a
   flush every 1, 7 or a random number of messages; the held-string incr chain one message per
   flush (PropTable.version: the device's table follows the chain, and nothing else uploads it).
3. Wide-key tracking (mt_ctx::doc_wide) across mt_checkpoint / mt_docs_open / mt_restore and
   device-built batches: known answers on maps of more than 64 keys.

Every check runs on the host emulation and, marked gpu, on the device.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (device buffers for mt_upload_batch_dev; imported before the engine's library loads the
#                            HIP runtime, so that both use one copy of it, as tests/test_shard.py's import sees to)

import batch_cut_cases as bc
from emu_lib import emu_engine
from fluidframework_amd.batch import BatchBuilder, ClientNames, OpBatch, PropTable
from fluidframework_amd.engine import ClientGroup, Engine
from msg_gen import stream
from oracle_lib import OracleDoc, gen_params, generate
from test_combine_known_answers import ann, ins, msg, props_texts
from test_message_surface import COLS, LIMITS, SURFACES

bc.FACTORIES["emu"] = emu_engine
bc.FACTORIES["gpu"] = lambda n, **kw: Engine(n, device=0, **kw)
N_DOCS = {"emu": 3, "gpu": 6}
gpu = pytest.mark.gpu
RES = pytest.mark.parametrize("res,cont", bc.RESIDENCIES, ids=bc.RES_IDS)
SMALL = pytest.mark.parametrize("res,cont", bc.SMALL, ids=bc.RES_IDS[:4])


# ---- 1. device level -------------------------------------------------------------------------
@RES
@pytest.mark.parametrize("cutting", bc.CUTTINGS)
@pytest.mark.parametrize("cfg", bc.STREAMS)
def test_cuts_match_oracle_on_emulation(cfg, cutting, res, cont):
    bc.run_cut("emu", cfg, 3, cutting, res, cont)


@gpu
@RES
@pytest.mark.parametrize("cutting", bc.CUTTINGS)
@pytest.mark.parametrize("cfg", bc.STREAMS)
def test_cuts_match_oracle_on_gpu(cfg, cutting, res, cont):
    bc.run_cut("gpu", cfg, 6, cutting, res, cont)


def test_cut_helper_covers_the_cuttings():
    """The plans do what they say: every message once and in order, different numbers of cuts per
    document, documents absent from batches, about 40 random cuts per document."""
    batch, _ = bc.generated("cfg3", 3)
    n = bc.n_messages(batch)
    for name, plan_of in bc.PLANS.items():
        plan = plan_of(n)
        pieces = bc.cut_batch(batch, plan)
        seqs = {r: [] for r in range(3)}
        for b, runs in pieces:
            for i, r in enumerate(runs):
                seqs[r] += b.arrays["seq"][int(b.op_offsets[i]):int(b.op_offsets[i + 1])].tolist()
        for r in range(3):
            assert seqs[r] == batch.arrays["seq"][int(batch.op_offsets[r]):int(batch.op_offsets[r + 1])].tolist(), name
        if name == "per_message":
            assert len(pieces) == bc.PER_MESSAGE + 1 and all(len(runs) == 3 for _, runs in pieces)
        if name == "random":
            cuts = [len(p) for p in plan]
            assert len(set(cuts)) > 1 and all(25 <= c <= 60 for c in cuts), cuts
            w = np.diff([0] + [e for _, e in plan[0]])
            assert w.min() >= 1 and w.max() <= 200 and w.max() > 100 and (w <= 3).any(), w
        if name.startswith("late"):
            assert all(len(runs) == 3 and b.n_ops == 3 for b, runs in pieces[:24])
        if name == "ragged":
            for j, (b, runs) in enumerate(pieces[:12]):
                assert runs == [r for r in range(3) if (j + 1) % (r + 1) == 0], (j, runs)


LATE = pytest.mark.parametrize("cfg,cutting", [("cfg3", "late_random"), ("grow", "per_message"), ("cfg3", "late_ragged")])


@RES
@LATE
def test_props_arriving_late_on_emulation(cfg, cutting, res, cont):
    bc.run_late_props("emu", cfg, 3, cutting, res, cont)


@gpu
@RES
@LATE
def test_props_arriving_late_on_gpu(cfg, cutting, res, cont):
    bc.run_late_props("gpu", cfg, 6, cutting, res, cont)


@RES
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_checkpoint_across_cuts_on_emulation(cfg, res, cont):
    bc.run_checkpoint("emu", cfg, 3, res, cont)


@gpu
@RES
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_checkpoint_across_cuts_on_gpu(cfg, res, cont):
    bc.run_checkpoint("gpu", cfg, 6, res, cont)


@RES
def test_autogrow_across_cuts_on_emulation(res, cont):
    bc.run_autogrow("emu", "grow", 3, res, cont)


@gpu
@RES
def test_autogrow_across_cuts_on_gpu(res, cont):
    bc.run_autogrow("gpu", "grow", 6, res, cont)


@RES
def test_reads_between_cuts_on_emulation(res, cont):
    bc.run_reads("emu", "cfg3", 3, res, cont)


@gpu
@RES
def test_reads_between_cuts_on_gpu(res, cont):
    bc.run_reads("gpu", "cfg3", 6, res, cont)


# ---- 2. host level ---------------------------------------------------------------------------
HOST_SURFACES = ["mixed", "groups", "markers_props", "relative", "registers", "combine", "wide_props", "very_wide_props",
                 "churn"]
FLUSHES = [1, 7, "random"]


def schedule(n_docs, n_msgs, flush_every, seed=5):
    """[[messages of document d before flush f]]: documents receive different numbers of messages
    per flush and sit some flushes out.  flush_every 1: one message, every fourth flush none;
    7: six to eight; "random": 1 to 60 from a seeded generator, one flush in five none."""
    rng = np.random.RandomState(seed)
    left, out, f = [n_msgs] * n_docs, [], 0
    while any(left):
        row = []
        for d in range(n_docs):
            if flush_every == "random":
                n = 0 if rng.randint(5) == 0 else int(rng.randint(1, 61))
            else:
                n = 0 if (f + d) % 4 == 3 else (1 if flush_every == 1 else flush_every + d % 3 - 1)
            n = min(n, left[d])
            left[d] -= n
            row.append(n)
        out.append(row)
        f += 1
    return out


@functools.lru_cache(maxsize=4)
def surface_streams(surface, n_docs, n_msgs):
    return [stream(101 + d, n_msgs, **SURFACES[surface]) for d in range(n_docs)]


def host_state(eng, n, msn, seq):
    dumps = [eng.dump(d)[:, COLS].tobytes() for d in range(n)]
    return ([int(s) for s in eng.status(range(n))], eng.get_text(range(n)), dumps, eng.snapshot(range(n), msn, seq),
            eng.snapshot(range(n), msn, seq, legacy=True), [int(x) for x in eng.snapshot_digests(range(n), msn, seq)])


def host_oracle_state(docs, msn, seq):
    st = list(bc.oracle_state(docs, msn, seq))
    st[2] = [od.dump()[:, COLS].tobytes() for od in docs]
    return tuple(st)


def check_host(kind, surface, flush_every):
    n_docs = N_DOCS[kind]
    n_msgs = 400 if flush_every == 1 else 1200
    streams = surface_streams(surface, n_docs, n_msgs)
    g = ClientGroup(bc.FACTORIES[kind](n_docs, **LIMITS))
    clients = [g.new_client({"newMergeTreeSnapshotFormat": True}) for _ in range(n_docs)]
    for c in clients:
        c.startOrUpdateCollaboration("observer")
    docs = [OracleDoc(True) for _ in range(n_docs)]
    at, msn, seq = [0] * n_docs, [0] * n_docs, [0] * n_docs
    sched = schedule(n_docs, n_msgs, flush_every)
    every = {1: 25, 7: 10}.get(flush_every, 1)
    for f, row in enumerate(sched):
        for d, n in enumerate(row):
            for m in streams[d][0][at[d]:at[d] + n]:
                clients[d].applyMsg(m)
                assert docs[d].apply_msg(m) == 0
                msn[d], seq[d] = m["minimumSequenceNumber"], m["sequenceNumber"]
            at[d] += n
        g.flush()
        if (f + 1) % every == 0 or f == len(sched) - 1:
            bc.assert_same_state(host_state(g.engine, n_docs, msn, seq), host_oracle_state(docs, msn, seq),
                                 f"{surface}: after flush {f} of {len(sched)}")
    # the stream's own observer (msg_gen) saw the same messages: the prefix oracle ended where it did
    assert [od.get_text() for od in docs] == [obs.get_text() for _, obs in streams]
    assert len({tuple(r) for r in sched}) > 2 and any(0 in r for r in sched)
    g.engine.close()


@pytest.mark.parametrize("flush_every", FLUSHES)
@pytest.mark.parametrize("surface", HOST_SURFACES)
def test_flush_windows_on_emulation(surface, flush_every):
    check_host("emu", surface, flush_every)


@gpu
@pytest.mark.parametrize("flush_every", FLUSHES)
@pytest.mark.parametrize("surface", HOST_SURFACES)
def test_flush_windows_on_gpu(surface, flush_every):
    check_host("gpu", surface, flush_every)


def chain_msgs(n=6):
    """A held string under one key, then n incr annotates of it (test_combine_known_answers'
    incr_string_twice, longer): "v" + n x "undefined"."""
    ops = [ins(0, {"text": "ab", "props": {"s": "v"}})] + [ann(0, 2, {"s": 1}, {"name": "incr"}) for _ in range(n)]
    return [msg(i + 1, i, i, op) for i, op in enumerate(ops)]


CHAIN_WANT = ['{"s":"v' + "undefined" * 6 + '"}']


def check_incr_chain(kind, n_docs):
    """Each incr in a flush of its own, the annotates alternating between the documents: the
    second incr names no new set, yet the device must know "vundefined" + "undefined".  The table
    is uploaded once per change (the insert's set, then one step of the chain per incr op) and
    never when a flush changes nothing."""
    g = ClientGroup(bc.FACTORIES[kind](n_docs, **LIMITS))
    clients = [g.new_client({"newMergeTreeSnapshotFormat": True}) for _ in range(n_docs)]
    uploads = []
    real = g.engine.upload_props
    g.engine.upload_props = lambda *a, **k: (uploads.append(1), real(*a, **k))[1]
    msgs = chain_msgs()
    for c in clients:
        c.applyMsg(msgs[0])
    g.flush()
    for m in msgs[1:]:
        for c in clients:
            c.applyMsg(m)
            g.flush()
    st = g.engine.status(range(n_docs))
    assert (st == 0).all(), st
    assert len(uploads) == 1 + 6 * n_docs, len(uploads)
    tail = msg(8, 7, 7, ins(0, "zz"))
    for c in clients:
        c.applyMsg(tail)
        g.flush()
    assert len(uploads) == 1 + 6 * n_docs, "a flush that changed nothing in the table uploaded it"
    st = g.engine.status(range(n_docs))
    assert (st == 0).all(), st
    o = OracleDoc(True)
    for m in msgs + [tail]:
        assert o.apply_msg(m) == 0
    for d in range(n_docs):
        for legacy in (False, True):
            (eb, edig), = g.engine.snapshot([d], [7], [8], legacy=legacy)
            ob, odig = o.snapshot(7, 8, legacy=legacy)
            assert eb == ob and edig == odig, (d, legacy)
        assert props_texts(eb) == CHAIN_WANT
        assert (g.engine.dump(d)[:, COLS] == o.dump()[:, COLS]).all()
    g.engine.close()


@pytest.mark.parametrize("n_docs", [1, 2])
def test_incr_chain_per_flush_on_emulation(n_docs):
    check_incr_chain("emu", n_docs)


@gpu
@pytest.mark.parametrize("n_docs", [1, 2])
def test_incr_chain_per_flush_on_gpu(n_docs):
    check_incr_chain("gpu", n_docs)


def test_prop_table_version_follows_what_to_c_builds():
    pt = PropTable()
    seen = [pt.version]

    def changed():
        seen.append(pt.version)
        return seen[-1] != seen[-2]
    pt.intern({"a": 1})
    assert changed()
    pt.intern({"a": 1})
    assert not changed()
    pt.intern({"a": 2})
    assert changed()                                   # a value and a set
    pt.intern_combine({"a": 1}, {"name": "incr"}, 3)
    assert changed()                                   # a set, an incr key, a deeper chain
    pt.intern_combine({"a": 1}, {"name": "incr"}, 4)
    assert changed()                                   # no new set: the chain alone
    for i in range(70):
        pt.intern_combine({"a": 1}, {"name": "incr"}, 5 + i)
    v = pt.version
    pt.intern_combine({"a": 1}, {"name": "incr"}, 99)  # past INCR_CHAIN_MAX the table stays as it is
    assert pt.version == v
    pt.intern_combine({"a": 1}, {"name": "consensus"}, 5)
    c0 = pt.to_c()
    assert pt.to_c() is c0
    pt.key_id("b")
    assert pt.to_c() is not c0


# ---- the Node host -------------------------------------------------------------------------------
NODE_LIMITS = dict(rowsPerDoc=30000, windowPerDoc=8192, propsetsPerDoc=30000, textPerDoc=1 << 19, blocksPerDoc=16384,
                   heapPerDoc=30000)


def node_addon(kind):
    from js_lib import NODE, ROOT
    if NODE is None:
        pytest.skip("node is not installed")
    if kind == "gpu":
        return os.path.join(ROOT, "fluidframework_amd", "js", "mtgpu.node")
    from emu_lib import build_emu_napi
    return build_emu_napi()


def run_node_schedule(kind, doc_msgs, sched):
    from js_lib import run_driver
    return run_driver("replay_check.js", {"docs": doc_msgs, "limits": NODE_LIMITS, "schedule": sched}, addon=node_addon(kind))


def check_node_flush(kind, surface, flush_every):
    n_docs = N_DOCS[kind]
    n_msgs = 400 if flush_every == 1 else 1200
    streams = surface_streams(surface, n_docs, n_msgs)
    got = run_node_schedule(kind, [m for m, _ in streams], schedule(n_docs, n_msgs, flush_every))
    for d, (msgs, obs) in enumerate(streams):
        assert got["texts"][d] == obs.get_text(), f"doc {d}: text"
        assert got["lengths"][d] == obs.get_length()
        blobs, dig = obs.snapshot(msgs[-1]["minimumSequenceNumber"], msgs[-1]["sequenceNumber"])
        want = [("header" if i == 0 else f"body_{i - 1}", b.decode("utf-8", "surrogatepass")) for i, b in enumerate(blobs)]
        assert [tuple(x) for x in got["blobs"][d]] == want, f"doc {d}: snapshot"
        assert int(got["digests"][d], 16) == dig


NODE_CASES = pytest.mark.parametrize("surface,flush_every", [(s, k) for s in ("mixed", "combine", "very_wide_props")
                                                             for k in (1, 7)])


@NODE_CASES
def test_flush_windows_node_host_on_emulation(surface, flush_every):
    check_node_flush("emu", surface, flush_every)


@gpu
@NODE_CASES
def test_flush_windows_node_host_on_gpu(surface, flush_every):
    check_node_flush("gpu", surface, flush_every)


def check_node_incr(kind, n_docs):
    """check_incr_chain through the Node Client: js/builder.js PropTable.version."""
    msgs = chain_msgs() + [msg(8, 7, 7, ins(0, "zz")), msg(9, 8, 8, ins(0, "yy"))]
    sched = [[1] * n_docs] + [[1 if e == d else 0 for e in range(n_docs)] for _ in msgs[1:] for d in range(n_docs)]
    got = run_node_schedule(kind, [msgs] * n_docs, sched)
    o = OracleDoc(True)
    for m in msgs:
        assert o.apply_msg(m) == 0
    blobs, dig = o.snapshot(8, 9)
    for d in range(n_docs):
        assert [b.encode() for _, b in got["blobs"][d]] == blobs
        assert int(got["digests"][d], 16) == dig
        assert props_texts([b.encode() for _, b in got["blobs"][d]]) == CHAIN_WANT
    assert got["propUploads"] == 1 + 6 * n_docs, got["propUploads"]


def check_node_incr_twice(kind):
    from test_combine_known_answers import CASES, stream_of
    _, ops, want = CASES[[c[0] for c in CASES].index("incr_string_twice")]
    got = run_node_schedule(kind, [stream_of(ops, msn_lag=0)], [[1]] * len(ops))
    assert props_texts([b.encode() for _, b in got["blobs"][0]]) == want


def check_parts_incr(kind):
    """The chain through the parallel packers' path (js/parallel.js absorb carries the incr inputs
    of each worker's table into the engine's): one message per window, packed by fresh tables and
    applied as parts (mt_apply_batch_parts), against one builder's single batch and the oracle."""
    from js_lib import run_driver
    msgs = chain_msgs()
    got = run_driver("parts_check.js", {"docs": [msgs] * 3, "parts": 2, "windows": len(msgs)}, addon=node_addon(kind))
    o = OracleDoc(True)
    for m in msgs:
        assert o.apply_msg(m) == 0
    _, dig = o.snapshot(6, 7)
    assert got["b"]["digests"] == got["a"]["digests"] == ["%x" % dig] * 3
    assert got["b"]["texts"] == got["a"]["texts"]
    assert got["propUploads"] == len(msgs), got["propUploads"]      # the insert's set, then a step per window


def test_incr_chain_batch_parts_node_host_on_emulation():
    check_parts_incr("emu")


@gpu
def test_incr_chain_batch_parts_node_host_on_gpu():
    check_parts_incr("gpu")


@pytest.mark.parametrize("n_docs", [1, 2])
def test_incr_chain_node_host_on_emulation(n_docs):
    check_node_incr("emu", n_docs)


def test_incr_string_twice_per_message_node_host_on_emulation():
    check_node_incr_twice("emu")


@gpu
@pytest.mark.parametrize("n_docs", [1, 2])
def test_incr_chain_node_host_on_gpu(n_docs):
    check_node_incr("gpu", n_docs)


@gpu
def test_incr_string_twice_per_message_node_host_on_gpu():
    check_node_incr_twice("gpu")


# ---- 3. wide-key tracking across lifecycle calls ---------------------------------------------
def widths(blobs):
    """The number of keys of every segment map of a SnapshotV1."""
    segs = [x["json"] if isinstance(x, dict) and "json" in x else x for b in blobs for x in json.loads(b).get("segments", [])]
    return [len(j["props"]) for j in segs if isinstance(j, dict) and "props" in j]


def wide_msgs(seq0=0, text="abcdefgh"):
    """One segment that two annotates of 40 keys each make 80 keys wide."""
    ops = [ins(0, text), ann(0, len(text), {f"a{i}": i for i in range(40)}), ann(0, len(text), {f"b{i}": i for i in range(40)})]
    return [msg(seq0 + i + 1, seq0 + i, 0, op) for i, op in enumerate(ops)]


class WideHarness:
    """Two documents on one engine, fed message lists as host batches (one BatchBuilder batch per
    call), beside one oracle document each."""

    def __init__(self, kind, n=2):
        self.n = n
        self.eng = bc.FACTORIES[kind](n, **LIMITS)
        self.props = PropTable()
        self.eng.props = self.props
        self.names = [ClientNames() for _ in range(n)]
        self.eng.open_docs(0, n)
        self.ora = [OracleDoc(True) for _ in range(n)]
        self.msn, self.seq = [0] * n, [0] * n

    def batch(self, per_doc, oracle=True, resident=False):
        """resident: mt_upload_batch and mt_replay_resident in place of mt_apply_batch (the host
        counts the batch's keys at the upload; the caller may replay it again)."""
        bb = BatchBuilder(self.props, None)
        for d, msgs in per_doc.items():
            bb.names = self.names[d]
            bb.begin_doc(d)
            for m in msgs:
                bb.add_message(m)
                if oracle:
                    assert self.ora[d].apply_msg(m) == 0
                    self.msn[d], self.seq[d] = m["minimumSequenceNumber"], m["sequenceNumber"]
            self.eng.upload_doc_names(d, self.names[d].json_literals())
        if resident:
            self.eng.upload(bb.build())
            self.eng.replay_resident()
        else:
            self.eng.apply(bb.build())
        self.eng.sync()

    def max_width(self, d):
        return max(widths(self.ora[d].snapshot(self.msn[d], self.seq[d])[0]) or [0])

    def check(self, where):
        bc.assert_same_state(host_state(self.eng, self.n, self.msn, self.seq),
                             host_oracle_state(self.ora, self.msn, self.seq), where)


def coalesce_at_msn(h, d):
    """Adjacent segments with equal maps of more than 64 keys, then the MSN moves over them: an
    annotate that rewrites three keys with the values they hold splits the segment in two equal
    maps, and the next message's MSN lets zamboni merge them (propsMatch on wide maps).  The
    snapshot coalesces them as the oracle's does."""
    s = h.seq[d]
    same = {"a0": 0, "b0": 0, "a1": 1}
    h.batch({d: [msg(s + 1, s, h.msn[d], ann(5, 7, same))]})
    before = len(h.ora[d].dump())
    h.batch({d: [msg(s + 2, s + 1, s + 1, ins(0, "x")), msg(s + 3, s + 2, s + 2, ins(0, "y"))]})
    assert len(h.ora[d].dump()) < before + 2, "the oracle's zamboni merged nothing"
    assert h.max_width(d) > 64
    h.check("after the MSN moved over equal wide maps")


def check_reopen_restore(kind):
    """checkpoint, mt_docs_open, restore: the device's maps are wide again, and so must the
    host's mark be (a three-key annotate in the narrow kernels would raise MT_DS_PROPS_TOO_MANY)."""
    h = WideHarness(kind)
    h.batch({0: wide_msgs(), 1: [msg(1, 0, 0, ins(0, "narrow"))]})
    assert h.max_width(0) > 64, h.max_width(0)          # the test proves nothing otherwise
    h.check("wide")
    h.eng.checkpoint()
    h.eng.open_docs(0, 1)
    h.eng.restore()
    h.check("restored")
    h.batch({0: [msg(4, 3, 0, ann(2, 5, {"a0": "x", "b0": "y", "c0": "z"}))]})
    assert h.max_width(0) > 64
    h.check("narrow annotate after reopen and restore")
    coalesce_at_msn(h, 0)
    h.eng.close()


def check_restore_alone(kind):
    """A checkpoint taken while document 0 is wide; document 1 widens in two batches after it;
    restore brings both back, with what the host knew of their keys then."""
    h = WideHarness(kind)
    h.batch({0: wide_msgs(), 1: [msg(1, 0, 0, ins(0, "abcdefgh"))]})
    assert h.max_width(0) > 64
    h.eng.checkpoint()
    saved = (list(h.msn), list(h.seq))
    w = wide_msgs(1)[1:]
    h.batch({1: [msg(2, 1, 0, w[0]["contents"])]}, oracle=False)
    h.batch({1: [msg(3, 2, 0, w[1]["contents"])]}, oracle=False)
    assert int(h.eng.status([1])[0]) == 0
    h.eng.restore()
    h.msn, h.seq = saved
    h.check("restored")
    narrow = {"a0": "x", "b0": "y", "c0": "z"}
    h.batch({0: [msg(4, 3, 0, ann(2, 5, narrow))], 1: [msg(2, 1, 0, ann(2, 5, narrow))]})
    assert h.max_width(0) > 64 and h.max_width(1) == 3
    h.check("narrow annotates after restore")
    # document 1 widens again, 40 keys a batch: its keys are counted from the checkpoint's on
    h.batch({1: [msg(3, 2, 0, w[0]["contents"])]})
    h.batch({1: [msg(4, 3, 0, w[1]["contents"])]})
    h.batch({1: [msg(5, 4, 0, ann(1, 3, narrow))]})
    assert h.max_width(1) > 64
    h.check("document 1 wide after the restore")
    coalesce_at_msn(h, 0)
    h.eng.close()


def keys(prefix, n, first=0):
    return {f"{prefix}{i}": i for i in range(first, first + n)}


def check_restore_replay_resident(kind, case):
    """A batch uploaded after the checkpoint and replayed again after the restore (the flow
    mt_checkpoint exists for): the host counted its keys once, at the upload, and the restore must
    not roll that count back, or the narrow batch that follows runs in the narrow kernels on maps
    the second replay made wide again.
    wide: the resident batch alone takes the document from 0 to 80 keys; reopen: mt_docs_open
    between the replay and the restore as well; partial: 30 keys before the checkpoint, 30 more
    in the resident batch, 10 more in the host batch after the second replay (70 in all)."""
    h = WideHarness(kind)
    h.batch({0: [msg(1, 0, 0, ins(0, "abcdefgh"))], 1: [msg(1, 0, 0, ins(0, "narrow"))]})
    if case == "partial":
        # (the table must name more than 64 keys for any document to count: document 1 names the rest)
        h.batch({0: [msg(2, 1, 0, ann(0, 8, keys("a", 30)))], 1: [msg(2, 1, 0, ann(0, 6, keys("z", 40)))]})
        res = [msg(3, 2, 0, ann(0, 8, keys("b", 30)))]
        after = [msg(4, 3, 0, ann(2, 5, keys("c", 10))), msg(5, 4, 0, ann(1, 3, {"a0": "x", "b0": "y", "c0": "z"}))]
    else:
        res = [msg(2, 1, 0, ann(0, 8, keys("a", 40))), msg(3, 2, 0, ann(0, 8, keys("b", 40)))]
        after = [msg(4, 3, 0, ann(2, 5, {"a0": "x", "b0": "y", "c0": "z"}))]
    h.eng.checkpoint()
    h.batch({0: res}, resident=True)
    h.check("first replay")
    if case == "reopen":
        h.eng.open_docs(0, 1)
    h.eng.restore()
    h.eng.replay_resident()
    h.eng.sync()
    h.check("second replay")
    for m in after:
        h.batch({0: [m]})
    assert h.max_width(0) > 64, h.max_width(0)
    h.check("host batches after the second replay")
    if case != "partial":
        coalesce_at_msn(h, 0)
    h.eng.close()


RESIDENT_CASES = ["wide", "reopen", "partial"]


@pytest.mark.parametrize("case", RESIDENT_CASES)
def test_wide_keys_survive_restore_and_replay_resident_on_emulation(case):
    check_restore_replay_resident("emu", case)


@gpu
@pytest.mark.parametrize("case", RESIDENT_CASES)
def test_wide_keys_survive_restore_and_replay_resident_on_gpu(case):
    check_restore_replay_resident("gpu", case)


GEN_WIDE = dict(clients=2, lag=4, ins=10, rem=2, ins_len=16, rem_len=32, ops=1500, ann_sets=48, rewrite=0)


@functools.lru_cache(maxsize=None)
def wide_generated(n_docs):
    """A generated stream whose annotates (48 sets of 4 keys of their own, 88 % of the ops, ranges
    of up to 32 units over inserts of 8 to 16) leave maps of more than 64 keys, some of them on
    segments of two units or more; set 48 is the narrow annotate that follows."""
    props = PropTable()
    for i in range(48):
        props.intern({f"k{4 * i + j}": i for j in range(4)})
    narrow = props.intern({"k0": "x", "k7": "y", "z": 1})
    p = gen_params(seed=77, n_docs=n_docs, **GEN_WIDE)
    p.ins_len_min = 8
    batch, st, _ = generate(p, props)
    assert st == [0] * n_docs
    return p, batch, props, narrow


def host_op(batch, n_docs, k, pos1, pos2, prop, move_msn=False):
    """One host message per document following its generated run (k: how many came before): an
    annotate of [pos1[d], pos2[d]) with set `prop`, or with prop None a no-op message; move_msn:
    the MSN follows the sequence number, so zamboni passes over everything before it."""
    last = batch.op_offsets[1:].astype(np.int64) - 1
    seq = batch.arrays["seq"][last] + 1 + k
    one = np.ones(n_docs, np.int32)
    return OpBatch.from_arrays(np.arange(n_docs), np.arange(n_docs + 1), np.zeros(1, np.uint16),
                               type=(3 if prop is None else 2) * one, flags=one, client=0 * one, seq=seq, ref_seq=seq - 1,
                               msn=seq - 1 if move_msn else batch.arrays["msn"][last], pos1=np.asarray(pos1) * one,
                               pos2=np.asarray(pos2) * one, payload_off=0 * one, payload_len=0 * one,
                               prop_id=(-1 if prop is None else prop) * one)


ZAMBONI_MSGS = 48       # no-op messages that move the MSN after the split (check_device_built)


def segment_at(od, pos):
    """(start, length, number of keys) of the oracle's segment at `pos` in the local view."""
    info, js = od.containing_segment(pos)
    j = json.loads(js)
    return pos - int(info[1]), int(info[3]), len(j["props"]) if isinstance(j, dict) and "props" in j else 0


def wide_segment(od):
    """The first segment of at least 2 units whose map holds more than 64 keys."""
    p, n = 0, od.get_length()
    while p < n:
        start, ln, w = segment_at(od, p)
        if w > 64 and ln >= 2:
            return start, ln, w
        p = start + max(ln, 1)
    raise AssertionError("no segment of two units or more holds more than 64 keys")


def check_device_built(kind, path):
    """Documents made wide by batches the host never scanned (mt_generate applies as it generates;
    mt_upload_batch_dev / mt_generated_to_resident replay device arrays), then a narrow host
    batch: it must replay in the kernels that build wide maps."""
    n_docs = N_DOCS[kind]
    p, batch, props, narrow = wide_generated(n_docs)
    ora = bc.Oracle(n_docs, props)
    ora.apply(batch, list(range(n_docs)))
    wide = [max(widths(od.snapshot(int(m), int(s))[0]) or [0]) for od, m, s in zip(ora.docs, ora.msn, ora.seq)]
    assert min(wide) > 64, wide                       # every document is wide before the host batch
    eng = bc.FACTORIES[kind](n_docs, **{**bc.CAPS, "propsets_per_doc": 1 << 17})      # maps of a dozen chunks each
    eng.upload_props(props)
    eng.upload_names(bc.NAMES)
    eng.generate(p)
    eng.sync()
    if path == "to_resident":
        eng.open_docs(0, n_docs)
        eng.generated_to_resident()
        eng.replay_resident()
        eng.sync()
    elif path == "upload_dev":
        gb = eng.generated_download()
        for k in ("type", "seq", "pos1", "prop_id"):
            assert np.array_equal(gb.arrays[k], batch.arrays[k]), k
        n = gb.n_ops
        rec = torch.empty(32 * n, dtype=torch.uint8, device="cuda:0" if kind == "gpu" else "cpu")
        pay = torch.empty(n * p.ins_len_max + 1, dtype=torch.int16, device=rec.device)
        eng.generated_copy_dev(0, n_docs, rec.data_ptr(), pay.data_ptr())
        if kind == "gpu":
            torch.cuda.synchronize()
        eng.open_docs(0, n_docs)
        eng.upload_batch_dev(np.arange(n_docs), gb.op_offsets, rec.data_ptr(), pay.data_ptr(), n * p.ins_len_max)
        eng.replay_resident()
        eng.sync()
    assert_gen = bc.engine_state(eng, n_docs, ora.msn, ora.seq)
    bc.assert_same_state(assert_gen, ora.state(), f"generated ({path})")
    docs = list(range(n_docs))

    def host(nb, where):
        eng.apply(nb)
        eng.sync()
        ora.apply(nb, docs)
        bc.assert_same_state(bc.engine_state(eng, n_docs, ora.msn, ora.seq), ora.state(), f"{where} ({path})")
    # a narrow annotate of one whole wide segment per document; then of its first unit, with the
    # values it holds: two adjacent segments with equal maps of more than 64 keys (asserted from
    # the oracle); then the MSN moves over them and zamboni merges them back (propsMatch on wide maps)
    seg = [wide_segment(od) for od in ora.docs]
    host(host_op(batch, n_docs, 0, [a for a, _, _ in seg], [a + n for a, n, _ in seg], narrow), "narrow host batch")
    host(host_op(batch, n_docs, 1, [a for a, _, _ in seg], [a + 1 for a, _, _ in seg], narrow), "split in equal wide maps")
    for od, (a, n, _) in zip(ora.docs, seg):
        left, right = segment_at(od, a), segment_at(od, a + 1)
        assert left[:2] == (a, 1) and right[:2] == (a + 1, n - 1) and left[2] == right[2] > 64, (left, right)
    # (zamboni takes a bounded number of blocks off its heap per message: the split's turn comes
    # after the backlog the generated stream left)
    for k in range(2, 2 + ZAMBONI_MSGS):
        nb = host_op(batch, n_docs, k, 0, 0, None, move_msn=True)
        eng.apply(nb)
        ora.apply(nb, docs)
    host(host_op(batch, n_docs, 2 + ZAMBONI_MSGS, 0, 0, None, move_msn=True), "the MSN moved over the split")
    for od, (a, n, _) in zip(ora.docs, seg):
        start, ln, w = segment_at(od, a)
        assert start == a and ln >= n and w > 64, f"the oracle's zamboni did not merge the halves: {(start, ln, w)} of {(a, n)}"
    eng.close()


def test_wide_keys_survive_reopen_and_restore_on_emulation():
    check_reopen_restore("emu")


def test_wide_keys_survive_restore_on_emulation():
    check_restore_alone("emu")


@pytest.mark.parametrize("path", ["generate", "to_resident", "upload_dev"])
def test_wide_keys_of_device_built_batches_on_emulation(path):
    check_device_built("emu", path)


@gpu
def test_wide_keys_survive_reopen_and_restore_on_gpu():
    check_reopen_restore("gpu")


@gpu
def test_wide_keys_survive_restore_on_gpu():
    check_restore_alone("gpu")


@gpu
@pytest.mark.parametrize("path", ["generate", "to_resident", "upload_dev"])
def test_wide_keys_of_device_built_batches_on_gpu(path):
    check_device_built("gpu", path)
