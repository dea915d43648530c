"""Documents that outgrow their pools (mt_docs_resize, mt_set_autogrow) on the host emulation:
a document relocated into larger slices, by hand or by the grow-and-resume loop, stays bit-exact
with the oracle.  tests/test_gpu_growth.py repeats the checks on the device.

Every engine here starts from TINY capacities, which the streams cross several times in every
pool; the unarmed runs show that they really do (an MT_DS_OOM_* bit per document).
"""
import functools

import numpy as np
import pytest

from emu_lib import emu_engine
from fluidframework_amd.engine import CAP_FIELDS, ClientGroup, MergeTreeError
from msg_gen import stream
from oracle_lib import OracleDoc, gen_params, generate, replay
from test_emu_parity import ADVERSARIAL, CONFIGS, NAMES, ann_props, compare, split_batch

TINY = dict(rows_per_doc=64, blocks_per_doc=16, heap_per_doc=64, window_per_doc=64, text_per_doc=256, propsets_per_doc=16)
OOM_BITS = 0x10 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200       # MT_DS_OOM_ROWS ... MT_DS_OOM_WINDOW
MT_E_INVALID, MT_E_OOM = 1, 3
RESIDENCIES = [(0, 0, 0, 0), (1, 40, 40, 12), (2, 0, 40, 12), (3, 16, 0, 12)]


def tiny(factory, armed=True, budget=0, **more):
    """An engine factory for compare() and the message-surface checks: whatever capacities the
    caller passes, the engine gets the TINY ones (and `more`), with autogrow armed."""
    def make(n, **_):
        eng = factory(n, **{**TINY, **more})
        if armed:
            eng.set_autogrow(True, budget)
        return eng
    return make


@functools.lru_cache(maxsize=None)
def generated(cfg, n_docs, seed, ops=None):
    """One generated stream per (configuration, documents, seed), shared by the tests (read only)."""
    props = ann_props()
    c = dict(ADVERSARIAL if cfg == "adversarial" else CONFIGS[cfg])
    if ops:
        c["ops"] = ops
    batch, st, _ = generate(gen_params(seed=seed, n_docs=n_docs, **c), props)
    assert st == [0] * n_docs
    return batch, props


def replay_on(eng, batch, props, n_docs, check=True):
    eng.upload_props(props)
    eng.upload_names(NAMES)
    eng.open_docs(0, n_docs)
    eng.apply(batch)
    eng.sync()
    return eng.status(range(n_docs))


# ---- 1. autogrow parity -------------------------------------------------------------------
def check_autogrow_parity(factory, n_docs=6):
    batch, props = generated("grow", n_docs, 11)
    st = replay_on(tiny(factory, armed=False)(n_docs), batch, props, n_docs)
    assert all(int(s) & OOM_BITS for s in st), f"the stream does not overflow the tiny pools: {st}"
    eng = compare(batch, props, n_docs, factory=tiny(factory))
    gs = eng.grow_stats()
    assert gs["relocations"] >= n_docs and gs["pool_reallocations"] >= 1 and gs["launches"] > 1, gs
    # every document was relocated: each one's rows, blocks, text and property sets outgrew TINY
    caps = eng.doc_caps(range(n_docs))
    for d, c in enumerate(caps):
        for k in ("rows_per_doc", "blocks_per_doc", "text_per_doc", "propsets_per_doc"):
            assert c[k] > TINY[k], (d, k, c)
    return gs


def test_autogrow_matches_oracle():
    check_autogrow_parity(emu_engine)


# ---- 2. the same under each residency -----------------------------------------------------
def check_autogrow_residency(factory, res, cont, n_docs=3):
    batch, props = generated("grow", n_docs, 21)
    eng = compare(batch, props, n_docs, factory=tiny(factory), residency=res, cont=cont)
    assert eng.grow_stats()["relocations"] >= n_docs


@pytest.mark.parametrize("cont", [0, 1 << 30])
@pytest.mark.parametrize("res", RESIDENCIES)
def test_autogrow_under_residency_matches_oracle(res, cont):
    check_autogrow_residency(emu_engine, res, cont)


# ---- 3. adversarial ranges ----------------------------------------------------------------
def check_autogrow_adversarial(factory, n_docs=3):
    batch, props = generated("adversarial", n_docs, 41, ops=2000)
    eng = compare(batch, props, n_docs, factory=tiny(factory))
    assert eng.grow_stats()["relocations"] >= n_docs


def test_autogrow_adversarial_matches_oracle():
    check_autogrow_adversarial(emu_engine)


# ---- 4. explicit resize mid-stream --------------------------------------------------------
AMPLE = dict(rows_per_doc=20000, window_per_doc=8192, propsets_per_doc=8192, text_per_doc=1 << 18)


def observe(eng, n, msn, seq):
    """Everything the hosts can see of the documents: text, dump, both snapshot formats."""
    return (eng.get_text(range(n)), [eng.dump(d).tobytes() for d in range(n)], eng.snapshot(range(n), msn, seq),
            eng.snapshot(range(n), msn, seq, legacy=True), [int(x) for x in eng.snapshot_digests(range(n), msn, seq)])


def check_explicit_resize(factory, armed, n=4):
    batch, props = generated("cfg3", n, 17)
    first, second = split_batch(batch, 2)
    eng = factory(n, **AMPLE)
    assert (replay_on(eng, first, props, n) == 0).all()
    last = first.op_offsets[1:] - 1
    msn, seq = first.arrays["msn"][last], first.arrays["seq"][last]
    before = observe(eng, n, msn, seq)
    occ, caps0 = eng.doc_occupancy(range(n)), eng.doc_caps(range(n))
    assert all(o["text_per_doc"] > 0 and o["propsets_per_doc"] > 0 and o["rows_per_doc"] > 0 for o in occ), occ

    # a capacity one below what a document holds: MT_E_INVALID names it, and nothing moves
    for k in ("rows_per_doc", "blocks_per_doc", "text_per_doc", "propsets_per_doc", "heap_per_doc", "window_per_doc"):
        if occ[1][k] == 0:
            continue
        with pytest.raises(MergeTreeError) as ei:
            eng.resize_docs([0, 1], **{k: [0, occ[1][k] - 1]})
        assert ei.value.rc == MT_E_INVALID and "document 1" in str(ei.value), str(ei.value)
    assert eng.doc_caps(range(n)) == caps0 and eng.grow_stats()["relocations"] == 0
    assert observe(eng, n, msn, seq) == before

    # document 0 enlarged, 1 shrunk to exactly what it holds, 2 moved as it is, 3's property sets
    # shrunk to the live maps
    want = [dict(caps0[d]) for d in range(n)]
    want[0] = {k: 2 * v for k, v in caps0[0].items()}
    want[1] = {k: max(occ[1][k], 1) for k in CAP_FIELDS}
    want[3]["propsets_per_doc"] = occ[3]["propsets_per_doc"]
    req = {k: [0 if d == 2 else want[d][k] for d in range(n)] for k in CAP_FIELDS}
    eng.resize_docs(range(n), **req)
    assert eng.doc_caps(range(n)) == want
    assert observe(eng, n, msn, seq) == before, "the resize itself changed a document"
    pools = eng.pools(range(n))
    for d in (0, 1, 3):     # a moved property arena holds the live maps alone, a moved text arena the live text
        assert int(pools[d][5]) == occ[d]["propsets_per_doc"], (d, pools[d], occ[d])
        assert d == 3 or int(pools[d][4]) == occ[d]["text_per_doc"], (d, pools[d], occ[d])
    assert eng.doc_occupancy(range(n)) == occ
    gs = eng.grow_stats()
    assert gs["relocations"] == n and gs["dead_bytes"] > 0 and gs["bytes_moved"] > 0, gs

    # the second half
    if armed:
        eng.set_autogrow(True)
    eng.apply(second)
    eng.sync()
    st = eng.status(range(n))
    if not armed:
        assert int(st[1]) & OOM_BITS and not (int(st[0]) | int(st[2])), st     # the exact fit overflows, as it always did
        return
    assert (st == 0).all(), st
    assert eng.grow_stats()["relocations"] > n
    grown = eng.doc_caps([1])[0]
    assert any(grown[k] > want[1][k] for k in CAP_FIELDS), grown
    oracle_docs = replay(batch, props, NAMES)
    last = batch.op_offsets[1:] - 1
    msn, seq = batch.arrays["msn"][last], batch.arrays["seq"][last]
    texts, snaps, legacy = eng.get_text(range(n)), eng.snapshot(range(n), msn, seq), eng.snapshot(range(n), msn, seq, legacy=True)
    for d in range(n):
        od = oracle_docs[d][0]
        assert texts[d] == od.get_text(), d
        assert np.array_equal(eng.dump(d), od.dump()), d
        assert tuple(snaps[d]) == tuple(od.snapshot(int(msn[d]), int(seq[d]))), d
        assert tuple(legacy[d]) == tuple(od.snapshot(int(msn[d]), int(seq[d]), legacy=True)), d


@pytest.mark.parametrize("armed", [True, False])
def test_explicit_resize_mid_stream(armed):
    check_explicit_resize(emu_engine, armed)


# ---- 5. capture with growth ---------------------------------------------------------------
def check_capture_with_growth(factory):
    """Records captured while documents are relocated in the same batch equal the oracle's
    callbacks, the property maps of ANNOTATE records captured before a relocation included."""
    from test_message_surface import check_delta_records
    made = []

    def make(n, **_):
        made.append(tiny(factory)(n))
        return made[-1]
    kinds = check_delta_records(make, "markers_props", n_msgs=500, min_launches=3)
    assert {0, 1, 2} <= kinds
    assert made[0].grow_stats()["relocations"] >= 3


def test_capture_with_growth_matches_oracle():
    check_capture_with_growth(emu_engine)


# ---- 6. registers with growth -------------------------------------------------------------
def check_registers_with_growth(factory, n_docs=2, n_msgs=700):
    """Clone rows keep their text and maps across relocations; the register arena and the
    marker table, which autogrow does not grow, are pre-sized by resize_docs."""
    from test_message_surface import check
    made = []

    def make(n, **_):
        eng = tiny(factory)(n)
        eng.resize_docs(range(n), register_rows_per_doc=8192, markers_per_doc=4096)
        made.append(eng)
        return eng
    check(make, "registers_wide", n_docs=n_docs, n_msgs=n_msgs)
    eng = made[0]
    assert eng.grow_stats()["relocations"] > 2 * n_docs
    assert all(c["register_rows_per_doc"] == 8192 and c["markers_per_doc"] == 4096 for c in eng.doc_caps(range(n_docs)))


def test_registers_with_growth_match_oracle():
    check_registers_with_growth(emu_engine)


# ---- 7. checkpoint ------------------------------------------------------------------------
def check_checkpoint(factory, n=3):
    batch, props = generated("grow", n, 23)
    first, second = split_batch(batch, 2)
    eng = tiny(factory)(n)
    assert (replay_on(eng, first, props, n) == 0).all()
    last = first.op_offsets[1:] - 1
    msn, seq = first.arrays["msn"][last], first.arrays["seq"][last]
    eng.checkpoint()
    at_ck = observe(eng, n, msn, seq)
    caps_ck, bytes_ck = eng.doc_caps(range(n)), eng.pool_bytes()
    oracle_docs = replay(batch, props, NAMES)
    lastf = batch.op_offsets[1:] - 1
    for again in range(2):
        eng.apply(second)
        eng.sync()
        assert (eng.status(range(n)) == 0).all()
        assert eng.doc_caps(range(n)) != caps_ck and eng.pool_bytes() >= bytes_ck
        texts = eng.get_text(range(n))
        digs = eng.snapshot_digests(range(n), batch.arrays["msn"][lastf], batch.arrays["seq"][lastf])
        for d in range(n):
            od = oracle_docs[d][0]
            assert texts[d] == od.get_text(), (again, d)
            assert int(digs[d]) == od.snapshot(int(batch.arrays["msn"][lastf[d]]), int(batch.arrays["seq"][lastf[d]]))[1]
        eng.restore()
        assert eng.doc_caps(range(n)) == caps_ck
        assert observe(eng, n, msn, seq) == at_ck, "restore after a relocation"


def test_checkpoint_restore_across_growth():
    check_checkpoint(emu_engine)


# ---- 8. budget ----------------------------------------------------------------------------
def check_budget(factory, n=3):
    batch, props = generated("grow", n, 29)
    eng = tiny(factory, armed=False)(n)
    eng.set_autogrow(True, eng.pool_bytes() + 4096)
    eng.upload_props(props)
    eng.upload_names(NAMES)
    eng.open_docs(0, n)
    with pytest.raises(MergeTreeError) as ei:
        eng.apply(batch)
    assert ei.value.rc == MT_E_OOM, str(ei.value)
    assert (eng.status(range(n)) == 0).all()
    at = eng.last_resume(n)
    texts = eng.get_text(range(n))
    for d in range(n):
        a, b = int(batch.op_offsets[d]), int(batch.op_offsets[d + 1])
        assert a <= int(at[d]) < b, (d, at)
        od = OracleDoc(True, props, NAMES)
        idx = np.arange(a, int(at[d]))
        part = type(batch).from_arrays([0], [0, len(idx)], batch.payload, **{k: batch.arrays[k][idx] for k in batch.arrays})
        assert od.apply_run(part, 0) == 0
        assert texts[d] == od.get_text(), f"doc {d} after {int(at[d]) - a} messages"


def test_budget_stops_growth_consistently():
    check_budget(emu_engine)


# ---- 9. hosts -----------------------------------------------------------------------------
def check_client_group(factory, n_docs=2, n_msgs=300):
    """ClientGroup(autogrow=True), one message per flush, on a tiny engine."""
    streams = [stream(700 + d, n_msgs, clients=4, lag=12, p_annotate=0.3) for d in range(n_docs)]
    eng = factory(n_docs, **TINY)
    g = ClientGroup(eng, autogrow=True)
    clients = [g.new_client({"newMergeTreeSnapshotFormat": True}) for _ in range(n_docs)]
    for c in clients:
        c.startOrUpdateCollaboration("observer")
    v0 = g.version
    for i in range(n_msgs):
        for c, (msgs, _) in zip(clients, streams):
            c.applyMsg(msgs[i])
        g.flush()
    assert g.version > v0
    assert eng.grow_stats()["relocations"] >= n_docs
    for c, (msgs, obs) in zip(clients, streams):
        assert c.getText() == obs.get_text()
        msn, seq = msgs[-1]["minimumSequenceNumber"], msgs[-1]["sequenceNumber"]
        (blobs, dig), = eng.snapshot([c.doc_id], [msn], [seq])
        assert (blobs, dig) == tuple(obs.snapshot(msn, seq))
    # without autogrow the same flushes fail the documents, as they always did
    g2 = ClientGroup(factory(n_docs, **TINY))
    c2 = g2.new_client({"newMergeTreeSnapshotFormat": True})
    c2.startOrUpdateCollaboration("observer")
    for m in streams[0][0]:
        c2.applyMsg(m)
    g2.flush()
    assert int(g2.engine.status([0])[0]) & OOM_BITS


def test_client_group_autogrow():
    check_client_group(emu_engine)


def check_node(addon, n_docs=2, n_msgs=300):
    from js_lib import run_driver
    streams = [stream(700 + d, n_msgs, clients=4, lag=12, p_annotate=0.3) for d in range(n_docs)]
    limits = dict(rowsPerDoc=64, blocksPerDoc=16, heapPerDoc=64, windowPerDoc=64, textPerDoc=256, propsetsPerDoc=16)
    got = run_driver("growth_check.js", {"docs": [m for m, _ in streams], "limits": limits}, addon=addon)
    assert got["relocations"] >= n_docs and got["unarmedStatus"] & OOM_BITS
    assert got["capsAfterResize"]["rowsPerDoc"] == 4096 and got["occupancy"]["rowsPerDoc"] > 64
    assert got["textAfterResize"] == got["texts"][0]
    for d, (msgs, obs) in enumerate(streams):
        assert got["texts"][d] == obs.get_text(), d
        blobs, dig = obs.snapshot(msgs[-1]["minimumSequenceNumber"], msgs[-1]["sequenceNumber"])
        assert int(got["digests"][d], 16) == dig, d


def test_node_host_autogrow_on_emulation():
    from js_lib import NODE
    from emu_lib import build_emu_napi
    addon = build_emu_napi() if NODE else None
    if addon is None:
        pytest.skip("node or its headers are not installed")
    check_node(addon)


# ---- 10. a copy's clones count as text ----------------------------------------------------
def _copy_msgs(n_seg=10, seg_len=12):
    """n_seg segments, each inserted in front of the last (so their text is not contiguous in the
    arena and a merge has to allocate; the MSN stays 0, nothing merges yet), then one message that copies the whole document into a register and moves the MSN to the
    current sequence number: its end-of-message zamboni merges the segments while the clones,
    which a text compaction copies separately, have just doubled the live text."""
    def msg(seq, msn, contents, cid="a"):
        return dict(clientId=cid, sequenceNumber=seq, referenceSequenceNumber=seq - 1, minimumSequenceNumber=msn, type="op",
                    contents=contents)
    m = [msg(i + 1, 0, {"type": 0, "pos1": 0, "seg": chr(ord("a") + i) * seg_len}, "ab"[i % 2]) for i in range(n_seg)]
    m.append(msg(n_seg + 1, n_seg, {"type": 0, "pos1": 0, "pos2": n_seg * seg_len, "register": "clip"}))
    m.append(msg(n_seg + 2, n_seg + 1, {"type": 0, "pos1": 0, "seg": "z"}))
    return m


def check_copy_text_headroom(factory):
    msgs = _copy_msgs()
    o = OracleDoc(True)
    for m in msgs:
        assert o.apply_msg(m) == 0
    for armed in (False, True):
        g = ClientGroup(factory(1, **TINY), autogrow=armed)          # 256 text units: 2 * 120 fit before the copy
        c = g.new_client({"newMergeTreeSnapshotFormat": True})
        for m in msgs:
            c.applyMsg(m)
        g.flush()
        st = int(g.engine.status([0])[0])
        if not armed:
            assert st & 0x40, st                                     # MT_DS_OOM_TEXT: the stream does overflow
            continue
        assert st == 0, st
        assert g.engine.get_text([0])[0] == o.get_text()
        assert g.engine.doc_caps([0])[0]["text_per_doc"] > TINY["text_per_doc"]


def test_copy_text_headroom():
    check_copy_text_headroom(emu_engine)


# ---- 11. the addon's growth calls ---------------------------------------------------------
def test_product_addon_has_growth_calls():
    """The growth calls are properties of the product addon (not enumerated: Object.keys(addon)
    stays the surface the hosts were written against)."""
    import json
    import subprocess
    import __graft_entry__
    from js_lib import NODE
    if NODE is None:
        pytest.skip("node is not installed")
    __graft_entry__.build_engine()
    path = __graft_entry__.build_napi()
    if path is None:
        pytest.skip("node headers are not installed")
    names = ["setAutogrow", "resizeDocs", "docCaps", "docOccupancy", "growStats"]
    out = subprocess.run([NODE, "-e", f"const a = require({json.dumps(path)}); "
                          f"console.log(JSON.stringify({json.dumps(names)}.map((n) => typeof a[n])))"],
                         check=True, capture_output=True, text=True).stdout
    assert json.loads(out) == ["function"] * len(names)
