"""Times mt_walk_segments beside what the library offered for the same information before it
("Segment walks").

Shape and method of the text-range measurement: N copies of the 3,000-message marker document of
tests/test_tile_search.py (one packed run replicated over N slots and replayed once), the raw ABI
call with the stream synchronised before and after it, median (min-max) of 7 calls after 2
warm-up calls, one process.  Prints one JSON line:
  (a) mt_walk_segments of the whole documents with text and maps, local view
  (b) the same without MT_WALK_TEXT
  (c) one walk per "pg" paragraph (between consecutive mt_tile_index tiles)
  (d) (a) under a remote view that differs from the observer's
  (e) mt_get_containing_segment with JSON, one query per segment start of the same documents
      (the starts are (a)'s records): the only per-segment path there was
  (f) mt_get_text_range of (a)'s and of (c)'s ranges: a floor for the text part
  (g) mt_tile_index of the same documents, label "pg"; (h) mt_get_text of them, its yardstick;
      (i) mt_find_tile, one query per document, no JSON ("Tile search")
and the ratios e / a, a / f_whole, c / f_paragraphs.
usage: python tools/walk_measure.py [--docs 4096] [--emu] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text_range_measure import CAPS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--emu", action="store_true", help="the host emulation (to try the tool, not to measure)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from fluidframework_amd.batch import BatchBuilder, ClientNames, OpBatch
    from fluidframework_amd.engine import MT_WALK_TEXT, WALK_REC_DTYPE, Engine
    from test_tile_search import streams
    N = args.docs
    if args.emu:
        from emu_lib import emu_engine
        eng = emu_engine(N, **CAPS)
    else:
        eng = Engine(N, device=0, **CAPS)
    msgs, od = streams()[3]
    names = ClientNames()
    bb = BatchBuilder(eng.props, names)
    bb.begin_doc(0)
    for m in msgs:
        bb.add_message(m)
    one = bb.build()
    n = one.n_ops
    batch = OpBatch.from_arrays(np.arange(N), np.arange(N + 1) * n, one.payload, **{k: np.tile(v, N) for k, v in one.arrays.items()})
    eng.upload_props()
    eng.upload_names(names.json_literals())
    eng.open_docs(0, N)
    eng.apply(batch)
    eng.sync()
    docs = np.arange(N, dtype=np.uint32)
    assert (eng.status(docs) == 0).all()
    whole = od.get_text()
    pools = eng.pools([0])[0]
    fn, h = eng.fn, eng.h
    P = ctypes.c_void_p
    recs, off, arena, maps = P(), P(), P(), P()
    res = {"docs": N, "msgs_per_doc": len(msgs), "rows_per_doc": int(pools[0]), "height": int(pools[6]), "text_units_per_doc": len(whole)}
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def walk(d, s, e, r, c, text=True):
        rc = fn["walk_segments"](h, len(d), d.ctypes.data, ptr(s), ptr(e), ptr(r), ptr(c), MT_WALK_TEXT if text else 0, ctypes.byref(recs),
                                 ctypes.byref(off), ctypes.byref(arena) if text else None, ctypes.byref(maps))
        assert rc == 0, rc
        return int(ctypes.cast(off, ctypes.POINTER(ctypes.c_uint64))[len(d)])

    def text_range(d, s, e):
        rc = fn["get_text_range"](h, len(d), d.ctypes.data, ptr(s), ptr(e), None, None, None, 0, ctypes.byref(arena), ctypes.byref(off))
        assert rc == 0, rc

    # (a) the whole documents with text and maps, local view
    w0 = eng.walk_segments([0, N - 1])
    per_doc = int(w0.off[1])
    assert int(w0.off[2]) == 2 * per_doc and "".join(t for t in w0[1][1] if t is not None) == whole
    total = walk(docs, None, None, None, None)
    assert total == N * per_doc
    res["records_per_doc"], res["records"], res["distinct_maps_per_doc"] = per_doc, total, len(w0.maps) // 2
    res["a_walk_whole_ms"] = a = timed(eng, lambda: walk(docs, None, None, None, None))
    res["a_million_records_per_s"] = round(total / (a["median"] * 1e-3) / 1e6, 2)
    # the segment starts of every document, for (e)
    walk(docs, None, None, None, None)
    starts = np.frombuffer(ctypes.string_at(recs, total * WALK_REC_DTYPE.itemsize), WALK_REC_DTYPE)["pos"].astype(np.int32)
    # (b) without text
    res["b_walk_no_text_ms"] = timed(eng, lambda: walk(docs, None, None, None, None, False))
    # (c) one walk per "pg" paragraph
    trecs, _ = eng.tile_index([0], "pg")
    cuts = [0] + [int(x) for x in trecs["pos"]] + [-(1 << 31)]
    k = len(cuts) - 1
    qd = np.repeat(docs, k)
    qs = np.ascontiguousarray(np.tile(np.asarray(cuts[:-1], np.int32), N))
    qe = np.ascontiguousarray(np.tile(np.asarray(cuts[1:], np.int32), N))
    got = walk(qd, qs, qe, None, None)
    assert got == total, (got, total)           # the paragraphs' cuts fall on segment boundaries
    res["c_queries"] = len(qd)
    res["c_paragraphs_ms"] = c = timed(eng, lambda: walk(qd, qs, qe, None, None))
    # (d) the whole documents under a remote view: the stream client whose view at its last
    # refSeq differs most from the observer's
    last = {}
    for m in msgs:
        last[m["clientId"]] = m["referenceSequenceNumber"]
    who = min(last, key=last.get)
    ref = np.full(N, last[who], np.int32)
    cli = np.full(N, names.ids[who], np.int32)
    wr = eng.walk_segments([0], None, None, [last[who]], [names.ids[who]])
    assert int(wr.recs["len"].sum()) == od.get_length_of(last[who], who)
    res["d_view"] = {"ref_seq": int(last[who]), "current_seq": len(msgs), "records_per_doc": len(wr.recs),
                     "removed_rows_visited": int((wr.recs["removed_seq"] != -(1 << 31)).sum())}
    res["d_walk_remote_ms"] = timed(eng, lambda: walk(docs, None, None, ref, cli))
    # (e) the per-segment path there was: one mt_get_containing_segment query, with JSON, per segment start
    sd = np.repeat(docs, per_doc)
    minus = np.full(total, -1, np.int32)
    info = np.zeros(total * 16, np.int32)
    ja, jo = P(), P()

    def containing():
        rc = fn["get_containing_segment"](h, total, sd.ctypes.data, starts.ctypes.data, minus.ctypes.data, minus.ctypes.data,
                                          info.ctypes.data, ctypes.byref(ja), ctypes.byref(jo))
        assert rc == 0, rc
    containing()
    assert (info.reshape(-1, 16)[:, 0] == 1).all() and (info.reshape(-1, 16)[:, 1] == 0).all()
    print(json.dumps({"progress": "containing_segment works", **res}), flush=True)
    res["e_containing_segment_per_start_ms"] = e = timed(eng, containing)
    # (f) mt_get_text_range of the same ranges
    res["f_text_range_whole_ms"] = fw = timed(eng, lambda: text_range(docs, None, None))
    res["f_text_range_paragraphs_ms"] = fp = timed(eng, lambda: text_range(qd, qs, qe))
    # (g)-(i) the tile search's figures on the same documents
    lab = np.zeros(N, np.uint32)
    labels = eng._tile_labels("pg")
    tr, to = P(), P()

    def tile_index():
        rc = fn["tile_index"](h, N, docs.ctypes.data, lab.ctypes.data, ctypes.byref(labels), ctypes.byref(tr), ctypes.byref(to))
        assert rc == 0, rc
        return int(ctypes.cast(to, ctypes.POINTER(ctypes.c_uint64))[N])
    assert tile_index() == N * len(trecs)
    res["g_tile_index_ms"] = timed(eng, tile_index)
    res["g_records"] = N * len(trecs)
    res["h_get_text_ms"] = timed(eng, lambda: fn["get_text"](h, N, docs.ctypes.data, ctypes.byref(arena), ctypes.byref(off)))
    tpos, tfl, tinfo = np.full(N, len(whole) // 2, np.int32), np.ones(N, np.uint8), np.zeros(N * 16, np.int32)

    def find_tile():
        rc = fn["find_tile"](h, N, docs.ctypes.data, tpos.ctypes.data, tfl.ctypes.data, lab.ctypes.data, ctypes.byref(labels),
                             tinfo.ctypes.data, None, None)
        assert rc == 0, rc
    find_tile()
    assert (tinfo.reshape(-1, 16)[:, 0] == 1).all()
    res["i_find_tile_ms"] = timed(eng, find_tile)
    res["ratio_e_over_a"] = round(e["median"] / a["median"], 2)
    res["ratio_a_over_f_whole"] = round(a["median"] / fw["median"], 2)
    res["ratio_c_over_f_paragraphs"] = round(c["median"] / fp["median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
