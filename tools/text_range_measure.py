"""Times mt_get_text_range beside mt_get_text ("Text ranges").

Shape and method of the tile-search measurement: N copies of the 3,000-message marker document of
tests/test_tile_search.py (one packed run replicated over N slots and replayed once), the raw ABI
call with the stream synchronised before and after it, median (min-max) of 7 calls after 2
warm-up calls, one process.  Prints one JSON line:
  (a) mt_get_text_range of the whole documents, local view (with the bytes per second achieved:
      text units read plus written over the time)
  (b) mt_get_text of the same documents (the yardstick)
  (c) one query per "pg" paragraph from the tile index
  (d) (a) under a remote view that differs from the observer's
usage: python tools/text_range_measure.py [--docs 4096] [--emu] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAPS = dict(rows_per_doc=4096, window_per_doc=4096, propsets_per_doc=1024, text_per_doc=1 << 14, blocks_per_doc=2048,
            heap_per_doc=4096)


def timed(eng, call, reps=7, warm=2):
    ms = []
    for k in range(warm + reps):
        eng.sync()
        t0 = time.perf_counter()
        call()
        eng.sync()
        if k >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--emu", action="store_true", help="the host emulation (to try the tool, not to measure)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from fluidframework_amd.batch import BatchBuilder, ClientNames, OpBatch
    from fluidframework_amd.engine import Engine
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
    assert eng.get_text([0, N - 1]) == [whole, whole]
    pools = eng.pools([0])[0]
    fn, h = eng.fn, eng.h
    arena, off = ctypes.c_void_p(), ctypes.c_void_p()
    res = {"docs": N, "msgs_per_doc": len(msgs), "rows_per_doc": int(pools[0]), "height": int(pools[6]), "text_units_per_doc": len(whole)}

    def text_range(d, s, e, r, c, ph=""):
        p = np.frombuffer(ph.encode("utf-16-le"), np.uint16)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        rc = fn["get_text_range"](h, len(d), d.ctypes.data, ptr(s), ptr(e), ptr(r), ptr(c), p.ctypes.data if len(p) else None, len(p),
                                  ctypes.byref(arena), ctypes.byref(off))
        assert rc == 0, rc
        return int(ctypes.cast(off, ctypes.POINTER(ctypes.c_uint64))[len(d)])

    # (a) the whole documents, local view
    units = text_range(docs, None, None, None, None)
    assert units == N * len(whole) and eng.get_text_range([N - 1])[0] == whole
    res["a_text_range_whole_ms"] = a = timed(eng, lambda: text_range(docs, None, None, None, None))
    res["a_units"] = units
    res["a_gbytes_per_s"] = round(2 * 2 * units / (a["median"] * 1e-3) / 1e9, 2)
    # (b) mt_get_text, the yardstick
    res["b_get_text_ms"] = timed(eng, lambda: fn["get_text"](h, N, docs.ctypes.data, ctypes.byref(arena), ctypes.byref(off)))
    # (c) one query per "pg" paragraph
    recs, toff = eng.tile_index([0], "pg")
    cuts = [0] + [int(x) for x in recs["pos"]] + [-(1 << 31)]
    k = len(cuts) - 1
    qd = np.repeat(docs, k)
    qs = np.ascontiguousarray(np.tile(np.asarray(cuts[:-1], np.int32), N))
    qe = np.ascontiguousarray(np.tile(np.asarray(cuts[1:], np.int32), N))
    got = text_range(qd, qs, qe, None, None, " ")
    assert got == N * eng.get_length([0], [0x7FFFFFFF], [-1])[0], got
    res["c_queries"] = len(qd)
    res["c_paragraphs_ms"] = timed(eng, lambda: text_range(qd, qs, qe, None, None, " "))
    # (d) the whole documents under a remote view: the stream client whose view at its last
    # refSeq differs most from the observer's
    last = {}
    for m in msgs:
        last[m["clientId"]] = m["referenceSequenceNumber"]
    who = min(last, key=last.get)
    ref = np.full(N, last[who], np.int32)
    cli = np.full(N, names.ids[who], np.int32)
    remote = eng.get_text_range([0], None, None, [last[who]], [names.ids[who]])[0]
    assert len(eng.get_text_range([0], None, None, [last[who]], [names.ids[who]], " ")[0]) == od.get_length_of(last[who], who)
    res["d_view"] = {"ref_seq": int(last[who]), "current_seq": len(msgs), "differs_from_local": remote != whole, "units_per_doc": len(remote)}
    res["d_text_range_remote_ms"] = timed(eng, lambda: text_range(docs, None, None, ref, cli))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
