"""The query kinds in mixed order on one context: a call's arguments travel in the
call's own record (MtQueryCall, mt_query.h), so no call can see what an earlier one, failed or
not, left behind.

* Three documents on one context, one per case of the scan: tree height 0 (the root's rows alone),
  height 1 (one unit) and height 2 (several units); each holds Tile markers of two labels and one
  property map of 70 keys (five chunks), and one row the observer has removed that a remote view
  still sees.
* The calls, in order: tile_index, get_text_range with a placeholder, walk_segments with maps,
  find_tile, get_containing_segment, get_text_range without a placeholder.  Between them three
  failing calls, each followed by a valid call of another kind; then a few more messages are
  replayed and the same calls run again.
* Expected: every answer equals the answer of that call alone on a fresh context brought to the
  same state; a failing call gives MT_E_INVALID and its message; the documents' dumps do not move.
"""
import ctypes

import numpy as np
import pytest

from emu_lib import emu_engine
from fluidframework_amd.engine import SEG_INFO_DTYPE, ClientGroup, Engine, MergeTreeError
from test_reference_known_answers import LIMITS, ins, msg, rem
from test_tile_search import tile

GPU = lambda n, **kw: Engine(n, device=0, **kw)  # noqa: E731
WIDE = {f"k{i:03d}": i for i in range(70)}
ROWS = (5, 30, 90)          # rows per document before the remove: height 0, 1, 2
HEIGHTS = (0, 1, 2)
IDS = [2, 0, 1, 2]          # the documents of every call: not sorted, one of them twice


def seg_of(k):
    """Row k of a document: text, with a Tile marker of label "pg" or "cell" at every fifth row
    and the 70-key map on row 3 (a marker) and row 4 (text)."""
    if k == 3:
        return tile(("pg",), **WIDE)
    if k == 4:
        return {"text": "wx", "props": WIDE}
    if k % 5 == 1:
        return tile(("pg",) if k % 10 == 1 else ("cell", "pg"))
    return chr(0x41 + k % 26) * (1 + k % 3)


def seg_len(s):
    return len(s) if isinstance(s, str) else len(s["text"]) if "text" in s else 1


def first_messages(n):
    """n rows appended one message each by A at msn 0 (nothing merges), then B removes [1, 3)."""
    out, at = [], 0
    for k in range(n):
        out.append(msg("A", k + 1, k, 0, ins(at, seg_of(k))))
        at += seg_len(seg_of(k))
    return out + [msg("B", n + 1, n, 0, rem(1, 3))]


def more_messages(n):
    """A few more: a tile and a text at the front, a remove further in."""
    return [msg("B", n + 2, n + 1, 0, ins(0, tile(("cell",), a=1))), msg("A", n + 3, n + 2, 0, ins(1, "new")),
            msg("B", n + 4, n + 3, 0, rem(5, 7))]


def context(factory, more):
    """One context holding the three documents, after the first messages and, with `more`, the
    later ones in a second batch."""
    g = ClientGroup(factory(len(ROWS), **LIMITS))
    cs = [g.new_client() for _ in ROWS]
    for c, n in zip(cs, ROWS):
        for m in first_messages(n):
            c.applyMsg(m)
    g.flush()
    if more:
        later(g, cs)
    return g, cs


def later(g, cs):
    for c, n in zip(cs, ROWS):
        for m in more_messages(n):
            c.applyMsg(m)
    g.flush()


def fields(a):
    return [a[f].tolist() for f in a.dtype.names if not f.startswith("pad")]


def views(cs):
    """Per query of IDS: the local view, A's view before B's remove (it still sees the removed
    rows), the local view, B's view at message 40 (A's later rows are not in it)."""
    ref = [-1, ROWS[0], -1, 40]
    who = [-1, cs[0].names.ids["A"], -1, cs[2].names.ids["B"]]
    return ref, who


def call_tile_index(eng, cs):
    recs, off = eng.tile_index(IDS, "pg")
    return fields(recs), off.tolist()


def call_text_placeholder(eng, cs):
    ref, who = views(cs)
    return eng.get_text_range(IDS, [0, 0, 2, None], [None, None, 40, 60], ref, who, "<marker>")


def call_walk(eng, cs):
    ref, who = views(cs)
    w = eng.walk_segments(IDS, [None, 0, 3, 60], [None, None, 50, 75], ref, who)
    assert WIDE in w.maps
    return fields(w.recs), w.off.tolist(), w.units.tobytes(), w.maps, w.maps_json


def call_find_tile(eng, cs):
    info, texts = eng.find_tile(IDS, [None, 2, 20, 70], "cell", [True, False, True, False])
    return fields(info), texts


def call_containing(eng, cs):
    ref, who = views(cs)
    info, texts = eng.containing_segment(IDS, [70, 1, 9, 0], ref, who)
    return fields(info), texts


def call_text_plain(eng, cs):
    ref, who = views(cs)
    return eng.get_text_range(IDS, [None, 1, 30, 5], [None, 6, 12, None], ref, who, "")


CALLS = [call_tile_index, call_text_placeholder, call_walk, call_find_tile, call_containing, call_text_plain]


def fail_walk(eng):
    eng.walk_segments([0], [(1 << 30) + 1], [5])


def fail_placeholder(eng):
    eng.get_text_range([1], None, None, None, None, "x" * 17)


def fail_label(eng):
    """mt_find_tile through the raw call: label 1 of a table of one label."""
    d, p, fl, lab = np.zeros(1, np.uint32), np.zeros(1, np.int32), np.ones(1, np.uint8), np.ones(1, np.uint32)
    out = np.zeros(1, SEG_INFO_DTYPE)
    t = eng._tile_labels("pg")
    eng._check(eng.fn["find_tile"](eng.h, 1, d.ctypes.data, p.ctypes.data, fl.ctypes.data, lab.ctypes.data, ctypes.byref(t),
                                   out.ctypes.data, None, None), "mt_find_tile")


# after the call of this index: the failing call and its message; the next call is of another kind
FAILS = {0: (fail_walk, "walk: start / end outside [-2^30, 2^30]"),
         1: (fail_placeholder, "text range: the placeholder is longer than MT_TEXT_PLACEHOLDER_MAX units"),
         3: (fail_label, "tile label out of range")}


def mixed(eng, cs):
    """The calls in order on one context with the failing calls between them: the answers."""
    ids = list(range(len(ROWS)))
    before = [eng.dump(d).tobytes() for d in ids]
    got = []
    for k, call in enumerate(CALLS):
        got.append(call(eng, cs))
        if k in FAILS:
            bad, text = FAILS[k]
            with pytest.raises(MergeTreeError) as ei:
                bad(eng)
            assert ei.value.rc == 1 and str(ei.value).endswith(f"failed (1): {text}"), str(ei.value)
    assert [eng.dump(d).tobytes() for d in ids] == before and (eng.status(ids) == 0).all()
    return got


def check_mixed(factory):
    g, cs = context(factory, False)
    eng = g.engine
    assert [int(h) for h in eng.pools(range(len(ROWS)))[:, 6]] == list(HEIGHTS)
    for more in (False, True):
        if more:
            later(g, cs)
        got = mixed(eng, cs)
        for k, call in enumerate(CALLS):
            fg, fcs = context(factory, more)
            assert call(fg.engine, fcs) == got[k], (more, call.__name__)
    # the answers are not empty ones: every document has tiles, text and visited rows
    idx, text, walk, found = got[0], got[1], got[2], got[3]
    assert all(b > a for a, b in zip(idx[1], idx[1][1:])) and all("<marker>" in t for t in text) and got[5][0] and got[5][3]
    assert all(b > a for a, b in zip(walk[1], walk[1][1:])) and any(found[0][0])


def test_mixed_query_calls_on_emulation():
    check_mixed(emu_engine)


@pytest.mark.gpu
def test_mixed_query_calls_on_gpu():
    check_mixed(GPU)
