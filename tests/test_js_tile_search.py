"""Tile search through the Node host (fluidframework_amd/js MergeTreeClient.findTile over the
addon's findTile / tileIndex): the seven client.spec.ts:28-233 cases, the removed trailing tile
(MT/mergeTree.ts:1841-1855, :993-1007), an undefined startPos and the refusal on a document whose
referenceTileLabels were annotated.  CPU: the addon built against the host emulation; GPU: the
product addon."""
import os

import pytest

from emu_lib import build_emu_napi
from js_lib import NODE, ROOT, run_driver
from test_reference_known_answers import ann, ins, msg, rem
from test_tile_search import TL, tile

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def msgs_of(ops):
    out = []
    for i, o in enumerate(ops):
        body = rem(o[1], o[2]) if o[0] == "rem" else ann(o[1], o[2], o[3]) if o[0] == "ann" else ins(o[0], o[1])
        out.append(msg("remote", i + 1, i, 0, body))
    return out


# (ops, [(startPos, label, preceding | None for the default) -> expected pos or None])
CASES = [
    ([(0, tile()), (0, "abc")], [((0, "EOP", False), 3)]),                                   # :29-51
    ([(0, "abc d"), (0, tile())], [((0, "EOP", False), 0)]),                                 # :53-73
    ([(0, tile()), (0, "abc d"), (0, tile()), (7, "ef"), (8, tile())],
     [((5, "EOP", None), 0), ((5, "EOP", False), 6)]),                                       # :75-151
    ([(0, tile())], [((0, "EOP", None), 0), ((0, "EOP", False), 0)]),                        # :153-178
    ([(0, tile()), (0, "abc")], [((5, "EOP", None), 3), ((5, "EOP", False), None)]),         # :180-204
    ([(0, "abc")], [((1, "EOP", None), None), ((1, "EOP", False), None)]),                   # :206-220
    ([], [((1, "EOP", None), None), ((1, "EOP", False), None)]),                             # :222-232
    # the removed trailing tile: (2, false) is the removed tile at 2 == L, (2) and (1, false) nothing
    ([(0, "ab"), (2, tile()), ("rem", 2, 3)],
     [((2, "EOP", False), 2), ((2, "EOP", True), None), ((1, "EOP", False), None)]),
    # an undefined startPos: the last / the first visible tile
    ([(0, tile()), (1, "abc"), (4, tile()), (5, "d"), (6, tile())],
     [((None, "EOP", None), 6), ((None, "EOP", False), 0), ((None, "pg", False), None)]),
]
LENGTHS = [4, 6, 10, 1, 4, 3, 0, 2, 7]
INDEX = [[[3, 3]], [[0, 0]], [[0, 0], [6, 5], [8, 6]], [[0, 0]], [[3, 3]], [], [], [], [[0, 0], [4, 3], [6, 4]]]


def check(addon):
    cases = [{"msgs": msgs_of(ops), "calls": [list(q) for q, _ in calls]} for ops, calls in CASES]
    marked = [(0, tile()), (1, "xy"), ("ann", 0, 1, {TL: ["pg"]})]
    cases.append({"msgs": msgs_of(marked), "calls": [[0, "EOP", True]]})
    got = run_driver("tile_check.js", {"cases": cases, "limits": dict(rowsPerDoc=256, textPerDoc=4096)}, addon=addon)
    for k, (ops, calls) in enumerate(CASES):
        assert got[k]["length"] == LENGTHS[k] and got[k]["index"] == INDEX[k], (k, got[k])
        for (q, want), r in zip(calls, got[k]["calls"]):
            assert (r["pos"] if r else None) == want, (k, q, r)
            if r:
                assert r["refType"] == 1 and r["labels"] == ["EOP"] and r["json"] == tile()
    assert got[7]["calls"][0]["removedSeq"] == 3 and got[0]["calls"][0]["removedSeq"] is None
    assert "referenceTileLabels were annotated" in got[-1]["calls"][0]["error"]


def test_node_find_tile_on_emulation():
    addon = build_emu_napi()
    if addon is None:
        pytest.skip("Node headers are not installed")
    check(addon)


@pytest.mark.gpu
def test_node_find_tile_on_gpu():
    check(os.path.join(ROOT, "fluidframework_amd", "js", "mtgpu.node"))
