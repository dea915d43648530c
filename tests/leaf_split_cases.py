"""Hand-built batches for inserts applied in one visit to their leaf block (MT_INSERT_LEAF,
csrc/mt_core.h opInsert and insertAtPath<true>): one document per case, each an insert on a leaf
block whose rows the test lays out itself (tests/range_leaf_cases.py: k rows of W units, MSN 0,
so a leaf of k rows until the 8th child splits it 4 / 4).

An insert inside row j (row index in its block) cuts the row and puts two children into the
block, the new row at j + 1 and the right half at j + 2.  `paired` is the number of the document's
inserts that must go in that way, `split` how many of those must split their block: a block of 6
rows under the new row, a block of 7 under the half alone, after which the new row joins the
block of its left neighbour.
"""
from fluidframework_amd.batch import BatchBuilder, PropTable
from range_leaf_cases import MARKER, W, ins, leaf, msg, rng, stream_names


def mid(k, pos, seg="IJ", client=1):
    """The leaf, then one insert at pos by a client that has seen it all."""
    return leaf(k) + [msg(client, k + 1, k, ins(pos, seg))]


def tie_unseen():
    """c1 inserts XX at the boundary of rows 0 and 1; c2 has not seen it, so XX is a zero-length
    row in its view and its own insert inside row 1 cuts block child 2 of 7."""
    m = leaf(6)
    m.append(msg(1, 7, 6, ins(W, "XX")))
    m.append(msg(2, 8, 6, ins(W + 2, "YY")))
    return m


def tie_at_boundary():
    """As above with c2's insert at the boundary itself: no row is cut (the tie goes to the
    walk's rule) and the block of 7 splits under the new row alone."""
    m = leaf(6)
    m.append(msg(1, 7, 6, ins(W, "XX")))
    m.append(msg(2, 8, 6, ins(W, "YY")))
    return m


def two_in_a_row():
    """Two more inserts into what the first left: leaf of 7 -> 5 + 4 rows -> 7 + 4 -> 7 + 6."""
    m = leaf(7)
    m.append(msg(1, 8, 7, ins(6, "IJ")))
    m.append(msg(2, 9, 8, ins(3, "KL")))             # row 0 of the old block, which now has 5 rows
    m.append(msg(3, 10, 7, ins(21, "MN")))           # has not seen either; inside row 5, now in the new block
    return m


def below_full_parent():
    """A leaf of 7 rows below a full root.  8 appended rows make a root over two leaves of 4; every
    4 rows put in front split leaf 0 again (it keeps 4), so 20 of them leave the root with 7
    leaves and 3 more leaf 0 with 7 rows.  The insert inside its first row splits it, the cascade
    splits the root (8 children) and a new root grows above."""
    m = leaf(8)
    for s in range(9, 32):
        m.append(msg(0, s, s - 1, ins(0, "PQRS")))
    m.append(msg(1, 32, 31, ins(1, "IJ")))
    return m


def after_range_op(mode):
    """A remove or annotate that cuts two rows (rangeLeaf, 5 + 2 = 7 rows), then an insert inside
    one of the covered halves: the half of a removed row, and a block of 7."""
    def f():
        m = leaf(5)
        m.append(msg(1, 6, 5, rng(mode, 5, 11)))
        m.append(msg(2, 7, 5, ins(9, "IJ")))          # has not seen the range op; inside row 2 as it was
        return m
    return f


# name -> (builder, inserts that go in together with a right half, of those that split their block)
CASES = {
    "five_rows": (lambda: mid(5, 6), 1, 0),                 # 5 + 2 = 7: no block split
    "six_rows": (lambda: mid(6, 6), 1, 1),                  # splits 4 / 4 under the new row, which stays left
    "six_rows_j3": (lambda: mid(6, 14), 1, 1),              # the new row becomes the new block's first child
    "six_rows_j4": (lambda: mid(6, 18), 1, 1),
    "six_rows_last": (lambda: mid(6, 23), 1, 1),
    "seven_rows_j0": (lambda: mid(7, 1), 1, 1),
    "seven_rows_j1": (lambda: mid(7, 6), 1, 1),             # 5 + 4
    "seven_rows_j2": (lambda: mid(7, 10), 1, 1),            # the half is the old block's last child of 5
    "seven_rows_j3": (lambda: mid(7, 14), 1, 1),            # the half is the new block's first: new row at the old block's end
    "seven_rows_j4": (lambda: mid(7, 18), 1, 1),            # 4 + 5
    "seven_rows_last": (lambda: mid(7, 27), 1, 1),          # the half in the ninth place
    "row_boundary": (lambda: mid(7, 8), 0, 0),              # nothing cut: one child, the usual split
    "block_end": (lambda: mid(7, 28), 0, 0),
    "first_unit": (lambda: mid(7, 0), 0, 0),
    "marker": (lambda: mid(7, 14, MARKER), 1, 1),
    "marker_five_rows": (lambda: mid(5, 9, MARKER), 1, 0),
    "payload_100": (lambda: mid(7, 14, "q" * 50 + "\n" + "r" * 49), 1, 1),
    "tie_unseen_row": (tie_unseen, 1, 1),
    "tie_at_boundary": (tie_at_boundary, 0, 0),
    "two_in_a_row": (two_in_a_row, 3, 1),
    "below_full_parent": (below_full_parent, 1, 1),
    "after_remove": (after_range_op("remove"), 1, 1),
    "after_annotate": (after_range_op("annotate"), 1, 1),
    "client_63": (lambda: mid(7, 14, client=63), 1, 1),
}


def build():
    """(batch, props, [paired per document], [split per document]) with one document per case."""
    props = PropTable()
    bb = BatchBuilder(props, stream_names())
    paired, split = [], []
    for d, (name, (f, p, s)) in enumerate(CASES.items()):
        bb.begin_doc(d)
        for m in f():
            bb.add_message(m)
        paired.append(p)
        split.append(s)
    return bb.build(), props, paired, split


# ---- range ops whose right halves split their leaf block (MT_LEAF_SPLIT, rangeLeaf) ----
# A remove or annotate of [a, b) inside one leaf of n rows cuts row j at a and row je at b (ns = 1 or
# 2 right halves) with n + ns = 8 or 9: the start's half goes in first, the end's second.

def one(k, a, b, client=1):
    return lambda mode: leaf(k) + [msg(client, k + 1, k, rng(mode, a, b))]


def range_below_full_parent(mode):
    """below_full_parent's tree (a leaf of 7 rows under a root of 7 leaves), then a range op inside
    its first row: 9 children, the root splits and a new root grows."""
    m = below_full_parent()[:-1]
    m.append(msg(1, 32, 31, rng(mode, 1, 3)))
    return m


def range_tie(mode):
    """Rows r0 XX r1 YY r2 r3 r4; c2 has seen neither XX nor YY: its range starts at the boundary
    that the zero-length XX breaks the tie for and ends inside r1."""
    m = leaf(5)
    m.append(msg(1, 6, 5, ins(W, "XX")))
    m.append(msg(1, 7, 6, ins(2 * W + 2, "YY")))
    m.append(msg(2, 8, 5, rng(mode, W, 2 * W - 1)))
    return m


def range_then_insert(mode):
    """What a block-splitting range op leaves feeds a second range op and an insert."""
    m = leaf(7)
    m.append(msg(1, 8, 7, rng(mode, 5, 22)))
    m.append(msg(2, 9, 7, rng(mode, 3, 9)))           # has not seen the first; rows 0..2 of the old block
    m.append(msg(0, 10, 9, ins(6, "ZZ")))
    return m


# name -> (builder, range ops that must be applied in the leaf visit with a block split)
RANGE_CASES = {
    "seven_rows_end_split": (one(7, 4, 6), 1),                # ns = 1: the end's half alone
    "seven_rows_start_split": (one(7, 5, 8), 1),              # ns = 1: the start's half alone
    "seven_rows_start_split_last": (one(7, 25, 28), 1),
    "seven_rows_both_old_block": (one(7, 1, 6), 1),           # the end's half is child 3: 5 + 4
    "seven_rows_end_fifth": (one(7, 1, 10), 1),               # the end's half is the old block's last child of 5
    "seven_rows_end_follows": (one(7, 1, 14), 1),             # its left neighbour is the new block's first: 4 + 5
    "seven_rows_both_new_block": (one(7, 17, 26), 1),
    "seven_rows_across": (one(7, 5, 22), 1),                  # covered rows in both blocks: two LRU entries
    "seven_rows_three": (one(7, 13, 15), 1),                  # je == j: row 3 becomes three, the halves lead the new block
    "seven_rows_three_first": (one(7, 1, 3), 1),
    "seven_rows_three_last": (one(7, 25, 27), 1),
    "six_rows_both": (one(6, 5, 22), 1),                      # splits 4 / 4 under the end's half
    "six_rows_three": (one(6, 5, 7), 1),
    "six_rows_three_last": (one(6, 21, 23), 1),
    "whole_leaf_inside": (one(7, 1, 27), 1),
    "below_full_parent": (range_below_full_parent, 1),
    "tie_at_start": (range_tie, 1),
    "client_63": (one(7, 5, 22, client=63), 0),               # refused as ever: the three-visit path
    "range_then_insert": (range_then_insert, 1),
}


def build_ranges(mode):
    """(batch, props, [block-splitting fused range ops per document]) in RANGE_CASES order."""
    props = PropTable()
    bb = BatchBuilder(props, stream_names())
    hits = []
    for d, (name, (f, h)) in enumerate(RANGE_CASES.items()):
        bb.begin_doc(d)
        for m in f(mode):
            bb.add_message(m)
        hits.append(h)
    return bb.build(), props, hits
