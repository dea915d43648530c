"""Hand-built batches for the fused leaf step of range ops (MT_RANGE_LEAF, csrc/mt_core.h
rangeLeaf): one document per case, each forcing one shape of a remove or an annotate on a
leaf block whose rows the test lays out itself.

The MSN stays 0, so no row ever merges or leaves: k inserts of W units by c0 leave a leaf of
exactly k rows (the root, up to 7 rows; 8 rows split 4 / 4 under a new root).  `hits` is the
number of range ops of the document that the fused step must apply (0: all fall back).
"""
from fluidframework_amd.batch import BatchBuilder, ClientNames, PropTable

W = 4                                   # units per laid-out row
MARKER = {"marker": {"refType": 1}}


def msg(client, seq, ref, op):
    return dict(clientId="c%d" % client, sequenceNumber=seq, referenceSequenceNumber=ref, minimumSequenceNumber=0,
                type="op", contents=op)


def ins(pos, seg):
    return {"type": 0, "pos1": pos, "seg": seg}


def rng(mode, a, b):
    if mode == "remove":
        return {"type": 1, "pos1": a, "pos2": b}
    return {"type": 2, "pos1": a, "pos2": b, "props": {"k1": "r%d_%d" % (a, b), "k9": a}}


def leaf(k):
    """k rows of W units each, appended by c0 at seq 1..k."""
    return [msg(0, i + 1, i, ins(i * W, "abcdefghijklmnopqrstuvwxyz"[i] * W)) for i in range(k)]


def one(k, a, b, client=1):
    """mode -> messages: the leaf, then one range op [a, b) by a client that has seen it all."""
    return lambda mode: leaf(k) + [msg(client, k + 1, k, rng(mode, a, b))]


def overlap(mode):
    """c1 removes row 1.  c2 has not seen that (row 1 counts for it: removing it again sets the
    overlap bit and keeps the first remover); c3 has seen it (a zero-length row inside its
    span) but not c2's op."""
    m = leaf(5)
    m.append(msg(1, 6, 5, rng("remove", 4, 8)))
    m.append(msg(2, 7, 5, rng(mode, 0, 16)))
    m.append(msg(3, 8, 6, rng(mode, 0, 8)))          # rows 0 and 2 in its view, row 1 between them
    return m


def ties(mode):
    """c1 inserts at both ends of row 1; c2 has seen neither insert, so both are zero-length
    rows that break the tie at its range's boundaries."""
    m = leaf(3)
    m.append(msg(1, 4, 3, ins(4, "XX")))
    m.append(msg(1, 5, 4, ins(10, "YY")))
    m.append(msg(2, 6, 3, rng(mode, 4, 8)))
    return m


def marker_at(a, b):
    def f(mode):
        m = leaf(3)
        m.append(msg(0, 4, 3, ins(4, MARKER)))      # rows: r0 M r1 r2
        m.append(msg(1, 5, 4, rng(mode, a, b)))
        return m
    return f


def two_ops(mode):
    """A second range op on the rows the first one split (the landing spot, the window and the
    U set after the fused step feed the next message)."""
    m = leaf(3)
    m.append(msg(1, 4, 3, rng(mode, 5, 7)))
    m.append(msg(2, 5, 3, rng(mode, 6, 10)))         # has not seen the first
    m.append(msg(0, 6, 5, ins(6, "ZZ")))
    return m


# name -> (builder, fused range ops expected)
CASES = {
    "inside_one_row": (one(3, 5, 7), 1),               # the row becomes three
    "whole_rows": (one(4, 4, 12), 1),                  # no split at either end
    "split_at_start": (one(4, 6, 12), 1),
    "split_at_end": (one(4, 4, 10), 1),
    "whole_leaf": (one(4, 0, 16), 1),                  # from the first unit to the last
    "to_last_unit": (one(4, 9, 16), 1),
    "from_first_unit": (one(4, 0, 7), 1),
    "overlap_and_zero_length": (overlap, 3),
    "ties_at_both_boundaries": (ties, 1),
    "marker_at_start": (marker_at(4, 9), 1),
    "marker_at_end": (marker_at(2, 4), 1),
    "marker_inside": (marker_at(3, 6), 1),
    "five_rows_two_splits": (one(5, 5, 7), 1),         # 5 + 2 < 8
    "six_rows_one_split": (one(6, 4, 6), 1),           # 6 + 1 < 8
    "six_rows_two_splits": (one(6, 5, 7), 0),          # the block would split
    "seven_rows_no_split": (one(7, 4, 8), 1),
    "seven_rows_one_split": (one(7, 4, 6), 0),
    "below_the_root": (one(8, 13, 15), 1),             # leaf 0 of two: the root's length changes too
    "end_in_next_leaf": (one(8, 12, 17), 0),           # one unit into leaf 1
    "second_leaf": (one(8, 17, 30), 1),
    "client_63": (one(3, 5, 7, client=63), 0),
    "two_ops": (two_ops, 2),
}
MODES = ("remove", "annotate")


def stream_names(n=64):
    cn = ClientNames()
    for i in range(n):
        cn.index("c%d" % i)
    return cn


def build(mode):
    """(batch, props, [hits per document]) with one document per case, in CASES order."""
    props = PropTable()
    bb = BatchBuilder(props, stream_names())
    hits = []
    for d, (name, (f, h)) in enumerate(CASES.items()):
        bb.begin_doc(d)
        for m in f(mode):
            bb.add_message(m)
        hits.append(h)
    return bb.build(), props, hits
