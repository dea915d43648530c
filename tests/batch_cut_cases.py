"""One stream, many ways to cut it into batches: the shared code of tests/test_batch_cuts.py.

The engine's promise is that a document's state is a function of its message stream alone.
Everything here serves one property: for a fixed stream, every way of cutting it into batches
at message boundaries gives, at every cut, the oracle's state at that prefix, and at the end
also the state of an engine that took the stream in one batch.  "State" is what the hosts can
see: statuses, text, the segment dump, SnapshotV1 and SnapshotLegacy bytes and digests.  Nothing
is approximate.

A cutting is a *plan*: plan[r] lists, for run r of the stream's batch, (slot, end) pairs with
both members increasing: batch number `slot` brings the run's messages up to message `end`
(exclusive, counted from the run's first message).  Runs may have different numbers of cuts and
may be absent from any slot.
"""
import functools

import numpy as np

from fluidframework_amd.batch import OpBatch, PropTable
from oracle_lib import OracleDoc, gen_params, generate
from test_emu_parity import CONFIGS, NAMES, ann_props

CAPS = dict(rows_per_doc=20000, window_per_doc=8192, propsets_per_doc=8192, text_per_doc=1 << 18)
TINY = dict(rows_per_doc=64, blocks_per_doc=16, heap_per_doc=64, window_per_doc=64, text_per_doc=256, propsets_per_doc=16)
# (residency, continuation threshold or None); the last is the default residency
SMALL = [((1, 40, 40, 12), None), ((2, 0, 40, 12), 0), ((2, 0, 40, 12), 1 << 30), ((3, 16, 0, 12), None)]
RESIDENCIES = SMALL + [((0, 0, 0, 0), None), (None, None)]
RES_IDS = ["lds", "blk_cont", "blk_handover", "big", "hbm", "default"]
STREAMS = ["cfg2", "cfg3", "grow"]
CUTTINGS = ["per_message", "random", "ragged"]
OPS = 1500
PER_MESSAGE = 300          # messages cut one by one; the rest of the run follows in one batch
PER_MESSAGE_CHECK = 25     # ... with the oracle's prefix compared at every 25th cut


@functools.lru_cache(maxsize=None)
def generated(cfg, n_docs, seed=23):
    """(batch, props) of one generated stream per (configuration, documents): shared, read only."""
    props = ann_props()
    batch, st, _ = generate(gen_params(seed=seed, n_docs=n_docs, **{**CONFIGS[cfg], "ops": OPS}), props)
    assert st == [0] * n_docs
    return batch, props


def message_ends(batch, r):
    """Op indices (into the batch's arrays) one past each message's last member, for run r."""
    a, b = int(batch.op_offsets[r]), int(batch.op_offsets[r + 1])
    return (np.nonzero(batch.arrays["flags"][a:b] & 1)[0] + a + 1).tolist()


def n_messages(batch):
    return [len(message_ends(batch, r)) for r in range(len(batch.doc_ids))]


def cut_batch(batch, plan, start=None):
    """The batches of `plan` (module docstring), run r starting at message start[r] (default 0).
    Returns [(OpBatch, runs)], one per slot that holds anything, in slot order; `runs` lists the
    batch's runs as indices into the stream's."""
    R = len(batch.doc_ids)
    slots = {}
    for r in range(R):
        ends = [int(batch.op_offsets[r])] + message_ends(batch, r)
        at = 0 if start is None else int(start[r])
        prev = -1
        for slot, end in plan[r]:
            assert slot > prev and at < end <= len(ends) - 1, (r, slot, end, at)
            slots.setdefault(slot, []).append((r, ends[at], ends[end]))
            prev, at = slot, end
    out = []
    for slot in sorted(slots):
        pieces = slots[slot]
        idx = np.concatenate([np.arange(a, b) for _, a, b in pieces])
        offs = np.concatenate([[0], np.cumsum([b - a for _, a, b in pieces])])
        out.append((OpBatch.from_arrays([batch.doc_ids[r] for r, _, _ in pieces], offs, batch.payload,
                                        **{n: batch.arrays[n][idx] for n in batch.arrays}),
                    [r for r, _, _ in pieces]))
    return out


# ---- the cuttings ------------------------------------------------------------------------
def plan_per_message(n_msgs, start=None):
    """A cut after each of the first PER_MESSAGE messages, then the rest at once."""
    plan = []
    for r, n in enumerate(n_msgs):
        s = 0 if start is None else start[r]
        k = min(PER_MESSAGE, n - s)
        p = [(j, s + j + 1) for j in range(k)]
        if s + k < n:
            p.append((k, n))
        plan.append(p)
    return plan


def _windows(rng, lo, hi, n):
    """Window sizes from lo to hi, log-uniform (mean (hi - lo) / ln(hi / lo): 37.6 for 1..200,
    so a run of 1,500 messages is cut about 40 times), until they cover n messages."""
    out, left = [], n
    while left > 0:
        w = min(left, int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))))
        out.append(max(w, 1))
        left -= out[-1]
    return out


def plan_random(n_msgs, seed=7, start=None):
    """Each run cut on its own, windows of 1 to 200 messages; its k-th window rides in slot k, so
    the runs end in different slots."""
    rng = np.random.RandomState(seed)
    plan = []
    for r, n in enumerate(n_msgs):
        s = 0 if start is None else start[r]
        ends = s + np.cumsum(_windows(rng, 1, 200, n - s))
        plan.append([(k, int(e)) for k, e in enumerate(ends)])
    return plan


def plan_ragged(n_msgs, seed=9, start=None):
    """Run r is present only in every (r + 1)-th batch (slots r, 2r + 1, 3r + 2, ...)."""
    rng = np.random.RandomState(seed)
    plan = []
    for r, n in enumerate(n_msgs):
        s = 0 if start is None else start[r]
        ends = s + np.cumsum(_windows(rng, 20, 160, n - s))
        plan.append([((k + 1) * (r + 1) - 1, int(e)) for k, e in enumerate(ends)])
    return plan


def plan_late(rest, head=24):
    """`rest`'s cutting behind `head` one-message batches: the first launches name few property
    sets, whatever the number of documents (run_late_props)."""
    def plan(n_msgs):
        tail = rest(n_msgs, start=[head] * len(n_msgs))
        return [[(j, j + 1) for j in range(head)] + [(head + s, e) for s, e in t] for t in tail]
    return plan


PLANS = {"per_message": plan_per_message, "random": plan_random, "ragged": plan_ragged,
         "late_random": plan_late(plan_random), "late_ragged": plan_late(plan_ragged)}


def open_window_share(pieces):
    """Of the cuts (the last op of every run of every batch), the share that lands with
    msn < seq: the collaboration window is not empty at the boundary.  From the arrays alone."""
    inside = total = 0
    for b, _ in pieces:
        last = b.op_offsets[1:].astype(np.int64) - 1
        inside += int((b.arrays["msn"][last] < b.arrays["seq"][last]).sum())
        total += len(last)
    return inside / total


# ---- states ------------------------------------------------------------------------------
def engine_state(eng, n, msn, seq):
    """(statuses, texts, dumps, SnapshotV1 (blobs, digest), SnapshotLegacy, mt_snapshot_digests)."""
    return ([int(s) for s in eng.status(range(n))], eng.get_text(range(n)), [eng.dump(d).tobytes() for d in range(n)],
            eng.snapshot(range(n), msn, seq), eng.snapshot(range(n), msn, seq, legacy=True),
            [int(x) for x in eng.snapshot_digests(range(n), msn, seq, threads=3)])


def oracle_state(docs, msn, seq):
    v1 = [od.snapshot(int(m), int(s)) for od, m, s in zip(docs, msn, seq)]
    return ([0] * len(docs), [od.get_text() for od in docs], [od.dump().tobytes() for od in docs], v1,
            [od.snapshot(int(m), int(s), legacy=True) for od, m, s in zip(docs, msn, seq)], [d for _, d in v1])


PARTS = ("status", "text", "dump", "SnapshotV1", "SnapshotLegacy", "mt_snapshot_digests")


def assert_same_state(got, want, where):
    for name, g, w in zip(PARTS, got, want):
        if g != w:
            bad = [d for d in range(len(w)) if g[d] != w[d]]
            what = (g[bad[0]], w[bad[0]]) if name in ("status", "mt_snapshot_digests") else ""
            raise AssertionError(f"{where}: {name} differs on documents {bad} {what}")


class Oracle:
    """The oracle's documents fed the same pieces; its state after each slot on request."""

    def __init__(self, n, props):
        self.docs = [OracleDoc(True, props, NAMES) for _ in range(n)]
        self.msn, self.seq = np.zeros(n, np.int32), np.zeros(n, np.int32)

    def apply(self, b, runs, props=None):
        for i, r in enumerate(runs):
            if props is not None:
                self.docs[r].set_props(props)
            assert self.docs[r].apply_run(b, i) == 0
            last = int(b.op_offsets[i + 1]) - 1
            self.msn[r], self.seq[r] = b.arrays["msn"][last], b.arrays["seq"][last]

    def state(self):
        return oracle_state(self.docs, self.msn, self.seq)


def check_every(cutting):
    return PER_MESSAGE_CHECK if cutting == "per_message" else 1


@functools.lru_cache(maxsize=4)
def reference(cfg, n_docs, cutting):
    """(pieces, {slot index: the oracle's state after it}, final (msn, seq)): computed once per
    (stream, cutting), shared by the residencies, read only.  Every cut is kept for the random and
    ragged cuttings, every 25th and the last for the per-message one."""
    batch, props = generated(cfg, n_docs)
    pieces = cut_batch(batch, PLANS[cutting](n_messages(batch)))
    ora, want, k = Oracle(n_docs, props), {}, check_every(cutting)
    for j, (b, runs) in enumerate(pieces):
        ora.apply(b, runs)
        if (j + 1) % k == 0 or j == len(pieces) - 1:
            want[j] = (ora.state(), ora.msn.copy(), ora.seq.copy())
    return pieces, want


def new_engine(factory, n_docs, props, res=None, cont=None, caps=CAPS, upload=True):
    eng = factory(n_docs, **caps)
    if res is not None:
        eng.set_residency(*res)
    if cont is not None:
        eng.set_continuation(cont)
    if upload:
        eng.upload_props(props)
    eng.upload_names(NAMES)
    eng.open_docs(0, n_docs)
    return eng


@functools.lru_cache(maxsize=None)
def one_batch_state(kind, cfg, n_docs):
    """The state of an engine (default residency) that took the whole stream in one batch."""
    batch, props = generated(cfg, n_docs)
    eng = new_engine(FACTORIES[kind], n_docs, props)
    eng.apply(batch)
    eng.sync()
    last = batch.op_offsets[1:] - 1
    st = engine_state(eng, n_docs, batch.arrays["msn"][last], batch.arrays["seq"][last])
    eng.close()
    return st


FACTORIES = {}            # kind ("emu" / "gpu") -> engine factory, filled by the test module


def left_lds_later(eng, b, j, seen):
    """Notes in `seen` whether a run of batch j (not the first) entered LDS from what the launch
    before left in HBM and outgrew it again inside the batch (mt_last_cursors strictly inside the
    run): the hand-over of per-document state between launches that the small residencies are
    run for."""
    cur = eng.last_cursors(len(b.doc_ids)).astype(np.int64) & 0x7FFFFFFF
    if j > 0 and ((cur > b.op_offsets[:-1]) & (cur < b.op_offsets[1:])).any():
        seen.append(j)


def run_cut(kind, cfg, n_docs, cutting, res, cont):
    """The property, for one stream, cutting and residency."""
    batch, props = generated(cfg, n_docs)
    pieces, want = reference(cfg, n_docs, cutting)
    eng = new_engine(FACTORIES[kind], n_docs, props, res, cont)
    small = res is not None and res[0] != 0
    seen = []
    for j, (b, runs) in enumerate(pieces):
        eng.apply(b)
        eng.sync()
        if small:
            left_lds_later(eng, b, j, seen)
        if j in want:
            st, msn, seq = want[j]
            assert_same_state(engine_state(eng, n_docs, msn, seq), st, f"after batch {j} of {len(pieces)}")
    last = len(pieces) - 1
    st, msn, seq = want[last]
    assert_same_state(engine_state(eng, n_docs, msn, seq), one_batch_state(kind, cfg, n_docs), "one-batch engine")
    share = open_window_share(pieces)
    assert share >= 1 / 3, f"only {share:.2f} of the cuts land inside an open collaboration window"
    if small and cutting == "random":
        assert seen, "no document left LDS in a batch after the first: the hand-over was not reached"
    eng.close()
    return seen, share


# ---- props arriving late -----------------------------------------------------------------
def ann_prop_dicts():
    """The property sets of test_emu_parity.ann_props(), in its interning order."""
    vals = ["s0", "s1", "s2", "s3", 1, 2, None]
    rng = np.random.RandomState(5)
    out = []
    for _ in range(24):
        keys = rng.choice(8, size=rng.randint(1, 4), replace=False)
        out.append({f"k{k}": vals[rng.randint(0, len(vals))] for k in sorted(keys)})
    return out


def run_late_props(kind, cfg, n_docs, cutting, res, cont):
    """The device's table holds only the sets named so far: before each batch the host interns,
    in the full table's order, the sets up to the highest id the batch names, so Engine.apply
    uploads between launches (and the device's property pointers move) exactly when the table
    grew."""
    batch, full = generated(cfg, n_docs)
    dicts = ann_prop_dicts()
    pieces, want = reference(cfg, n_docs, cutting)
    late = PropTable()
    eng = new_engine(FACTORIES[kind], n_docs, late, res, cont, upload=False)
    eng.props = late
    uploads = []
    real = eng.upload_props
    eng.upload_props = lambda *a, **k: (uploads.append(late.version), real(*a, **k))[1]
    versions = set()                          # of the table, as the batches found it
    at = []                                   # the batches that found a new one
    for j, (b, runs) in enumerate(pieces):
        need = int(b.arrays["prop_id"].max()) + 1
        while len(late.sets) < need:
            assert late.intern(dicts[len(late.sets)]) == len(late.sets) - 1
        assert late.sets == full.sets[:len(late.sets)], "set ids differ from the full table's"
        if late.version not in versions:
            at.append(j)
        versions.add(late.version)
        eng.apply(b)
        eng.sync()
        assert len(uploads) == len(versions), f"batch {j}: {len(uploads)} uploads for {len(versions)} tables"
        if j in want:
            st, msn, seq = want[j]
            assert_same_state(engine_state(eng, n_docs, msn, seq), st, f"after batch {j}")
    # the table grew between launches at least once (ids equal to the full table's mean interning
    # up to the highest id named, so one early annotate of set 23 brings the whole table)
    assert late.sets == full.sets and len(versions) >= 2, f"{len(versions)} tables, uploaded before batches {at}"
    eng.close()
    return len(versions)


# ---- checkpoint across cuts --------------------------------------------------------------
def run_checkpoint(kind, cfg, n_docs, res, cont, at=12):
    """Checkpoint after batch `at` of the random cutting; the rest under that cutting, restore,
    the rest under the ragged one: the same state, the oracle's."""
    batch, props = generated(cfg, n_docs)
    pieces, want = reference(cfg, n_docs, "random")
    eng = new_engine(FACTORIES[kind], n_docs, props, res, cont)
    done = [0] * n_docs                       # messages each run has taken at the checkpoint
    plan = plan_random(n_messages(batch))
    for j, (b, runs) in enumerate(pieces[:at + 1]):
        eng.apply(b)
        for r in runs:
            done[r] = dict(plan[r])[j]
    eng.sync()
    eng.checkpoint()
    for b, _ in pieces[at + 1:]:
        eng.apply(b)
    eng.sync()
    st, msn, seq = want[len(pieces) - 1]
    first = engine_state(eng, n_docs, msn, seq)
    assert_same_state(first, st, "first pass")
    eng.restore()
    for b, _ in cut_batch(batch, plan_ragged(n_messages(batch), seed=31, start=done), start=done):
        eng.apply(b)
    eng.sync()
    assert_same_state(engine_state(eng, n_docs, msn, seq), first, "second pass")
    eng.close()


# ---- autogrow across cuts ----------------------------------------------------------------
def run_autogrow(kind, cfg, n_docs, res, cont):
    batch, props = generated(cfg, n_docs)
    pieces, want = reference(cfg, n_docs, "random")
    eng = new_engine(FACTORIES[kind], n_docs, props, res, cont, caps=TINY)
    eng.set_autogrow(True)
    for j, (b, _) in enumerate(pieces):
        eng.apply(b)
        eng.sync()
        st, msn, seq = want[j]
        assert_same_state(engine_state(eng, n_docs, msn, seq), st, f"after batch {j}")
    gs = eng.grow_stats()
    assert gs["relocations"] >= n_docs, gs
    eng.close()


# ---- reads between cuts ------------------------------------------------------------------
def run_reads(kind, cfg, n_docs, res, cont):
    """Every query the hosts have, after every fifth batch: none of them may change the state,
    and the digests read along the way are the oracle's at that prefix."""
    batch, props = generated(cfg, n_docs)
    pieces, want = reference(cfg, n_docs, "random")
    eng = new_engine(FACTORIES[kind], n_docs, props, res, cont)
    docs = list(range(n_docs))
    for j, (b, _) in enumerate(pieces):
        eng.apply(b)
        eng.sync()
        if j % 5 == 4:
            st, msn, seq = want[j]
            texts = st[1]
            assert [int(x) for x in eng.get_length(docs, [0x7FFFFFFF] * n_docs, [-1] * n_docs)] == [len(t) for t in texts]
            assert eng.get_text_range(docs) == texts
            w = eng.walk_segments(docs)
            for d in docs:
                recs, ts, _ = w[d]
                assert "".join(ts) == texts[d] and int(recs["len"].sum()) == len(texts[d])
            recs, off = eng.tile_index(docs, "pg")
            assert len(recs) == 0 and int(off[-1]) == 0          # the generated streams hold no markers
            assert [int(x) for x in eng.snapshot_digests(docs, msn, seq)] == st[5], f"digests after batch {j}"
    st, msn, seq = want[len(pieces) - 1]
    assert_same_state(engine_state(eng, n_docs, msn, seq), st, "after the reads")
    eng.close()
