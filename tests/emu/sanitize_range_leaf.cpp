// sanitize_range_leaf.cpp — TEST-ONLY, beside sanitize_driver.cpp: hand-built range ops that take
// the fused leaf step (MT_RANGE_LEAF, mt_core.h rangeLeaf) on the engine's host emulation under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a standalone executable.  Rows of four units
// are appended by client 0 at MSN 0 (nothing merges, so the leaf holds exactly those rows), then
// one op by client 1 that has seen them all.  Document 0: a remove strictly inside row 1 of five
// (the row becomes three).  Document 1: an annotate from inside row 1 of four to the block's
// last unit (one split, the end used up at the block end).  Block residency and all-HBM pools;
// status words and SnapshotV1 digests must equal the oracle's replay of the same batch.
// Build + run: tests/emu/sanitize_range_leaf.sh (a report or a mismatch: non-zero status).
#include "mt_emu.cpp"
#include "../../oracle/mtoracle.h"

#include <stdio.h>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s: ", name); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

struct Props {                                     // four one-key sets: k0 = "s0" / 1 / 2.5 / ""
    std::vector<uint32_t> off{0, 1, 2, 3, 4};
    std::vector<uint16_t> key{0, 0, 0, 0};
    std::vector<int32_t> val{0, 1, 2, 3};
    std::vector<const char*> kj{"\"k0\""};
    std::vector<uint32_t> kidx{0xFFFFFFFFu};
    std::vector<const char*> vj{"\"s0\"", "1", "2.5", "\"\""};
    std::vector<uint8_t> falsy{0, 0, 0, 1}, kind{0, 1, 1, 0};
    std::vector<uint32_t> cls{0, 1, 2, 3};
    std::vector<int32_t> incr{MT_VAL_UNSUP, MT_VAL_UNSUP, MT_VAL_UNSUP, MT_VAL_UNSUP};
    mt_prop_table t{};
    Props() {
        t.n_sets = (uint32_t)off.size() - 1; t.set_off = off.data(); t.key = key.data(); t.value = val.data();
        t.n_keys = (uint32_t)kj.size(); t.key_json = kj.data(); t.key_index = kidx.data();
        t.n_values = (uint32_t)vj.size(); t.value_json = vj.data(); t.value_falsy = falsy.data(); t.value_class = cls.data();
        t.value_kind = kind.data(); t.value_incr = incr.data(); t.incr_object = MT_VAL_UNSUP;
    }
};

static void run(Props& P, int residency) {
    const char* name = residency == 2 ? "hand-built range ops, blk" : "hand-built range ops, hbm";
    struct Op { uint8_t type; int32_t p1, p2, pid; };
    const std::vector<std::vector<Op>> docs = {
        {{MT_OP_INSERT, 0, 0, -1}, {MT_OP_INSERT, 4, 0, -1}, {MT_OP_INSERT, 8, 0, -1}, {MT_OP_INSERT, 12, 0, -1},
         {MT_OP_INSERT, 16, 0, -1}, {MT_OP_REMOVE, 5, 7, -1}},
        {{MT_OP_INSERT, 0, 0, -1}, {MT_OP_INSERT, 4, 0, -1}, {MT_OP_INSERT, 8, 0, -1}, {MT_OP_INSERT, 12, 0, -1},
         {MT_OP_ANNOTATE, 6, 16, 2}},
    };
    const uint32_t n = (uint32_t)docs.size();
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen, off{0}, ids;
    for (uint32_t d = 0; d < n; d++) {
        int s = 0;
        for (const Op& o : docs[d]) {
            const bool in = o.type == MT_OP_INSERT;
            type.push_back(o.type); flags.push_back(MT_OPF_END_OF_MSG); client.push_back(in ? 0 : 1);
            seq.push_back(s + 1); ref.push_back(s); msn.push_back(0); p1.push_back(o.p1); p2.push_back(o.p2); pid.push_back(o.pid);
            poff.push_back((uint32_t)payload.size()); plen.push_back(in ? 4 : 0);
            if (in) for (int i = 0; i < 4; i++) payload.push_back((uint16_t)('a' + s));
            s++;
        }
        off.push_back((uint32_t)type.size()); ids.push_back(d);
    }
    mt_op_batch b{};
    b.n_runs = n; b.doc_ids = ids.data(); b.op_offsets = off.data(); b.n_ops = off[n]; b.type = type.data(); b.flags = flags.data();
    b.client = client.data(); b.seq = seq.data(); b.ref_seq = ref.data(); b.msn = msn.data(); b.pos1 = p1.data(); b.pos2 = p2.data();
    b.payload_off = poff.data(); b.payload_len = plen.data(); b.prop_id = pid.data(); b.payload = payload.data();
    b.payload_units = (uint32_t)payload.size();
    mt_limits L{}; L.max_docs = n; L.rows_per_doc = 64; L.blocks_per_doc = 64; L.heap_per_doc = 64; L.window_per_doc = 64;
    L.text_per_doc = 4096; L.propsets_per_doc = 64;
    mt_ctx* c = nullptr;
    CHECK(emu_create(0, &L, &c) == MT_OK, "create");
    CHECK(emu_set_props(c, &P.t) == MT_OK, "set_props");
    const char* np[2] = {"\"c0\"", "\"c1\""};
    emu_set_client_names(c, 2, np);
    emu_set_residency(c, residency, 0, 0, 0);
    CHECK(emu_docs_open(c, 0, n) == MT_OK, "open");
    CHECK(emu_apply_batch(c, &b) == MT_OK, "apply");
    emu_sync(c);
    std::vector<uint32_t> st(n), ost(n);
    emu_doc_status(c, n, ids.data(), st.data());
    std::vector<int32_t> neg(n, -1);
    std::vector<uint64_t> dig(n), odg(n);
    const char* arena; const uint64_t* boff; const uint32_t* bfirst;
    CHECK(emu_snapshot_v1(c, n, ids.data(), neg.data(), neg.data(), dig.data(), &arena, &boff, &bfirst) == MT_OK, "snapshot");
    ora_replay_batch(&b, &P.t, 1, odg.data(), ost.data(), nullptr);
    for (uint32_t d = 0; d < n; d++) {
        CHECK(st[d] == 0 && ost[d] == 0, "doc %u status %#x, oracle %#x", d, st[d], ost[d]);
        CHECK(dig[d] == odg[d], "doc %u SnapshotV1 digest vs oracle", d);
    }
    emu_destroy(c);
    fprintf(stderr, "%-28s %u docs: %s\n", name, n, fails ? "FAILED" : "ok");
}

int main() {
    Props P;
    run(P, 2);
    run(P, 0);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    fprintf(stderr, "sanitize_range_leaf: both residencies equal to the oracle, no sanitizer report\n");
    return 0;
}
