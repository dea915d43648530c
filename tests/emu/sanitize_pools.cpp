// sanitize_pools.cpp — TEST-ONLY, beside sanitize_range_leaf.cpp: the life of the pools and of the
// resident batch on the engine's host emulation under AddressSanitizer (leak detection on) +
// UndefinedBehaviorSanitizer, as a standalone executable.  Two documents of different capacities:
// create, a first batch replayed, a resize that reallocates the full rows pool, checkpoint, a
// second resize, restore, a parts upload that needs a larger region and fails on a bad op, the
// replay that must then be refused, a valid upload and replay, destroy.  The final SnapshotV1
// digests must equal the oracle's replay of both batches as one; a clean exit says that
// mt_destroy freed every pool, shadow and buffer that create, resize and checkpoint allocated.
// Build + run: tests/emu/sanitize_pools.sh (a report, a leak or a mismatch: non-zero status).
#include "mt_emu.cpp"
#include "../../oracle/mtoracle.h"

#include <stdio.h>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL: "); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

// Ops [first, last) of every document's stream (message s: client 0 inserts four units at 0), as one batch.
struct Batch {
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen, off{0}, ids;
    mt_op_batch b{};
    Batch(uint32_t n_docs, int first, int last) {
        for (uint32_t d = 0; d < n_docs; d++) {
            for (int s = first; s < last; s++) {
                type.push_back(MT_OP_INSERT); flags.push_back(MT_OPF_END_OF_MSG); client.push_back(0);
                seq.push_back(s + 1); ref.push_back(s); msn.push_back(0); p1.push_back(0); p2.push_back(0); pid.push_back(-1);
                poff.push_back((uint32_t)payload.size()); plen.push_back(4);
                for (int i = 0; i < 4; i++) payload.push_back((uint16_t)('a' + (s + d) % 26));
            }
            off.push_back((uint32_t)type.size()); ids.push_back(d);
        }
        b.n_runs = n_docs; b.doc_ids = ids.data(); b.op_offsets = off.data(); b.n_ops = off[n_docs]; b.type = type.data();
        b.flags = flags.data(); b.client = client.data(); b.seq = seq.data(); b.ref_seq = ref.data(); b.msn = msn.data();
        b.pos1 = p1.data(); b.pos2 = p2.data(); b.payload_off = poff.data(); b.payload_len = plen.data(); b.prop_id = pid.data();
        b.payload = payload.data(); b.payload_units = (uint32_t)payload.size();
    }
};

int main() {
    const uint32_t n = 2;
    uint32_t set_off[1] = {0};
    mt_prop_table props{};
    props.set_off = set_off; props.incr_object = MT_VAL_UNSUP;
    mt_limits L[2] = {};
    L[0].rows_per_doc = 256; L[0].text_per_doc = 2048; L[0].window_per_doc = 256; L[0].propsets_per_doc = 16;
    L[1].rows_per_doc = 300; L[1].blocks_per_doc = 200; L[1].markers_per_doc = 8;          // the rest: the defaults
    mt_ctx* c = nullptr;
    CHECK(emu_create_docs(0, n, L, &c) == MT_OK, "create_docs");
    CHECK(emu_set_props(c, &props) == MT_OK, "set_props");
    const char* names[1] = {"\"c0\""};
    emu_set_client_names(c, 1, names);
    CHECK(emu_docs_open(c, 0, n) == MT_OK, "open");
    Batch first(n, 0, 6), second(n, 6, 206), all(n, 0, 206);
    CHECK(emu_apply_batch(c, &first.b) == MT_OK, "apply the first batch: %s", emu_last_error(c));

    const uint32_t d0 = 0, d1 = 1;
    uint64_t bytes0 = 0, bytes1 = 0, gs[6];
    emu_pool_bytes(c, &bytes0);
    mt_limits q{};
    q.rows_per_doc = 512;                                  // the rows pool is full: reallocated
    CHECK(emu_docs_resize(c, 1, &d1, &q) == MT_OK, "resize: %s", emu_last_error(c));
    emu_pool_bytes(c, &bytes1);
    emu_grow_stats(c, gs);
    CHECK(bytes1 > bytes0 && gs[0] == 1 && gs[1] == 1 && gs[4] > 0, "after the resize: %llu -> %llu bytes, %llu relocations, %llu reallocations",
          (unsigned long long)bytes0, (unsigned long long)bytes1, (unsigned long long)gs[0], (unsigned long long)gs[1]);
    CHECK(emu_checkpoint(c) == MT_OK, "checkpoint");
    q = mt_limits{};
    q.text_per_doc = 4096; q.window_per_doc = 512;
    CHECK(emu_docs_resize(c, 1, &d0, &q) == MT_OK, "second resize: %s", emu_last_error(c));
    CHECK(emu_restore(c) == MT_OK, "restore");
    mt_limits caps[2];
    const uint32_t both[2] = {0, 1};
    emu_doc_caps(c, 2, both, caps);
    CHECK(caps[0].text_per_doc == 2048 && caps[0].window_per_doc == 256 && caps[1].rows_per_doc == 512, "capacities after restore");

    // parts that need a larger region than the resident batch's, one op of an unknown type
    Batch bad(n, 6, 206);
    bad.type[137] = 200;
    CHECK(emu_upload_batch_parts(c, 1, &bad.b, nullptr, nullptr) == MT_E_INVALID, "a bad part was accepted");
    CHECK(std::string(emu_last_error(c)) == "unknown op type", "message: %s", emu_last_error(c));
    CHECK(emu_replay_resident(c) == MT_E_INVALID, "a replay without a resident batch was accepted");
    CHECK(emu_upload_batch(c, &second.b) == MT_OK, "upload: %s", emu_last_error(c));
    CHECK(emu_replay_resident(c) == MT_OK, "replay: %s", emu_last_error(c));
    emu_sync(c);

    std::vector<uint32_t> st(n), ost(n);
    emu_doc_status(c, n, both, st.data());
    std::vector<int32_t> neg(n, -1);
    std::vector<uint64_t> dig(n), odg(n);
    const char* arena; const uint64_t* boff; const uint32_t* bfirst;
    CHECK(emu_snapshot_v1(c, n, both, neg.data(), neg.data(), dig.data(), &arena, &boff, &bfirst) == MT_OK, "snapshot");
    ora_replay_batch(&all.b, &props, 1, odg.data(), ost.data(), nullptr);
    for (uint32_t d = 0; d < n; d++) {
        CHECK(st[d] == 0 && ost[d] == 0, "doc %u status %#x, oracle %#x", d, st[d], ost[d]);
        CHECK(dig[d] == odg[d], "doc %u SnapshotV1 digest vs oracle", d);
    }
    emu_destroy(c);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    fprintf(stderr, "sanitize_pools: pools, shadows and the resident batch through resize, checkpoint, restore and a failed upload: "
                    "equal to the oracle, no sanitizer report, no leak\n");
    return 0;
}
