// sanitize_tiles.cpp — TEST-ONLY, beside sanitize_driver.cpp: the tile search (mt_query.h: the
// document-order scan, mt_find_tile, mt_tile_index) on the engine's host emulation under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a standalone executable.  One document of
// alternating two-unit text rows and markers (refType 1 labelled "pg", 33 labelled "cell", 17
// labelled "pg" by a map of 71 keys with referenceTileLabels last: the wide-map rounds, 0
// labelled "pg" but no tile), appended by one client at MSN 0 so nothing merges (height >= 2),
// then removes that take markers with them, the document's last one included.  Every query kind:
// findTile at every position 0..L, L + 3 and undefined, both directions, both labels, against
// the rule of include/mtgpu.h evaluated on mt_dump_segments; the index (count and fill passes)
// against the same rows.  Build + run: tests/emu/sanitize_tiles.sh (a report or a mismatch:
// non-zero status).
#include "mt_emu.cpp"

#include <stdio.h>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL: "); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

static const int WIDE = 70;
struct Props {                                     // sets: 0 {tl: ["pg"]}, 1 {tl: ["cell"]}, 2 {k0..k69: 1, tl: ["pg"]}
    std::vector<uint32_t> off; std::vector<uint16_t> key; std::vector<int32_t> val;
    std::vector<std::string> kjs; std::vector<const char*> kj; std::vector<uint32_t> kidx;
    std::vector<const char*> vj{"[\"pg\"]", "[\"cell\"]", "1"};
    std::vector<uint8_t> falsy{0, 0, 0}, kind{0, 0, 1};
    std::vector<uint32_t> cls{0, 1, 2};
    std::vector<int32_t> incr{MT_VAL_UNSUP, MT_VAL_UNSUP, MT_VAL_UNSUP};
    mt_prop_table t{};
    Props() {
        kjs.push_back("\"referenceTileLabels\"");
        for (int i = 0; i < WIDE; i++) kjs.push_back("\"k" + std::to_string(i) + "\"");
        for (auto& s : kjs) { kj.push_back(s.c_str()); kidx.push_back(0xFFFFFFFFu); }
        off = {0, 1, 2};
        key = {0, 0}; val = {0, 1};
        for (int i = 0; i < WIDE; i++) { key.push_back((uint16_t)(1 + i)); val.push_back(2); }
        key.push_back(0); val.push_back(0);
        off.push_back((uint32_t)key.size());
        t.n_sets = (uint32_t)off.size() - 1; t.set_off = off.data(); t.key = key.data(); t.value = val.data();
        t.n_keys = (uint32_t)kj.size(); t.key_json = kj.data(); t.key_index = kidx.data();
        t.n_values = (uint32_t)vj.size(); t.value_json = vj.data(); t.value_falsy = falsy.data(); t.value_class = cls.data();
        t.value_kind = kind.data(); t.value_incr = incr.data(); t.incr_object = MT_VAL_UNSUP;
    }
};

struct Row { int len; bool removed; int rt; };
static bool matches(const Row& r, int label) {      // label 0 "pg", 1 "cell"
    if (r.rt < 0 || !(r.rt & 1)) return false;
    return label == 0 ? (r.rt == 1 || r.rt == 17) : r.rt == 33;
}
// the rule of include/mtgpu.h: the row's index, or -1
static int expected(const std::vector<Row>& rows, const std::vector<int>& start, int L, bool undef, int pos, int label, bool preceding) {
    const int n = (int)rows.size();
    if (preceding) {
        for (int i = n - 1; i >= 0; i--) if (!rows[i].removed && matches(rows[i], label) && (undef || start[i] <= pos)) return i;
        return -1;
    }
    if (!undef && pos > L) return -1;
    int leaf = -1;
    if (!undef) for (int i = 0; i < n; i++) if (start[i] <= pos) leaf = i;
    if (leaf >= 0 && matches(rows[leaf], label)) return leaf;
    for (int i = leaf + 1; i < n; i++) if (!rows[i].removed && matches(rows[i], label)) return i;
    return -1;
}

int main() {
    Props P;
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen;
    int s = 0, len = 0;
    auto op = [&](uint8_t ty, uint8_t fl, int a, int b, int set, int units) {
        type.push_back(ty); flags.push_back((uint8_t)(MT_OPF_END_OF_MSG | fl)); client.push_back(ty == MT_OP_INSERT ? 0 : 1);
        seq.push_back(s + 1); ref.push_back(s); msn.push_back(0); p1.push_back(a); p2.push_back(b); pid.push_back(set);
        poff.push_back((uint32_t)payload.size()); plen.push_back((uint32_t)units);
        for (int i = 0; i < units; i++) payload.push_back((uint16_t)('a' + s % 26));
        s++;
    };
    const int refTypes[4] = {1, 33, 17, 0}, sets[4] = {0, 1, 2, 0};
    for (int i = 0; i < 90; i++) {
        op(MT_OP_INSERT, 0, len, 0, -1, 2); len += 2;
        op(MT_OP_INSERT, MT_OPF_MARKER | MT_OPF_SEG_PROPS, len, refTypes[i % 4], sets[i % 4], 0); len += 1;
    }
    op(MT_OP_REMOVE, 0, len - 1, len, -1, 0); len -= 1;        // the document's last row, a "cell" tile... removed
    op(MT_OP_REMOVE, 0, 30, 41, -1, 0); len -= 11;             // rows in the middle, markers included
    op(MT_OP_REMOVE, 0, 0, 3, -1, 0); len -= 3;                // the first text row and tile
    const uint32_t ids[1] = {0}, off[2] = {0, (uint32_t)type.size()};
    mt_op_batch b{};
    b.n_runs = 1; b.doc_ids = ids; b.op_offsets = off; b.n_ops = off[1]; b.type = type.data(); b.flags = flags.data();
    b.client = client.data(); b.seq = seq.data(); b.ref_seq = ref.data(); b.msn = msn.data(); b.pos1 = p1.data(); b.pos2 = p2.data();
    b.payload_off = poff.data(); b.payload_len = plen.data(); b.prop_id = pid.data(); b.payload = payload.data();
    b.payload_units = (uint32_t)payload.size();
    mt_limits L{}; L.max_docs = 1; L.rows_per_doc = 512; L.blocks_per_doc = 256; L.heap_per_doc = 512; L.window_per_doc = 512;
    L.text_per_doc = 4096; L.propsets_per_doc = 512;
    mt_ctx* c = nullptr;
    CHECK(emu_create(0, &L, &c) == MT_OK, "create");
    CHECK(emu_set_props(c, &P.t) == MT_OK, "set_props");
    const char* np[2] = {"\"c0\"", "\"c1\""};
    emu_set_client_names(c, 2, np);
    CHECK(emu_docs_open(c, 0, 1) == MT_OK, "open");
    CHECK(emu_apply_batch(c, &b) == MT_OK, "apply: %s", emu_last_error(c));
    emu_sync(c);
    uint32_t st = 1; int32_t pools[10];
    emu_doc_status(c, 1, ids, &st);
    emu_doc_pools(c, 1, ids, pools);
    CHECK(st == 0, "status %#x", st);
    CHECK(pools[6] >= 2, "tree height %d", pools[6]);
    int32_t* dump = nullptr; uint32_t nr = 0;
    CHECK(emu_dump_segments(c, 0, &dump, &nr) == MT_OK, "dump");
    std::vector<Row> rows; std::vector<int> start;
    int Lobs = 0, removedTiles = 0;
    for (uint32_t i = 0; i < nr; i++) {
        const int32_t* r = dump + 12 * i;
        Row w{r[0], r[3] != INT32_MIN, r[8]};
        start.push_back(Lobs); rows.push_back(w);
        if (!w.removed) Lobs += w.len;
        removedTiles += w.removed && w.rt >= 0;
    }
    emu_free(dump);
    CHECK(Lobs == len && removedTiles >= 3 && rows.back().removed && rows.back().rt == 33, "document shape: L %d (%d), %d removed markers", Lobs, len, removedTiles);
    const uint8_t match[2 * 3] = {1, 0, 0, 0, 1, 0};
    mt_tile_labels T{2, 0, 3, match};
    // findTile: every position, both directions, both labels
    std::vector<uint32_t> qd, ql; std::vector<int32_t> qp; std::vector<uint8_t> qf;
    for (int label = 0; label < 2; label++)
        for (int pre = 0; pre < 2; pre++)
            for (int p = 0; p <= Lobs + 2; p++) {
                qd.push_back(0); ql.push_back((uint32_t)label); qf.push_back((uint8_t)pre);
                qp.push_back(p == Lobs + 1 ? Lobs + 3 : (p == Lobs + 2 ? MT_POS_UNDEFINED : p));
            }
    std::vector<mt_seg_info> out(qd.size());
    const char* arena = nullptr; const uint64_t* joff = nullptr;
    CHECK(emu_find_tile(c, (uint32_t)qd.size(), qd.data(), qp.data(), qf.data(), ql.data(), &T, out.data(), &arena, &joff) == MT_OK,
          "find_tile: %s", emu_last_error(c));
    int found = 0, removedHits = 0;
    for (size_t i = 0; i < qd.size(); i++) {
        const bool undef = qp[i] == MT_POS_UNDEFINED;
        const int want = expected(rows, start, Lobs, undef, qp[i], (int)ql[i], qf[i] != 0);
        CHECK((out[i].found != 0) == (want >= 0), "query %zu (pos %d label %u pre %u): found %d, want row %d", i, qp[i], ql[i], qf[i], out[i].found, want);
        if (want < 0 || !out[i].found) continue;
        CHECK(out[i].obs_pos == start[want] && out[i].resolved == start[want] && out[i].offset == 0 &&
              out[i].marker_ref_type == rows[want].rt && (out[i].removed_seq != INT32_MIN) == rows[want].removed,
              "query %zu (pos %d label %u pre %u): pos %d refType %d, want %d %d", i, qp[i], ql[i], qf[i], out[i].obs_pos,
              out[i].marker_ref_type, start[want], rows[want].rt);
        CHECK(joff[i + 1] > joff[i], "query %zu: no JSON", i);
        found++; removedHits += rows[want].removed;
    }
    CHECK(found > Lobs && removedHits == 1, "%d found, %d removed answers", found, removedHits);
    int32_t neg = -1;
    CHECK(emu_find_tile(c, 1, ids, &neg, nullptr, ql.data(), &T, out.data(), nullptr, nullptr) == MT_E_INVALID, "negative pos accepted");
    // the index, both labels (a repeat of the document: two queries of one wave)
    const uint32_t idocs[3] = {0, 0, 0}, ilab[3] = {0, 1, 0};
    const mt_tile_rec* recs = nullptr; const uint64_t* roff = nullptr;
    CHECK(emu_tile_index(c, 3, idocs, ilab, &T, &recs, &roff) == MT_OK, "tile_index: %s", emu_last_error(c));
    for (int k = 0; k < 3; k++) {
        uint64_t at = roff[k];
        int tpos = 0;
        for (size_t i = 0; i < rows.size(); i++) {
            if (!rows[i].removed && matches(rows[i], (int)ilab[k])) {
                CHECK(at < roff[k + 1] && recs[at].pos == start[i] && recs[at].text_pos == tpos && recs[at].ref_type == rows[i].rt,
                      "index %d: record %llu", k, (unsigned long long)at);
                at++;
            }
            if (!rows[i].removed && rows[i].rt < 0) tpos += rows[i].len;
        }
        CHECK(at == roff[k + 1] && at > roff[k], "index %d: %llu records", k, (unsigned long long)(at - roff[k]));
    }
    emu_destroy(c);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    fprintf(stderr, "sanitize_tiles: %zu findTile queries (%d found) and the index equal to the rule, no sanitizer report\n",
            qd.size(), found);
    return 0;
}
