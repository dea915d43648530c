// sanitize_walk.cpp — TEST-ONLY, beside sanitize_text.cpp: segment walks (mt_query.h: the scan's
// walk kinds and MT_QK_PSET, mt_walk_segments) on the engine's host emulation under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a standalone executable.  Document 0 holds
// the known shapes (rows "hello" | "world", a marker, rows of 300, 64 and 65 units).  Document 1
// is 70 one-unit rows: two units of the scan.  Document 2 is a random stream of three clients
// (text inserts, markers, removes; every insert's units are one letter chosen by its seq, so a
// row's text follows from mt_dump_segments alone), tall enough for several units.  Every kind: the
// local view and each client's view at its last refSeq (rows the observer removed are visible
// there), S < E, S == E and S > E, with and without MT_WALK_TEXT, the count and the fill pass,
// against the rule of include/mtgpu.h evaluated on the dump.  Rows of documents 0 and 2 carry
// property maps of 1 and of 71 keys (five chunks), some shared.  The record, text and map-chunk
// buffers are released before every call, so the fill pass and the maps' launch write into buffers
// of exactly the counted sizes and a store past any of them is reported.  Build + run:
// tests/emu/sanitize_walk.sh (a report or a mismatch: non-zero status).
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
static const int SETKEYS[3] = {1, 1, WIDE + 1};

struct Batch {
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen;
    int s = 0;
    static uint16_t unit_of(int seq) { return (uint16_t)('a' + seq % 26); }
    std::vector<int> setOfSeq{-1};                 // the interned set an insert of that seq carries (-1: none)
    void op(uint8_t ty, uint8_t fl, int cl, int a, int b, int units, int set = -1) {
        type.push_back(ty); flags.push_back((uint8_t)(MT_OPF_END_OF_MSG | fl | (set >= 0 ? MT_OPF_SEG_PROPS : 0))); client.push_back((uint16_t)cl);
        seq.push_back(s + 1); ref.push_back(s); msn.push_back(0); p1.push_back(a); p2.push_back(b); pid.push_back(set);
        setOfSeq.push_back(set);
        poff.push_back((uint32_t)payload.size()); plen.push_back((uint32_t)units);
        for (int i = 0; i < units; i++) payload.push_back(unit_of(s + 1));
        s++;
    }
};

struct Row { int len, seq, client, rseq, rclient, rt; };
// nodeLength (MT/mergeTree.ts:1652-1692) of a dumped row under (r, c); c < 0: the local view
static int view_len(const Row& w, int r, int c) {
    const bool removed = w.rseq != INT32_MIN;
    if (c < 0) return removed ? 0 : w.len;
    const bool seen = w.client == c || w.seq <= r;
    const bool gone = removed && (w.rclient == c || w.rseq <= r);
    return seen && !gone ? w.len : 0;
}
struct Want { int pos, start, end, len, seq, rseq, rt, obs; };
// the rule of include/mtgpu.h
static std::vector<Want> expected(const std::vector<Row>& rows, int r, int c, bool sUndef, int S, bool eUndef, int E) {
    std::vector<Want> out;
    long L = 0;
    for (const Row& w : rows) L += view_len(w, r, c);
    const long s = sUndef ? 0 : S, e = eUndef ? L : E;
    long p = 0, o = 0;
    for (const Row& w : rows) {
        const long l = view_len(w, r, c);
        if (e - p > 0 && l > 0 && s - p < l)                // nodeMap's visit test (:2964)
            out.push_back(Want{(int)p, (int)(s - p), (int)(e - p), w.len, w.seq, w.rseq, w.rt, (int)o});
        p += l;
        o += view_len(w, 0, -1);
    }
    return out;
}

int main() {
    Batch B[3];
    // document 0: the known shapes
    // ("hello" and "world" share one interned set, so one device map; the marker's has 71 keys)
    B[0].op(MT_OP_INSERT, 0, 0, 0, 0, 5, 0); B[0].op(MT_OP_INSERT, 0, 0, 5, 0, 5, 0);
    B[0].op(MT_OP_INSERT, MT_OPF_MARKER, 0, 10, 1, 0, 2);
    B[0].op(MT_OP_INSERT, 0, 0, 11, 0, 300); B[0].op(MT_OP_INSERT, 0, 0, 311, 0, 64, 1); B[0].op(MT_OP_INSERT, 0, 0, 375, 0, 65);
    // document 1: 70 one-unit rows
    for (int k = 0; k < 70; k++) B[1].op(MT_OP_INSERT, 0, 0, k, 0, 1);
    // document 2: random; ops at refSeq = seq - 1, so the writer sees the observer's length
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](int n) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (int)((lcg >> 33) % (uint64_t)n); };
    int len = 0, lastOp[3] = {0, 0, 0};
    for (int i = 0; i < 500; i++) {
        const int cl = rnd(3), x = rnd(100);
        if (x < 55 || len < 4) { const int n = 1 + rnd(12); B[2].op(MT_OP_INSERT, 0, cl, rnd(len + 1), 0, n, rnd(4) == 0 ? 1 : -1); len += n; }
        else if (x < 70) { B[2].op(MT_OP_INSERT, MT_OPF_MARKER, cl, rnd(len + 1), 1, 0, rnd(2) ? 2 : 0); len += 1; }
        else { const int a = rnd(len), w = a + 1 + rnd(15), b = w > len ? len : w; B[2].op(MT_OP_REMOVE, 0, cl, a, b, 0); len -= b - a; }
        lastOp[cl] = B[2].s;
    }
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen;
    const uint32_t ids[3] = {0, 1, 2};
    uint32_t off[4] = {0, 0, 0, 0};
    for (int d = 0; d < 3; d++) {
        const Batch& b = B[d];
        for (size_t i = 0; i < b.type.size(); i++) {
            type.push_back(b.type[i]); flags.push_back(b.flags[i]); client.push_back(b.client[i]); seq.push_back(b.seq[i]);
            ref.push_back(b.ref[i]); msn.push_back(b.msn[i]); p1.push_back(b.p1[i]); p2.push_back(b.p2[i]); pid.push_back(b.pid[i]);
            poff.push_back((uint32_t)payload.size() + b.poff[i]); plen.push_back(b.plen[i]);
        }
        payload.insert(payload.end(), b.payload.begin(), b.payload.end());
        off[d + 1] = (uint32_t)type.size();
    }
    mt_op_batch b{};
    b.n_runs = 3; b.doc_ids = ids; b.op_offsets = off; b.n_ops = off[3]; b.type = type.data(); b.flags = flags.data();
    b.client = client.data(); b.seq = seq.data(); b.ref_seq = ref.data(); b.msn = msn.data(); b.pos1 = p1.data(); b.pos2 = p2.data();
    b.payload_off = poff.data(); b.payload_len = plen.data(); b.prop_id = pid.data(); b.payload = payload.data();
    b.payload_units = (uint32_t)payload.size();
    mt_limits L{}; L.max_docs = 3; L.rows_per_doc = 2048; L.blocks_per_doc = 1024; L.heap_per_doc = 2048; L.window_per_doc = 2048;
    L.text_per_doc = 8192; L.propsets_per_doc = 2048;
    mt_ctx* c = nullptr;
    Props P;
    CHECK(emu_create(0, &L, &c) == MT_OK, "create");
    CHECK(emu_set_props(c, &P.t) == MT_OK, "set_props");
    const char* np[3] = {"\"c0\"", "\"c1\"", "\"c2\""};
    emu_set_client_names(c, 3, np);
    CHECK(emu_docs_open(c, 0, 3) == MT_OK, "open");
    CHECK(emu_apply_batch(c, &b) == MT_OK, "apply: %s", emu_last_error(c));
    emu_sync(c);
    uint32_t st[3] = {1, 1, 1}; int32_t pools[30];
    emu_doc_status(c, 3, ids, st);
    emu_doc_pools(c, 3, ids, pools);
    CHECK(st[0] == 0 && st[1] == 0 && st[2] == 0, "status %#x %#x %#x", st[0], st[1], st[2]);
    CHECK(pools[10 + 6] == 2 && pools[20 + 6] >= 2, "tree heights %d %d", pools[10 + 6], pools[20 + 6]);
    std::vector<Row> rows[3];
    for (int d = 0; d < 3; d++) {
        int32_t* dump = nullptr; uint32_t nr = 0;
        CHECK(emu_dump_segments(c, (uint32_t)d, &dump, &nr) == MT_OK, "dump");
        for (uint32_t i = 0; i < nr; i++) { const int32_t* r = dump + 12 * i; rows[d].push_back(Row{r[0], r[1], r[2], r[3], r[4], r[8]}); }
        emu_free(dump);
    }
    int Lobs = 0;
    for (const Row& w : rows[2]) Lobs += view_len(w, 0, -1);
    CHECK(Lobs == len, "document 2: L %d (%d)", Lobs, len);
    struct Q { uint32_t doc; bool su; int s; bool eu; int e; int r, c; };
    std::vector<Q> qs;
    auto grid = [&](uint32_t doc, int r, int cl, int Lv, int nrand) {
        const int edge[6] = {0, 1, Lv - 1, Lv, Lv + 3, 0};
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) qs.push_back(Q{doc, i == 5, edge[i], j == 5, edge[j], r, cl});
        for (int i = 0; i < nrand; i++) qs.push_back(Q{doc, false, rnd(Lv + 6) - 2, false, rnd(Lv + 6) - 2, r, cl});
        for (int i = 0; i < nrand; i++) { const int p = rnd(Lv + 1); qs.push_back(Q{doc, false, p + rnd(12), false, p - rnd(4), r, cl}); }
    };
    // hand-checked answers first (they pin the evaluator above): records per query
    const int known[][3] = {{0, 3, 7}, {0, 5, 10}, {0, 0, 5}, {0, 4, 2}, {0, 7, 3}, {0, 11, 10}, {0, 10, 376}, {0, 374, 376}, {0, 3, 3},
                            {1, 60, 68}, {1, 0, 70}, {1, 64, 65}, {1, 66, 65}};
    const size_t knownRecs[] = {2, 1, 1, 1, 0, 0, 4, 2, 1, 8, 70, 1, 0};
    for (auto& k : known) qs.push_back(Q{(uint32_t)k[0], false, k[1], false, k[2], -1, -1});
    grid(0, -1, -1, 440, 100);
    grid(1, -1, -1, 70, 60);
    grid(2, -1, -1, Lobs, 150);
    int differing = 0;
    for (int cl = 0; cl < 3; cl++) {
        const int r = lastOp[cl] - 1;
        int Lv = 0, diff = 0;
        for (const Row& w : rows[2]) { Lv += view_len(w, r, cl); diff += view_len(w, r, cl) != view_len(w, 0, -1); }
        differing += diff > 0;
        grid(2, r, cl, Lv, 150);
        grid(2, B[2].s, cl, Lobs, 20);
    }
    CHECK(differing >= 1, "no client's view differs from the observer's");
    std::vector<uint32_t> qd; std::vector<int32_t> s, e, r, cl;
    for (const Q& q : qs) {
        qd.push_back(q.doc); s.push_back(q.su ? MT_POS_UNDEFINED : q.s); e.push_back(q.eu ? MT_POS_UNDEFINED : q.e);
        r.push_back(q.r); cl.push_back(q.c);
    }
    size_t visited = 0, insideHits = 0, removedSeen = 0, mapped = 0, wideSeen = 0;
    for (int withText = 1; withText >= 0; withText--) {
        // the fill pass gets buffers of exactly the counted sizes
        free(c->b_wout.p); c->b_wout = mt_ctx::DevBuf{};
        free(c->b_wtext.p); c->b_wtext = mt_ctx::DevBuf{};
        free(c->b_wmaps.p); c->b_wmaps = mt_ctx::DevBuf{};
        const mt_walk_rec* recs = nullptr; const uint64_t* roff = nullptr; const uint16_t* arena = nullptr; const mt_walk_maps* maps = nullptr;
        CHECK(emu_walk_segments(c, (uint32_t)qd.size(), qd.data(), s.data(), e.data(), r.data(), cl.data(), withText ? MT_WALK_TEXT : 0u, &recs,
                                &roff, withText ? &arena : nullptr, &maps) == MT_OK, "walk_segments: %s", emu_last_error(c));
        if (!recs || !roff) break;
        uint64_t tunits = 0;
        for (uint64_t k = 0; k < roff[qd.size()]; k++) if (withText && recs[k].marker_ref_type < 0) tunits += (uint64_t)recs[k].len;
        CHECK(c->b_wout.cap == sizeof(mt_walk_rec) * roff[qd.size()], "the record buffer is %zu bytes for %llu records", c->b_wout.cap,
              (unsigned long long)roff[qd.size()]);
        CHECK(c->b_wtext.cap == (withText ? 2 * tunits : 0), "the text buffer is %zu bytes for %llu units", c->b_wtext.cap, (unsigned long long)tunits);
        if (!maps) break;
        uint64_t chunks = 0;
        for (uint32_t m = 0; m < maps->n; m++) {
            const uint64_t nk = maps->key_off[m + 1] - maps->key_off[m];
            CHECK(nk == 1 || nk == (uint64_t)WIDE + 1, "map %u has %llu keys", m, (unsigned long long)nk);
            CHECK(maps->json_off[m + 1] - maps->json_off[m] > 2 && maps->json[maps->json_off[m]] == '{', "map %u has no JSON", m);
            chunks += (nk + MT_PSK - 1) / MT_PSK;
            wideSeen += nk > MT_PSK;
        }
        CHECK(c->b_wmaps.cap == sizeof(MtPSet) * chunks, "the maps' buffer is %zu bytes for %llu chunks", c->b_wmaps.cap, (unsigned long long)chunks);
        uint64_t tnext = 0;
        for (size_t i = 0; i < qs.size(); i++) {
            const Q& q = qs[i];
            const auto want = expected(rows[q.doc], q.r, q.c, q.su, q.s, q.eu, q.e);
            const uint64_t n = roff[i + 1] - roff[i];
            CHECK(n == want.size(), "query %zu (doc %u, [%d, %d), view %d/%d): %llu records, want %zu", i, q.doc, q.s, q.e, q.r, q.c,
                  (unsigned long long)n, want.size());
            if (i < sizeof knownRecs / sizeof knownRecs[0]) CHECK(n == knownRecs[i], "known answer %zu: %llu records", i, (unsigned long long)n);
            for (uint64_t k = 0; k < n && k < want.size(); k++) {
                const mt_walk_rec& g = recs[roff[i] + k];
                const Want& w = want[k];
                bool ok = g.pos == w.pos && g.start == w.start && g.end == w.end && g.len == w.len && g.seq == w.seq && g.removed_seq == w.rseq &&
                          g.marker_ref_type == w.rt && g.obs_pos == w.obs;
                // the row's map: the interned set its insert carried (no annotate runs here)
                const int set = B[q.doc].setOfSeq[(size_t)w.seq];
                ok = ok && (set < 0 ? (g.prop_set == -1 && g.map == -1) : (g.prop_set >= 0 && g.map >= 0 && (uint32_t)g.map < maps->n));
                if (ok && set >= 0) {
                    const uint32_t m = (uint32_t)g.map;
                    ok = maps->doc[m] == q.doc && maps->prop_set[m] == g.prop_set && maps->key_off[m + 1] - maps->key_off[m] == (uint64_t)SETKEYS[set] &&
                         maps->key[maps->key_off[m + 1] - 1] == 0 && maps->value[maps->key_off[m + 1] - 1] == (set == 1 ? 1 : 0);
                    mapped++;
                }
                if (withText && w.rt < 0) {
                    ok = ok && g.text_off == tnext;
                    for (int u = 0; u < w.len && ok; u++) ok = arena[g.text_off + (uint64_t)u] == Batch::unit_of(w.seq);
                    tnext += (uint64_t)w.len;
                }
                CHECK(ok, "query %zu (doc %u, [%d, %d), view %d/%d), record %llu differs", i, q.doc, q.s, q.e, q.r, q.c, (unsigned long long)k);
                removedSeen += w.rseq != INT32_MIN;
            }
            visited += n;
            insideHits += n > 0 && !q.su && !q.eu && q.s >= q.e;
        }
        CHECK(!withText || tnext == tunits, "text units %llu, records say %llu", (unsigned long long)tnext, (unsigned long long)tunits);
    }
    // NULL start / end / views: every visible row of the local view; the bounds
    {
        const mt_walk_rec* recs = nullptr; const uint64_t* roff = nullptr;
        CHECK(emu_walk_segments(c, 3, ids, nullptr, nullptr, nullptr, nullptr, 0, &recs, &roff, nullptr, nullptr) == MT_OK, "defaults");
        for (int d = 0; d < 3 && roff; d++) {
            size_t vis = 0;
            for (const Row& w : rows[d]) vis += view_len(w, 0, -1) > 0;
            CHECK(roff[d + 1] - roff[d] == vis, "document %d: %llu records, %zu visible rows", d, (unsigned long long)(roff[d + 1] - roff[d]), vis);
        }
        const int32_t big = (1 << 30) + 1, zero = 0;
        CHECK(emu_walk_segments(c, 1, ids, &big, &zero, nullptr, nullptr, 0, &recs, &roff, nullptr, nullptr) == MT_E_INVALID, "a start above 2^30 was taken");
        CHECK(emu_walk_segments(c, 1, ids, &zero, &zero, nullptr, nullptr, 2u, &recs, &roff, nullptr, nullptr) == MT_E_INVALID, "an unknown flag was taken");
    }
    CHECK(insideHits > 50, "%zu non-empty S >= E answers", insideHits);
    CHECK(removedSeen > 0, "no visited row the observer has removed");
    CHECK(mapped > 1000 && wideSeen > 0, "%zu records with a map, %zu maps of more than one chunk", mapped, wideSeen);
    emu_destroy(c);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    fprintf(stderr, "sanitize_walk: %zu queries with and without text (%zu records, %zu of them with a property map, %zu non-empty S >= E answers, %zu records of "
            "removed rows) equal to the rule, no sanitizer report\n", qs.size(), visited, mapped, insideHits, removedSeen);
    return 0;
}
