// sanitize_text.cpp — TEST-ONLY, beside sanitize_tiles.cpp: text ranges (mt_query.h: the scan's
// text kinds, mt_get_text_range) on the engine's host emulation under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a standalone executable.  Document 0 holds the known answers
// (rows "hello" | " " | "world", a marker, rows of 300, 64 and 65 units).  Document 1 is a random
// stream of three clients (text inserts, markers, removes; every insert's units are one letter
// chosen by its seq, so a row's text follows from mt_dump_segments alone), tall enough for
// several units.  Every kind: the local view and each client's view at its last refSeq (rows the
// observer removed are visible there), S <= E and S > E, placeholders of 0, 1, 3 and 16 units,
// the count and the fill pass, against the rule of include/mtgpu.h evaluated on the dump.  The
// output arena is released before every call, so each fill pass writes into a buffer of exactly
// the counted size and a store past it is reported.  Build + run: tests/emu/sanitize_text.sh
// (a report or a mismatch: non-zero status).
#include "mt_emu.cpp"

#include <stdio.h>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL: "); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

static bool same(const uint16_t* a, const uint16_t* b, size_t n) { return n == 0 || !memcmp(a, b, 2 * n); }

struct Batch {
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen;
    int s = 0;
    static uint16_t unit_of(int seq) { return (uint16_t)('a' + seq % 26); }
    void op(uint8_t ty, uint8_t fl, int cl, int a, int b, int units) {
        type.push_back(ty); flags.push_back((uint8_t)(MT_OPF_END_OF_MSG | fl)); client.push_back((uint16_t)cl);
        seq.push_back(s + 1); ref.push_back(s); msn.push_back(0); p1.push_back(a); p2.push_back(b); pid.push_back(-1);
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
// the rule of include/mtgpu.h
static std::vector<uint16_t> expected(const std::vector<Row>& rows, int r, int c, bool sUndef, int S, bool eUndef, int E,
                                      const std::vector<uint16_t>& ph) {
    std::vector<uint16_t> out;
    int L = 0;
    for (const Row& w : rows) L += view_len(w, r, c);
    const long s = sUndef ? 0 : S, e = eUndef ? L : E;
    long p = 0;
    for (const Row& w : rows) {
        const long l = view_len(w, r, c);
        if (e - p > 0 && l > 0 && s - p < l) {              // nodeMap's visit test (:2964)
            if (w.rt >= 0) out.insert(out.end(), ph.begin(), ph.end());
            else {
                long a = s - p < 0 ? 0 : s - p, b = e - p >= l ? l : e - p;
                if (a > b) { const long t = a; a = b; b = t; }      // substring swaps
                for (long k = a; k < b; k++) out.push_back(Batch::unit_of(w.seq));
            }
        }
        p += l;
    }
    return out;
}

int main() {
    Batch B[2];
    // document 0: the known answers
    B[0].op(MT_OP_INSERT, 0, 0, 0, 0, 5); B[0].op(MT_OP_INSERT, 0, 0, 5, 0, 1); B[0].op(MT_OP_INSERT, 0, 0, 6, 0, 5);
    B[0].op(MT_OP_INSERT, MT_OPF_MARKER, 0, 11, 1, 0);
    B[0].op(MT_OP_INSERT, 0, 0, 12, 0, 300); B[0].op(MT_OP_INSERT, 0, 0, 312, 0, 64); B[0].op(MT_OP_INSERT, 0, 0, 376, 0, 65);
    // document 1: random; ops at refSeq = seq - 1, so the writer sees the observer's length
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](int n) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (int)((lcg >> 33) % (uint64_t)n); };
    int len = 0, lastOp[3] = {0, 0, 0};
    for (int i = 0; i < 500; i++) {
        const int cl = rnd(3), x = rnd(100);
        if (x < 55 || len < 4) { const int n = 1 + rnd(12); B[1].op(MT_OP_INSERT, 0, cl, rnd(len + 1), 0, n); len += n; }
        else if (x < 70) { B[1].op(MT_OP_INSERT, MT_OPF_MARKER, cl, rnd(len + 1), 1, 0); len += 1; }
        else { const int a = rnd(len), w = a + 1 + rnd(15), b = w > len ? len : w; B[1].op(MT_OP_REMOVE, 0, cl, a, b, 0); len -= b - a; }
        lastOp[cl] = B[1].s;
    }
    std::vector<uint8_t> type, flags; std::vector<uint16_t> client, payload;
    std::vector<int32_t> seq, ref, msn, p1, p2, pid;
    std::vector<uint32_t> poff, plen;
    const uint32_t ids[2] = {0, 1};
    uint32_t off[3] = {0, 0, 0};
    for (int d = 0; d < 2; d++) {
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
    b.n_runs = 2; b.doc_ids = ids; b.op_offsets = off; b.n_ops = off[2]; b.type = type.data(); b.flags = flags.data();
    b.client = client.data(); b.seq = seq.data(); b.ref_seq = ref.data(); b.msn = msn.data(); b.pos1 = p1.data(); b.pos2 = p2.data();
    b.payload_off = poff.data(); b.payload_len = plen.data(); b.prop_id = pid.data(); b.payload = payload.data();
    b.payload_units = (uint32_t)payload.size();
    mt_limits L{}; L.max_docs = 2; L.rows_per_doc = 2048; L.blocks_per_doc = 1024; L.heap_per_doc = 2048; L.window_per_doc = 2048;
    L.text_per_doc = 8192; L.propsets_per_doc = 64;
    mt_ctx* c = nullptr;
    CHECK(emu_create(0, &L, &c) == MT_OK, "create");
    const char* np[3] = {"\"c0\"", "\"c1\"", "\"c2\""};
    emu_set_client_names(c, 3, np);
    CHECK(emu_docs_open(c, 0, 2) == MT_OK, "open");
    CHECK(emu_apply_batch(c, &b) == MT_OK, "apply: %s", emu_last_error(c));
    emu_sync(c);
    uint32_t st[2] = {1, 1}; int32_t pools[20];
    emu_doc_status(c, 2, ids, st);
    emu_doc_pools(c, 2, ids, pools);
    CHECK(st[0] == 0 && st[1] == 0, "status %#x %#x", st[0], st[1]);
    CHECK(pools[10 + 6] >= 2, "tree height %d", pools[10 + 6]);
    std::vector<Row> rows[2];
    for (int d = 0; d < 2; d++) {
        int32_t* dump = nullptr; uint32_t nr = 0;
        CHECK(emu_dump_segments(c, (uint32_t)d, &dump, &nr) == MT_OK, "dump");
        for (uint32_t i = 0; i < nr; i++) { const int32_t* r = dump + 12 * i; rows[d].push_back(Row{r[0], r[1], r[2], r[3], r[4], r[8]}); }
        emu_free(dump);
    }
    int Lobs = 0;
    for (const Row& w : rows[1]) Lobs += view_len(w, 0, -1);
    CHECK(Lobs == len, "document 1: L %d (%d)", Lobs, len);
    // mt_get_text is the local view without placeholders
    {
        const uint16_t* ta = nullptr; const uint64_t* to = nullptr;
        CHECK(emu_get_text(c, 2, ids, &ta, &to) == MT_OK, "get_text");
        for (int d = 0; d < 2; d++) {
            const auto want = expected(rows[d], 0, -1, true, 0, true, 0, {});
            CHECK(to[d + 1] - to[d] == want.size() && same(ta + to[d], want.data(), want.size()), "document %d: the dump's text differs from mt_get_text", d);
        }
    }
    // the queries of one call share a placeholder
    struct Q { uint32_t doc; bool su; int s; bool eu; int e; int r, c; };
    std::vector<Q> qs;
    auto grid = [&](uint32_t doc, int r, int cl, int Lv, int nrand) {
        const int edge[6] = {0, 1, Lv - 1, Lv, Lv + 3, 0};
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) qs.push_back(Q{doc, i == 5, edge[i], j == 5, edge[j], r, cl});
        for (int i = 0; i < nrand; i++) qs.push_back(Q{doc, false, rnd(Lv + 6) - 2, false, rnd(Lv + 6) - 2, r, cl});
        for (int i = 0; i < nrand; i++) { const int p = rnd(Lv + 1); qs.push_back(Q{doc, false, p + rnd(12), false, p - rnd(4), r, cl}); }
    };
    // document 0: hand-checked answers first (they pin the evaluator above), then a grid
    const int known[][2] = {{3, 8}, {-4, 3}, {6, 11}, {0, 0}, {11, 13}, {4, 2}, {8, 2}, {12, 11}, {311, 13}, {375, 313}, {376, 311}, {12, 441}};
    for (auto& k : known) qs.push_back(Q{0, false, k[0], false, k[1], -1, -1});
    grid(0, -1, -1, 441, 150);
    grid(1, -1, -1, Lobs, 200);
    int differing = 0;
    for (int cl = 0; cl < 3; cl++) {
        const int r = lastOp[cl] - 1;
        int Lv = 0, diff = 0;
        for (const Row& w : rows[1]) { Lv += view_len(w, r, cl); diff += view_len(w, r, cl) != view_len(w, 0, -1); }
        differing += diff > 0;
        grid(1, r, cl, Lv, 200);
        grid(1, B[1].s, cl, Lobs, 20);
    }
    CHECK(differing >= 1, "no client's view differs from the observer's");
    std::vector<uint32_t> qd; std::vector<int32_t> s, e, r, cl;
    for (const Q& q : qs) {
        qd.push_back(q.doc); s.push_back(q.su ? MT_POS_UNDEFINED : q.s); e.push_back(q.eu ? MT_POS_UNDEFINED : q.e);
        r.push_back(q.r); cl.push_back(q.c);
    }
    const std::vector<uint16_t> phs[4] = {{}, {' '}, {'<', 'm', '>'}, {'0', '1', '2', '3', '4', '5', '6', '7', '8', '9', 'a', 'b', 'c', 'd', 'e', 'f'}};
    size_t answered = 0, swappedHits = 0;
    for (const auto& ph : phs) {
        free(c->b_xout.p); c->b_xout = mt_ctx::DevBuf{};     // the fill pass gets a buffer of exactly the counted size
        const uint16_t* arena = nullptr; const uint64_t* aoff = nullptr;
        CHECK(emu_get_text_range(c, (uint32_t)qd.size(), qd.data(), s.data(), e.data(), r.data(), cl.data(), ph.data(), (uint32_t)ph.size(),
                                 &arena, &aoff) == MT_OK, "get_text_range: %s", emu_last_error(c));
        if (!arena) break;
        CHECK(c->b_xout.cap == 2 * aoff[qd.size()], "the arena is %zu bytes for %llu units", c->b_xout.cap, (unsigned long long)aoff[qd.size()]);
        for (size_t i = 0; i < qs.size(); i++) {
            const Q& q = qs[i];
            const auto want = expected(rows[q.doc], q.r, q.c, q.su, q.s, q.eu, q.e, ph);
            const uint64_t n = aoff[i + 1] - aoff[i];
            CHECK(n == want.size() && same(arena + aoff[i], want.data(), want.size()),
                  "query %zu (doc %u, [%d, %d), view %d/%d, placeholder %zu): %llu units, want %zu", i, q.doc, q.s, q.e, q.r, q.c, ph.size(),
                  (unsigned long long)n, want.size());
            answered += n > 0;
            swappedHits += n > 0 && !q.su && !q.eu && q.s > q.e;
        }
    }
    // the known answers of document 0, by hand: "hello world" + marker + 300 + 64 + 65 units
    {
        const uint16_t* arena = nullptr; const uint64_t* aoff = nullptr;
        const uint16_t star = '#';
        CHECK(emu_get_text_range(c, 12, qd.data(), s.data(), e.data(), r.data(), cl.data(), &star, 1, &arena, &aoff) == MT_OK, "known answers");
        const size_t want[12] = {5, 3, 5, 0, 2, 2, 0, 0, 298, 62, 0, 429};
        for (int i = 0; i < 12 && arena; i++) CHECK(aoff[i + 1] - aoff[i] == want[i], "known answer %d: %llu units, want %zu", i, (unsigned long long)(aoff[i + 1] - aoff[i]), want[i]);
        CHECK(arena && arena[aoff[4]] == '#' && arena[aoff[4] + 1] == Batch::unit_of(5), "a range starting on the marker");
    }
    // NULL start / end / views: the whole local text; a 17-unit placeholder is refused
    {
        const uint16_t* arena = nullptr; const uint64_t* aoff = nullptr;
        CHECK(emu_get_text_range(c, 2, ids, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &arena, &aoff) == MT_OK, "defaults");
        const uint16_t* ta = nullptr; const uint64_t* to = nullptr;
        CHECK(emu_get_text(c, 2, ids, &ta, &to) == MT_OK, "get_text");
        CHECK(aoff && to && aoff[2] == to[2] && aoff[1] == to[1] && same(arena, ta, to[2]), "the default range differs from mt_get_text");
        const uint16_t big[17] = {0};
        CHECK(emu_get_text_range(c, 2, ids, nullptr, nullptr, nullptr, nullptr, big, 17, &arena, &aoff) == MT_E_INVALID, "a 17-unit placeholder was taken");
    }
    CHECK(swappedHits > 50, "%zu non-empty S > E answers", swappedHits);
    emu_destroy(c);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    fprintf(stderr, "sanitize_text: %zu queries x 4 placeholders (%zu non-empty, %zu of them S > E) equal to the rule, no sanitizer report\n",
            qs.size(), answered, swappedHits);
    return 0;
}
