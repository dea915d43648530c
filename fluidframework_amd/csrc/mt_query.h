// mt_query.h — position queries on replayed documents (mt_get_containing_segment):
//   MergeTree.getContainingSegment        MT/mergeTree.ts:1616-1627 (searchBlock :1786-1815)
//   MergeTree.resolveRemoteClientPosition MT/mergeTree.ts:2125-2145
//   MergeTree.getPosition                 MT/mergeTree.ts:1578-1596 (the local view)
// and tile search (mt_find_tile, mt_tile_index) over a document-order scan of the rows:
//   MergeTree.findTile                    MT/mergeTree.ts:1752-1778 (search :1780-1820,
//                                         backwardSearch :1822-1866; the rule: include/mtgpu.h)
// and the range queries, two visitors of one scan of a range under any view (MtViewScan: enter,
// load a unit, advance; mt_scan_copy places a unit's text), which runs on the same cursor:
//   MergeTreeTextHelper.getText           MT/textSegment.ts:163-194 (gatherText :196-284, over
//                                         mapRange -> nodeMap MT/mergeTree.ts:2927-2994):
//                                         mt_get_text_range, each row's clip to the range
//   Client.walkSegments                   MT/client.ts:282-295 (mapRange -> nodeMap, as above):
//                                         mt_walk_segments, a record per visited row
// Batched: the host groups the queries by document, one wave takes a document's queries
// in order (the perspective's U set is reused while consecutive queries share it).  A
// query reads the document and writes only the wave's U scratch of that document; a tile
// query writes nothing of the document at all (its stack is the wave's LDS scratch), nor does
// a text range in the local view.
#pragma once
#include "mt_core.h"

// ref < 0 selects the query's kind: the local view, or a tile search (client: the label's
// index, with MT_QT_PRECEDING for findTile's `preceding`; pos: startPos, or the first record
// of the document for the index's fill pass)
#define MT_QK_LOCAL (-1)
#define MT_QK_TILE (-2)
#define MT_QK_TILE_COUNT (-3)
#define MT_QK_TILE_FILL (-4)
// a text range (mt_get_text_range): pos is the query's record (MtRangeQ) in MtQueryCall::q, which
// holds the range and the view; the count pass and the fill pass of the same scan
#define MT_QK_TEXT_COUNT (-5)
#define MT_QK_TEXT_FILL (-6)
// a segment walk (mt_walk_segments): pos is the query's record in MtQueryCall::q, as a text range's;
// the count pass and the fill pass of the same scan.  MT_QK_PSET: pos is a property-set id of the
// document, whose chunks are copied to MtQueryCall::maps from chunk `client` on (the walk's distinct
// maps, fetched after its fill; no answer record is written).
#define MT_QK_WALK_COUNT (-7)
#define MT_QK_WALK_FILL (-8)
#define MT_QK_PSET (-9)
#define MT_QT_PRECEDING 0x40000000
struct __attribute__((aligned(16))) MtQuery { uint32_t doc; int32_t pos, ref, client; };   // ref < 0: local view / kind
// One answer: the ABI record, where the found row's text sits in the text pool, and the
// chunks of its property map (the host writes the segment's JSON from them).
struct __attribute__((aligned(16))) MtQueryOut {
    mt_seg_info info;
    unsigned long long text_at;            // element index into MtState::text (text rows)
    unsigned long long pad;
    MtPSet ps[MT_PKEYS / MT_PSK];
};
// One range query, a text range or a segment walk: the range and the view as the caller gave them,
// where the answer goes (a text range's units, a walk's records), what the count pass found and
// what the fill pass wrote; the same three for a walk's text, which a text range leaves zero.
struct __attribute__((aligned(16))) MtRangeQ {
    int32_t start, end, ref, client;
    unsigned long long at, count, filled, tat, tcount, tfilled;
};
// What one launch of the query kernel needs beyond the pools: the kernel's second argument, by
// value, built by the ABI's entry point on its stack.  A query's kind says which members it reads;
// a member no kind of the launch reads stays zero.
struct MtQueryCall {
    // the tile kinds: the labels' match arrays ([label * nvalues + value id]), the key id of
    // "referenceTileLabels", and the index's record array (MT_QK_TILE_FILL; tile_cap records)
    const uint8_t* match; uint32_t key, nvalues;
    mt_tile_rec* tiles; unsigned long long tile_cap;
    // the range kinds: the query records (MtQuery::pos indexes them) and a walk's MT_WALK_* flags
    MtRangeQ* q; uint32_t nq, flags;
    // the placeholder a marker stands for in a text range (phlen <= 16 UTF-16 units, two a word)
    uint32_t phlen, ph[MT_TEXT_PLACEHOLDER_MAX / 2];
    // the fill passes' outputs: a text range's units or a walk's text (text_cap units), a walk's
    // records (rec_cap records); where MT_QK_PSET copies the maps, chunk by chunk (map_cap chunks)
    uint16_t* text; unsigned long long text_cap;
    mt_walk_rec* recs; unsigned long long rec_cap;
    MtPSet* maps; unsigned long long map_cap;
};
static_assert(sizeof(MtQueryCall) == 136, "MtQueryCall is 136 bytes of kernel arguments");
static_assert(sizeof(mt_seg_info) == 64, "mt_seg_info is 16 dwords");
static_assert(sizeof(mt_tile_rec) == 32, "mt_tile_rec is 8 dwords");
static_assert(sizeof(mt_walk_rec) == 64, "mt_walk_rec is 16 dwords");

/* ------------------------------------------------------- document-order scan -- */
// The rows of a document in document order, a unit at a time.  A unit is the up-to-64 rows
// under one block of height 1 (lane l: row l & 7 of leaf block l >> 3), or the root's up-to-8
// rows when the tree has height 0.  The cursor's stack (block, child index, observer start
// per level above the unit) lives in the wave's scratch (MtScratch::pathB / pathJ / pathOff).
// Control flow is wave-uniform; a unit's rows are lane data.
struct MtTileCursor {
    int U;           // the unit's block (-1: past either end)
    int lvl;         // stack levels above the unit
    int base;        // observer start of the unit
};
// One unit's rows: ids (-1: no row in that lane), the quads' fields, the visible lengths'
// exclusive scans (all rows / text rows only) and the candidate masks.
struct MtTileUnit {
    LaneArr<int> row, len, seq, rseq, toff, props, pre, tpre;
    LaneArr<uint32_t> meta;
    uint64_t present;    // lanes holding a row
    uint64_t cand;       // visible Tile markers
    uint64_t candAny;    // Tile markers, removed ones included
    int vis, tvis;       // the unit's visible length, and that of its text rows
    int height;          // the unit block's height (0: the root alone)
};
enum { MT_TD_POS = 0, MT_TD_FIRST_VIS, MT_TD_LAST_VIS, MT_TD_FIRST, MT_TD_LAST, MT_TD_PATH };

template <class Eng> MT_HD bool mt_tile_blk_ok(const Eng& e, int b) { return b >= 0 && b < e.blkTop; }
// Block B's children: the child count clamped to a block's room, the child ids, their observer
// lengths (0 for an id outside the document's blocks) and the lengths' exclusive scan.
template <class Eng>
MT_HD int mt_tile_children(Eng& e, int B, LaneArr<int>& ch, LaneArr<int>& lens, LaneArr<int>& pre) {
    BlkH h;
    ch = e.blkLoad(B, h);
    const int n = h.n < 0 ? 0 : (h.n > MT_MAXN ? MT_MAXN : h.n);
    const int top = e.blkTop;
    lens = wave_map(n, [&](int j) MT_LAM {
        const int b = own(ch, j);
        const bool ok = (b >= 0) & (b < top);
        return ok ? e.bk(ok ? b : 0).len : 0;
    });
    pre = wave_excl_scan8(lens);
    return n;
}

// Down from block B (observer start `base`) to a unit: at each level the child holding
// observer position P (MT_TD_POS; P < the block's length), the first / last child of non-zero
// observer length, the first / last child, or the child a containing() path names (MT_TD_PATH:
// `depth` levels from the root, 3 bits each, root first).  False: no such child (or a broken tree).
template <class Eng>
MT_HD bool mt_tile_down(Eng& e, MtTileCursor& c, int B, int base, int P, int mode, unsigned long long path = 0, int depth = 0) {
    for (;;) {
        if (!mt_tile_blk_ok(e, B)) { c.U = -1; return false; }
        if (uni(e.bk(B).height) <= 1) { c.U = B; c.base = base; return true; }
        if (c.lvl >= MT_MAXH + 1) { c.U = -1; return false; }
        LaneArr<int> ch, lens, pre;
        const int n = mt_tile_children(e, B, ch, lens, pre);
        int j;
        if (mode == MT_TD_POS) {
            const int p = P - base;
            j = wave_first(wave_map(n, [&](int k) MT_LAM { return p - own(pre, k) < own(lens, k); }));
        } else if (mode == MT_TD_FIRST_VIS || mode == MT_TD_LAST_VIS) {
            const uint64_t m = wave_ballot(wave_map(n, [&](int k) MT_LAM { return own(lens, k) > 0; }));
            j = !m ? -1 : (mode == MT_TD_FIRST_VIS ? __builtin_ctzll(m) : 63 - __builtin_clzll(m));
        } else if (mode == MT_TD_PATH) {
            j = depth - 1 - c.lvl >= 0 ? (int)((path >> (3 * (depth - 1 - c.lvl))) & 7ull) : -1;
        } else j = mode == MT_TD_FIRST ? 0 : n - 1;
        if (j < 0 || j >= n) { c.U = -1; return false; }
        e.sc->pathB[c.lvl] = B; e.sc->pathJ[c.lvl] = j; e.sc->pathOff[c.lvl] = base;
        wave_sync();
        c.lvl++;
        base += wave_at(pre, j);
        B = wave_at(ch, j);
    }
}
// The next unit to the right (dir > 0) or left (dir < 0) of the cursor's; all: every unit,
// else only units of non-zero observer length (a subtree of length 0 holds no visible row).
template <class Eng>
MT_HD bool mt_tile_next(Eng& e, MtTileCursor& c, int dir, bool all) {
    while (c.lvl > 0) {
        const int l = c.lvl - 1;
        const int B = uni(e.sc->pathB[l]), j = uni(e.sc->pathJ[l]), base = uni(e.sc->pathOff[l]);
        LaneArr<int> ch, lens, pre;
        const int n = mt_tile_children(e, B, ch, lens, pre);
        const uint64_t m = wave_ballot(wave_map(n, [&](int k) MT_LAM {
            return (((dir > 0) ? (k > j) : (k < j)) & ((own(lens, k) > 0) | all)) != 0;
        }));
        if (m) {
            const int k = dir > 0 ? __builtin_ctzll(m) : 63 - __builtin_clzll(m);
            e.sc->pathJ[l] = k;
            wave_sync();
            const int mode = dir > 0 ? (all ? MT_TD_FIRST : MT_TD_FIRST_VIS) : (all ? MT_TD_LAST : MT_TD_LAST_VIS);
            return mt_tile_down(e, c, wave_at(ch, k), base + wave_at(pre, k), 0, mode);
        }
        c.lvl--;
    }
    c.U = -1;
    return false;
}
// The row ids of the cursor's unit (-1: no row in that lane): each lane its leaf block's child
// id and count, every block and row id checked against the document's tops.
template <class Eng>
MT_HD LaneArr<int> mt_tile_unit_rows(Eng& e, const MtTileCursor& c, int& height, int& span) {
    BlkH h;
    const auto ch = e.blkLoad(c.U, h);
    height = h.height;
    const int U = c.U, hn = h.n < 0 ? 0 : (h.n > MT_MAXN ? MT_MAXN : h.n);
    const bool leafRoot = h.height == 0;
    const int nb = leafRoot ? 1 : hn;
    const auto blks = wave_map(8, [&](int j) MT_LAM { return leafRoot ? (j == 0 ? U : -1) : own(ch, j); });
    span = 8 * nb;
    const auto bsel = wave_gather8(blks);
    const int btop = e.blkTop, rtop = e.rowTop;
    return wave_map(span, [&](int t) MT_LAM {
        const int b = own(bsel, t);
        const bool ok = (b >= 0) & (b < btop);
        const int bb = ok ? b : 0;
        const int g = e.bk(bb).c[t & 7];
        return (ok & ((t & 7) < e.bk(bb).n) & (g >= 0) & (g < rtop)) ? g : -1;
    });
}
// Quad k of each row of a unit (len seq rseq meta | toff props parent tcap | ovl rcl mid), zero
// where the lane holds no row; lanes [0, span).
template <class Eng>
MT_HD LaneArr<MtQ16a> mt_unit_quad(Eng& e, const LaneArr<int>& row, int span, int k) {
    return wave_map(span, [&](int t) MT_LAM {
        const int g = own(row, t);
        return g >= 0 ? ((const MtQ16a*)&e.row(g))[k] : MtQ16a{0u, 0u, 0u, 0u};
    });
}
// Loads the cursor's unit: the row ids, then the row's first two quads, as scourLeaves does.
template <class Eng>
MT_HD void mt_tile_unit(Eng& e, const MtTileCursor& c, MtTileUnit& u) {
    int span = 0;
    u.row = mt_tile_unit_rows(e, c, u.height, span);
    const auto q0 = mt_unit_quad(e, u.row, span, 0), q1 = mt_unit_quad(e, u.row, span, 1);
    u.len = wave_map(span, [&](int t) MT_LAM { return (int)own(q0, t).x; });
    u.seq = wave_map(span, [&](int t) MT_LAM { return (int)own(q0, t).y; });
    u.rseq = wave_map(span, [&](int t) MT_LAM { return (int)own(q0, t).z; });
    u.meta = wave_map(span, [&](int t) MT_LAM { return own(q0, t).w; });
    u.toff = wave_map(span, [&](int t) MT_LAM { return (int)own(q1, t).x; });
    u.props = wave_map(span, [&](int t) MT_LAM { return (int)own(q1, t).y; });
    u.present = wave_ballot(wave_map(span, [&](int t) MT_LAM { return own(u.row, t) >= 0; }));
    // the candidate test, branch-free per lane: marker, refType & Tile, not removed
    u.candAny = wave_ballot(wave_map(span, [&](int t) MT_LAM {
        return ((own(u.row, t) >= 0) & ((own(u.meta, t) & MT_M_MARKER) != 0) & ((own(u.toff, t) & 1) != 0)) != 0;
    }));
    u.cand = u.candAny & wave_ballot(wave_map(span, [&](int t) MT_LAM { return (own(u.meta, t) & MT_M_REMOVED) == 0; }));
    const auto vl = wave_map(span, [&](int t) MT_LAM {
        return ((own(u.row, t) >= 0) & ((own(u.meta, t) & MT_M_REMOVED) == 0)) ? own(u.len, t) : 0;
    });
    const auto tl = wave_map(span, [&](int t) MT_LAM { return (own(u.meta, t) & MT_M_MARKER) ? 0 : own(vl, t); });
    u.pre = wave_excl_scan(vl);
    u.tpre = wave_excl_scan(tl);
    u.vis = wave_sum(vl);
    u.tvis = wave_sum(tl);
}

// Does property map `ps` yield label `lab`?  The wave reads the map one key per lane, in
// rounds of 64, looks for the key id of "referenceTileLabels" and tests that key's value id
// against the label's match array.  Maps are immutable and shared between segments: the last
// map tested and its result are remembered (wave-uniform).
struct MtTileMemo { int lab, ps; bool res; };
template <class Eng>
MT_HD bool mt_tile_map_has(Eng& e, const MtQueryCall& call, int ps, int lab, MtTileMemo& memo) {
    if (ps < 0 || ps >= e.psetTop) return false;
    if (memo.ps == ps && memo.lab == lab) return memo.res;
    int n = uni(e.pset[ps].n);
    const int room = (e.psetTop - ps) * MT_PSK;
    n = n < 0 ? 0 : (n > MT_PKEYS ? MT_PKEYS : n);
    n = n > room ? room : n;
    const int key = (int)call.key;
    const uint32_t nv = call.nvalues;
    const uint8_t* mrow = call.match + (size_t)lab * nv;
    bool res = false;
    for (int base = 0; base < n && !res; base += MT_WAVE) {
        const int m = (n - base) < MT_WAVE ? (n - base) : MT_WAVE;
        res = wave_ballot(wave_map(m, [&](int k) MT_LAM {
            const int v = e.pval(ps, base + k);
            const bool q = (e.pkey(ps, base + k) == key) & (v >= 0) & ((uint32_t)v < nv);
            return (q & (mrow[q ? v : 0] != 0)) != 0;
        })) != 0;
    }
    memo.ps = ps; memo.lab = lab; memo.res = res;
    return res;
}

// The nch chunks of property map ps to `to`, one dword per lane (28 dwords a chunk).  The caller
// has checked that the chunks lie in the document's maps and fit at `to`.
template <class Eng>
MT_HD void mt_copy_pset(Eng& e, MtPSet* to, int ps, int nch) {
    constexpr int W = (int)(sizeof(MtPSet) / 4);
    for (int base = 0; base < nch * W; base += MT_WAVE) {
        const int m = (nch * W - base) < MT_WAVE ? (nch * W - base) : MT_WAVE;
        wave_for(m, [&](int k) MT_LAM { ((int*)to)[base + k] = ((const int*)(e.pset + ps))[base + k]; });
    }
    wave_sync();
}

// One answer record (the 16 dwords of mt_seg_info, the row's text, its map's chunks): row s
// found at `off` into it with observer start op; s < 0: not found, `resolved` as given.
template <class Eng>
MT_HD void mt_query_emit(Eng& e, const MtState& S, MtQueryOut& o, int s, int off, int op, int depth,
                         unsigned long long path, int resolved) {
    int f[16];
    for (int k = 0; k < 16; k++) f[k] = 0;
    unsigned long long tat = 0;
    int nch = 0, ps = -1;
    if (s >= 0) {
        const uint32_t mt = uni(e.row(s).meta);
        const bool removed = (mt & MT_M_REMOVED) != 0, marker = (mt & MT_M_MARKER) != 0;
        const int cl = (int)(mt & MT_M_CLIENT);
        ps = uni(e.row(s).props);
        f[0] = 1; f[1] = off; f[2] = op; f[3] = uni(e.row(s).len); f[4] = uni(e.row(s).seq);
        f[5] = cl == MT_NONCOLLAB ? -1 : cl;
        f[6] = removed ? uni(e.row(s).rseq) : (int)0x80000000;
        f[7] = removed ? (int)uni(e.row(s).rcl) : -1;
        f[8] = ps; f[9] = marker ? uni(e.row(s).toff) : -1;
        f[10] = depth; f[11] = (int)(uint32_t)path; f[12] = (int)(uint32_t)(path >> 32);
        f[13] = s; f[14] = op + off;
        if (!marker) tat = (unsigned long long)(e.text - S.text) + (unsigned long long)uni(e.row(s).toff);
        if (ps >= 0) { const int n = uni(e.pset[ps].n); nch = n > MT_PSK ? (n + MT_PSK - 1) / MT_PSK : 1; }
    } else {
        f[1] = -1; f[2] = -1; f[5] = -1; f[6] = (int)0x80000000; f[7] = -1; f[8] = -1; f[9] = -1; f[13] = -1;
        f[14] = resolved;
    }
    const auto fv = wave_map(16, [&](int k) MT_LAM { return pick16(f, k); });
    wave_for(16, [&](int k) MT_LAM { ((int*)&o.info)[k] = own(fv, k); });
    wave_for(1, [&](int) MT_LAM { o.text_at = tat; o.pad = 0; });
    mt_copy_pset(e, o.ps, ps, nch);
}

// The tree path of lane t of the cursor's unit, root first, 3 bits a level (as containing's).
template <class Eng>
MT_HD unsigned long long mt_tile_path(Eng& e, const MtTileCursor& c, const MtTileUnit& u, int t, int& depth) {
    unsigned long long path = 0;
    for (int l = 0; l < c.lvl; l++) path = (path << 3) | (unsigned long long)(uni(e.sc->pathJ[l]) & 7);
    depth = c.lvl + 1;
    if (u.height != 0) { path = (path << 3) | (unsigned long long)(t >> 3); depth++; }
    return (path << 3) | (unsigned long long)(t & 7);
}

// findTile (the rule: include/mtgpu.h).  Returns the row (-1: undefined) with its observer
// start, depth and path.
template <class Eng>
MT_HD int mt_find_tile_doc(Eng& e, const MtQueryCall& call, int pos, int lab, bool preceding, MtTileMemo& memo, int& op, int& depth,
                           unsigned long long& path) {
    if (!mt_tile_blk_ok(e, e.root)) return -1;
    const int L = uni(e.bk(e.root).len);
    const bool undef = pos == (int)0x80000000;
    MtTileCursor c; c.U = -1; c.lvl = 0; c.base = 0;
    MtTileUnit u;
    if (!preceding && !undef && pos >= L) {
        if (pos > L) return -1;
        // the leaf is the document's last row (`pos >= segpos` holds for every row): the
        // answer if it matches, removed or not (MT/mergeTree.ts:1841-1855, :993-1007)
        if (!mt_tile_down(e, c, e.root, 0, 0, MT_TD_LAST)) return -1;
        for (;;) {
            mt_tile_unit(e, c, u);
            if (u.present) break;
            if (!mt_tile_next(e, c, -1, true)) return -1;
        }
        const int t = 63 - __builtin_clzll(u.present);
        if (!((u.candAny >> t) & 1ull) || !mt_tile_map_has(e, call, wave_at(u.props, t), lab, memo)) return -1;
        op = c.base + wave_at(u.pre, t);
        path = mt_tile_path(e, c, u, t, depth);
        return wave_at(u.row, t);
    }
    if (L <= 0) return -1;                          // no visible row
    const int dir = preceding ? -1 : 1;
    // the unit holding the start position; every comparison with an undefined pos is false
    const int at = preceding ? ((undef || pos >= L) ? L - 1 : pos) : (undef ? 0 : pos);
    const int lim = preceding ? ((undef || pos >= L) ? 0x7FFFFFFF : pos) : (undef ? 0 : pos);
    if (!mt_tile_down(e, c, e.root, 0, at, MT_TD_POS)) return -1;
    for (;;) {
        mt_tile_unit(e, c, u);
        const int ub = c.base;
        uint64_t m = u.cand & wave_ballot(wave_map(MT_WAVE, [&](int t) MT_LAM {
            const int st = ub + own(u.pre, t);
            return dir < 0 ? st <= lim : st >= lim;
        }));
        while (m) {                                 // candidates nearest first
            const int t = dir < 0 ? 63 - __builtin_clzll(m) : __builtin_ctzll(m);
            m &= ~(1ull << t);
            if (mt_tile_map_has(e, call, wave_at(u.props, t), lab, memo)) {
                op = ub + wave_at(u.pre, t);
                path = mt_tile_path(e, c, u, t, depth);
                return wave_at(u.row, t);
            }
        }
        if (!mt_tile_next(e, c, dir, false)) return -1;
    }
}

// The tile index of one document: every visible matching tile in document order.  out null:
// count only.  Returns the count; records go to out[0 .. count), as far as `room` reaches.
template <class Eng>
MT_HD int mt_tile_index_doc(Eng& e, const MtQueryCall& call, int lab, MtTileMemo& memo, mt_tile_rec* out, unsigned long long room) {
    if (!mt_tile_blk_ok(e, e.root) || uni(e.bk(e.root).len) <= 0) return 0;
    MtTileCursor c; c.U = -1; c.lvl = 0; c.base = 0;
    MtTileUnit u;
    int cnt = 0, tbase = 0;
    if (!mt_tile_down(e, c, e.root, 0, 0, MT_TD_FIRST_VIS)) return 0;
    for (;;) {
        mt_tile_unit(e, c, u);
        uint64_t m = u.cand, hit = 0;
        while (m) {
            const int t = __builtin_ctzll(m);
            m &= ~(1ull << t);
            if (mt_tile_map_has(e, call, wave_at(u.props, t), lab, memo)) hit |= 1ull << t;
        }
        if (hit && out) {
            const int ub = c.base, tb = tbase, c0 = cnt;
            wave_for(MT_WAVE, [&](int t) MT_LAM {
                const unsigned long long k = (unsigned long long)c0 + (unsigned long long)__builtin_popcountll(hit & ((1ull << t) - 1ull));
                if (((hit >> t) & 1ull) && k < room) {      // guards the stores only
                    const int g = own(u.row, t);
                    mt_tile_rec r;
                    r.pos = ub + own(u.pre, t); r.text_pos = tb + own(u.tpre, t); r.row = g; r.prop_set = own(u.props, t);
                    r.ref_type = own(u.toff, t); r.marker_id = e.row(g).mid - 1; r.pad[0] = 0; r.pad[1] = 0;
                    out[k] = r;
                }
            });
        }
        cnt += __builtin_popcountll(hit);
        tbase += u.tvis;
        if (!mt_tile_next(e, c, 1, false)) return cnt;
    }
}

/* ------------------------------------------------------------- range scan -- */
// The rows of a range [lo, end) of a view, in document order, a unit at a time: the one scan under
// mt_get_text_range and mt_walk_segments, which differ in what they do with a unit's rows.  A
// unit's rows are lane data: each row's length under the view (vis_rc, branch-free per lane,
// DESIGN.md §4) and the exclusive scan that places it in the view.
// The view of a query's (ref, client): true for the local one, every sequenced op applied
// (removals included), as (refSeq = max, a client id no row carries) sees it.
MT_INLINE bool mt_view_of(int ref, int qc, int& r, int& c) {
    const bool local = ref < 0;
    r = local ? 0x7FFFFFFF : ref;
    c = (local || qc < 0 || qc >= MT_NONCOLLAB) ? MT_NOBODY : qc;
    return local;
}
struct MtViewScan {
    MtTileCursor cur;
    bool local;
    int r, c;            // the view
    int pos;             // the view position the cursor's unit starts at
    int s0;              // remote, until the first unit is loaded: the row containing() found (pos: that row's start)
};
struct MtScanUnit {
    LaneArr<int> row, vl, pre;       // row ids (-1: none), lengths under the view, their exclusive scan
    LaneArr<MtQ16a> q0, q1, q2;      // the rows' quads (mt_unit_quad); q2 zero where it was not asked for
    int span, vsum;                  // lanes, and the unit's length under the view
    int ub, ob;                      // the unit's start in the view, and in the observer's (the cursor's base)
};
// Puts the cursor on the unit holding view position lo.  False: the view holds no such position.
template <class Eng>
MT_HD bool mt_scan_enter(Eng& e, MtViewScan& s, bool local, int r, int c, int lo) {
    s.cur.U = -1; s.cur.lvl = 0; s.cur.base = 0;
    s.local = local; s.r = r; s.c = c; s.pos = 0; s.s0 = -1;
    if (local) {
        // the observer's lengths are the view's: subtrees of length 0 hold nothing
        if (lo >= uni(e.bk(e.root).len)) return false;
        if (!mt_tile_down(e, s.cur, e.root, 0, lo, MT_TD_POS)) return false;
        s.pos = s.cur.base;
        return true;
    }
    // one descent under the view (it computes U once); the cursor is rebuilt from its path
    int off = 0, depth = 0;
    unsigned long long path = 0;
    s.s0 = e.containing(lo, r, c, off, depth, path);
    s.pos = lo - off;
    return s.s0 >= 0 && mt_tile_down(e, s.cur, e.root, 0, 0, MT_TD_PATH, path, depth);
}
// Loads the cursor's unit.  The third quad is read for a remote view (vis_rc needs it) or where
// the caller asks for it.  False: the first unit does not hold the row containing() found.
template <class Eng>
MT_HD bool mt_scan_unit(Eng& e, MtViewScan& s, MtScanUnit& u, bool third) {
    int height = 0;
    u.row = mt_tile_unit_rows(e, s.cur, height, u.span);
    const int span = u.span, r = s.r, c = s.c;
    const bool local = s.local;
    u.q0 = mt_unit_quad(e, u.row, span, 0);
    u.q1 = mt_unit_quad(e, u.row, span, 1);
    u.q2 = mt_unit_quad(e, u.row, (third || !local) ? span : 0, 2);
    u.vl = wave_map(span, [&](int t) MT_LAM {
        const MtQ16a a = own(u.q0, t), x = own(u.q2, t);
        const int g = own(u.row, t), l = (int)a.x;
        const unsigned long long ovl = (unsigned long long)x.x | ((unsigned long long)x.y << 32);
        const bool vis = local ? (a.w & MT_M_REMOVED) == 0 : vis_rc((int)a.y, a.w, (int)a.z, x.z, ovl, r, c, e.ovx, e.ovxN, g);
        return ((g >= 0) & vis & (l > 0)) ? l : 0;
    });
    u.pre = wave_excl_scan(u.vl);
    u.vsum = wave_sum(u.vl);
    if (s.s0 >= 0) {                                // the first unit's start under the view, from the row containing() found
        const int s0 = s.s0;
        const int t0 = wave_first(wave_map(span, [&](int t) MT_LAM { return own(u.row, t) == s0; }));
        if (t0 < 0) return false;
        s.pos -= wave_at(u.pre, t0);
        s.s0 = -1;
    }
    u.ub = s.pos; u.ob = s.cur.base;
    return true;
}
// Past a unit of length vsum under the view.  False: the view position reached `end`, or no unit follows.
template <class Eng>
MT_HD bool mt_scan_next(Eng& e, MtViewScan& s, int vsum, int end) {
    s.pos += vsum;
    if (s.pos >= end) return false;
    if (!mt_tile_next(e, s.cur, 1, !s.local)) return false;     // remote: a row the observer removed may be visible
    if (s.local) s.pos = s.cur.base;
    return true;
}
// A unit's output: row t gives olen[t] UTF-16 units (opre: their exclusive scan, T: their sum),
// the document's text from index src[t] on, or for src[t] == -1 the placeholder in the words phw.
// One lane per *output* unit in rounds of 64: the lane finds its row by a binary search of the
// inclusive output scan (kept in the wave's scratch), so the stores are contiguous and one long
// row costs what many short ones do.  Units go to out[at .. at + T), as far as `room` reaches.
template <class Eng>
MT_HD void mt_scan_copy(Eng& e, const LaneArr<int>& olen, const LaneArr<int>& opre, int T, const LaneArr<int>& src,
                        const int* phw, uint16_t* out, unsigned long long at, unsigned long long room) {
    const int ttop = e.textTop;
    wave_for(MT_WAVE, [&](int t) MT_LAM {
        e.sc->hold[t] = own(opre, t) + own(olen, t);
        e.sc->holdLen[t] = own(src, t);
    });
    wave_sync();
    for (int base = 0; base < T; base += MT_WAVE) {
        const int m = (T - base) < MT_WAVE ? (T - base) : MT_WAVE;
        const unsigned long long d0 = at + (unsigned long long)base;
        wave_for(m, [&](int k) MT_LAM {
            const int j = base + k;
            int t = 0;                              // the first row whose inclusive end passes j
            for (int step = 32; step; step >>= 1) t += (e.sc->hold[t + step - 1] <= j) ? step : 0;
            const int before = e.sc->hold[t ? t - 1 : 0];
            const int kk = j - (t ? before : 0), sx = e.sc->holdLen[t];
            // the text index clamped to the live half's top; stores bounded by the answer's room
            int ti = sx + kk;
            ti = ti >= ttop ? ttop - 1 : ti;
            ti = ti < 0 ? 0 : ti;
            const bool tx = ((sx >= 0) & (ttop > 0)) != 0;
            const uint32_t w = (uint32_t)pick8(phw, (kk >> 1) & 7);
            const uint16_t v = tx ? e.text[ti] : (uint16_t)((kk & 1) ? (w >> 16) : (w & 0xFFFFu));
            if (d0 + (unsigned long long)k < room) out[d0 + (unsigned long long)k] = v;
        });
    }
    wave_sync();
}

/* ------------------------------------------------------------ text ranges -- */
// getText(refSeq, clientId, placeholder, start, end) of one document (the rule: include/mtgpu.h)
// as a visitor of the range scan, entered at the unit holding the range's start: each row's clip
// to the range and a second scan over the output lengths.  out null: count only.  Returns the
// answer's length; units go to out[0 .. length), as far as `room` reaches.
template <class Eng>
MT_HD unsigned long long mt_text_range_doc(Eng& e, const MtQueryCall& call, int start, int end, int ref, int qc, uint16_t* out,
                                           unsigned long long room) {
    if (!mt_tile_blk_ok(e, e.root)) return 0;
    const int E = end == (int)0x80000000 ? 0x7FFFFFFF : end;       // undefined: the view's length
    // S > E: substring swaps, and only a text row holding both ends strictly inside answers;
    // it is the row holding E, so the scan enters there and ends with that unit
    const bool swapped = start > E;
    const int lo = swapped ? E : (start < 0 ? 0 : start), hi = swapped ? start : E;
    if (swapped ? lo <= 0 : hi <= lo) return 0;
    int r, c;
    const bool local = mt_view_of(ref, qc, r, c);
    const int plen = call.phlen > MT_TEXT_PLACEHOLDER_MAX ? MT_TEXT_PLACEHOLDER_MAX : (int)call.phlen;
    static_assert(MT_TEXT_PLACEHOLDER_MAX == 16, "the placeholder is picked from eight words");
    MtViewScan sc;
    MtScanUnit u;
    if (!mt_scan_enter(e, sc, local, r, c, lo)) return 0;
    unsigned long long done = 0;
    do {
        if (!mt_scan_unit(e, sc, u, false)) return 0;
        const int ub = u.ub;
        // output units per row: the clip of [p, p + l) to [lo, hi); a marker 0 or the placeholder
        const auto olen = wave_map(u.span, [&](int t) MT_LAM {
            const int p = ub + own(u.pre, t), l = own(u.vl, t);
            const bool marker = (own(u.q0, t).w & MT_M_MARKER) != 0;
            const int a = lo > p ? lo : p, b = hi < p + l ? hi : p + l;
            const bool one = ((p < lo) & (hi < p + l) & !marker) != 0;
            const int n = swapped ? (one ? hi - lo : 0) : (b > a ? b - a : 0);
            return marker ? (n > 0 ? plen : 0) : n;
        });
        const auto opre = wave_excl_scan(olen);
        const int T = wave_sum(olen);
        if (out && T > 0) {
            // each row's first source unit (-1: the placeholder)
            const auto src = wave_map(MT_WAVE, [&](int t) MT_LAM {
                const int p = ub + own(u.pre, t);
                const bool marker = (own(u.q0, t).w & MT_M_MARKER) != 0;
                return marker ? -1 : (int)own(u.q1, t).x + ((lo > p ? lo : p) - p);
            });
            mt_scan_copy(e, olen, opre, T, src, (const int*)call.ph, out, done, room);
        }
        done += (unsigned long long)T;
    } while (!swapped && mt_scan_next(e, sc, u.vsum, hi));
    return done;
}

/* ---------------------------------------------------------- segment walks -- */
// walkSegments(handler, start, end) of one document under a view (the rule: include/mtgpu.h), a
// visitor of the range scan with nodeMap's visit test (:2964) as lane data:
// E - p > 0 && l > 0 && S - p < l, p from the exclusive scan of the lengths under the
// view.  For S < E the first visited row holds max(S, 0) and the scan runs until the view
// position reaches E; for S >= E the one row that can pass holds E, and the scan ends with its
// unit.  A visited row's record goes to rec[popcount of the visited lanes before it]; its
// obs_pos is the unit's observer start (the cursor's base, kept by every descent mode) plus the
// exclusive scan of the observer's lengths, which in the local view is p itself.  With text, the
// visited text rows' whole texts follow each other in the arena.  rec null: count only.  Returns
// the records; tcount: the text units.  Stores reach rec[0 .. room) and txt[0 .. troom) only;
// tat: where txt starts in the call's arena (a record's text_off is absolute).
template <class Eng>
MT_HD unsigned long long mt_walk_doc(Eng& e, const MtQueryCall& call, int start, int end, int ref, int qc, bool text, mt_walk_rec* rec,
                                     unsigned long long room, uint16_t* txt, unsigned long long tat, unsigned long long troom,
                                     unsigned long long& tcount) {
    tcount = 0;
    if (!mt_tile_blk_ok(e, e.root)) return 0;
    int r, c;
    const bool local = mt_view_of(ref, qc, r, c);
    const int Sx = start == (int)0x80000000 ? 0 : start;
    int E = end;
    if (end == (int)0x80000000) E = local ? uni(e.bk(e.root).len) : e.perspectiveLength(r, c);   // undefined: L
    if (E <= 0) return 0;
    const bool one = Sx >= E;                       // at most one row, the one holding E
    MtViewScan sc;
    MtScanUnit u;
    if (!mt_scan_enter(e, sc, local, r, c, one ? E : (Sx < 0 ? 0 : Sx))) return 0;
    unsigned long long done = 0, tdone = 0;
    do {
        if (!mt_scan_unit(e, sc, u, true)) return 0;
        const int span = u.span, ub = u.ub, ob = u.ob;
        // the observer's lengths: the view's own in the local view
        const auto opos = local ? u.pre : wave_excl_scan(wave_map(span, [&](int t) MT_LAM {
            const MtQ16a a = own(u.q0, t);
            return ((own(u.row, t) >= 0) & ((a.w & MT_M_REMOVED) == 0) & ((int)a.x > 0)) ? (int)a.x : 0;
        }));
        const uint64_t hit = wave_ballot(wave_map(span, [&](int t) MT_LAM {
            const int p = ub + own(u.pre, t), l = own(u.vl, t);
            return ((E - p > 0) & (l > 0) & (Sx - p < l)) != 0;     // :2964
        }));
        // text units per visited row: a text row's whole text
        const auto olen = wave_map(span, [&](int t) MT_LAM {
            const bool marker = (own(u.q0, t).w & MT_M_MARKER) != 0;
            return (text & ((hit >> t) & 1ull) & !marker) ? own(u.vl, t) : 0;
        });
        const auto opre = wave_excl_scan(olen);
        const int T = wave_sum(olen);
        if (rec && hit) {
            const unsigned long long d0 = done, t0 = tat + tdone;
            wave_for(span, [&](int t) MT_LAM {
                const unsigned long long k = d0 + (unsigned long long)__builtin_popcountll(hit & ((1ull << t) - 1ull));
                if (((hit >> t) & 1ull) && k < room) {          // guards the stores only
                    const MtQ16a a = own(u.q0, t), b = own(u.q1, t), x = own(u.q2, t);
                    const bool removed = (a.w & MT_M_REMOVED) != 0, marker = (a.w & MT_M_MARKER) != 0;
                    const int cl = (int)(a.w & MT_M_CLIENT), p = ub + own(u.pre, t);
                    mt_walk_rec w;
                    w.pos = p; w.start = Sx - p; w.end = E - p; w.len = (int)a.x;
                    w.seq = (int)a.y; w.client = cl == MT_NONCOLLAB ? -1 : cl;
                    w.removed_seq = removed ? (int)a.z : (int)0x80000000; w.removed_client = removed ? (int)x.z : -1;
                    // map: the map's key count for now (the host places the maps' chunks by it, then
                    // writes the map's index there)
                    const int ps = (int)b.y;
                    w.prop_set = ps; w.map = (ps >= 0 && ps < e.psetTop) ? e.pset[ps].n : -1;
                    w.marker_ref_type = marker ? (int)b.x : -1; w.marker_id = (int)x.w - 1;
                    w.row = own(u.row, t); w.obs_pos = ob + own(opos, t);
                    w.text_off = (text && !marker) ? t0 + (unsigned long long)own(opre, t) : 0ull;
                    rec[k] = w;
                }
            });
        }
        if (txt && T > 0) {
            // each row's first source unit: a visited text row's toff (no row asks for the placeholder)
            const auto src = wave_map(MT_WAVE, [&](int t) MT_LAM { return (int)own(u.q1, t).x; });
            mt_scan_copy(e, olen, opre, T, src, (const int*)call.ph, txt, tdone, troom);
        }
        done += (unsigned long long)__builtin_popcountll(hit);
        tdone += (unsigned long long)T;
    } while (!one && mt_scan_next(e, sc, u.vsum, E));
    tcount = tdone;
    return done;
}
// The chunks of property map ps of the document to maps[dst ..), as far as the map lies below
// the document's top and the chunks below mcap (else nothing is copied).
template <class Eng>
MT_HD void mt_query_pset(Eng& e, MtPSet* maps, unsigned long long mcap, int ps, int dst) {
    if (!maps || dst < 0 || ps < 0 || ps >= e.psetTop) return;
    int n = uni(e.pset[ps].n);
    n = n < 0 ? 0 : (n > MT_PKEYS ? MT_PKEYS : n);
    const int nch = n > MT_PSK ? (n + MT_PSK - 1) / MT_PSK : 1;
    if (nch > e.psetTop - ps || (unsigned long long)dst + (unsigned long long)nch > mcap) return;
    mt_copy_pset(e, maps + dst, ps, nch);
}

template <class Eng>
MT_HD void mt_query_run(Eng& e, const MtState& S, const MtQueryCall& call, const MtQuery* q, uint32_t q0, uint32_t q1, MtQueryOut* out) {
    MtTileMemo memo; memo.lab = -1; memo.ps = -1; memo.res = false;
    for (uint32_t i = q0; i < q1; i++) {
        const int pos = uni(q[i].pos), ref = uni(q[i].ref), qc = uni(q[i].client);
        if (ref == MT_QK_PSET) { mt_query_pset(e, call.maps, call.map_cap, pos, qc); continue; }
        if (ref <= MT_QK_TEXT_COUNT) {              // a range kind: its record holds the query and takes the counts
            if (!call.q || (uint32_t)pos >= call.nq) continue;
            MtRangeQ* xp = &call.q[(uint32_t)pos];
            const bool walk = ref <= MT_QK_WALK_COUNT, fill = ref == MT_QK_WALK_FILL || ref == MT_QK_TEXT_FILL;
            const bool text = !walk || (call.flags & MT_WALK_TEXT) != 0;
            const unsigned long long at = uni64(xp->at), cap = uni64(xp->count);
            // the text: a text range's answer, at `at`; a walk's rows' texts, at the record's tat
            const unsigned long long tat = walk ? uni64(xp->tat) : at, tcap = walk ? uni64(xp->tcount) : cap;
            unsigned long long troom = (fill && text && call.text && tat < call.text_cap) ? call.text_cap - tat : 0ull;
            troom = troom < tcap ? troom : tcap;
            uint16_t* txt = troom ? call.text + tat : nullptr;
            if (!walk) {
                const unsigned long long cnt = mt_text_range_doc(e, call, uni(xp->start), uni(xp->end), uni(xp->ref), uni(xp->client),
                                                                 txt, troom);
                wave_for(1, [&](int) MT_LAM { if (fill) xp->filled = cnt; else xp->count = cnt; });
                wave_sync();
                continue;
            }
            unsigned long long room = (fill && call.recs && at < call.rec_cap) ? call.rec_cap - at : 0ull;
            room = room < cap ? room : cap;
            unsigned long long tcnt = 0;
            const unsigned long long cnt = mt_walk_doc(e, call, uni(xp->start), uni(xp->end), uni(xp->ref), uni(xp->client), text,
                                                       room ? call.recs + at : nullptr, room, txt, tat, troom, tcnt);
            wave_for(1, [&](int) MT_LAM {
                if (fill) { xp->filled = cnt; xp->tfilled = tcnt; } else { xp->count = cnt; xp->tcount = tcnt; }
            });
            wave_sync();
            continue;
        }
        if (ref <= MT_QK_TILE) {                    // tile search: the local view, nothing written to the document
            const int lab = qc & (MT_QT_PRECEDING - 1);
            if (ref == MT_QK_TILE) {
                int op = 0, depth = 0;
                unsigned long long path = 0;
                const int s = mt_find_tile_doc(e, call, pos, lab, (qc & MT_QT_PRECEDING) != 0, memo, op, depth, path);
                mt_query_emit(e, S, out[i], s, 0, op, depth, path, (int)0x80000000);
            } else {
                const bool fill = ref == MT_QK_TILE_FILL;
                const unsigned long long at = fill ? (unsigned long long)(uint32_t)pos : 0ull;
                const unsigned long long room = (fill && call.tiles && at < call.tile_cap) ? call.tile_cap - at : 0ull;
                const int cnt = mt_tile_index_doc(e, call, lab, memo, room ? call.tiles + at : nullptr, room);
                MtQueryOut& o = out[i];
                wave_for(16, [&](int k) MT_LAM { ((int*)&o.info)[k] = k == 0 ? cnt : 0; });
                wave_sync();
            }
            continue;
        }
        int r, c;
        mt_view_of(ref, qc, r, c);
        int off = 0, depth = 0;
        unsigned long long path = 0;
        const int s = e.containing(pos, r, c, off, depth, path);
        int op = 0, resolved = 0;
        if (s >= 0) op = e.obsPosition(s);
        else {
            // resolveRemoteClientPosition's fall-through: the end of the remote view maps to the
            // end of the local one
            const int L = e.perspectiveLength(r, c);
            resolved = pos == L ? uni(e.bk(e.root).len) : (int)0x80000000;
        }
        mt_query_emit(e, S, out[i], s, off, op, depth, path, resolved);
    }
}
// The form without a record, as backend sources written before MtQueryCall call it: only position
// queries are answered (they read no member of the record; every other kind finds none).
template <class Eng>
[[deprecated("pass the call's MtQueryCall")]] MT_HD void mt_query_run(Eng& e, const MtState& S, const MtQuery* q, uint32_t q0,
                                                                      uint32_t q1, MtQueryOut* out) {
    mt_query_run(e, S, MtQueryCall{}, q, q0, q1, out);
}
