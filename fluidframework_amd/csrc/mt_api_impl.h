// mt_api_impl.h — implementation of the mtgpu.h C ABI over a backend.
//
// Included by mt_engine.hip (backend HIP: pools in HBM, one wavefront per
// document on gfx950) — the product — and by tests/emu/mt_emu.cpp (backend
// EMU: host memory + host-emulated waves), which exists only so the CPU test
// suite can exercise the identical engine logic against the oracle.
//
// Required from the includer (c: the context; a launch returns MT_OK or MT_E_HIP):
//   MT_FN(name)           exported symbol name
//   mtb_init(c), mtb_fini(c), mtb_malloc(&p, bytes), mtb_free(p), mtb_memset(p, v, bytes)
//   mtb_h2d / mtb_d2h / mtb_d2d(c, dst, src, bytes), mtb_sync(c)
//   mtb_stage_get(c, bytes), mtb_stage_send(c, dev, bytes), mtb_host_stage(c, bytes, buf)
//   mtb_cu_count(c); with MTB_HAVE_MASKED_STREAMS, mtb_masked_streams(c): may the plan use MT_LANE_A / B?
//   mt_plan.h, included after the above; mtb_launch_replay(c, gen, n_runs): the generator, or its plan
//   mtb_launch_open(c, first, n), mtb_launch_load(c, load, n)
//   mtb_launch_update_seq(c, docs, msn, seq, n), mtb_launch_get_length(c, docs, ref, cli, out, n)
//   mtb_launch_gather_text(c, at, len, off, dst, n)
//   mtb_launch_pack_size(c, docs, out, n, epoch), mtb_launch_pack(c, docs, off, stage, n, epoch)
//   mtb_launch_rows(c, pack, first, n, L, dst, rows, checksums)
//   with MTB_HAVE_QUERY: mtb_launch_query(c, call, q, groups, out, n_groups), the call's record by value
//   with MTB_HAVE_RELOCATE: mtb_launch_occupancy(c, docs, out, n, epoch), mtb_launch_relocate(c, docs, ny, n, epoch, compact)
#pragma once
#include <algorithm>
#include <chrono>
#include <functional>
#include <thread>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "mt_ctx.h"
#include "mt_plan.h"
#include "mt_shard.h"

// Host loops over a batch's ops run on up to 16 threads once a batch is large enough to pay
// for them (ingest: validation and the SoA -> 32-byte record packing).
template <class F> static void mt_par_for(size_t n, F f) {
    unsigned T = std::thread::hardware_concurrency();
    T = T < 1 ? 1 : (T > 16 ? 16 : T);
    if (n < (size_t)1 << 16 || T == 1) { f((size_t)0, n, 0u); return; }
    const size_t per = (n + T - 1) / T;
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < T; t++) {
        const size_t a = per * t, b = a + per < n ? a + per : n;
        if (a < b) pool.emplace_back(f, a, b, t);
    }
    f((size_t)0, per < n ? per : n, 0u);
    for (auto& th : pool) th.join();
}

extern "C" {

const char* MT_FN(last_error)(mt_ctx* c) { return c ? c->err.c_str() : "null context"; }
#ifndef MT_SRC_HASH
#define MT_SRC_HASH "unhashed"
#endif
// The same hash behind a tag, so a build script can read it from the file's bytes without
// loading the library into its own process (dlopen caches a path's first handle).
__attribute__((used)) const char MT_FN(source_hash_tag)[] = "mt-src-hash:" MT_SRC_HASH;
const char* MT_FN(source_hash)(void) { return MT_FN(source_hash_tag) + 12; }

// Pools of every document, laid out back to back with per-document capacities.
static void mt_caps_default(mt_limits& q) {
    if (!q.rows_per_doc) q.rows_per_doc = 4096;
    if (!q.blocks_per_doc) q.blocks_per_doc = q.rows_per_doc / 2 + 64;
    if (!q.heap_per_doc) q.heap_per_doc = q.rows_per_doc;
    if (!q.window_per_doc) q.window_per_doc = 4096;
    if (!q.text_per_doc) q.text_per_doc = q.rows_per_doc * 8;
    if (!q.propsets_per_doc) q.propsets_per_doc = 1024;
    if (!q.markers_per_doc) q.markers_per_doc = 1024;
    if (!q.register_rows_per_doc) q.register_rows_per_doc = 256;
}
static bool mt_caps_too_large(mt_ctx* c, const MtDocLayout& y) {
    for (const MtCapDesc& k : MT_CAPS)
        if (y.*k.cap > k.max) { c->err = "per-document capacity too large"; return true; }
    return false;
}
static int mt_rederive(mt_ctx* c);
static int mt_delta_size(mt_ctx* c, uint64_t capacity);
static int mt_create_impl(int device, uint32_t n_docs, const mt_limits* caps, bool uniform, mt_ctx** out) {
    mt_ctx* c = new mt_ctx();
    *out = c;
    c->device = device; c->lim = caps[0]; c->lim.max_docs = n_docs;
    if (mtb_init(c) != 0) return MT_E_HIP;
    MtState& S = c->S;
    S.maxDocs = n_docs;
    S.holdCap = MT_RFL;
    c->layout_h.resize(n_docs);
    MtDocLayout tot{};
    for (uint32_t d = 0; d < n_docs; d++) {
        mt_limits q = caps[uniform ? 0 : d];
        mt_caps_default(q);
        MtDocLayout& y = c->layout_h[d];
        for (const MtCapDesc& k : MT_CAPS) y.*k.cap = q.*k.lim;
        if (mt_caps_too_large(c, y)) return MT_E_INVALID;
        const MtDocLayout s = mt_slice(y);
        for (auto f : MT_LY_OFF) { y.*f = tot.*f; tot.*f += s.*f; }
    }
    const size_t D = S.maxDocs;
    for (const MtPoolDesc& d : MT_POOLS) {
        void* p;
        if (mtb_malloc(&p, mt_pool_bytes(d, tot, D)) != 0) { c->err = std::string("pool allocation failed: ") + d.field; return MT_E_OOM; }
        mt_pool_set(S, d, p);
    }
    mtb_h2d(c, (void*)S.layout, c->layout_h.data(), sizeof(MtDocLayout) * D);
    mtb_memset(S.hdr, 0, sizeof(MtDocHdr) * D);
    c->tot = tot; c->cap = tot;
    return mt_rederive(c);
}

int MT_FN(create)(int device, const mt_limits* L, mt_ctx** out) {
    if (!L || !out || L->max_docs == 0) return MT_E_INVALID;
    return mt_create_impl(device, L->max_docs, L, true, out);
}
int MT_FN(create_docs)(int device, uint32_t n_docs, const mt_limits* per_doc, mt_ctx** out) {
    if (!per_doc || !out || n_docs == 0) return MT_E_INVALID;
    return mt_create_impl(device, n_docs, per_doc, false, out);
}
// Device-side checkpoint of every document's state (rows, blocks, heap, window,
// text, property sets, headers, recycled-row stacks): the engine's equivalent of
// a summary to resume from (SURVEY.md §5 checkpoint/resume), used by benchmarks
// that replay the same stream on the same starting state.
// The pools up to their tails (documents relocated since the last checkpoint may have moved
// them: the shadows grow with them), and the host's layout beside them.
int MT_FN(checkpoint)(mt_ctx* c) {
    if (!c) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    c->ck_valid = false;
    for (size_t k = 0; k < MT_NPOOLS; k++) {
        if (!MT_POOLS[k].ck) continue;
        const size_t bytes = mt_pool_bytes(MT_POOLS[k], c->tot, c->S.maxDocs), want = bytes ? bytes : 16;
        if (c->ck[k] && c->ck_bytes[k] < want) { mtb_free(c->ck[k]); c->ck[k] = nullptr; c->ck_bytes[k] = 0; }
        if (!c->ck[k]) {
            if (mtb_malloc(&c->ck[k], want) != 0) { c->ck[k] = nullptr; c->err = "checkpoint allocation failed"; return MT_E_OOM; }
            c->ck_bytes[k] = want;
        }
        if (bytes) mtb_d2d(c, c->ck[k], mt_pool_get(c->S, MT_POOLS[k]), bytes);
    }
    c->ck_layout = c->layout_h; c->ck_tot = c->tot; c->ck_dead = c->dead;
    c->ck_doc_keys = c->doc_keys; c->ck_doc_wide = c->doc_wide; c->ck_props_wide = c->props_wide;
    c->ck_valid = true;
    return MT_OK;
}
// Documents, layout table and tails as of the checkpoint: a pool reallocated since holds the
// shadow as its prefix; slices handed out since are free again.
int MT_FN(restore)(mt_ctx* c) {
    if (!c || !c->ck_valid) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    for (size_t k = 0; k < MT_NPOOLS; k++) {
        const size_t bytes = MT_POOLS[k].ck ? mt_pool_bytes(MT_POOLS[k], c->ck_tot, c->S.maxDocs) : 0;
        if (bytes) mtb_d2d(c, mt_pool_get(c->S, MT_POOLS[k]), c->ck[k], bytes);
    }
    if (c->layout_h.size() == c->ck_layout.size() &&
        memcmp(c->layout_h.data(), c->ck_layout.data(), sizeof(MtDocLayout) * c->layout_h.size()) != 0) {
        c->layout_h = c->ck_layout;
        mtb_h2d(c, (void*)c->S.layout, c->layout_h.data(), sizeof(MtDocLayout) * c->layout_h.size());
        rc = mt_rederive(c);
    }
    c->tot = c->ck_tot; c->dead = c->ck_dead;
    // The maps are the checkpoint's again, so the keys counted for them count again: a document
    // wide then is wide now, whatever mt_docs_open cleared since.  If the table first passed
    // MT_WAVE keys after the checkpoint, nobody counted the checkpoint's keys (as in mt_set_props).
    // The marks only ever err towards wide: what was counted since the checkpoint stays counted
    // (the resident batch, counted once at its upload, may be replayed onto the restored maps), so
    // each document gets the union of the two counts.
    if (c->props_wide) {
        if (c->doc_wide.size() < c->S.maxDocs) { c->doc_wide.resize(c->S.maxDocs, 0); c->doc_keys.resize(c->S.maxDocs); }
        if (c->ck_props_wide && c->ck_doc_wide.size() == c->doc_wide.size()) {
            for (size_t d = 0; d < c->doc_wide.size(); d++) {
                if (c->doc_wide[d]) continue;
                std::vector<uint16_t>& ks = c->doc_keys[d];
                const std::vector<uint16_t>& ck = c->ck_doc_keys[d];
                if (!ck.empty()) {
                    std::vector<uint16_t> u(ks.size() + ck.size());
                    u.resize((size_t)(std::set_union(ks.begin(), ks.end(), ck.begin(), ck.end(), u.begin()) - u.begin()));
                    ks.swap(u);
                }
                if (c->ck_doc_wide[d] || ks.size() > MT_WAVE) { c->doc_wide[d] = 1; std::vector<uint16_t>().swap(ks); }
            }
        } else {
            std::fill(c->doc_wide.begin(), c->doc_wide.end(), (uint8_t)1);
            for (auto& k : c->doc_keys) std::vector<uint16_t>().swap(k);
        }
    }
    return rc;
}
int MT_FN(pool_bytes)(mt_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return MT_E_INVALID;
    *bytes = c->pool_bytes;
    return MT_OK;
}

/* ------------------------------------------------------------- growth ---- */
#ifndef MTB_HAVE_RELOCATE
// A backend whose pools the host addresses (the emulation) takes these plain per-document
// loops; the HIP backend defines its own over the kernels and MTB_HAVE_RELOCATE.
static int mtb_launch_occupancy(mt_ctx* c, const uint32_t* docs, MtOcc* out, uint32_t n, uint32_t epoch) {
    for (uint32_t i = 0; i < n; i++) { MtScratch sc; MtEng e; e.bind(c->S, docs[i], &sc); out[i] = mt_doc_occupancy(e, epoch); }
    return MT_OK;
}
static int mtb_launch_relocate(mt_ctx* c, const uint32_t* docs, const MtDocLayout* ny, uint32_t n, uint32_t epoch, bool compact) {
    for (uint32_t i = 0; i < n; i++) { MtScratch sc; MtEng e; e.bind(c->S, docs[i], &sc); mt_relocate_doc(e, c->S, ny[i], epoch, compact); }
    return MT_OK;
}
#endif
// Everything the library derives from the documents' capacities: the per-pool maxima, the
// pools' bytes and the capture buffers' minimum sizes (staging sizes are taken per call).
static int mt_rederive(mt_ctx* c) {
    MtState& S = c->S;
    for (const MtCapDesc& k : MT_CAPS) if (k.most) S.*k.most = 0;
    for (const MtDocLayout& y : c->layout_h)
        for (const MtCapDesc& k : MT_CAPS) if (k.most) S.*k.most = std::max(S.*k.most, y.*k.cap);
    c->pool_bytes = mt_pool_bytes_of(c->cap, S.maxDocs);
    return c->delta_req ? mt_delta_size(c, c->delta_req) : MT_OK;
}
static int mt_occupancy(mt_ctx* c, uint32_t n, const uint32_t* docs, std::vector<MtOcc>& occ, uint32_t* epoch) {
    int rc;
    if ((rc = mtb_sync(c))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp0, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp2, sizeof(MtOcc) * n))) return rc;
    mtb_h2d(c, c->b_tmp0.p, docs, 4ull * n);
    *epoch = ++c->stage_epoch;
    if ((rc = mtb_launch_occupancy(c, (const uint32_t*)c->b_tmp0.p, (MtOcc*)c->b_tmp2.p, n, *epoch))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    occ.resize(n);
    mtb_d2h(c, occ.data(), c->b_tmp2.p, sizeof(MtOcc) * n);
    return MT_OK;
}
// mt_docs_resize: sizing pass, validation, room at the pools' tails (a pool is reallocated
// first when its tail cannot hold the new slices), the move, then the layout table.  Nothing
// has changed when it fails.
static int mt_resize_impl(mt_ctx* c, uint32_t n, const uint32_t* docs, const mt_limits* caps) {
    if (n == 0) return MT_OK;
    const size_t D = c->S.maxDocs;
    {
        std::vector<uint32_t> seen(docs, docs + n);
        std::sort(seen.begin(), seen.end());
        if (seen.back() >= D) { c->err = "doc id out of range"; return MT_E_INVALID; }
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { c->err = "a document is named twice"; return MT_E_INVALID; }
    }
    std::vector<MtOcc> occ;
    uint32_t epoch = 0;
    int rc = mt_occupancy(c, n, docs, occ, &epoch);
    if (rc) return rc;
    std::vector<MtDocLayout> ny(n);
    MtDocLayout nt = c->tot;
    uint64_t moved = 0;
    for (uint32_t i = 0; i < n; i++) {
        const MtDocLayout& y = c->layout_h[docs[i]];
        const mt_limits& q = caps[i];
        MtDocLayout& z = ny[i];
        for (const MtCapDesc& k : MT_CAPS) z.*k.cap = q.*k.lim ? q.*k.lim : y.*k.cap;
        if (mt_caps_too_large(c, z)) return MT_E_INVALID;
        const MtOcc& o = occ[i];
        for (const MtCapDesc& k : MT_CAPS)
            if (z.*k.cap < o.*k.occ) {
                char b[160];
                snprintf(b, sizeof b, "document %u: %s capacity %u is below what it holds (%u)", docs[i], k.name, z.*k.cap, o.*k.occ);
                c->err = b;
                return MT_E_INVALID;
            }
        // a property arena copied whole (capture armed) must hold the arena as it is
        if (c->delta_cap) {
            MtDocHdr h;
            mtb_d2h(c, &h, c->S.hdr + docs[i], sizeof h);
            if (h.psetTop > 0 && z.psetCap < (uint32_t)h.psetTop) {
                char b[160];
                snprintf(b, sizeof b, "document %u: property sets capacity %u is below its arena (%d; delta capture is armed)",
                         docs[i], z.psetCap, h.psetTop);
                c->err = b;
                return MT_E_INVALID;
            }
        }
        // a pool whose capacity stays keeps its slice; the others get new ones at the tails
        const MtDocLayout s = mt_slice(z), s0 = mt_slice(y);
        for (auto f : MT_LY_OFF) {
            if (s.*f == s0.*f) z.*f = y.*f;
            else { z.*f = nt.*f; nt.*f += s.*f; }
        }
        // what moves: the holdings (the heap's entry 0 with them; the marker table whole)
        for (const MtCapDesc& k : MT_CAPS) {
            if (z.*k.off == y.*k.off) continue;
            const uint64_t held = k.off == &MtDocLayout::mid ? std::min(y.midCap, z.midCap) : (uint64_t)(o.*k.occ) + (k.off == &MtDocLayout::heap);
            moved += k.esz * held;
        }
    }
    // room: every pool whose tail would pass its allocation goes to twice its size or more
    MtDocLayout ncap = c->cap;
    bool re = false;
    for (auto f : MT_LY_OFF)
        if (nt.*f > c->cap.*f) { ncap.*f = std::max(2 * (c->cap.*f), nt.*f); re = true; }
    if (re) {
        if (c->grow_budget && mt_pool_bytes_of(ncap, D) > c->grow_budget) {
            c->err = "growing the pools would pass the budget (mt_set_autogrow max_pool_bytes)";
            return MT_E_OOM;
        }
        void* np[MT_NPOOLS] = {nullptr};
        for (size_t k = 0; k < MT_NPOOLS; k++) {
            const MtPoolDesc& d = MT_POOLS[k];
            if (!d.n || ncap.*d.n == c->cap.*d.n) continue;
            const size_t bytes = mt_pool_bytes(d, ncap, D);
            if (mtb_malloc(&np[k], bytes ? bytes : 16) != 0) {
                for (void* q : np) if (q) mtb_free(q);
                c->err = std::string("pool reallocation failed: ") + d.name;
                return MT_E_OOM;
            }
        }
        for (size_t k = 0; k < MT_NPOOLS; k++) {
            if (!np[k]) continue;
            void* old = mt_pool_get(c->S, MT_POOLS[k]);
            const size_t used = mt_pool_bytes(MT_POOLS[k], c->tot, D);
            if (used) mtb_d2d(c, np[k], old, used);
            mtb_free(old);
            mt_pool_set(c->S, MT_POOLS[k], np[k]);
            c->grow_realloc++;
        }
        c->cap = ncap;
        c->pool_bytes = mt_pool_bytes_of(c->cap, D);
    }
    if ((rc = mtb_ensure(c, c->b_tmp1, sizeof(MtDocLayout) * n))) return rc;
    mtb_h2d(c, c->b_tmp1.p, ny.data(), sizeof(MtDocLayout) * n);
    if ((rc = mtb_launch_relocate(c, (const uint32_t*)c->b_tmp0.p, (const MtDocLayout*)c->b_tmp1.p, n, epoch, c->delta_cap == 0))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    for (uint32_t i = 0; i < n; i++) {
        MtDocLayout& y = c->layout_h[docs[i]];
        const MtDocLayout s = mt_slice(y);
        for (auto f : MT_LY_OFF) if (ny[i].*f != y.*f) c->dead.*f += s.*f;
        y = ny[i];
    }
    MtDocLayout* table = (MtDocLayout*)c->S.layout;
    if ((size_t)n * 8 > D) mtb_h2d(c, table, c->layout_h.data(), sizeof(MtDocLayout) * D);
    else for (uint32_t i = 0; i < n; i++) mtb_h2d(c, table + docs[i], &c->layout_h[docs[i]], sizeof(MtDocLayout));
    c->tot = nt;
    c->grow_reloc += n; c->grow_moved += moved;
    // (the documents have moved; a capture buffer that cannot follow is reported as such)
    if ((rc = mt_rederive(c))) { c->err = "the documents were moved, but the delta capture buffers could not be sized for them"; return rc; }
    return MT_OK;
}
int MT_FN(docs_resize)(mt_ctx* c, uint32_t n, const uint32_t* docs, const mt_limits* caps) {
    if (!c || (n && (!docs || !caps))) return MT_E_INVALID;
    return mt_resize_impl(c, n, docs, caps);
}
int MT_FN(doc_caps)(mt_ctx* c, uint32_t n, const uint32_t* docs, mt_limits* out) {
    if (!c || (n && (!docs || !out))) return MT_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (docs[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
        const MtDocLayout& y = c->layout_h[docs[i]];
        mt_limits& q = out[i];
        q.max_docs = c->S.maxDocs;
        for (const MtCapDesc& k : MT_CAPS) q.*k.lim = y.*k.cap;
    }
    return MT_OK;
}
int MT_FN(doc_occupancy)(mt_ctx* c, uint32_t n, const uint32_t* docs, mt_limits* out) {
    if (!c || (n && (!docs || !out))) return MT_E_INVALID;
    if (n == 0) return MT_OK;
    for (uint32_t i = 0; i < n; i++) if (docs[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
    std::vector<MtOcc> occ;
    uint32_t epoch = 0;
    int rc = mt_occupancy(c, n, docs, occ, &epoch);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
        mt_limits& q = out[i];
        q.max_docs = c->S.maxDocs;
        for (const MtCapDesc& k : MT_CAPS) q.*k.lim = occ[i].*k.occ;
    }
    return MT_OK;
}
int MT_FN(set_autogrow)(mt_ctx* c, int on, uint64_t max_pool_bytes) {
    if (!c) return MT_E_INVALID;
    c->autogrow = on != 0; c->grow_budget = max_pool_bytes;
    return MT_OK;
}
int MT_FN(grow_stats)(mt_ctx* c, uint64_t out[6]) {
    if (!c || !out) return MT_E_INVALID;
    uint64_t dead = 0;                               // vacated slices, in bytes
    for (const MtPoolDesc& d : MT_POOLS) if (d.n) dead += mt_pool_bytes(d, c->dead, 0);
    const uint64_t used = mt_pool_bytes_of(c->tot, c->S.maxDocs);
    out[0] = c->grow_reloc; out[1] = c->grow_realloc; out[2] = c->grow_moved; out[3] = used - dead; out[4] = dead;
    out[5] = c->grow_launches;
    return MT_OK;
}
int MT_FN(last_resume)(mt_ctx* c, uint32_t n, uint32_t* out) {
    if (!c || (n && !out) || n > c->grow_resume.size()) return MT_E_INVALID;
    for (uint32_t i = 0; i < n; i++) out[i] = c->grow_resume[i];
    return MT_OK;
}

void MT_FN(destroy)(mt_ctx* c) {
    if (!c) return;
    for (size_t k = 0; k < MT_NPOOLS; k++)
        for (void* p : {mt_pool_get(c->S, MT_POOLS[k]), c->ck[k]}) if (p) mtb_free(p);
    for (auto* b : c->dev_bufs()) if (b->p) mtb_free(b->p);
    mtb_fini(c);
    delete c;
}

int MT_FN(docs_open)(mt_ctx* c, uint32_t first, uint32_t n) {
    if (!c || (uint64_t)first + n > c->S.maxDocs) return MT_E_INVALID;
    if (n == 0) return MT_OK;
    for (uint32_t d = first; d < first + n && d < c->snap_chunk.size(); d++) c->snap_chunk[d] = 0;   // a new Client's options
    for (uint32_t d = first; d < first + n && d < c->doc_wide.size(); d++) { c->doc_wide[d] = 0; c->doc_keys[d].clear(); }
    return mtb_launch_open(c, first, n);
}
int MT_FN(set_doc_snapshot_chunk)(mt_ctx* c, uint32_t n, const uint32_t* docs, const uint64_t* chunk) {
    if (!c || (n && (!docs || !chunk))) return MT_E_INVALID;
    for (uint32_t i = 0; i < n; i++) if (docs[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
    if (c->snap_chunk.size() < c->S.maxDocs) c->snap_chunk.resize(c->S.maxDocs, 0);
    for (uint32_t i = 0; i < n; i++) c->snap_chunk[docs[i]] = chunk[i];
    return MT_OK;
}

int MT_FN(set_props)(mt_ctx* c, const mt_prop_table* P) {
    if (!c || !P) return MT_E_INVALID;
    const uint32_t npairs = P->set_off[P->n_sets];
    int rc;
    if ((rc = mtb_ensure(c, c->b_pset_off, 4ull * (P->n_sets + 1)))) return rc;
    if ((rc = mtb_ensure(c, c->b_pkey, 2ull * npairs + 2))) return rc;
    if ((rc = mtb_ensure(c, c->b_pval, 4ull * npairs + 4))) return rc;
    if ((rc = mtb_ensure(c, c->b_pfalsy, 1ull * P->n_values + 1))) return rc;
    if ((rc = mtb_ensure(c, c->b_pclass, 4ull * P->n_values + 4))) return rc;
    if ((rc = mtb_ensure(c, c->b_pkind, 4ull * P->n_values + 8))) return rc;
    mtb_h2d(c, c->b_pset_off.p, P->set_off, 4ull * (P->n_sets + 1));
    if (npairs) { mtb_h2d(c, c->b_pkey.p, P->key, 2ull * npairs); mtb_h2d(c, c->b_pval.p, P->value, 4ull * npairs); }
    if (P->n_values) { mtb_h2d(c, c->b_pfalsy.p, P->value_falsy, P->n_values); mtb_h2d(c, c->b_pclass.p, P->value_class, 4ull * P->n_values); }
    // per value: what incr yields from it held, and the consensus seq -1 mark (MtState::p_vinfo);
    // element 0: incr of a fresh consensus object
    std::vector<int32_t> vinfo(P->n_values + 1);
    vinfo[0] = P->value_incr && P->incr_object >= 0 && (uint32_t)P->incr_object < P->n_values ? P->incr_object : MT_VINFO_NONE;
    for (uint32_t v = 0; P->value_kind && v < P->n_values; v++) {
        const uint8_t k = P->value_kind[v];
        const int32_t inc = P->value_incr ? P->value_incr[v] : MT_VAL_UNSUP;
        vinfo[v + 1] = (k & MT_VK_NUM) ? MT_VAL_NAN
                                       : (((inc >= 0 && (uint32_t)inc < P->n_values) ? inc : MT_VINFO_NONE) |
                                          ((k & MT_VK_SEQM1) ? MT_VINFO_SEQM1 : 0));
    }
    mtb_h2d(c, c->b_pkind.p, vinfo.data(), 4ull * vinfo.size());
    mtb_sync(c);
    c->S.p_off = (const uint32_t*)c->b_pset_off.p; c->S.p_key = (const uint16_t*)c->b_pkey.p;
    c->S.p_val = (const int32_t*)c->b_pval.p; c->S.p_falsy = (const uint8_t*)c->b_pfalsy.p;
    c->S.p_class = (const uint32_t*)c->b_pclass.p; c->S.p_nsets = P->n_sets;
    c->S.p_vinfo = (P->value_kind || !P->n_values) ? (const int32_t*)c->b_pkind.p + 1 : nullptr;
    c->h_set_off.assign(P->set_off, P->set_off + P->n_sets + 1);
    c->h_set_key.assign(P->key, P->key + npairs);
    {
        std::vector<uint16_t> ks(c->h_set_key);
        std::sort(ks.begin(), ks.end());
        const size_t nkeys = (size_t)(std::unique(ks.begin(), ks.end()) - ks.begin());
        const bool wide = nkeys > MT_WAVE;
        c->prop_nkeys = (uint32_t)nkeys; c->prop_maxset = 0;
        for (uint32_t i = 0; i < P->n_sets; i++) c->prop_maxset = std::max(c->prop_maxset, P->set_off[i + 1] - P->set_off[i]);
        // Below MT_WAVE keys in all no document can outgrow the lanes, and batches are not
        // scanned (mt_scan_wide); when the table first passes them, the documents open now
        // have keys nobody counted: they replay in the FULL kernels until reopened.
        if (wide && !c->props_wide) {
            if (c->doc_wide.size() < c->S.maxDocs) { c->doc_wide.resize(c->S.maxDocs, 0); c->doc_keys.resize(c->S.maxDocs); }
            std::fill(c->doc_wide.begin(), c->doc_wide.end(), (uint8_t)1);
            for (auto& k : c->doc_keys) std::vector<uint16_t>().swap(k);
        }
        c->props_wide = wide;
    }
    c->names.key_json.assign(P->key_json, P->key_json + P->n_keys);
    c->names.key_index.assign(P->key_index, P->key_index + P->n_keys);
    c->names.value_json.assign(P->value_json, P->value_json + P->n_values);
    c->names.value_class.assign(P->value_class, P->value_class + P->n_values);
    return MT_OK;
}

int MT_FN(set_client_names)(mt_ctx* c, uint32_t n, const char* const* cj) {
    if (!c || (n && !cj)) return MT_E_INVALID;
    c->names.client_json.assign(cj, cj + n);
    return MT_OK;
}
int MT_FN(set_doc_client_names)(mt_ctx* c, uint32_t doc, uint32_t n, const char* const* cj) {
    if (!c || doc >= c->S.maxDocs || (n && !cj)) return MT_E_INVALID;
    if (n == 0) c->doc_clients.erase(doc);
    else c->doc_clients[doc].assign(cj, cj + n);
    return MT_OK;
}

// Notes property set `ps` on document `doc` (mt_ctx::doc_keys); true once the document's keys
// pass a wave's lanes (its maps may then outgrow the non-FULL kernels).
static bool mt_note_set(mt_ctx* c, uint32_t doc, int ps) {
    if (ps < 0 || (size_t)ps + 1 >= c->h_set_off.size()) return false;
    if (c->doc_wide.size() < c->S.maxDocs) { c->doc_wide.resize(c->S.maxDocs, 0); c->doc_keys.resize(c->S.maxDocs); }
    if (c->doc_wide[doc]) return true;
    std::vector<uint16_t>& ks = c->doc_keys[doc];
    for (uint32_t q = c->h_set_off[ps]; q < c->h_set_off[ps + 1]; q++) {
        const uint16_t k = c->h_set_key[q];
        auto it = std::lower_bound(ks.begin(), ks.end(), k);
        if (it == ks.end() || *it != k) ks.insert(it, k);
    }
    if (ks.size() > MT_WAVE) { c->doc_wide[doc] = 1; std::vector<uint16_t>().swap(ks); return true; }
    return false;
}
// batch_wide for a batch of n_runs runs: run r's document doc(r) and its ops' property sets
// pid(i) over [op0(r), op1(r)) (sets named twice in a run are noted once).
extern "C++" {
template <class DocOf, class Op0, class Op1, class Pid>
static bool mt_scan_wide(mt_ctx* c, size_t n_runs, DocOf doc, Op0 op0, Op1 op1, Pid pid) {
    bool wide = false;
    if (!c->props_wide) return false;                 // no document can pass MT_WAVE keys
    std::vector<uint32_t> seen(c->h_set_off.size() - 1, 0);
    for (size_t r = 0; r < n_runs; r++) {
        const uint32_t d = doc(r);
        if (d < c->doc_wide.size() && c->doc_wide[d]) { wide = true; continue; }
        for (size_t i = op0(r); i < op1(r); i++) {
            const int ps = pid(i);
            if (ps < 0 || (size_t)ps >= seen.size() || seen[ps] == (uint32_t)r + 1) continue;
            seen[ps] = (uint32_t)r + 1;
            if (mt_note_set(c, d, ps)) { wide = true; break; }
        }
    }
    return wide;
}
}
// Device-built batches (the generators, the exchange: ops never seen on the host): wide when the
// property sets together could make a document wide.  Nobody counts the keys such a batch names,
// so its documents are wide from then on (sticky, as mt_note_set's): a later host batch for one of
// them replays in the FULL kernels too, some of them without need.
static bool mt_dev_wide(mt_ctx* c, uint32_t n_runs, const uint32_t* doc_ids) {
    if (!c->props_wide) return false;
    if (c->doc_wide.size() < c->S.maxDocs) { c->doc_wide.resize(c->S.maxDocs, 0); c->doc_keys.resize(c->S.maxDocs); }
    for (uint32_t r = 0; r < n_runs; r++) { c->doc_wide[doc_ids[r]] = 1; std::vector<uint16_t>().swap(c->doc_keys[doc_ids[r]]); }
    return true;
}
// Such a batch's arrays (b_doc, b_off, b_rec, b_pay; per-run payload bases in b_pbase): generated
// and exchanged streams hold no relative positions, and no register ops either.
static MtOps mt_dev_ops(mt_ctx* c, uint32_t n_runs, uint64_t payload_units, bool pay_base) {
    MtOps o{};
    o.doc_ids = (const uint32_t*)c->b_doc.p; o.op_off = (const uint32_t*)c->b_off.p; o.rec = (MtOpRec*)c->b_rec.p;
    o.payload = (uint16_t*)c->b_pay.p; o.n_runs = n_runs; o.payload_units = payload_units;
    o.pay_base = pay_base ? (const unsigned long long*)c->b_pbase.p : nullptr;
    return o;
}

// The batch's arrays in one device region, one pinned staging copy and one asynchronous H2D
// (stream-ordered before the replay that follows; no host synchronization): doc ids, op
// offsets, the op records packed to mt_op_rec, the payload and the relative positions.  The
// caller's arrays are consumed before this returns.
struct MtStageLayout { size_t o_doc, o_off, o_rec, o_pay, o_rel, total; };
static MtStageLayout mt_stage_layout(size_t R, size_t N, size_t PU, size_t NR) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    static_assert(sizeof(mt_rel_pos) == sizeof(MtRelPos), "relative position layout");
    MtStageLayout y{};
    y.o_off = al(y.o_doc + 4 * R); y.o_rec = al(y.o_off + 4 * (R + 1)); y.o_pay = al(y.o_rec + sizeof(MtOpRec) * N);
    y.o_rel = al(y.o_pay + 2 * PU); y.total = al(y.o_rel + sizeof(MtRelPos) * NR) + 256;
    return y;
}
// The staged arrays at device region d, as the MtOps members they become.
static MtOps mt_staged_ops(uint8_t* d, const MtStageLayout& y, size_t R, size_t PU, size_t NR) {
    MtOps o{};
    o.doc_ids = (const uint32_t*)(d + y.o_doc); o.op_off = (const uint32_t*)(d + y.o_off); o.rec = (MtOpRec*)(d + y.o_rec);
    o.payload = (uint16_t*)(d + y.o_pay); o.rel = (const MtRelPos*)(d + y.o_rel);
    o.n_runs = (uint32_t)R; o.payload_units = PU; o.n_rel = (uint32_t)NR;
    return o;
}
// The one place a batch becomes resident.  `o` carries the device pointers and the counts;
// run_off is the host's copy of its op offsets (n_runs + 1).  Capture, resume, start and growth
// headroom are cleared: every launch sets them first (mt_replay_resident, mt_replay_capture;
// mt_generate_docs launches with them clear).  keep_gen: a host upload leaves gen.enabled (and
// gen_docs) as they are, as it always did, so mt_generated_to_resident still answers for the
// last generated stream; a device-built batch disarms the generator.
static void mt_install_batch(mt_ctx* c, MtOps o, const uint32_t* run_off, const uint32_t* run_docs, bool reg, bool wide, bool keep_gen) {
    o.drec = nullptr; o.dcount = nullptr; o.dcap = 0; o.dtext = nullptr; o.dtcap = 0;
    o.resume = nullptr; o.start = nullptr; o.grow_pch = 0;
    c->ops = o;
    c->n_runs = o.n_runs;
    c->run_off.assign(run_off, run_off + o.n_runs + 1); c->batch_gen++;
    c->run_docs.assign(run_docs, run_docs + o.n_runs); c->batch_dev = !keep_gen; c->batch_replays = 0;
    c->batch_reg = reg; c->batch_wide = wide;
    if (!keep_gen) c->gen.enabled = 0;
}
// An upload that failed after the regions of the resident batch may have been freed
// (mtb_ensure): no batch is resident (mt_replay_resident: MT_E_INVALID), and none generated.
static int mt_drop_batch(mt_ctx* c, int rc) {
    c->ops = MtOps{};
    c->n_runs = 0; c->run_off.clear(); c->run_docs.clear(); c->batch_dev = false; c->batch_replays = 0; c->batch_gen++;
    c->batch_reg = c->batch_wide = false;
    c->gen.enabled = 0; c->gen_docs = 0;
    return rc;
}
// A batch's run list: documents in range, op offsets monotone.
static int mt_check_runs(mt_ctx* c, uint32_t n_runs, const uint32_t* doc_ids, const uint32_t* op_offsets) {
    for (uint32_t r = 0; r < n_runs; r++) {
        if (doc_ids[r] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
        if (op_offsets[r] > op_offsets[r + 1]) { c->err = "op_offsets not monotone"; return MT_E_INVALID; }
    }
    return MT_OK;
}
// What every op of a host batch must satisfy (op i of batch B, its property set as the device
// will see it): the first violation's message, or null.
static inline __attribute__((always_inline)) const char* mt_op_rule(const mt_op_batch* B, size_t i, int32_t pid, uint32_t nsets) {
    const uint8_t ty = B->type[i], fl = B->flags[i];
    if (ty > MT_OP_PASTE) return "unknown op type";
    if (ty == MT_OP_INSERT && !(fl & MT_OPF_MARKER) && (uint64_t)B->payload_off[i] + B->payload_len[i] > B->payload_units)
        return "payload out of range";
    if (pid >= 0 && (uint32_t)pid >= nsets) return "prop_id out of range (mt_set_props first)";
    if (pid > 32767) return "more than 32767 property sets";
    if (B->payload_len[i] > 65535) return "insert longer than 65535 UTF-16 units";
    if (((fl & MT_OPF_REL1) && (uint32_t)B->pos1[i] >= B->n_rel) || ((fl & MT_OPF_REL2) && (uint32_t)B->pos2[i] >= B->n_rel))
        return "relative position index out of range";
    return nullptr;
}
static int mt_upload_ops(mt_ctx* c, const mt_op_batch* B) {
    const size_t N = B->n_ops, R = B->n_runs, PU = (size_t)B->payload_units, NR = B->rel ? B->n_rel : 0;
    const MtStageLayout y = mt_stage_layout(R, N, PU, NR);
    if (int rc = mtb_ensure(c, c->b_batch, y.total)) return mt_drop_batch(c, rc);
    uint8_t* h = (uint8_t*)mtb_stage_get(c, y.total);
    if (!h) { c->err = "pinned staging allocation failed"; return mt_drop_batch(c, MT_E_OOM); }
    if (R) memcpy(h + y.o_doc, B->doc_ids, 4 * R);
    memcpy(h + y.o_off, B->op_offsets, 4 * (R + 1));
    MtOpRec* rec = (MtOpRec*)(h + y.o_rec);
    uint8_t regT[16] = {0};
    mt_par_for(N, [&](size_t i0, size_t i1, unsigned t) {
        bool reg = false;
        for (size_t i = i0; i < i1; i++) {
            MtOpRec& o = rec[i];
            o.type = B->type[i]; o.flags = B->flags[i]; o.client = B->client[i]; o.seq = B->seq[i]; o.ref_seq = B->ref_seq[i];
            o.msn = B->msn[i]; o.pos1 = B->pos1[i]; o.pos2 = B->pos2[i]; o.payload_off = B->payload_off[i];
            o.payload_len = (uint16_t)B->payload_len[i]; o.prop_id = (int16_t)B->prop_id[i];
            reg |= B->type[i] >= MT_OP_CUT && B->type[i] <= MT_OP_PASTE;
        }
        // this thread's share of the payload (same split, in units)
        const size_t p0 = N ? PU * i0 / N : 0, p1 = N ? PU * i1 / N : PU;
        if (p1 > p0) memcpy(h + y.o_pay + 2 * p0, B->payload + p0, 2 * (p1 - p0));
        regT[t] = reg;
    });
    if (!N && PU) memcpy(h + y.o_pay, B->payload, 2 * PU);
    bool reg = false;
    for (int t = 0; t < 16; t++) reg |= regT[t] != 0;
    if (NR) memcpy(h + y.o_rel, B->rel, sizeof(MtRelPos) * NR);
    mtb_stage_send(c, c->b_batch.p, y.total);
    const bool wide = mt_scan_wide(c, R, [&](size_t r) { return B->doc_ids[r]; }, [&](size_t r) { return B->op_offsets[r]; },
                                   [&](size_t r) { return B->op_offsets[r + 1]; }, [&](size_t i) { return B->prop_id[i]; });
    mt_install_batch(c, mt_staged_ops((uint8_t*)c->b_batch.p, y, R, PU, NR), B->op_offsets, B->doc_ids, reg, wide, true);
    return MT_OK;
}

static int mt_check_batch(mt_ctx* c, const mt_op_batch* B) {
    if (!B || !B->op_offsets || (B->n_runs && !B->doc_ids)) { c->err = "null batch arrays"; return MT_E_INVALID; }
    if (B->op_offsets[B->n_runs] != B->n_ops) { c->err = "op_offsets[n_runs] != n_ops"; return MT_E_INVALID; }
    if (B->n_rel && !B->rel) { c->err = "n_rel without rel"; return MT_E_INVALID; }
    if (int rc = mt_check_runs(c, B->n_runs, B->doc_ids, B->op_offsets)) return rc;
    // per op: the first violation's message (threads check disjoint ranges; the lowest op wins)
    const char* errT[16] = {nullptr};
    size_t errI[16];
    const uint32_t nsets = c->S.p_nsets;
    mt_par_for(B->n_ops, [&](size_t i0, size_t i1, unsigned t) {
        for (size_t i = i0; i < i1; i++)
            if (const char* e = mt_op_rule(B, i, B->prop_id[i], nsets)) { errT[t] = e; errI[t] = i; return; }
    });
    const char* e = nullptr; size_t ei = 0;
    for (int t = 0; t < 16; t++) if (errT[t] && (!e || errI[t] < ei)) { e = errT[t]; ei = errI[t]; }
    if (e) { c->err = e; return MT_E_INVALID; }
    return MT_OK;
}

int MT_FN(upload_batch)(mt_ctx* c, const mt_op_batch* B) {
    if (!c) return MT_E_INVALID;
    int rc = mt_check_batch(c, B);
    if (rc) return rc;
    return mt_upload_ops(c, B);                           // stream-ordered: no synchronization
}
// Parts concatenated into the staging layout of mt_upload_ops, re-based while packed (one pass
// over every op on the library's host threads; validation as mt_check_batch, on the re-based
// values).
static int mt_upload_parts(mt_ctx* c, uint32_t P, const mt_op_batch* parts, const int32_t* const* pmap,
                           const uint32_t* pmapLen) {
    std::vector<uint64_t> opB(P + 1, 0), payB(P + 1, 0), relB(P + 1, 0), runB(P + 1, 0);
    for (uint32_t p = 0; p < P; p++) {
        const mt_op_batch* B = &parts[p];
        if (!B->op_offsets || (B->n_runs && !B->doc_ids) || B->op_offsets[B->n_runs] != B->n_ops ||
            (B->n_rel && !B->rel) || (B->payload_units && !B->payload)) { c->err = "bad batch part"; return MT_E_INVALID; }
        if (int rc = mt_check_runs(c, B->n_runs, B->doc_ids, B->op_offsets)) return rc;
        opB[p + 1] = opB[p] + B->n_ops; payB[p + 1] = payB[p] + B->payload_units;
        relB[p + 1] = relB[p] + (B->rel ? B->n_rel : 0); runB[p + 1] = runB[p] + B->n_runs;
    }
    const size_t N = opB[P], R = runB[P], PU = payB[P], NR = relB[P];
    if (N >= (1ull << 32) || R >= (1ull << 32) || PU >= (1ull << 32)) { c->err = "batch parts exceed 32-bit indices"; return MT_E_INVALID; }
    const MtStageLayout y = mt_stage_layout(R, N, PU, NR);
    // from here on the resident batch's region may be gone: a failure leaves none resident
    if (int rc = mtb_ensure(c, c->b_batch, y.total)) return mt_drop_batch(c, rc);
    uint8_t* h = (uint8_t*)mtb_stage_get(c, y.total);
    if (!h) { c->err = "pinned staging allocation failed"; return mt_drop_batch(c, MT_E_OOM); }
    uint32_t* docs = (uint32_t*)(h + y.o_doc);
    uint32_t* off = (uint32_t*)(h + y.o_off);
    std::vector<uint32_t> runOff(R + 1);
    off[0] = 0; runOff[0] = 0;
    for (uint32_t p = 0; p < P; p++) {
        const mt_op_batch* B = &parts[p];
        for (uint32_t r = 0; r < B->n_runs; r++) {
            docs[runB[p] + r] = B->doc_ids[r];
            off[runB[p] + r + 1] = runOff[runB[p] + r + 1] = (uint32_t)(opB[p] + B->op_offsets[r + 1]);
        }
        if (B->rel && B->n_rel) memcpy(h + y.o_rel + sizeof(MtRelPos) * relB[p], B->rel, sizeof(MtRelPos) * B->n_rel);
    }
    MtOpRec* rec = (MtOpRec*)(h + y.o_rec);
    const uint32_t nsets = c->S.p_nsets;
    const char* errT[16] = {nullptr};
    size_t errI[16];
    uint8_t regT[16] = {0};
    mt_par_for(N, [&](size_t i0, size_t i1, unsigned t) {
        bool reg = false;
        uint32_t p = (uint32_t)(std::upper_bound(opB.begin(), opB.end(), (uint64_t)i0) - opB.begin()) - 1;
        for (size_t i = i0; i < i1; i++) {
            while (i >= opB[p + 1]) p++;
            const mt_op_batch* B = &parts[p];
            const size_t j = i - opB[p];
            MtOpRec& o = rec[i];
            const uint8_t ty = B->type[j], fl = B->flags[j];
            int32_t pid = B->prop_id[j];
            const char* e = nullptr;
            if (pid >= 0 && pmap && pmap[p]) {
                if ((uint32_t)pid >= pmapLen[p]) e = "prop_id out of its part's map";
                else pid = pmap[p][pid];
            }
            const bool text = ty == MT_OP_INSERT && !(fl & MT_OPF_MARKER);
            if (const char* m = mt_op_rule(B, j, pid, nsets)) e = m;
            if (e && !errT[t]) { errT[t] = e; errI[t] = i; }
            o.type = ty; o.flags = fl; o.client = B->client[j]; o.seq = B->seq[j]; o.ref_seq = B->ref_seq[j]; o.msn = B->msn[j];
            o.pos1 = B->pos1[j] + ((fl & MT_OPF_REL1) ? (int32_t)relB[p] : 0);
            o.pos2 = B->pos2[j] + ((fl & MT_OPF_REL2) ? (int32_t)relB[p] : 0);
            o.payload_off = B->payload_off[j] + (text ? (uint32_t)payB[p] : 0u);
            o.payload_len = (uint16_t)B->payload_len[j]; o.prop_id = (int16_t)pid;
            reg |= ty >= MT_OP_CUT && ty <= MT_OP_PASTE;
        }
        regT[t] = reg;
    });
    const char* e = nullptr; size_t ei = 0;
    for (int t = 0; t < 16; t++) if (errT[t] && (!e || errI[t] < ei)) { e = errT[t]; ei = errI[t]; }
    if (e) { c->err = e; return mt_drop_batch(c, MT_E_INVALID); }
    mt_par_for(P, [&](size_t p0, size_t p1, unsigned) {           // payloads, part by part
        for (size_t p = p0; p < p1; p++)
            if (parts[p].payload_units) memcpy(h + y.o_pay + 2 * payB[p], parts[p].payload, 2 * parts[p].payload_units);
    });
    bool reg = false;
    for (int t = 0; t < 16; t++) reg |= regT[t] != 0;
    mtb_stage_send(c, c->b_batch.p, y.total);
    const bool wide = mt_scan_wide(c, R, [&](size_t r) { return docs[r]; }, [&](size_t r) { return (size_t)runOff[r]; },
                                   [&](size_t r) { return (size_t)runOff[r + 1]; }, [&](size_t i) { return (int)rec[i].prop_id; });
    mt_install_batch(c, mt_staged_ops((uint8_t*)c->b_batch.p, y, R, PU, NR), runOff.data(), docs, reg, wide, true);
    return MT_OK;
}
int MT_FN(upload_batch_parts)(mt_ctx* c, uint32_t n_parts, const mt_op_batch* parts, const int32_t* const* prop_map,
                              const uint32_t* prop_map_len) {
    if (!c || (n_parts && !parts) || (prop_map && !prop_map_len)) return MT_E_INVALID;
    return mt_upload_parts(c, n_parts, parts, prop_map, prop_map_len);
}
int MT_FN(replay_resident)(mt_ctx* c);
int MT_FN(apply_batch_parts)(mt_ctx* c, uint32_t n_parts, const mt_op_batch* parts, const int32_t* const* prop_map,
                             const uint32_t* prop_map_len) {
    int rc = MT_FN(upload_batch_parts)(c, n_parts, parts, prop_map, prop_map_len);
    if (rc) return rc;
    return MT_FN(replay_resident)(c);
}
// The stop-and-resume loop of capture batches (mt_delta_capture armed) and growing batches
// (mt_set_autogrow armed), or both at once.
// Capture: each launch appends records until a document has no headroom left for its next
// message (MtEngT::dReserve); that run stops there, the records and pasted text so far move to
// the host, and the next launch resumes the stopped runs (ops.start).  The host copies keep op
// order per document, so one stable sort by op index restores callback order (mt_delta_records).
// Growth: a run stops before an op record its document's pools could not hold
// (MtEngT::growShort) and leaves the capacities that op needs; the documents are relocated
// into larger slices (each short pool to max(need, twice its capacity)) and resumed.
static int mt_resize_impl(mt_ctx* c, uint32_t n, const uint32_t* docs, const mt_limits* caps);
static uint32_t mt_grow_pch(const mt_ctx* c) {
    // chunks one new map can take: a map holds at most every key of the table; maps built past
    // a wave's lanes (applyPropSetWide) reserve room for the old map's keys plus the op set's
    const uint32_t K = c->prop_nkeys, M = c->prop_maxset;
    const uint32_t room = K + M <= MT_WAVE ? K : (K + M < MT_PKEYS ? K + M : MT_PKEYS);
    return room > MT_PSK ? (room + MT_PSK - 1) / MT_PSK : 1;
}
static int mt_replay_capture(mt_ctx* c, const MtGen& g) {
    const uint32_t R = c->n_runs;
    const bool cap = c->delta_cap != 0, grow = c->autogrow && !g.enabled;
    const size_t gbase = mt_grow_base(R);
    int rc;
    if ((rc = mtb_ensure(c, c->b_resume, 4ull * (gbase + (grow ? (size_t)MT_GROW_N * R : 0)) + 4))) return rc;
    if ((rc = mtb_ensure(c, c->b_start, 4ull * R + 4))) return rc;
    std::vector<uint32_t> off(R + 1), resume(R), start(R), need, docs, grownAt(R, 0xFFFFFFFFu);
    if (c->run_off.size() == R + 1) off = c->run_off;
    else mtb_d2h(c, off.data(), c->ops.op_off, 4ull * (R + 1));
    for (uint32_t r = 0; r < R; r++) start[r] = off[r];
    c->delta_host.clear(); c->delta_text.clear(); c->delta_over = false; c->delta_launches = 0;
    c->grow_launches = 0;
    MtOps& o = c->ops;
    o.resume = (uint32_t*)c->b_resume.p;
    o.start = nullptr;
    o.grow_pch = grow ? mt_grow_pch(c) : 0;
    // the growth test lives in the FULL kernels only: an armed batch replays there, as a batch
    // holding register ops does
    const bool reg0 = c->batch_reg;
    if (grow) c->batch_reg = true;
    const std::vector<uint32_t> zeros(grow ? (size_t)MT_GROW_N * R : 0, 0u);
    for (;;) {
        if (cap) {   // (the buffers may have been sized again by a relocation)
            o.drec = (MtDeltaRec*)c->b_drec.p; o.dcount = (unsigned long long*)c->b_dcount.p; o.dcap = c->delta_cap;
            o.dtext = (uint16_t*)c->b_dtext.p; o.dtcap = c->delta_tcap;
            const unsigned long long zero[4] = {0, 0, 0, 0};
            mtb_h2d(c, c->b_dcount.p, zero, sizeof zero);
        } else { o.drec = nullptr; o.dcount = nullptr; o.dcap = 0; o.dtext = nullptr; o.dtcap = 0; }
        if (grow && R) mtb_h2d(c, o.resume + gbase, zeros.data(), 4ull * zeros.size());
        if ((rc = mtb_launch_replay(c, g, R))) break;
        if ((rc = mtb_sync(c))) break;
        c->delta_launches++; c->grow_launches++;
        if (cap) {
            unsigned long long cnt[4];
            mtb_d2h(c, cnt, c->b_dcount.p, sizeof cnt);
            if (cnt[MT_DC_REC] > c->delta_cap || cnt[MT_DC_TXT] > c->delta_tcap) { c->delta_over = true; break; }
            const size_t r0 = c->delta_host.size(), t0 = c->delta_text.size();
            c->delta_host.resize(r0 + cnt[MT_DC_REC]);
            if (cnt[MT_DC_REC]) mtb_d2h(c, c->delta_host.data() + r0, c->b_drec.p, sizeof(MtDeltaRec) * cnt[MT_DC_REC]);
            c->delta_text.resize(t0 + cnt[MT_DC_TXT]);
            if (cnt[MT_DC_TXT]) mtb_d2h(c, c->delta_text.data() + t0, c->b_dtext.p, 2ull * cnt[MT_DC_TXT]);
            for (size_t i = r0; i < c->delta_host.size(); i++) {      // pasted text offsets: into the batch's arena
                MtDeltaRec& q = c->delta_host[i];
                if (q.kind == MT_DK_INSERT && q.b == 0 && q.pad >= 0) q.pad += (int)t0;
            }
        }
        mtb_d2h(c, resume.data(), c->b_resume.p, 4ull * R);
        bool done = true, progress = false;
        for (uint32_t r = 0; r < R; r++) {
            if (resume[r] < off[r + 1]) done = false;
            if (resume[r] != start[r]) progress = true;
        }
        if (done) break;
        if (grow) {
            need.resize((size_t)MT_GROW_N * R);
            mtb_d2h(c, need.data(), o.resume + gbase, 4ull * need.size());
            if (docs.empty()) { docs.resize(R); mtb_d2h(c, docs.data(), o.doc_ids, 4ull * R); }
            std::vector<uint32_t> ids; std::vector<mt_limits> want;
            bool stuck = false;
            for (uint32_t r = 0; r < R; r++) {
                const uint32_t* nd = &need[(size_t)MT_GROW_N * r];
                if (resume[r] >= off[r + 1] || !nd[MT_GROW_MASK]) continue;
                if (grownAt[r] == resume[r]) { stuck = true; break; }      // grown to what it asked for, and short again
                grownAt[r] = resume[r];
                const MtDocLayout& y = c->layout_h[docs[r]];
                auto up = [](uint32_t nd1, uint32_t cur) -> uint32_t {
                    if (!nd1) return 0u;
                    const uint64_t twice = 2ull * cur;
                    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nd1, twice), 0x7FFFFFFFull);
                };
                mt_limits q{};
                for (const MtCapDesc& k : MT_CAPS) if (k.grow >= 0) q.*k.lim = up(nd[k.grow], y.*k.cap);
                size_t at = 0;
                while (at < ids.size() && ids[at] != docs[r]) at++;
                if (at == ids.size()) { ids.push_back(docs[r]); want.push_back(q); }
                else   // (two runs of one document: the larger of each)
                    for (const MtCapDesc& k : MT_CAPS) want[at].*k.lim = std::max(want[at].*k.lim, q.*k.lim);
            }
            if (stuck) { c->err = "a document grown to what its next op asked for is short again"; rc = MT_E_OOM; break; }
            if (!ids.empty()) {
                rc = mt_resize_impl(c, (uint32_t)ids.size(), ids.data(), want.data());
                if (rc == MT_E_INVALID) rc = MT_E_OOM;                      // a capacity past the pools' limits
                if (rc) break;
                progress = true;
            }
        }
        if (!progress) { c->err = "delta capture capacity below one message's bound"; rc = MT_E_OOM; break; }
        start = resume;
        mtb_h2d(c, c->b_start.p, start.data(), 4ull * R);
        o.start = (const uint32_t*)c->b_start.p;
    }
    o.start = nullptr; o.resume = nullptr; o.grow_pch = 0;
    c->batch_reg = reg0;
    if (grow) c->grow_resume = resume;
    c->delta_valid = false;
    return rc;
}
int MT_FN(replay_resident)(mt_ctx* c) {
    if (!c || !c->ops.op_off) return MT_E_INVALID;
    int rc = mtb_ensure(c, c->b_cursor, 4ull * c->n_runs + 4);
    if (rc) return rc;
    MtGen g{}; g.enabled = 0;
    c->delta_valid = false;
    // While the table is wide, the marks must hold for what this replay builds.  A device-built
    // batch was never counted, and a host batch was counted once, at its upload: replayed again
    // (after mt_docs_open cleared the marks, or onto maps an mt_restore brought back) its count
    // stands for nothing, so its documents end wide (sticky).  And a batch uploaded before a
    // document of it was marked (mt_set_props turning the table wide, a restore) is wide now.
    if (c->props_wide && c->run_docs.size() == c->n_runs) {
        if (c->batch_dev || c->batch_replays) c->batch_wide = mt_dev_wide(c, c->n_runs, c->run_docs.data()) || c->batch_wide;
        for (uint32_t r = 0; r < c->n_runs && !c->batch_wide; r++)
            c->batch_wide = c->run_docs[r] < c->doc_wide.size() && c->doc_wide[c->run_docs[r]];
    }
    c->batch_replays++;
    if (c->delta_cap || c->autogrow) return mt_replay_capture(c, g);
    c->ops.drec = nullptr; c->ops.dcount = nullptr; c->ops.dcap = 0; c->ops.dtext = nullptr; c->ops.dtcap = 0;
    c->ops.resume = nullptr; c->ops.start = nullptr; c->ops.grow_pch = 0;
    return mtb_launch_replay(c, g, c->n_runs);
}
int MT_FN(apply_batch)(mt_ctx* c, const mt_op_batch* B) {
    int rc = MT_FN(upload_batch)(c, B);
    if (rc) return rc;
    return MT_FN(replay_resident)(c);
}
// SnapshotLoader.loadBody's insertSegments calls as a device plan
// (MT/snapshotLoader.ts:162-206).  Universal NonCollab segments collect in a
// batch that every flush appends as one insertSegments call; the batch is never
// emptied, so a later flush re-appends already-linked segments: such a flush
// becomes one REFLUSH step (a no-op where the reference's walk falls off the
// tree, aliasing -> MT_DS_UNSUPPORTED where it would link a segment twice).
static bool mt_load_seg_ok(const mt_load_seg& g, int ms, int cs) {
    if ((g.flags & MT_LS_CLIENT) && g.client >= MT_NONCOLLAB) return false;
    if (g.flags & MT_LS_SEQ) {
        if (g.seq < 0 || g.seq > cs) return false;
        if (g.seq != 0 && g.seq <= ms) return false;     // neither universal nor in the collab window
    }
    if (g.flags & MT_LS_REMOVED) {
        if (g.removed_client >= MT_NONCOLLAB || g.removed_seq <= ms || g.removed_seq > cs) return false;
    }
    return true;
}
static void mt_load_plan(const mt_load_batch* B, uint32_t i, std::vector<MtLoadStep>& plan) {
    const uint32_t s0 = B->seg_offsets[i], s1 = B->seg_offsets[i + 1], nh = B->header_segments[i];
    const int ms = B->min_seq[i], cs = B->seq[i];
    bool ok = ms >= 0 && ms <= cs;
    for (uint32_t k = s0; k < s1 && ok; k++) ok = mt_load_seg_ok(B->segs[k], ms, cs);
    if (!ok) { plan.push_back({0, MT_LD_UNSUPPORTED, 0, 0}); return; }
    auto seglen = [&](uint32_t k) -> int {
        const mt_load_seg& g = B->segs[s0 + k];
        return (g.flags & MT_LS_MARKER) ? 1 : (int)g.payload_len;
    };
    std::vector<uint32_t> batch;
    size_t linked = 0;                                   // batch entries appended by earlier flushes
    auto flush = [&]() {
        if (batch.empty()) return;
        bool oldLinked = false;
        for (size_t j = 0; j < linked; j++) if (seglen(batch[j]) > 0) { oldLinked = true; break; }
        if (oldLinked) plan.push_back({0, batch.size() > linked ? MT_LD_REFLUSH_NEW : MT_LD_REFLUSH, MT_NONCOLLAB, 0});
        else
            for (size_t j = linked; j < batch.size(); j++)
                plan.push_back({(int)batch[j], j == linked ? MT_LD_START : MT_LD_CONT, MT_NONCOLLAB, 0});
        linked = batch.size();
    };
    for (uint32_t k = nh; k < s1 - s0; k++) {
        const mt_load_seg& g = B->segs[s0 + k];
        const int cli = (g.flags & MT_LS_CLIENT) ? (int)g.client : MT_NONCOLLAB;
        const int sq = (g.flags & MT_LS_SEQ) ? g.seq : 0;
        if (cli == MT_NONCOLLAB && sq == 0) batch.push_back(k);
        else { flush(); plan.push_back({(int)k, MT_LD_START, cli, sq}); }
    }
    flush();
}
int MT_FN(load_snapshot)(mt_ctx* c, const mt_load_batch* B) {
    if (!c || !B || !B->seg_offsets || (B->n_docs && (!B->doc_ids || !B->header_segments || !B->min_seq || !B->seq)))
        { if (c) c->err = "null load batch arrays"; return MT_E_INVALID; }
    const uint32_t n = B->n_docs;
    if (n == 0) return MT_OK;
    const uint32_t nseg = B->seg_offsets[n];
    std::vector<uint32_t> meta(5ull * n + 1);           // docs | seg_off (n+1) | nhdr | ms | cs
    std::vector<uint32_t> plan_off(n + 1, 0);
    std::vector<MtLoadStep> plan;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t s0 = B->seg_offsets[i], s1 = B->seg_offsets[i + 1];
        if (B->doc_ids[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
        if (s1 < s0 || s1 > nseg || B->header_segments[i] > s1 - s0) { c->err = "bad seg_offsets/header_segments"; return MT_E_INVALID; }
        uint64_t expect = ~0ull;                          // text payloads contiguous per document
        for (uint32_t k = s0; k < s1; k++) {
            const mt_load_seg& g = B->segs[k];
            if (g.flags & MT_LS_MARKER) continue;
            if ((uint64_t)g.payload_off + g.payload_len > B->payload_units) { c->err = "payload out of range"; return MT_E_INVALID; }
            if (expect != ~0ull && g.payload_off != expect) { c->err = "document text payloads must be contiguous"; return MT_E_INVALID; }
            expect = (uint64_t)g.payload_off + g.payload_len;
        }
        for (uint32_t k = s0; k < s1; k++)
            if (B->segs[k].prop_id >= 0 && (uint32_t)B->segs[k].prop_id >= c->S.p_nsets) { c->err = "prop_id out of range (mt_set_props first)"; return MT_E_INVALID; }
        plan_off[i] = (uint32_t)plan.size();
        mt_load_plan(B, i, plan);
    }
    plan_off[n] = (uint32_t)plan.size();
    for (uint32_t i = 0; i < n; i++) {            // loaded maps count toward the documents' keys
        const uint32_t d = B->doc_ids[i];
        if (d < c->doc_wide.size()) { c->doc_wide[d] = 0; c->doc_keys[d].clear(); }
        for (uint32_t k = B->seg_offsets[i]; k < B->seg_offsets[i + 1]; k++)
            if (mt_note_set(c, d, B->segs[k].prop_id)) break;
    }
    for (uint32_t i = 0; i < n; i++) {
        meta[i] = B->doc_ids[i]; meta[n + i] = B->seg_offsets[i];
        meta[2ull * n + 1 + i] = B->header_segments[i];
        meta[3ull * n + 1 + i] = (uint32_t)B->min_seq[i]; meta[4ull * n + 1 + i] = (uint32_t)B->seq[i];
    }
    meta[2ull * n] = nseg;
    int rc;
#define UP(buf, src, bytes) if ((rc = mtb_ensure(c, c->buf, (bytes)))) return rc; if ((bytes) && (src)) mtb_h2d(c, c->buf.p, (src), (bytes));
    static_assert(sizeof(mt_load_seg) == sizeof(MtLoadSeg) && sizeof(MtLoadSeg) == 32, "load segment layout");
    UP(b_ld_meta, meta.data(), 4 * meta.size()) UP(b_ld_seg, B->segs, sizeof(MtLoadSeg) * nseg)
    UP(b_ld_pay, B->payload, 2 * B->payload_units) UP(b_ld_plan, plan.data(), sizeof(MtLoadStep) * plan.size())
    UP(b_ld_poff, plan_off.data(), 4ull * (n + 1))
#undef UP
    MtLoad L;
    const uint32_t* m = (const uint32_t*)c->b_ld_meta.p;
    L.docs = m; L.seg_off = m + n; L.nhdr = m + 2 * n + 1;
    L.ms = (const int32_t*)(m + 3 * n + 1); L.cs = (const int32_t*)(m + 4 * n + 1);
    L.segs = (const MtLoadSeg*)c->b_ld_seg.p; L.payload = (const uint16_t*)c->b_ld_pay.p;
    L.plan_off = (const uint32_t*)c->b_ld_poff.p; L.plan = (const MtLoadStep*)c->b_ld_plan.p;
    return mtb_launch_load(c, L, n);
}
static int mt_delta_size(mt_ctx* c, uint64_t capacity);
int MT_FN(delta_capture)(mt_ctx* c, uint64_t capacity) {
    if (!c) return MT_E_INVALID;
    return mt_delta_size(c, capacity);
}
// The capture buffers for `capacity` records, no smaller than the largest document's message
// bound (sized again when a document's capacities change: mt_rederive).
static int mt_delta_size(mt_ctx* c, uint64_t capacity) {
    c->delta_cap = 0; c->delta_tcap = 0; c->delta_req = capacity;
    if (capacity) {
        // one message of the largest document must fit a launch: its range (<= rowCap
        // records) plus the fixed slack; a paste's text is <= the document's text capacity
        uint64_t minr = MT_DREC_SLACK, mint = 1;
        for (const MtDocLayout& y : c->layout_h) {
            minr = std::max<uint64_t>(minr, (uint64_t)y.rowCap + MT_DREC_SLACK);
            mint = std::max<uint64_t>(mint, (uint64_t)y.textCap);
        }
        const uint64_t cap = std::max<uint64_t>(capacity, minr), tcap = std::max<uint64_t>(4 * capacity, mint);
        int rc;
        if ((rc = mtb_ensure(c, c->b_drec, sizeof(MtDeltaRec) * cap))) return rc;
        if ((rc = mtb_ensure(c, c->b_dcount, 32))) return rc;
        if ((rc = mtb_ensure(c, c->b_dtext, 2 * tcap))) return rc;
        c->delta_cap = cap; c->delta_tcap = tcap;
    }
    return MT_OK;
}
int MT_FN(delta_records)(mt_ctx* c, const mt_delta_rec** out, uint64_t* n) {
    static_assert(sizeof(mt_delta_rec) == sizeof(MtDeltaRec), "delta record layout");
    if (!c || !out || !n || !c->delta_cap) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    if (!c->delta_valid) {
        // documents interleave in the buffer; one wave appends a document's records in
        // program order (and later launches of a run follow earlier ones), so a stable sort
        // by op index restores callback order
        std::stable_sort(c->delta_host.begin(), c->delta_host.end(),
                         [](const MtDeltaRec& x, const MtDeltaRec& y) { return x.op < y.op; });
        c->delta_valid = true;
    }
    *out = (const mt_delta_rec*)c->delta_host.data();
    *n = c->delta_host.size();
    if (c->delta_over) { c->err = "delta capture capacity exceeded"; return MT_E_OOM; }
    return MT_OK;
}
int MT_FN(delta_text)(mt_ctx* c, const uint16_t** out, uint64_t* n, uint32_t* launches) {
    if (!c || !out || !n || !c->delta_cap) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    *out = c->delta_text.data();
    *n = c->delta_text.size();
    if (launches) *launches = c->delta_launches;
    return MT_OK;
}
int MT_FN(doc_pset)(mt_ctx* c, uint32_t doc, int32_t id, uint16_t* keys, int32_t* vals, uint32_t* n) {
    if (!c || doc >= c->S.maxDocs || !keys || !vals || !n || id < 0) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    const MtDocLayout& y = c->layout_h[doc];
    if ((uint32_t)id >= y.psetCap) return MT_E_INVALID;
    MtPSet p[MT_PKEYS / MT_PSK];
    mtb_d2h(c, p, c->S.pset + y.pset + (size_t)id, sizeof(MtPSet));
    const uint32_t nk = p[0].n < 0 ? 0u : ((uint32_t)p[0].n > MT_PKEYS ? MT_PKEYS : (uint32_t)p[0].n);
    const uint32_t nch = nk > MT_PSK ? (nk + MT_PSK - 1) / MT_PSK : 1;
    if ((uint32_t)id + nch > y.psetCap) return MT_E_INVALID;
    if (nch > 1) mtb_d2h(c, p + 1, c->S.pset + y.pset + (size_t)id + 1, sizeof(MtPSet) * (nch - 1));
    *n = nk;
    for (uint32_t i = 0; i < nk; i++) { keys[i] = p[i >> 4].key[i & 15]; vals[i] = p[i >> 4].val[i & 15]; }
    return MT_OK;
}
int MT_FN(set_size_class)(mt_ctx* c, uint32_t big_min_ops) {
    if (!c) return MT_E_INVALID;
    c->big_min_ops = big_min_ops;
    c->part_cus = 0; c->part_auto = false;
    return MT_OK;
}
int MT_FN(set_continuation)(mt_ctx* c, uint32_t min_ops) {
    if (!c) return MT_E_INVALID;
    c->cont_min_ops = min_ops;
    return MT_OK;
}
int MT_FN(set_partition)(mt_ctx* c, uint32_t min_ops, uint32_t cus) {
    if (!c) return MT_E_INVALID;
    c->part_auto = min_ops == MT_PARTITION_AUTO;
    c->auto_gen = ~0ull;
    c->big_min_ops = c->part_auto ? 0 : min_ops;
    c->part_cus = (min_ops && !c->part_auto) ? cus : 0;
    return MT_OK;
}
int MT_FN(plan_partition)(const uint32_t* run_ops, uint32_t n, uint32_t n_cus, uint32_t* min_ops, uint32_t* cus,
                          double* est_ms) {
    if ((n && !run_ops) || !min_ops || !cus || n_cus == 0) return MT_E_INVALID;
    double us = 0;
    mt_plan_partition_impl(run_ops, n, n_cus, min_ops, cus, &us);
    if (est_ms) *est_ms = us / 1e3;
    return MT_OK;
}
int MT_FN(last_partition)(mt_ctx* c, uint32_t* min_ops, uint32_t* cus) {
    if (!c || !min_ops || !cus) return MT_E_INVALID;
    *min_ops = c->part_cus ? c->big_min_ops : 0; *cus = c->part_cus;
    return MT_OK;
}
int MT_FN(set_residency)(mt_ctx* c, int use_lds, int rows, int blocks, int heap) {
    const int maxHeap = use_lds == 3 ? MT_G_HEAP : (use_lds == 2 ? MT_B_HEAP : MT_L_HEAP);
    if (!c || use_lds < 0 || use_lds > 3 || rows < 0 || blocks < 0 || heap < 0 ||
        rows > (use_lds == 3 ? MT_G_WIN : MT_L_ROWS) ||
        blocks > (use_lds == 2 ? MT_B_BLKS : (use_lds == 3 ? 15 : MT_L_BLKS)) || heap > maxHeap)
        return MT_E_INVALID;
    c->use_lds = use_lds;
    c->lds_rows = rows ? rows : (use_lds == 3 ? MT_G_WIN : MT_L_ROWS);   // 3: window entries in LDS
    // 3: blocks = MT_BIGF_* switches (bit 0 reserved, no effect; zamboni prefetch, corrections table, parent cache off; A/B)
    c->lds_blks = use_lds == 3 ? blocks : (blocks ? blocks : (use_lds == 2 ? MT_B_BLKS : MT_L_BLKS));
    c->lds_heap = heap ? heap : maxHeap;
    return MT_OK;
}
// Where each run of the last LDS-resident replay handed over to the HBM kernel
// (op index; op_offsets[run+1] = finished in LDS).  Diagnostic.
int MT_FN(last_cursors)(mt_ctx* c, uint32_t n, uint32_t* out) {
    if (!c || !out || n > c->n_runs || !c->b_cursor.p) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    mtb_d2h(c, out, c->b_cursor.p, 4ull * n);
    return MT_OK;
}
int MT_FN(last_replay_ms)(mt_ctx* c, float* ms) { if (!c || !ms) return MT_E_INVALID; *ms = c->last_ms; return MT_OK; }
int MT_FN(sync)(mt_ctx* c) { if (!c) return MT_E_INVALID; return mtb_sync(c); }

static int mt_read_hdrs(mt_ctx* c, uint32_t n, const uint32_t* docs, std::vector<MtDocHdr>& h) {
    h.resize(n);
    mtb_sync(c);
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (docs[i] >= c->S.maxDocs) return MT_E_INVALID;
        lo = docs[i] < lo ? docs[i] : lo; hi = docs[i] > hi ? docs[i] : hi;
    }
    if (n == 0) return MT_OK;
    if (n < 8) {
        for (uint32_t i = 0; i < n; i++) mtb_d2h(c, &h[i], c->S.hdr + docs[i], sizeof(MtDocHdr));
        return MT_OK;
    }
    std::vector<MtDocHdr> all((size_t)(hi - lo + 1));      // one copy of the covering header range
    mtb_d2h(c, all.data(), c->S.hdr + lo, sizeof(MtDocHdr) * all.size());
    for (uint32_t i = 0; i < n; i++) h[i] = all[docs[i] - lo];
    return MT_OK;
}
int MT_FN(doc_pools)(mt_ctx* c, uint32_t n, const uint32_t* docs, int32_t* out) {
    if (!c || (n && (!docs || !out))) return MT_E_INVALID;
    std::vector<MtDocHdr> h;
    int rc = mt_read_hdrs(c, n, docs, h);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
        int32_t* o = out + 10 * (size_t)i;
        o[0] = h[i].rowTop; o[1] = h[i].blkTop; o[2] = h[i].heapN; o[3] = h[i].winN;
        o[4] = h[i].textTop; o[5] = h[i].psetTop; o[6] = h[i].height; o[7] = h[i].rfN;
        o[8] = h[i].heapHW; o[9] = h[i].winHW;
    }
    return MT_OK;
}
int MT_FN(doc_status)(mt_ctx* c, uint32_t n, const uint32_t* docs, uint32_t* out) {
    std::vector<MtDocHdr> h;
    int rc = mt_read_hdrs(c, n, docs, h);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) out[i] = h[i].status;
    return MT_OK;
}
int MT_FN(doc_counters_get)(mt_ctx* c, uint32_t n, const uint32_t* docs, mt_doc_counters* out) {
    std::vector<MtDocHdr> h;
    int rc = mt_read_hdrs(c, n, docs, h);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
        out[i].ops = h[i].cnt[0]; out[i].msgs = h[i].cnt[1]; out[i].ins_units = h[i].cnt[2];
        out[i].rows_rw = h[i].cnt[3]; out[i].depth = h[i].cnt[4]; out[i].scoured = h[i].cnt[5];
    }
    return MT_OK;
}

int MT_FN(update_seq)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* msn, const int32_t* seq) {
    if (!c) return MT_E_INVALID;
    int rc;
    if ((rc = mtb_ensure(c, c->b_tmp0, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp1, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp2, 4ull * n))) return rc;
    mtb_h2d(c, c->b_tmp0.p, docs, 4ull * n); mtb_h2d(c, c->b_tmp1.p, msn, 4ull * n); mtb_h2d(c, c->b_tmp2.p, seq, 4ull * n);
    return mtb_launch_update_seq(c, (const uint32_t*)c->b_tmp0.p, (const int32_t*)c->b_tmp1.p, (const int32_t*)c->b_tmp2.p, n);
}

int MT_FN(get_length)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* ref, const int32_t* cli, int32_t* out) {
    if (!c) return MT_E_INVALID;
    int rc;
    if ((rc = mtb_ensure(c, c->b_tmp0, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp1, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp2, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp3, 4ull * n))) return rc;
    mtb_h2d(c, c->b_tmp0.p, docs, 4ull * n); mtb_h2d(c, c->b_tmp1.p, ref, 4ull * n); mtb_h2d(c, c->b_tmp2.p, cli, 4ull * n);
    rc = mtb_launch_get_length(c, (const uint32_t*)c->b_tmp0.p, (const int32_t*)c->b_tmp1.p, (const int32_t*)c->b_tmp2.p,
                               (int32_t*)c->b_tmp3.p, n);
    if (rc) return rc;
    mtb_sync(c);
    mtb_d2h(c, out, c->b_tmp3.p, 4ull * n);
    return MT_OK;
}

// Position queries (mt_query.h): sorted by document (stable), one wave per document's group,
// answers back in query order; the found segments' text gathered on the device, their JSON
// written here from the text and the property-map chunks the kernel copied.
// kind: MT_QK_LOCAL for position queries (a caller's ref_seq < 0 is the local view whatever its
// value), else the tile-search kind every query of the call carries in `ref` (mt_query.h).
// A call's arguments beyond the pools travel in an MtQueryCall that the entry point builds on its
// stack and every launch takes by value: nothing here writes c->S.
// The staging both query paths share: the queries sorted by document into q (ord[k]: the caller's
// index of sorted query k), their groups uploaded with them.  ng: the groups.
static int mt_stage_queries(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* pos, const int32_t* ref,
                            const int32_t* cli, int kind, std::vector<uint32_t>& ord, std::vector<MtQuery>& q, uint32_t& ng) {
    for (uint32_t i = 0; i < n; i++) if (docs[i] >= c->S.maxDocs) { c->err = "query document out of range"; return MT_E_INVALID; }
    ord.resize(n);
    for (uint32_t i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return docs[a] < docs[b]; });
    q.resize(n);
    std::vector<uint32_t> grp;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = ord[k];
        q[k].doc = docs[i]; q[k].pos = pos ? pos[i] : (int32_t)i; q[k].client = cli ? cli[i] : -1;
        q[k].ref = kind != MT_QK_LOCAL ? kind : ((ref && ref[i] >= 0) ? ref[i] : MT_QK_LOCAL);
        if (k == 0 || docs[i] != docs[ord[k - 1]]) grp.push_back(k);
    }
    grp.push_back(n);
    ng = (uint32_t)grp.size() - 1;
    int rc;
    if ((rc = mtb_ensure(c, c->b_q, sizeof(MtQuery) * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_qgrp, 4ull * (ng + 1)))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    mtb_h2d(c, c->b_q.p, q.data(), sizeof(MtQuery) * n);
    mtb_h2d(c, c->b_qgrp.p, grp.data(), 4ull * (ng + 1));
    return MT_OK;
}
#ifndef MTB_HAVE_QUERY
// A backend whose pools the host addresses (the emulation) takes this plain loop over the groups;
// the HIP backend defines its own over the kernel and MTB_HAVE_QUERY.
static int mtb_launch_query(mt_ctx* c, const MtQueryCall& call, const MtQuery* q, const uint32_t* grp, MtQueryOut* out, uint32_t n_groups) {
    for (uint32_t g = 0; g < n_groups; g++) {
        MtScratch sc; MtEngFast e; e.bind(c->S, q[grp[g]].doc, &sc);
        mt_query_run(e, c->S, call, q, grp[g], grp[g + 1], out);
    }
    return MT_OK;
}
#endif
static int mt_run_queries(mt_ctx* c, const MtQueryCall& call, uint32_t n, const uint32_t* docs, const int32_t* pos,
                          const int32_t* ref, const int32_t* cli, std::vector<MtQueryOut>& res, int kind = MT_QK_LOCAL) {
    res.assign(n, MtQueryOut{});
    if (n == 0) return MT_OK;
    std::vector<uint32_t> ord;
    std::vector<MtQuery> q;
    uint32_t ng = 0;
    int rc;
    if ((rc = mt_stage_queries(c, n, docs, pos, ref, cli, kind, ord, q, ng))) return rc;
    if ((rc = mtb_ensure(c, c->b_qout, sizeof(MtQueryOut) * n))) return rc;
    if ((rc = mtb_launch_query(c, call, (const MtQuery*)c->b_q.p, (const uint32_t*)c->b_qgrp.p, (MtQueryOut*)c->b_qout.p, ng))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    std::vector<MtQueryOut> tmp(n);
    mtb_d2h(c, tmp.data(), c->b_qout.p, sizeof(MtQueryOut) * n);
    for (uint32_t k = 0; k < n; k++) res[ord[k]] = tmp[k];
    return MT_OK;
}

// The found segments' JSON (toJSONObject) into the library-owned arena: their text gathered on
// the device, the property maps from the chunks the kernel copied.
static int mt_seg_json(mt_ctx* c, uint32_t n, const std::vector<MtQueryOut>& res, const char** json_arena,
                       const uint64_t** json_off) {
    if (!json_arena) return MT_OK;
    int rc;
    // text of the found text segments, gathered on the device into one arena
    std::vector<unsigned long long> at, off(1, 0);
    std::vector<uint32_t> len, which;
    for (uint32_t i = 0; i < n; i++) {
        const mt_seg_info& f = res[i].info;
        if (!f.found || f.marker_ref_type >= 0 || f.len <= 0) continue;
        at.push_back(res[i].text_at); len.push_back((uint32_t)f.len); which.push_back(i);
        off.push_back(off.back() + (unsigned long long)f.len);
    }
    std::vector<uint16_t> txt(off.back());
    const uint32_t m = (uint32_t)len.size();
    if (m) {
        if ((rc = mtb_ensure(c, c->b_qat, 8ull * m))) return rc;
        if ((rc = mtb_ensure(c, c->b_qlen, 4ull * m))) return rc;
        if ((rc = mtb_ensure(c, c->b_qoff, 8ull * m))) return rc;
        if ((rc = mtb_ensure(c, c->b_qtext, 2ull * off.back()))) return rc;
        mtb_h2d(c, c->b_qat.p, at.data(), 8ull * m);
        mtb_h2d(c, c->b_qlen.p, len.data(), 4ull * m);
        mtb_h2d(c, c->b_qoff.p, off.data(), 8ull * m);
        if ((rc = mtb_launch_gather_text(c, (const unsigned long long*)c->b_qat.p, (const uint32_t*)c->b_qlen.p,
                                         (const unsigned long long*)c->b_qoff.p, (uint16_t*)c->b_qtext.p, m))) return rc;
        if ((rc = mtb_sync(c))) return rc;
        mtb_d2h(c, txt.data(), c->b_qtext.p, 2ull * off.back());
    }
    std::vector<int64_t> slot(n, -1);
    for (uint32_t k = 0; k < m; k++) slot[which[k]] = k;
    c->seg_json_arena.clear(); c->seg_json_off.assign(1, 0);
    for (uint32_t i = 0; i < n; i++) {
        const mt_seg_info& f = res[i].info;
        if (f.found) {
            const bool marker = f.marker_ref_type >= 0;
            const int64_t k = slot[i];
            std::string pj;
            if (f.prop_set >= 0) mtsnap::props_json(pj, res[i].ps, c->names);
            mtsnap::seg_json_of(c->seg_json_arena, marker, f.marker_ref_type, f.prop_set >= 0 ? &pj : nullptr,
                                k >= 0 ? txt.data() + off[k] : nullptr, k >= 0 ? (size_t)len[k] : 0);
        }
        c->seg_json_off.push_back(c->seg_json_arena.size());
    }
    *json_arena = c->seg_json_arena.data();
    if (json_off) *json_off = c->seg_json_off.data();
    return MT_OK;
}

int MT_FN(get_containing_segment)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* pos, const int32_t* ref,
                                  const int32_t* cli, mt_seg_info* out, const char** json_arena, const uint64_t** json_off) {
    if (!c || (n && (!docs || !pos))) return MT_E_INVALID;
    std::vector<MtQueryOut> res;
    int rc = mt_run_queries(c, MtQueryCall{}, n, docs, pos, ref, cli, res);
    if (rc) return rc;
    if (out) for (uint32_t i = 0; i < n; i++) out[i] = res[i].info;
    return mt_seg_json(c, n, res, json_arena, json_off);
}

// Tile search (mt_query.h): the labels' match arrays go to the device and into the call, where
// the query kernel's tile kinds read them.
static int mt_tile_setup(mt_ctx* c, const mt_tile_labels* T, uint32_t n, const uint32_t* label, MtQueryCall& call) {
    if (!T || (T->n_labels && T->n_values && !T->match)) { c->err = "tile labels missing"; return MT_E_INVALID; }
    if (T->n_values != c->names.value_json.size()) { c->err = "tile labels: n_values differs from the uploaded prop table"; return MT_E_INVALID; }
    if (T->n_labels >= (uint32_t)MT_QT_PRECEDING) { c->err = "too many tile labels"; return MT_E_INVALID; }
    for (uint32_t i = 0; i < n; i++) if (label[i] >= T->n_labels) { c->err = "tile label out of range"; return MT_E_INVALID; }
    const size_t bytes = (size_t)T->n_labels * T->n_values;
    int rc;
    if ((rc = mtb_ensure(c, c->b_tmatch, bytes + 1))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    if (bytes) mtb_h2d(c, c->b_tmatch.p, T->match, bytes);
    call.match = (const uint8_t*)c->b_tmatch.p; call.key = T->key; call.nvalues = T->n_values;
    return MT_OK;
}

int MT_FN(find_tile)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* pos, const uint8_t* flags,
                     const uint32_t* label, const mt_tile_labels* labels, mt_seg_info* out, const char** json_arena,
                     const uint64_t** json_off) {
    if (!c || (n && (!docs || !pos || !label))) return MT_E_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (pos[i] < 0 && pos[i] != MT_POS_UNDEFINED) { c->err = "findTile: negative start position"; return MT_E_INVALID; }
    MtQueryCall call{};
    int rc = mt_tile_setup(c, labels, n, label, call);
    if (rc) return rc;
    std::vector<int32_t> arg(n);
    for (uint32_t i = 0; i < n; i++) arg[i] = (int32_t)label[i] | ((flags && (flags[i] & MT_TILE_PRECEDING)) ? MT_QT_PRECEDING : 0);
    std::vector<MtQueryOut> res;
    if ((rc = mt_run_queries(c, call, n, docs, pos, nullptr, arg.data(), res, MT_QK_TILE))) return rc;
    if (out) for (uint32_t i = 0; i < n; i++) out[i] = res[i].info;
    return mt_seg_json(c, n, res, json_arena, json_off);
}

int MT_FN(tile_index)(mt_ctx* c, uint32_t n, const uint32_t* docs, const uint32_t* label, const mt_tile_labels* labels,
                      const mt_tile_rec** recs, const uint64_t** rec_off) {
    if (!c || !recs || !rec_off || (n && (!docs || !label))) return MT_E_INVALID;
    MtQueryCall call{};
    int rc = mt_tile_setup(c, labels, n, label, call);
    if (rc) return rc;
    // two passes over the same scan, as mt_pack_size / mt_pack_doc: count, then fill at the
    // offsets the counts give
    std::vector<int32_t> at(n, 0), arg(label, label + n);
    std::vector<MtQueryOut> res;
    if ((rc = mt_run_queries(c, call, n, docs, at.data(), nullptr, arg.data(), res, MT_QK_TILE_COUNT))) return rc;
    c->tile_off.assign((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) c->tile_off[i + 1] = c->tile_off[i] + (uint64_t)(uint32_t)res[i].info.found;
    const uint64_t total = c->tile_off[n];
    if (total > 0xFFFFFFFFull) { c->err = "tile index: more than 2^32 records"; return MT_E_INVALID; }
    c->tile_recs.assign((size_t)total, mt_tile_rec{});
    if (total) {
        if ((rc = mtb_ensure(c, c->b_tout, sizeof(mt_tile_rec) * total))) return rc;
        call.tiles = (mt_tile_rec*)c->b_tout.p; call.tile_cap = total;
        for (uint32_t i = 0; i < n; i++) at[i] = (int32_t)(uint32_t)c->tile_off[i];
        if ((rc = mt_run_queries(c, call, n, docs, at.data(), nullptr, arg.data(), res, MT_QK_TILE_FILL))) return rc;
        for (uint32_t i = 0; i < n; i++)
            if ((uint64_t)(uint32_t)res[i].info.found != c->tile_off[i + 1] - c->tile_off[i]) { c->err = "tile index: the passes disagree"; return MT_E_INVALID; }
        mtb_d2h(c, c->tile_recs.data(), c->b_tout.p, sizeof(mt_tile_rec) * total);
    }
    *recs = c->tile_recs.data();
    *rec_off = c->tile_off.data();
    return MT_OK;
}

// The range queries (mt_query.h: text ranges and segment walks, two visitors of one scan) share
// their records and the two passes over them: the queries staged by document once, the records up
// once per pass (the fill's carry the offsets the counts gave: off[i] for query i's answer, and the
// same for a walk's text), each pass one launch of the query kernel, with `count_kind` and then the
// fill kind below it.  The kernel's answer records are not used by the range kinds, so none is
// allocated or downloaded.  call: the entry point's record, which has the placeholder or the walk's
// flags and here gains the query records and the fill's outputs: a walk's records in b_wout and its
// text in b_wtext, a text range's units in b_xout.  total / ttotal: the answers' and the walk's
// text's lengths.
static int mt_range_passes(mt_ctx* c, MtQueryCall& call, const std::string& what, const char* capped, uint32_t n,
                           const uint32_t* docs, const int32_t* start, const int32_t* end, const int32_t* ref, const int32_t* cli,
                           int count_kind, uint64_t* off, uint64_t& total, uint64_t& ttotal) {
    if (n > 0x7FFFFFFFu) { c->err = what + ": too many queries"; return MT_E_INVALID; }
    const bool walk = count_kind == MT_QK_WALK_COUNT;
    std::vector<MtRangeQ> x(n, MtRangeQ{});
    for (uint32_t i = 0; i < n; i++) {
        x[i].start = start ? start[i] : 0; x[i].end = end ? end[i] : MT_POS_UNDEFINED;
        x[i].ref = (ref && ref[i] >= 0) ? ref[i] : -1; x[i].client = cli ? cli[i] : -1;
    }
    std::vector<uint32_t> ord;
    std::vector<MtQuery> q;
    uint32_t ng = 0;
    int rc;
    if ((rc = mt_stage_queries(c, n, docs, nullptr, nullptr, nullptr, count_kind, ord, q, ng))) return rc;
    if ((rc = mtb_ensure(c, c->b_xq, sizeof(MtRangeQ) * n))) return rc;
    auto pass = [&](std::vector<MtRangeQ>& y) {     // the records up, one launch, the records down to y
        mtb_h2d(c, c->b_xq.p, x.data(), sizeof(MtRangeQ) * n);
        int r = mtb_launch_query(c, call, (const MtQuery*)c->b_q.p, (const uint32_t*)c->b_qgrp.p, (MtQueryOut*)c->b_qout.p, ng);
        if (!r) r = mtb_sync(c);
        if (!r) mtb_d2h(c, y.data(), c->b_xq.p, sizeof(MtRangeQ) * n);
        return r;
    };
    call.q = (MtRangeQ*)c->b_xq.p; call.nq = n;
    if ((rc = pass(x))) return rc;
    total = ttotal = 0;
    for (uint32_t i = 0; i < n; i++) {
        x[i].at = total; x[i].tat = ttotal; off[i] = total;
        total += x[i].count; ttotal += x[i].tcount;
        if (total > 0x80000000ull || ttotal > 0x80000000ull) { c->err = what + capped; return MT_E_INVALID; }
    }
    off[n] = total;
    if (!total) return MT_OK;
    const uint64_t units = walk ? ttotal : total;
    mt_ctx::DevBuf& arena = walk ? c->b_wtext : c->b_xout;
    if (walk && (rc = mtb_ensure(c, c->b_wout, sizeof(mt_walk_rec) * total))) return rc;
    if (units && (rc = mtb_ensure(c, arena, 2ull * units))) return rc;
    if (walk) { call.recs = (mt_walk_rec*)c->b_wout.p; call.rec_cap = total; }
    if (units) { call.text = (uint16_t*)arena.p; call.text_cap = units; }
    for (uint32_t k = 0; k < n; k++) q[k].ref = count_kind - 1;
    mtb_h2d(c, c->b_q.p, q.data(), sizeof(MtQuery) * n);
    std::vector<MtRangeQ> y(n);
    if ((rc = pass(y))) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (y[i].filled != x[i].count || y[i].tfilled != x[i].tcount) { c->err = what + ": the passes disagree"; return MT_E_INVALID; }
    return MT_OK;
}
static_assert(MT_QK_TEXT_FILL == MT_QK_TEXT_COUNT - 1 && MT_QK_WALK_FILL == MT_QK_WALK_COUNT - 1, "a fill kind lies below its count kind");

// Text ranges: the text comes down once.
int MT_FN(get_text_range)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* start, const int32_t* end,
                          const int32_t* ref, const int32_t* cli, const uint16_t* placeholder, uint32_t placeholder_len,
                          const uint16_t** arena, const uint64_t** off) {
    if (!c || !arena || !off || (n && !docs) || (placeholder_len && !placeholder)) return MT_E_INVALID;
    if (placeholder_len > MT_TEXT_PLACEHOLDER_MAX) { c->err = "text range: the placeholder is longer than MT_TEXT_PLACEHOLDER_MAX units"; return MT_E_INVALID; }
    c->range_off.assign((size_t)n + 1, 0);
    c->range_arena.clear();
    *arena = c->range_arena.data(); *off = c->range_off.data();
    if (n == 0) return MT_OK;
    MtQueryCall call{};
    call.phlen = placeholder_len;
    for (uint32_t k = 0; k < MT_TEXT_PLACEHOLDER_MAX / 2; k++) {
        const uint32_t a = 2 * k < placeholder_len ? placeholder[2 * k] : 0u, b = 2 * k + 1 < placeholder_len ? placeholder[2 * k + 1] : 0u;
        call.ph[k] = a | (b << 16);
    }
    uint64_t total = 0, ttotal = 0;
    const int rc = mt_range_passes(c, call, "text range", ": the answers hold more than 2^31 units; split the call", n, docs, start, end,
                                   ref, cli, MT_QK_TEXT_COUNT, c->range_off.data(), total, ttotal);
    if (rc) return rc;
    c->range_arena.resize((size_t)total);
    if (total) mtb_d2h(c, c->range_arena.data(), c->b_xout.p, 2ull * total);
    *arena = c->range_arena.data(); *off = c->range_off.data();
    return MT_OK;
}

// Segment walks: the walk's records and text come down once.  Then the distinct (document,
// prop_set) pairs the records name are fetched by one more launch of the query kernel (MT_QK_PSET
// copies a map's chunks, packed, into a buffer the call names) and written out once each.
int MT_FN(walk_segments)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* start, const int32_t* end,
                         const int32_t* ref, const int32_t* cli, uint32_t flags, const mt_walk_rec** recs, const uint64_t** rec_off,
                         const uint16_t** text_arena, const mt_walk_maps** maps) {
    if (!c || !recs || !rec_off || (n && !docs)) return MT_E_INVALID;
    if (flags & ~MT_WALK_TEXT) { c->err = "walk: unknown flags"; return MT_E_INVALID; }
    const bool text = (flags & MT_WALK_TEXT) && text_arena;
    c->walk_off.assign((size_t)n + 1, 0);
    c->walk_recs.clear(); c->walk_arena.clear();
    c->walk_map_doc.clear(); c->walk_map_ps.clear(); c->walk_map_key.clear(); c->walk_map_val.clear(); c->walk_map_json.clear();
    c->walk_map_koff.assign(1, 0); c->walk_map_joff.assign(1, 0);
    auto give = [&]() {
        *recs = c->walk_recs.data(); *rec_off = c->walk_off.data();
        if (text_arena) *text_arena = c->walk_arena.data();
        c->walk_maps.n = (uint32_t)c->walk_map_doc.size();
        c->walk_maps.doc = c->walk_map_doc.data(); c->walk_maps.prop_set = c->walk_map_ps.data();
        c->walk_maps.key_off = c->walk_map_koff.data(); c->walk_maps.key = c->walk_map_key.data();
        c->walk_maps.value = c->walk_map_val.data(); c->walk_maps.json_off = c->walk_map_joff.data();
        c->walk_maps.json = c->walk_map_json.data();
        if (maps) *maps = &c->walk_maps;
    };
    give();
    if (n == 0) return MT_OK;
    for (uint32_t i = 0; i < n; i++)
        for (const int32_t v : {start ? start[i] : 0, end ? end[i] : 0})
            if (v != MT_POS_UNDEFINED && (v < -(1 << 30) || v > (1 << 30))) { c->err = "walk: start / end outside [-2^30, 2^30]"; return MT_E_INVALID; }
    MtQueryCall call{};
    call.flags = text ? MT_WALK_TEXT : 0u;
    auto fail = [&](int r) { c->walk_off.assign((size_t)n + 1, 0); return r; };
    uint64_t total = 0, ttotal = 0;
    int rc = mt_range_passes(c, call, "walk", ": the answers hold more than 2^31 records or text units; split the call", n, docs, start,
                             end, ref, cli, MT_QK_WALK_COUNT, c->walk_off.data(), total, ttotal);
    if (rc) return fail(rc);
    if (!total) return MT_OK;
    c->walk_recs.resize((size_t)total);
    mtb_d2h(c, c->walk_recs.data(), c->b_wout.p, sizeof(mt_walk_rec) * total);
    c->walk_arena.resize((size_t)ttotal);
    if (ttotal) mtb_d2h(c, c->walk_arena.data(), c->b_wtext.p, 2ull * ttotal);
    // the distinct maps, in the order the records first name them; the fill left each map's key
    // count in the record's `map`, which places the maps' chunks
    std::unordered_map<uint64_t, int32_t> seen;
    std::vector<int32_t> mpos, mat, mkeys;
    uint64_t chunks = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint64_t k = c->walk_off[i]; k < c->walk_off[i + 1]; k++) {
            mt_walk_rec& w = c->walk_recs[(size_t)k];
            if (!maps || w.prop_set < 0) { w.map = -1; continue; }
            const uint64_t key = ((uint64_t)docs[i] << 32) | (uint32_t)w.prop_set;
            auto it = seen.find(key);
            if (it == seen.end()) {
                it = seen.emplace(key, (int32_t)c->walk_map_doc.size()).first;
                const uint32_t nk = w.map < 0 ? 0u : ((uint32_t)w.map > MT_PKEYS ? MT_PKEYS : (uint32_t)w.map);
                c->walk_map_doc.push_back(docs[i]); c->walk_map_ps.push_back(w.prop_set);
                mpos.push_back(w.prop_set); mat.push_back((int32_t)chunks); mkeys.push_back((int32_t)nk);
                chunks += nk > MT_PSK ? (nk + MT_PSK - 1) / MT_PSK : 1;
                if (chunks > 0x7FFFFFFFull) { c->err = "walk: the distinct maps hold more than 2^31 chunks; split the call"; return fail(MT_E_INVALID); }
            }
            w.map = it->second;
        }
    if (!c->walk_map_doc.empty()) {
        const uint32_t m = (uint32_t)c->walk_map_doc.size();
        std::vector<uint32_t> ord;
        std::vector<MtQuery> q;
        uint32_t ng = 0;
        if ((rc = mt_stage_queries(c, m, c->walk_map_doc.data(), mpos.data(), nullptr, mat.data(), MT_QK_PSET, ord, q, ng))) return fail(rc);
        if ((rc = mtb_ensure(c, c->b_wmaps, sizeof(MtPSet) * chunks))) return fail(rc);
        call.maps = (MtPSet*)c->b_wmaps.p; call.map_cap = chunks;
        rc = mtb_launch_query(c, call, (const MtQuery*)c->b_q.p, (const uint32_t*)c->b_qgrp.p, (MtQueryOut*)c->b_qout.p, ng);
        if (!rc) rc = mtb_sync(c);
        if (rc) return fail(rc);
        std::vector<MtPSet> got((size_t)chunks);
        mtb_d2h(c, got.data(), c->b_wmaps.p, sizeof(MtPSet) * chunks);
        c->walk_map_key.reserve((size_t)chunks * MT_PSK); c->walk_map_val.reserve((size_t)chunks * MT_PSK);
        for (uint32_t k = 0; k < m; k++) {
            const MtPSet* p = got.data() + mat[k];
            const uint32_t nk = (uint32_t)mkeys[k];
            if (p[0].n != mkeys[k]) { c->err = "walk: the passes disagree on a property map"; return fail(MT_E_INVALID); }
            for (uint32_t j = 0; j < nk; j++) { c->walk_map_key.push_back(p[j >> 4].key[j & 15]); c->walk_map_val.push_back(p[j >> 4].val[j & 15]); }
            c->walk_map_koff.push_back(c->walk_map_key.size());
            mtsnap::props_json(c->walk_map_json, p, c->names);
            c->walk_map_joff.push_back(c->walk_map_json.size());
        }
    }
    give();
    return MT_OK;
}

int MT_FN(resolve_remote_position)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* pos, const int32_t* ref,
                                   const int32_t* cli, int32_t* out) {
    if (!c || (n && (!docs || !pos || !out))) return MT_E_INVALID;
    std::vector<MtQueryOut> res;
    int rc = mt_run_queries(c, MtQueryCall{}, n, docs, pos, ref, cli, res);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) out[i] = res[i].info.resolved;
    return MT_OK;
}

// Host copy of one document's state (for serialization).
struct MtHostDoc {
    MtDocHdr hdr;
    std::vector<MtRow> rows;
    std::vector<MtBlk> blk; std::vector<uint16_t> text; std::vector<MtPSet> pset;
    MtSnapView view() const {
        MtSnapView v; v.hdr = hdr; v.R = rows.data(); v.blk = blk.data(); v.text = text.data(); v.pset = pset.data();
        return v;
    }
};
static int mt_download_doc(mt_ctx* c, uint32_t d, MtHostDoc& h) {
    const MtState& S = c->S;
    const MtDocLayout& y = c->layout_h[d];
    mtb_d2h(c, &h.hdr, S.hdr + d, sizeof(MtDocHdr));
    const size_t R = (size_t)h.hdr.rowTop;
    h.rows.resize(R + 1);
    if (R) mtb_d2h(c, h.rows.data(), S.rows + y.row, sizeof(MtRow) * R);
    h.blk.resize((size_t)h.hdr.blkTop + 1);
    mtb_d2h(c, h.blk.data(), S.blk + y.blk, sizeof(MtBlk) * (size_t)h.hdr.blkTop);
    h.text.resize((size_t)h.hdr.textTop + 1);
    if (h.hdr.textTop) mtb_d2h(c, h.text.data(), S.text + y.text + (size_t)h.hdr.textHalf * y.textCap, 2 * (size_t)h.hdr.textTop);
    h.pset.resize((size_t)h.hdr.psetTop + 1);
    if (h.hdr.psetTop) mtb_d2h(c, h.pset.data(), S.pset + y.pset, sizeof(MtPSet) * (size_t)h.hdr.psetTop);
    return MT_OK;
}

// Gather documents' live state into host memory with two kernels and one copy
// (mt_pack.h); views[i] points into `host`.
static int mt_stage_docs(mt_ctx* c, uint32_t n, const uint32_t* docs, std::vector<MtSnapView>& views, int buf = 0) {
    views.clear();
    if (n == 0) return MT_OK;
    for (uint32_t i = 0; i < n; i++) if (docs[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
    int rc;
    if ((rc = mtb_ensure(c, c->b_pack_docs, 4ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_pack_sz, sizeof(MtPackSize) * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_pack_off, 8ull * n))) return rc;
    mtb_h2d(c, c->b_pack_docs.p, docs, 4ull * n);
    const uint32_t epoch = ++c->stage_epoch;
    if ((rc = mtb_launch_pack_size(c, (const uint32_t*)c->b_pack_docs.p, (MtPackSize*)c->b_pack_sz.p, n, epoch))) return rc;
    std::vector<MtPackSize> sz(n);
    mtb_d2h(c, sz.data(), c->b_pack_sz.p, sizeof(MtPackSize) * n);
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) off[i + 1] = off[i] + mt_pack_bytes(sz[i]);
    if ((rc = mtb_ensure(c, c->b_stage, off[n] + 16))) return rc;
    mtb_h2d(c, c->b_pack_off.p, off.data(), 8ull * n);
    if ((rc = mtb_launch_pack(c, (const uint32_t*)c->b_pack_docs.p, (const uint64_t*)c->b_pack_off.p, (uint8_t*)c->b_stage.p, n,
                              epoch))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = mtb_sync(c))) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    uint8_t* host = mtb_host_stage(c, off[n] + 16, buf);
    if (!host) { c->err = "pinned staging allocation failed"; return MT_E_OOM; }
    mtb_d2h(c, host, c->b_stage.p, off[n]);
    if (getenv("MT_SNAP_TIMING"))
        fprintf(stderr, "mt_stage_docs: %u docs, %.1f MB staged, pack kernel wait %.1f ms, host buffer + download %.1f ms\n", n,
                off[n] / 1e6, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    views.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const MtStagedDoc sd = MtStagedDoc::at(host + off[i]);
        MtSnapView& v = views[i];
        v.hdr = sd.hdr; v.R = sd.R; v.blk = sd.blk; v.text = sd.text; v.pset = sd.pset;
    }
    return MT_OK;
}

// Client.snapshot asserts on the window it moves to (updateSeqNumbers, client.ts:843-850 ->
// setMinSeq, mergeTree.ts:1712-1716): a document whose status word is set after that
// (or before it) has no snapshot; the call fails instead of serializing it.
static int mt_check_staged_status(mt_ctx* c, uint32_t n, const uint32_t* docs, const std::vector<MtSnapView>& v) {
    for (uint32_t i = 0; i < n; i++)
        if (v[i].hdr.status) {
            char b[96];
            snprintf(b, sizeof b, "document %u has status 0x%x (the reference would have thrown)", docs[i], v[i].hdr.status);
            c->err = b;
            return MT_E_DOC_STATUS;
        }
    return MT_OK;
}
// Documents staged in groups of at most MT_STAGE_BUDGET bytes (estimated from their headers:
// every row, block, text unit and property set, an upper bound of the packed size), so the
// pinned download buffers stay small (pinning a multi-GB buffer costs more than the copy) and
// are reused group after group; fn(first, count, views) consumes each group while the next is
// staged; a group holds a multiple of `mult` documents (whole rounds of the emitting threads).
#define MT_STAGE_BUDGET (384ull << 20)
typedef std::function<int(uint32_t, uint32_t, const std::vector<MtSnapView>&)> MtGroupFn;
static int mt_staged_groups(mt_ctx* c, uint32_t n, const uint32_t* docs, const MtGroupFn& fn, uint32_t mult = 1,
                            bool check_status = true) {
    std::vector<MtDocHdr> h;
    int rc = mt_read_hdrs(c, n, docs, h);
    if (rc) return rc;
    const char* bs = getenv("MT_STAGE_BUDGET");             // bytes per group (tests force small groups)
    const uint64_t budget = bs ? strtoull(bs, nullptr, 10) : MT_STAGE_BUDGET;
    auto groupEnd = [&](uint32_t a) {
        uint64_t bytes = 0; uint32_t m = 0;
        while (a + m < n && m < 32768) {
            const MtDocHdr& d = h[a + m];
            const uint64_t b = 48ull * (uint64_t)(d.rowTop > 0 ? d.rowTop : 0) + 64ull * (uint64_t)(d.blkTop > 0 ? d.blkTop : 0) +
                               2ull * (uint64_t)(d.textTop > 0 ? d.textTop : 0) +
                               (uint64_t)sizeof(MtPSet) * (uint64_t)(d.psetTop > 0 ? d.psetTop : 0) + 1024;
            if (m > 0 && bytes + b > budget) break;
            bytes += b; m++;
        }
        if (a + m < n && m > mult) m -= m % mult;             // whole rounds of the emitting threads
        return a + m;
    };
    const bool timing = getenv("MT_SNAP_TIMING") != nullptr;
    // double-buffered: group g+1 is staged (device pack + download into the other pinned
    // buffer) while group g is emitted on the host threads
    std::vector<MtSnapView> cur, nxt;
    {   // both pinned buffers sized once for the call's largest group (estimates bound the packed
        // bytes): no buffer is re-pinned between groups
        uint64_t big = 0;
        for (uint32_t g = 0; g < n;) {
            const uint32_t e = groupEnd(g);
            uint64_t bytes = 0;
            for (uint32_t i = g; i < e; i++) {
                const MtDocHdr& d = h[i];
                bytes += 48ull * (uint64_t)(d.rowTop > 0 ? d.rowTop : 0) + 64ull * (uint64_t)(d.blkTop > 0 ? d.blkTop : 0) +
                         2ull * (uint64_t)(d.textTop > 0 ? d.textTop : 0) +
                         (uint64_t)sizeof(MtPSet) * (uint64_t)(d.psetTop > 0 ? d.psetTop : 0) + 1024;
            }
            if (bytes > big) big = bytes;
            g = e;
        }
        for (int buf = 0; buf < 2 && n; buf++)
            if (!mtb_host_stage(c, big + 16, buf)) { c->err = "pinned staging allocation failed"; return MT_E_OOM; }
    }
    uint32_t a = 0, b = n ? groupEnd(0) : 0;
    if (n && ((rc = mt_stage_docs(c, b - a, docs + a, cur, 0)) ||
              (check_status && (rc = mt_check_staged_status(c, b - a, docs + a, cur)))))
        return rc;
    for (int buf = 0; a < n; buf ^= 1) {
        const auto t0 = std::chrono::steady_clock::now();
        int erc = MT_OK;
        std::thread emit([&] { erc = fn(a, b - a, cur); });
        const uint32_t b2 = b < n ? groupEnd(b) : b;
        int src = MT_OK;
        if (b < n && !(src = mt_stage_docs(c, b2 - b, docs + b, nxt, buf ^ 1)) && check_status)
            src = mt_check_staged_status(c, b2 - b, docs + b, nxt);
        const auto t1 = std::chrono::steady_clock::now();
        emit.join();
        if (timing)
            fprintf(stderr, "mt_staged_groups: docs %u..%u emitted in %.1f ms beside staging the next %u in %.1f ms\n", a, b,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), b2 - b,
                    std::chrono::duration<double, std::milli>(t1 - t0).count());
        if (erc) return erc;
        if (src) return src;
        std::swap(cur, nxt);
        a = b; b = b2;
    }
    return MT_OK;
}
int MT_FN(reserve_staging)(mt_ctx* c, uint64_t bytes) {
    if (!c) return MT_E_INVALID;
    if (!bytes) bytes = MT_STAGE_BUDGET + 16;
    for (int buf = 0; buf < 2; buf++)
        if (!mtb_host_stage(c, bytes, buf)) { c->err = "pinned staging allocation failed"; return MT_E_OOM; }
    return MT_OK;
}
// SnapshotV1 of a non-empty document whose chunk size no length is below (MT_CHUNK_NONE):
// the reference's chunk loop (snapshotV1.ts:98-114) never ends; reported instead.
static std::string mt_chunk_hang_msg(uint32_t doc) {
    return "document " + std::to_string(doc) + ": mergeTreeSnapshotChunkSize is not a positive number, and "
           "SnapshotV1's chunk loop (snapshotV1.ts:98-114) never ends on a non-empty document";
}
// Client.snapshot (client.ts:923-956): SnapshotV1 or, with legacy set, SnapshotLegacy.
static int mt_snapshot_blobs(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* msn, const int32_t* seq,
                             uint64_t* digest, const char** arena, const uint64_t** blob_off,
                             const uint32_t** blob_first, bool legacy) {
    if (!c) return MT_E_INVALID;
    int rc = MT_FN(update_seq)(c, n, docs, msn, seq);       // Client.snapshot: updateSeqNumbers first (client.ts:936)
    if (rc) return rc;
    c->snap_arena.clear(); c->blob_off.assign(1, 0); c->blob_first.assign(1, 0);
    rc = mt_staged_groups(c, n, docs, [&](uint32_t a, uint32_t m, const std::vector<MtSnapView>& views) {
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t i = a + j;
            auto dn = c->doc_clients.find(docs[i]);
            std::vector<std::string> blobs = legacy ? mtsnap::snapshot_legacy_blobs(views[j], c->names, c->chunk_of(docs[i]))
                                                    : mtsnap::snapshot_blobs(views[j], c->names,
                                                                             dn == c->doc_clients.end() ? nullptr : &dn->second,
                                                                             c->chunk_of(docs[i]));
            if (blobs.empty()) { c->err = mt_chunk_hang_msg(docs[i]); return (int)MT_E_INVALID; }
            if (digest) digest[i] = mtsnap::blobs_digest(blobs);
            for (auto& b : blobs) { c->snap_arena += b; c->blob_off.push_back(c->snap_arena.size()); }
            c->blob_first.push_back((uint32_t)(c->blob_off.size() - 1));
        }
        return (int)MT_OK;
    });
    if (rc) return rc;
    if (arena) *arena = c->snap_arena.data();
    if (blob_off) *blob_off = c->blob_off.data();
    if (blob_first) *blob_first = c->blob_first.data();
    return MT_OK;
}

int MT_FN(snapshot_v1)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* msn, const int32_t* seq,
                       uint64_t* digest, const char** arena, const uint64_t** blob_off, const uint32_t** blob_first) {
    return mt_snapshot_blobs(c, n, docs, msn, seq, digest, arena, blob_off, blob_first, false);
}

int MT_FN(snapshot_legacy)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* msn, const int32_t* seq,
                           uint64_t* digest, const char** arena, const uint64_t** blob_off, const uint32_t** blob_first) {
    return mt_snapshot_blobs(c, n, docs, msn, seq, digest, arena, blob_off, blob_first, true);
}

// Digests only, serialized on `threads` host threads (no blob arena).
int MT_FN(snapshot_digests)(mt_ctx* c, uint32_t n, const uint32_t* docs, const int32_t* msn, const int32_t* seq,
                            uint64_t* digest, int threads) {
    if (!c || (n && (!docs || !msn || !seq || !digest))) return MT_E_INVALID;
    int rc = MT_FN(update_seq)(c, n, docs, msn, seq);
    if (rc) return rc;
    if (threads < 1) threads = 1;
    // groups of documents (mt_staged_groups), so the staging buffers stay bounded however many
    // documents (a million Zipf documents stage ~20 GB)
    return mt_staged_groups(c, n, docs, [&](uint32_t a, uint32_t m, const std::vector<MtSnapView>& views) {
        const int th = (uint32_t)threads > m ? (int)m : threads;
        std::vector<uint32_t> hang(th, UINT32_MAX);
        auto work = [&](int t) {
            for (uint32_t i = (uint32_t)t; i < m; i += (uint32_t)th) {
                auto dn = c->doc_clients.find(docs[a + i]);
                std::vector<std::string> blobs = mtsnap::snapshot_blobs(views[i], c->names,
                                                                        dn == c->doc_clients.end() ? nullptr : &dn->second,
                                                                        c->chunk_of(docs[a + i]));
                if (blobs.empty()) { hang[t] = std::min(hang[t], a + i); continue; }
                digest[a + i] = mtsnap::blobs_digest(blobs);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < th; t++) pool.emplace_back(work, t);
        work(0);
        for (auto& t : pool) t.join();
        const uint32_t h = *std::min_element(hang.begin(), hang.end());
        if (h != UINT32_MAX) { c->err = mt_chunk_hang_msg(docs[h]); return (int)MT_E_INVALID; }
        return (int)MT_OK;
    }, (uint32_t)threads);
}

int MT_FN(get_text)(mt_ctx* c, uint32_t n, const uint32_t* docs, const uint16_t** arena, const uint64_t** off) {
    if (!c) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) if (docs[i] >= c->S.maxDocs) { c->err = "doc id out of range"; return MT_E_INVALID; }
    c->text_arena.clear(); c->text_off.assign(1, 0);
    // bounded groups through the two reused pinned buffers (mt_staged_groups), documents in order;
    // a document with a status word still has its text (no status check)
    rc = mt_staged_groups(c, n, docs, [&](uint32_t, uint32_t m, const std::vector<MtSnapView>& views) {
        for (uint32_t j = 0; j < m; j++) {
            mtsnap::observer_text(views[j], c->text_arena);
            c->text_off.push_back(c->text_arena.size());
        }
        return (int)MT_OK;
    }, 1, false);
    if (rc) return rc;
    if (arena) *arena = c->text_arena.data();
    if (off) *off = c->text_off.data();
    return MT_OK;
}

int MT_FN(dump_segments)(mt_ctx* c, uint32_t d, int32_t** rows, uint32_t* n_rows) {
    if (!c || d >= c->S.maxDocs) return MT_E_INVALID;
    mtb_sync(c);
    MtHostDoc h;
    mt_download_doc(c, d, h);
    std::vector<int32_t> r;
    mtsnap::dump_rows(h.view(), c->names, r);
    *n_rows = (uint32_t)(r.size() / 12);
    *rows = (int32_t*)malloc(r.size() * 4 + 4);
    if (!r.empty()) memcpy(*rows, r.data(), r.size() * 4);
    return MT_OK;
}
void MT_FN(free)(void* p) { free(p); }

// Diagnostic (MT_PROFILE builds fill it; product builds return zeros): phase cycles per doc.
int MT_FN(prof_get)(mt_ctx* c, uint32_t n, unsigned long long* out) {
    if (!c || n > c->S.maxDocs) return MT_E_INVALID;
    mtb_sync(c);
    std::vector<MtDocHdr> h(n);
    mtb_d2h(c, h.data(), c->S.hdr, sizeof(MtDocHdr) * n);
    for (uint32_t i = 0; i < n; i++) for (int k = 0; k < 8; k++) out[i * 8 + k] = h[i].prof[k];
    return MT_OK;
}

// Stream generation with per-document op counts and client counts (null arrays:
// P->ops_per_doc / P->clients for every document).
int MT_FN(generate_docs)(mt_ctx* c, const mt_gen_params* P, const uint32_t* ops_per_doc, const uint32_t* clients_per_doc) {
    if (!c || !P || P->n_docs == 0 || P->n_docs > c->S.maxDocs || P->ins_len_max == 0 || P->rem_len_max == 0 ||
        P->n_ann_sets == 0) return MT_E_INVALID;
    if (P->pct_insert + P->pct_remove < 100 && P->n_ann_sets > c->S.p_nsets) { c->err = "annotate prop sets not uploaded"; return MT_E_INVALID; }
    if (P->ins_len_min > P->ins_len_max) { c->err = "ins_len_min > ins_len_max"; return MT_E_INVALID; }
    if (P->seg_prop_sets > c->S.p_nsets) { c->err = "segment prop sets not uploaded"; return MT_E_INVALID; }
    std::vector<uint32_t> docs(P->n_docs), off(P->n_docs + 1), cl(P->n_docs);
    off[0] = 0;
    for (uint32_t i = 0; i < P->n_docs; i++) {
        docs[i] = i;
        const uint64_t n = ops_per_doc ? ops_per_doc[i] : P->ops_per_doc;
        cl[i] = clients_per_doc ? clients_per_doc[i] : P->clients;
        if (cl[i] == 0 || cl[i] > 64) { c->err = "clients per document must be in [1, 64]"; return MT_E_INVALID; }
        if ((uint64_t)off[i] + n > 0xFFFFFFFFull) { c->err = "more than 2^32 ops in one batch"; return MT_E_INVALID; }
        off[i + 1] = (uint32_t)(off[i] + n);
    }
    const size_t N = off[P->n_docs];
    if ((uint64_t)N * P->ins_len_max >= 0xFFFFFFFFull) { c->err = "payload arena exceeds 2^32 units"; return MT_E_INVALID; }
    const size_t PU = N * P->ins_len_max + 1;
    int rc;
#define AL(buf, bytes) if ((rc = mtb_ensure(c, c->buf, (bytes)))) return mt_drop_batch(c, rc);
    AL(b_doc, 4ull * P->n_docs) AL(b_off, 4ull * (P->n_docs + 1)) AL(b_rec, sizeof(MtOpRec) * (N + 1)) AL(b_pay, 2 * PU)
    AL(b_gencl, 4ull * P->n_docs)
#undef AL
    mtb_h2d(c, c->b_doc.p, docs.data(), 4ull * P->n_docs);
    mtb_h2d(c, c->b_off.p, off.data(), 4ull * (P->n_docs + 1));
    mtb_h2d(c, c->b_gencl.p, cl.data(), 4ull * P->n_docs);
    c->gen_off.assign(off.begin(), off.end());
    mt_install_batch(c, mt_dev_ops(c, P->n_docs, PU, false), off.data(), docs.data(), false, c->props_wide, false);   // (armed below)
    if (!P->continue_docs) {
        rc = MT_FN(docs_open)(c, 0, P->n_docs);
        if (rc) return rc;
    }
    mt_dev_wide(c, P->n_docs, docs.data());             // after mt_docs_open, which clears the marks
    MtGen g{};
    g.seed = P->seed; g.ops = P->ops_per_doc; g.clients = P->clients; g.lag_max = P->lag_max;
    g.pct_insert = P->pct_insert; g.pct_remove = P->pct_remove; g.ins_len_max = P->ins_len_max;
    g.rem_len_max = P->rem_len_max; g.n_ann_sets = P->n_ann_sets; g.pct_rewrite = P->pct_rewrite; g.enabled = 1;
    g.clients_per_run = (const uint32_t*)c->b_gencl.p; g.total_ops = N; g.doc_id_base = P->doc_id_base;
    g.ins_len_min = P->ins_len_min; g.seg_prop_sets = P->seg_prop_sets; g.ins_at_end = P->ins_at_end;
    c->gen = g; c->gen_docs = P->n_docs;
    return mtb_launch_replay(c, g, P->n_docs);
}
int MT_FN(generate)(mt_ctx* c, const mt_gen_params* P) {
    if (!P || P->clients == 0 || P->clients > 64) return MT_E_INVALID;
    return MT_FN(generate_docs)(c, P, nullptr, nullptr);
}
int MT_FN(generated_ops)(mt_ctx* c, uint64_t* n_ops) {
    if (!c || !n_ops || !c->gen_docs) return MT_E_INVALID;
    *n_ops = c->gen.total_ops;
    return MT_OK;
}

int MT_FN(generated_download)(mt_ctx* c, uint8_t* type, uint8_t* flags, uint16_t* client, int32_t* seq, int32_t* ref,
                              int32_t* msn, int32_t* pos1, int32_t* pos2, uint32_t* poff, uint32_t* plen, int32_t* pid,
                              uint16_t* payload) {
    if (!c || !c->gen_docs) return MT_E_INVALID;
    mtb_sync(c);
    const size_t N = c->gen.total_ops;
    std::vector<MtOpRec> rec(N ? N : 1);
    mtb_d2h(c, rec.data(), c->ops.rec, sizeof(MtOpRec) * N);
    for (size_t i = 0; i < N; i++) {
        const MtOpRec& o = rec[i];
        type[i] = o.type; flags[i] = o.flags; client[i] = o.client; seq[i] = o.seq; ref[i] = o.ref_seq; msn[i] = o.msn;
        pos1[i] = o.pos1; pos2[i] = o.pos2; poff[i] = o.payload_off; plen[i] = o.payload_len; pid[i] = o.prop_id;
    }
    mtb_d2h(c, payload, c->ops.payload, 2 * (N * c->gen.ins_len_max));
    return MT_OK;
}
static_assert(sizeof(mt_op_rec) == sizeof(MtOpRec) && sizeof(mt_op_rec) == 32, "op record layout");
int MT_FN(generated_copy_dev)(mt_ctx* c, uint32_t first, uint32_t n, mt_op_rec* rec, uint16_t* payload) {
    if (!c || !c->gen_docs || (uint64_t)first + n > c->gen_off.size() - 1 || (n && (!rec || !payload))) return MT_E_INVALID;
    int rc = mtb_sync(c);
    if (rc) return rc;
    const uint64_t o0 = c->gen_off[first], o1 = c->gen_off[first + n];
    const uint64_t L = c->gen.ins_len_max;
    mtb_d2d(c, rec, c->ops.rec + o0, sizeof(MtOpRec) * (o1 - o0));
    mtb_d2d(c, payload, c->ops.payload + o0 * L, 2 * (o1 - o0) * L);
    return MT_OK;
}
int MT_FN(upload_batch_dev)(mt_ctx* c, uint32_t n_runs, const uint32_t* doc_ids, const uint32_t* op_offsets,
                            const mt_op_rec* rec, const uint16_t* payload, uint64_t payload_units) {
    if (!c || !op_offsets || (n_runs && !doc_ids)) return MT_E_INVALID;
    int rc;
    if ((rc = mt_check_runs(c, n_runs, doc_ids, op_offsets))) return rc;
    const uint64_t N = op_offsets[n_runs];
    if (N && (!rec || !payload)) return MT_E_INVALID;
#define UP(buf, bytes) if ((rc = mtb_ensure(c, c->buf, (bytes)))) return mt_drop_batch(c, rc);
    UP(b_doc, 4ull * n_runs + 4) UP(b_off, 4ull * (n_runs + 1)) UP(b_rec, sizeof(MtOpRec) * N + 32) UP(b_pay, 2 * payload_units + 2)
#undef UP
    mtb_h2d(c, c->b_doc.p, doc_ids, 4ull * n_runs);
    mtb_h2d(c, c->b_off.p, op_offsets, 4ull * (n_runs + 1));
    if (N) mtb_d2d(c, c->b_rec.p, rec, sizeof(MtOpRec) * N);
    if (payload_units) mtb_d2d(c, c->b_pay.p, payload, 2 * payload_units);
    mt_install_batch(c, mt_dev_ops(c, n_runs, payload_units, false), op_offsets, doc_ids, false, mt_dev_wide(c, n_runs, doc_ids), false);
    return mtb_sync(c);
}
// Document exchange rows (mt_shard.h): the sender packs generated runs at their plan
// positions with per-document checksums; the receiver unpacks rows into its resident batch
// and checks every document's checksum against the sender's.
int MT_FN(generated_pack_rows)(mt_ctx* c, uint32_t first, uint32_t n, const uint64_t* dst_row, void* rows_dev,
                               uint64_t* checksum) {
    if (!c || !c->gen_docs || (uint64_t)first + n > c->gen_off.size() - 1 || (n && (!dst_row || !rows_dev || !checksum)))
        return MT_E_INVALID;
    if (c->gen.ins_len_max % 4) { c->err = "exchange rows need ins_len_max % 4 == 0"; return MT_E_INVALID; }
    if (n == 0) return MT_OK;
    int rc;
    if ((rc = mtb_sync(c))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp0, 8ull * n))) return rc;
    if ((rc = mtb_ensure(c, c->b_tmp1, 8ull * n))) return rc;
    mtb_h2d(c, c->b_tmp0.p, dst_row, 8ull * n);
    if ((rc = mtb_launch_rows(c, true, first, n, c->gen.ins_len_max, (const uint64_t*)c->b_tmp0.p, (uint64_t*)rows_dev,
                              (uint64_t*)c->b_tmp1.p))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    mtb_d2h(c, checksum, c->b_tmp1.p, 8ull * n);
    return MT_OK;
}
int MT_FN(upload_rows_dev)(mt_ctx* c, uint32_t n_runs, const uint32_t* doc_ids, const uint32_t* op_offsets,
                           const void* rows_dev, uint32_t payload_stride, const uint64_t* expect, uint32_t* bad_runs) {
    if (!c || !op_offsets || (n_runs && (!doc_ids || !expect)) || payload_stride == 0 || payload_stride % 4)
        return MT_E_INVALID;
    int rc;
    if ((rc = mt_check_runs(c, n_runs, doc_ids, op_offsets))) return rc;
    const uint64_t N = op_offsets[n_runs], L = payload_stride;
    if (N && !rows_dev) return MT_E_INVALID;
    // payload_off is relative to the run's base (op_off[run] * L, 64-bit), so only a run's own
    // slots must stay below 2^32 units
    for (uint32_t r = 0; r < n_runs; r++)
        if ((uint64_t)(op_offsets[r + 1] - op_offsets[r]) * L >= 0xFFFFFFFFull) {
            c->err = "one document's payload slots exceed 2^32 units"; return MT_E_INVALID;
        }
#define UP(buf, bytes) if ((rc = mtb_ensure(c, c->buf, (bytes)))) return mt_drop_batch(c, rc);
    UP(b_doc, 4ull * n_runs + 4) UP(b_off, 4ull * (n_runs + 1)) UP(b_rec, sizeof(MtOpRec) * N + 32) UP(b_pay, 2 * N * L + 2)
    UP(b_tmp1, 8ull * n_runs + 8) UP(b_pbase, 8ull * n_runs + 8)
#undef UP
    mtb_h2d(c, c->b_doc.p, doc_ids, 4ull * n_runs);
    mtb_h2d(c, c->b_off.p, op_offsets, 4ull * (n_runs + 1));
    {
        std::vector<unsigned long long> pbase(n_runs);
        for (uint32_t r = 0; r < n_runs; r++) pbase[r] = (unsigned long long)op_offsets[r] * L;
        if (n_runs) mtb_h2d(c, c->b_pbase.p, pbase.data(), 8ull * n_runs);
    }
    mt_install_batch(c, mt_dev_ops(c, n_runs, N * L, true), op_offsets, doc_ids, false, mt_dev_wide(c, n_runs, doc_ids), false);
    if (n_runs && (rc = mtb_launch_rows(c, false, 0, n_runs, (uint32_t)L, nullptr, (uint64_t*)rows_dev,
                                        (uint64_t*)c->b_tmp1.p))) return rc;
    if ((rc = mtb_sync(c))) return rc;
    std::vector<uint64_t> got(n_runs);
    if (n_runs) mtb_d2h(c, got.data(), c->b_tmp1.p, 8ull * n_runs);
    uint32_t bad = 0, first_bad = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        const bool b = got[r] != expect[r];
        if (bad_runs) bad_runs[r] = b ? 1u : 0u;
        if (b && !bad++) first_bad = r;
    }
    if (bad) {
        char m[128];
        snprintf(m, sizeof m, "exchange checksum mismatch on %u of %u documents (first: run %u)", bad, n_runs, first_bad);
        c->err = m;
        return MT_E_EXCHANGE;
    }
    return MT_OK;
}
int MT_FN(generated_to_resident)(mt_ctx* c) {
    if (!c || !c->gen.enabled) return MT_E_INVALID;
    c->gen.enabled = 0;
    return MT_OK;
}

}  // extern "C"
