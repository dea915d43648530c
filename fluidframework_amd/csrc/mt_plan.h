// mt_plan.h — which replay kernels the resident batch gets: the one statement of the rule.
//
// Both backends include this after their mtb_* primitives and before mtb_launch_replay: mt_plan_replay fills the
// launches, mt_engine.hip issues them on its streams, tests/emu/mt_emu.cpp runs them in order; neither decides.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>
#include "mt_ctx.h"

static int mtb_ensure(mt_ctx* c, mt_ctx::DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return MT_OK;
    if (b.p) mtb_free(b.p);
    b.p = nullptr; b.cap = 0;
    if (mtb_malloc(&b.p, bytes) != 0) { c->err = "device allocation failed"; return MT_E_OOM; }
    b.cap = bytes;
    return MT_OK;
}

// The run lists of the size classes for the resident batch (host lists uploaded once per
// batch): long runs (>= big_min_ops op records) in [0, n_long), the rest after them.
static int mt_size_class_lists(mt_ctx* c) {
    if (c->runs_gen == c->batch_gen && c->runs_min == c->big_min_ops) return MT_OK;
    const uint32_t R = c->n_runs;
    std::vector<uint32_t> lst; lst.reserve(R);
    for (uint32_t r = 0; r < R && c->run_off.size() == R + 1; r++)
        if (c->run_off[r + 1] - c->run_off[r] >= c->big_min_ops) lst.push_back(r);
    c->n_long = (uint32_t)lst.size();
    for (uint32_t r = 0; r < R && c->run_off.size() == R + 1; r++)
        if (c->run_off[r + 1] - c->run_off[r] < c->big_min_ops) lst.push_back(r);
    c->n_short = (uint32_t)lst.size() - c->n_long;
    int rc;
    if ((rc = mtb_ensure(c, c->b_runs, 4ull * lst.size() + 4))) return rc;
    if (!lst.empty()) mtb_h2d(c, c->b_runs.p, lst.data(), 4ull * lst.size());
    c->runs_gen = c->batch_gen; c->runs_min = c->big_min_ops;
    return MT_OK;
}

// The partition rule (mt_plan_partition): a model of the measured kernels.
// Per-message times of one document's wave, in microseconds: MT_PLAN_T_BLK in the block-
// residency kernel with 16 documents per CU (config 2: 153.5 ms / 10,000 messages; MT_PLAN_T_LONE
// alone), the same kernel's long document whose tree outgrows LDS and continues in HBM
// (MT_PLAN_T_CONT past about MT_PLAN_LDS_FIT messages: config 5's 1,302 ms / 65,521 messages
// unpartitioned), MT_PLAN_T_WIDE in the wide kernel with MT_PLAN_WIDE_PER_CU documents per CU
// (LDS-bound: 21.2 KB each; 1,048,576-document config 5 at 256:224, 5,338 ms for 699 M messages
// on 224 CUs) and MT_PLAN_T_WLONE its lone longest document (config 5: 887.9 ms / 65,521).
#define MT_PLAN_T_BLK   15.3
#define MT_PLAN_T_LONE  13.4
#define MT_PLAN_T_CONT  19.9
#define MT_PLAN_T_WIDE  12.0
#define MT_PLAN_WIDE_PER_CU 7
#define MT_PLAN_T_WLONE 13.5
#define MT_PLAN_LDS_FIT 10000u
struct MtPlanSide { double msgs = 0, extra = 0; uint32_t longest = 0; };
// Step estimate (microseconds) of one kernel on `cus` CUs holding `per_cu` documents each.
static double mt_plan_side(const MtPlanSide& s, double cus, double per_cu, double t_thr, double t_lone, bool cont) {
    if (s.msgs == 0) return 0;
    const double thr = (s.msgs * t_thr + (cont ? s.extra * (MT_PLAN_T_CONT - MT_PLAN_T_BLK) : 0)) / (cus * per_cu);
    const double lat = cont && s.longest > MT_PLAN_LDS_FIT
                           ? MT_PLAN_LDS_FIT * t_lone + (double)(s.longest - MT_PLAN_LDS_FIT) * MT_PLAN_T_CONT
                           : (double)s.longest * t_lone;
    return thr > lat ? thr : lat;
}
static void mt_plan_partition_impl(const uint32_t* len, uint32_t n, uint32_t ncu, uint32_t* min_ops, uint32_t* cus,
                                   double* est_us) {
    *min_ops = 0; *cus = 0;
    std::vector<uint32_t> L(len, len + n);
    std::sort(L.begin(), L.end(), std::greater<uint32_t>());
    // suffix sums over the sorted lengths: messages and continuation messages of the runs < m
    MtPlanSide all;
    for (uint32_t x : L) { all.msgs += x; all.extra += x > MT_PLAN_LDS_FIT ? x - MT_PLAN_LDS_FIT : 0; }
    all.longest = n ? L[0] : 0;
    const double off = mt_plan_side(all, ncu, 16, MT_PLAN_T_BLK, MT_PLAN_T_LONE, true);
    double best = off, bestSum = 0; uint32_t bm = 0, bk = 0;
    const uint32_t step = ncu >= 8 ? ncu / 8 : 1;                      // whole XCD shares
    for (uint32_t m = 256; m <= 32768 && ncu >= 2; m *= 2) {
        MtPlanSide A, B;
        for (uint32_t x : L) {
            MtPlanSide& s = x >= m ? A : B;
            s.msgs += x; s.extra += x > MT_PLAN_LDS_FIT ? x - MT_PLAN_LDS_FIT : 0;
            if (x > s.longest) s.longest = x;
        }
        if (A.msgs == 0) break;
        for (uint32_t k = step; k < ncu; k += step) {
            const double ta = mt_plan_side(A, k, MT_PLAN_WIDE_PER_CU, MT_PLAN_T_WIDE, MT_PLAN_T_WLONE, false);
            const double tb = mt_plan_side(B, ncu - k, 16, MT_PLAN_T_BLK, MT_PLAN_T_LONE, true);
            const double t = ta > tb ? ta : tb, sum = ta + tb;
            // the lowest step; within 1 % of it, the lowest total busy time
            if (t < best * 0.99 || (t <= best * 1.01 && bm && sum < bestSum)) { best = t < best ? t : best; bestSum = sum; bm = m; bk = k; }
        }
    }
    if (bm && best < off * 0.95) { *min_ops = bm; *cus = bk; if (est_us) *est_us = best; }
    else if (est_us) *est_us = off;
}
// MT_PARTITION_AUTO: the resident batch's partition from its run lengths (once per batch).
static void mt_auto_partition(mt_ctx* c) {
    if (!c->part_auto || c->use_lds != 2 || c->auto_gen == c->batch_gen) return;
    c->auto_gen = c->batch_gen;
    const uint32_t R = c->n_runs;
    if (c->run_off.size() != R + 1) { c->big_min_ops = 0; c->part_cus = 0; return; }
    std::vector<uint32_t> len(R);
    for (uint32_t r = 0; r < R; r++) len[r] = c->run_off[r + 1] - c->run_off[r];
    uint32_t m = 0, k = 0;
    mt_plan_partition_impl(len.data(), R, mtb_cu_count(c), &m, &k, nullptr);
    c->big_min_ops = m; c->part_cus = m ? k : 0;
}

// The continuation class of block residency for the resident batch: how many runs have at
// least cont_min_ops op records (n_cont > 0 launches the kernel with the in-wave continuation).
static void mt_cont_lists(mt_ctx* c) {
    if (c->cont_gen == c->batch_gen && c->cont_min_made == c->cont_min_ops) return;
    const uint32_t R = c->n_runs;
    c->n_cont = 0;
    for (uint32_t r = 0; r < R && c->run_off.size() == R + 1; r++) c->n_cont += c->run_off[r + 1] - c->run_off[r] >= c->cont_min_ops;
    c->cont_gen = c->batch_gen; c->cont_min_made = c->cont_min_ops;
}

// ------------------------------------------------------------------ the plan ----
// One replay launch: `n` one-document workgroups of `kernel` on `lane`.  Kernels: every pool in
// HBM for whole runs (HBM) or from each run's cursor, what an earlier launch left (REST); full LDS
// residency (LDS); block residency, where a document that outgrows LDS stops for REST (BLK) or
// continues in HBM in the same wave (BLK_CONT); wide block residency with that continuation (BLKW);
// the long-document kernel (BIG).  Lanes: the context's stream (MAIN), its second stream (SIDE), the
// CU-masked pair of a partition (A, B).  A lane's launches run in plan order; another lane than MAIN
// starts after what MAIN held before the plan; MAIN waits for the others before REST and at the end.
enum { MT_PK_HBM, MT_PK_REST, MT_PK_LDS, MT_PK_BLK, MT_PK_BLK_CONT, MT_PK_BLKW, MT_PK_BIG };
enum { MT_LANE_MAIN, MT_LANE_SIDE, MT_LANE_A, MT_LANE_B, MT_LANE_N };
struct MtLaunch {
    int kernel, lane; uint32_t n;
    const uint32_t* runs;       // the run of each workgroup (device memory), or null: run = index
    int l0, l1, l2;             // the residency caps mt_replay_doc takes
    uint32_t pad;               // dynamic LDS bytes per workgroup (fewer workgroups per CU)
};
struct MtPlan {
    bool full;                  // the FULL instantiation of every kernel (mt_replay_full)
    int n; MtLaunch l[4];
    void add(int kernel, int lane, uint32_t cnt, const uint32_t* runs = nullptr, int l0 = 0, int l1 = 0, int l2 = 0, uint32_t pad = 0) {
        l[n++] = MtLaunch{kernel, lane, cnt, runs, l0, l1, l2, pad};
    }
};
// FULL: a delta-capture buffer is armed, or the batch holds register ops or wide property maps.
static bool mt_replay_full(const mt_ctx* c) { return c->ops.drec || c->batch_reg || c->batch_wide; }

// The launches of the resident batch (c->n_runs > 0).  mtb_masked_streams(c): can lanes A / B be had (asked only
// when a partition wants them)?  The HIP backend defines its own and MTB_HAVE_MASKED_STREAMS; others always can.
#ifndef MTB_HAVE_MASKED_STREAMS
static bool mtb_masked_streams(mt_ctx*) { return true; }
#endif
static int mt_plan_replay(mt_ctx* c, bool full, MtPlan& P) {
    P = MtPlan{}; P.full = full;
    const uint32_t R = c->n_runs;
    const int lb = c->lds_blks, lh = c->lds_heap;
    bool rest = false;          // the plan ends with the all-HBM launch from every run's cursor
    mt_auto_partition(c);
    if (c->use_lds == 2 && c->big_min_ops)
        if (int rc = mt_size_class_lists(c)) return rc;
    if (c->use_lds == 2 && c->big_min_ops && c->n_long) {
        // Size classes: the long runs first, so they take their slots before the short ones fill the
        // CUs, the rest under block residency beside them (FULL: continuing in-wave).  (A) partitioned:
        // long runs in the wide kernel on lane A's part_cus CUs (~21 KB of LDS, up to 7 per CU), the rest
        // on lane B's; FULL: block residency, one workgroup per SIMD (each padded to a quarter of the CU's
        // 160 KB of LDS: any total in (160 KB / 5, 160 KB / 4] leaves four).  (B) otherwise: long runs on
        // the second stream; FULL: the long-document kernel.
        const uint32_t* runs = (const uint32_t*)c->b_runs.p;
        const bool part = c->part_cus && mtb_masked_streams(c);
        if (!full) P.add(MT_PK_BLKW, part ? MT_LANE_A : MT_LANE_SIDE, c->n_long, runs, 0, MT_BW_BLKS, MT_BW_HEAP);
        else if (part) P.add(MT_PK_BLK_CONT, MT_LANE_A, c->n_long, runs, 0, lb, lh, 27u << 10);
        else P.add(MT_PK_BIG, MT_LANE_SIDE, c->n_long, runs, MT_G_WIN, 0, MT_G_HEAP);
        if (c->n_short) P.add(full ? MT_PK_BLK_CONT : MT_PK_BLK, part ? MT_LANE_B : MT_LANE_MAIN, c->n_short, runs + c->n_long, 0, lb, lh);
        rest = c->n_short && !full;
    } else if (c->use_lds == 3) P.add(MT_PK_BIG, MT_LANE_MAIN, R, nullptr, c->lds_rows, lb, lh);   // (C)
    else if (c->use_lds == 2) {
        // (D) one launch with the in-wave continuation for FULL and for a batch with a run that reaches the
        // continuation threshold (the runs start in batch order, longest first under LPT; two kernels on two streams let
        // short runs take the slots first and measured slower); others without the second engine, then REST
        mt_cont_lists(c);
        rest = !full && !c->n_cont;
        P.add(rest ? MT_PK_BLK : MT_PK_BLK_CONT, MT_LANE_MAIN, R, nullptr, 0, lb, lh);
    } else if (c->use_lds) { P.add(MT_PK_LDS, MT_LANE_MAIN, R, nullptr, c->lds_rows, lb, lh); rest = true; }   // (E)
    else P.add(MT_PK_HBM, MT_LANE_MAIN, R);                                                  // (F)
    if (rest) P.add(MT_PK_REST, MT_LANE_MAIN, R);
    return MT_OK;
}
