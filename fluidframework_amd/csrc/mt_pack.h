// mt_pack.h — gather documents' live state into one contiguous staging buffer
// (device side of mt_snapshot_v1 / mt_snapshot_digests / mt_get_text for many
// documents: one download instead of four copies per document).
//
// Per document, at staging offset off[i] (16-byte aligned):
//   MtDocHdr | rows[0, rowTop) | blocks[0, blkTop) | referenced psets (compacted) | live text
// Live text is compacted (as textGC does): linked text rows' slices back to back,
// with each staged row's toff rewritten to its slice; markers keep refType in toff.
#pragma once
#include "mt_core.h"

struct MtPackSize { uint32_t rows, blks, psets, text; };

MT_INLINE uint64_t mt_pack_bytes(const MtPackSize& z) {
    const uint64_t t = ((uint64_t)z.text * 2 + 15) & ~15ull;
    return sizeof(MtDocHdr) + (uint64_t)z.rows * sizeof(MtRow) + (uint64_t)z.blks * sizeof(MtBlk) +
           (uint64_t)z.psets * sizeof(MtPSet) + t;
}
MT_INLINE int mt_pset_chunks(int n) { return n > MT_PSK ? (n + MT_PSK - 1) / MT_PSK : 1; }

// Only the property maps linked rows reference are staged (the pool is append-only: an
// annotate-heavy document holds tens of maps per live row).  mt_pack_size marks each
// referenced map's first chunk with the staging epoch (MtPSet::pad[0]) and counts the marked
// maps' chunks; mt_pack_doc stages them back to back, records each one's staged index in
// pad[1] and rewrites the staged rows' ids.  (The pads are not engine state.)
template <class Eng>
MT_HD MtPackSize mt_pack_size(Eng& e, uint32_t epoch) {
    MtPackSize z; z.rows = (uint32_t)e.rowTop; z.blks = (uint32_t)e.blkTop;
    int t = 0;
    for (int base = 0; base < e.rowTop; base += MT_WAVE) {
        const int m = (e.rowTop - base) < MT_WAVE ? (e.rowTop - base) : MT_WAVE;
        t += wave_sum(wave_map(m, [&](int k) MT_LAM {
            const int s = base + k;
            const bool linked = e.R[s].parent >= 0;
            const int p = e.R[s].props;
            if (linked && p >= 0) e.pset[p].pad[0] = (int32_t)epoch;
            return (linked && !(e.R[s].meta & MT_M_MARKER)) ? e.R[s].len : 0;
        }));
    }
    z.text = (uint32_t)t;
    wave_sync();
    int np = 0;
    for (int base = 0; base < e.psetTop; base += MT_WAVE) {
        const int m = (e.psetTop - base) < MT_WAVE ? (e.psetTop - base) : MT_WAVE;
        np += wave_sum(wave_map(m, [&](int k) MT_LAM {
            const MtPSet& q = e.pset[base + k];
            return q.pad[0] == (int32_t)epoch ? mt_pset_chunks(q.n) : 0;
        }));
    }
    z.psets = (uint32_t)np;
    return z;
}

template <class Eng>
MT_HD void mt_pack_doc(Eng& e, uint8_t* dst, uint32_t epoch) {
    const int rowTop = e.rowTop, blkTop = e.blkTop, psetTop = e.psetTop;
    MtRow* rows = (MtRow*)(dst + sizeof(MtDocHdr));
    MtBlk* blks = (MtBlk*)(rows + rowTop);
    MtPSet* ps = (MtPSet*)(blks + blkTop);
    {   // header
        const int* src = (const int*)e.hdrp;
        int* d = (int*)dst;
        wave_for((int)(sizeof(MtDocHdr) / 4), [&](int k) MT_LAM { d[k] = src[k]; });
    }
    int wp = 0;                                  // referenced property maps, compacted
    for (int base = 0; base < psetTop; base += MT_WAVE) {
        const int m = (psetTop - base) < MT_WAVE ? (psetTop - base) : MT_WAVE;
        auto nc = wave_map(m, [&](int k) MT_LAM {
            const MtPSet& q = e.pset[base + k];
            return q.pad[0] == (int32_t)epoch ? mt_pset_chunks(q.n) : 0;
        });
        auto pre = wave_excl_scan(nc);
        const int tot = wave_sum(nc);
        wave_for(m, [&](int k) MT_LAM {
            const int n = own(nc, k);
            if (!n) return;
            const int o = wp + own(pre, k);
            e.pset[base + k].pad[1] = o;
            const MtQ16* src = (const MtQ16*)(e.pset + base + k);
            MtQ16* d = (MtQ16*)(ps + o);
            for (int q = 0; q < n * (int)(sizeof(MtPSet) / 16); q++) d[q] = src[q];
        });
        wp += tot;
    }
    wave_sync();
    wave_for(1, [&](int) MT_LAM { ((MtDocHdr*)dst)->psetTop = wp; });   // the staged maps' count
    uint16_t* text = (uint16_t*)(ps + wp);
    int w = 0;
    for (int base = 0; base < rowTop; base += MT_WAVE) {
        const int m = (rowTop - base) < MT_WAVE ? (rowTop - base) : MT_WAVE;
        auto ln = wave_map(m, [&](int k) MT_LAM {
            const int s = base + k;
            return (e.R[s].parent >= 0 && !(e.R[s].meta & MT_M_MARKER)) ? e.R[s].len : 0;
        });
        auto pre = wave_excl_scan(ln);
        const int tot = wave_sum(ln);
        wave_for(m, [&](int k) MT_LAM {
            const int s = base + k, l = own(ln, k);
            MtRow r = e.R[s];
            if (l > 0) {
                const int o = w + own(pre, k);
                lane_copy16(text + o, e.text + r.toff, l);
                r.toff = o; r.tcap = l;
            }
            r.props = (r.parent >= 0 && r.props >= 0) ? e.pset[r.props].pad[1] : -1;
            rows[s] = r;
        });
        w += tot;
    }
    {
        const int nq = blkTop * (int)(sizeof(MtBlk) / 16);
        const MtQ16* src = (const MtQ16*)e.blk; MtQ16* d = (MtQ16*)blks;
        for (int base = 0; base < nq; base += MT_WAVE) {
            const int m = (nq - base) < MT_WAVE ? (nq - base) : MT_WAVE;
            wave_for(m, [&](int k) MT_LAM { d[base + k] = src[base + k]; });
        }
    }
    wave_sync();
}

// ------------------------------------------------- relocation (mt_docs_resize) ----
// What a document holds of each per-document pool, in mt_limits' order of the capacity
// fields: rows and blocks by their tops (both move by index), heap and window entries, the
// text units a compaction keeps (MtEngT::textLive), the chunks of the property maps that
// linked rows and register clones reference, the highest marker id a row carries and the
// register arena's used ids.
struct MtOcc { uint32_t rows, blks, text, psets, heap, win, mids, regs; };

// The sizing pass: marks the referenced maps with `epoch` as mt_pack_size does, but with
// textGC's liveness (register clones keep their maps and text).
template <class Eng>
MT_HD MtOcc mt_doc_occupancy(Eng& e, uint32_t epoch) {
    MtOcc z; z.rows = (uint32_t)e.rowTop; z.blks = (uint32_t)e.blkTop; z.heap = (uint32_t)e.heapN; z.win = (uint32_t)e.winN;
    z.regs = (uint32_t)e.regTop; z.text = (uint32_t)e.textLive();
    auto hi = wave_map(MT_WAVE, [&](int) MT_LAM { return 0; });
    for (int base = 0; base < e.rowTop; base += MT_WAVE) {
        const int m = (e.rowTop - base) < MT_WAVE ? (e.rowTop - base) : MT_WAVE;
        hi = wave_map(MT_WAVE, [&](int k) MT_LAM {
            const int h0 = own(hi, k);
            if (k >= m) return h0;
            const int s = base + k;
            const uint32_t mt = e.R[s].meta;
            const bool live = (e.R[s].parent >= 0) | ((mt & MT_M_REG) != 0);
            const int p = e.R[s].props;
            if (live && p >= 0) e.pset[p].pad[0] = (int32_t)epoch;
            const int id = (mt & MT_M_MARKER) ? e.R[s].mid : 0;
            return id > h0 ? id : h0;
        });
    }
    int top = 0;
    for (int k = 0; k < MT_WAVE; k++) { const int v = wave_at(hi, k); top = v > top ? v : top; }
    z.mids = (uint32_t)top;
    wave_sync();
    int np = 0;
    for (int base = 0; base < e.psetTop; base += MT_WAVE) {
        const int m = (e.psetTop - base) < MT_WAVE ? (e.psetTop - base) : MT_WAVE;
        np += wave_sum(wave_map(m, [&](int k) MT_LAM {
            const MtPSet& q = e.pset[base + k];
            return q.pad[0] == (int32_t)epoch ? mt_pset_chunks(q.n) : 0;
        }));
    }
    z.psets = (uint32_t)np;
    return z;
}

// Moves the document `e` is bound to into the slices `ny` of the pools S.  A slice of `ny`
// is either the one the document has (that pool stays as it is: no copy, and no compaction of
// text or property maps) or a new one, which never overlaps an old one.  Rows [0, rowTop) and blocks
// [0, blkTop) move by index, so row ids, block ids, the free list and the recycled-row stack
// stay valid; the heap moves with its heapN + 1 entries, the window with its winN, the marker
// table and the live half of the register arena as they are.  The U set is per-op scratch and
// is not moved.  Text is compacted as textGC does, into half 0.  Property maps are compacted
// to the maps mt_doc_occupancy marked with `epoch` and the rows' ids rewritten (rows neither
// linked nor held by a register lose theirs, as in a staged copy), unless !compact (delta
// capture armed: ids in records already captured stay valid), when the arena is copied whole.
// The header stays where it is (indexed by document); its textTop, textHalf and psetTop follow.
template <class Eng>
MT_HD void mt_relocate_doc(Eng& e, const MtState& S, const MtDocLayout& ny, uint32_t epoch, bool compact) {
    const int rowTop = e.rowTop, blkTop = e.blkTop, psetTop = e.psetTop;
    MtRow* rows = S.rows + ny.row;
    MtPSet* ps = S.pset + ny.pset;
    uint16_t* text = S.text + ny.text;
    // a pool whose slice is the one the document has stays as it is
    const bool mvRows = rows != e.R, mvPset = ps != e.pset, mvText = text != e.S.textBase;
    int wp = psetTop;
    if (mvPset && compact) {
        wp = 0;
        for (int base = 0; base < psetTop; base += MT_WAVE) {
            const int m = (psetTop - base) < MT_WAVE ? (psetTop - base) : MT_WAVE;
            auto nc = wave_map(m, [&](int k) MT_LAM {
                const MtPSet& q = e.pset[base + k];
                return q.pad[0] == (int32_t)epoch ? mt_pset_chunks(q.n) : 0;
            });
            auto pre = wave_excl_scan(nc);
            const int tot = wave_sum(nc);
            wave_for(m, [&](int k) MT_LAM {
                const int n = own(nc, k);
                if (!n) return;
                const int o = wp + own(pre, k);
                e.pset[base + k].pad[1] = o;
                const MtQ16* src = (const MtQ16*)(e.pset + base + k);
                MtQ16* d = (MtQ16*)(ps + o);
                for (int q = 0; q < n * (int)(sizeof(MtPSet) / 16); q++) d[q] = src[q];
            });
            wp += tot;
        }
        wave_sync();
    } else if (mvPset) Eng::copyQ((MtQ16*)ps, (const MtQ16*)e.pset, psetTop * (int)(sizeof(MtPSet) / 16));
    const bool ids = mvPset && compact;            // the rows' property-map ids change
    int w = e.textTop;
    if (mvRows || mvText || ids) {
        w = mvText ? 0 : w;
        for (int base = 0; base < rowTop; base += MT_WAVE) {
            const int m = (rowTop - base) < MT_WAVE ? (rowTop - base) : MT_WAVE;
            auto ln = wave_map(m, [&](int k) MT_LAM {
                const int s = base + k;
                const uint32_t mt = e.R[s].meta;
                const int l = e.R[s].len;
                return (mvText && (((e.R[s].parent >= 0) | ((mt & MT_M_REG) != 0)) & !(mt & MT_M_MARKER))) ? l : 0;
            });
            auto pre = wave_excl_scan(ln);
            const int tot = wave_sum(ln);
            wave_for(m, [&](int k) MT_LAM {
                const int s = base + k, l = own(ln, k);
                MtRow r = e.R[s];
                if (l > 0) {
                    const int o = w + own(pre, k);
                    lane_copy16(text + o, e.text + r.toff, l);
                    r.toff = o; r.tcap = l;
                }
                if (ids) {
                    const bool live = (r.parent >= 0) | ((r.meta & MT_M_REG) != 0);
                    r.props = (live && r.props >= 0) ? e.pset[r.props].pad[1] : -1;
                }
                rows[s] = r;
            });
            w += tot;
        }
    }
    if (S.blk + ny.blk != e.blk) Eng::copyQ((MtQ16*)(S.blk + ny.blk), (const MtQ16*)e.blk, blkTop * (int)(sizeof(MtBlk) / 16));
    if (S.heap + ny.heap != e.heap) Eng::copyI((int*)(S.heap + ny.heap), (const int*)e.heap, 2 * (e.heapN + 1));
    if (S.win + ny.win != e.win) Eng::copyI(S.win + ny.win, e.win, e.winN);
    if (S.mid + ny.mid != e.midt) {
        int* mid = S.mid + ny.mid;
        const int keep = e.midCap < (int)ny.midCap ? e.midCap : (int)ny.midCap;
        Eng::copyI(mid, e.midt, keep);
        for (int base = keep; base < (int)ny.midCap; base += MT_WAVE) {
            const int m = ((int)ny.midCap - base) < MT_WAVE ? ((int)ny.midCap - base) : MT_WAVE;
            wave_for(m, [&](int k) MT_LAM { mid[base + k] = -1; });
        }
    }
    if (S.regr + ny.regr != e.regr)
        Eng::copyI(S.regr + ny.regr + (size_t)e.regHalf * ny.regCap, e.regr + (size_t)e.regHalf * e.regCap, e.regTop);
    wave_sync();
    MtDocHdr* h = e.hdrp;
    const int half = mvText ? 0 : e.textHalf;
    wave_for(1, [&](int) MT_LAM { h->textTop = w; h->textHalf = half; h->psetTop = wp; });
    wave_sync();
}

// Host view of one staged document.
struct MtStagedDoc {
    MtDocHdr hdr; const MtRow* R; const MtBlk* blk; const MtPSet* pset; const uint16_t* text;
    static MtStagedDoc at(const uint8_t* p) {
        MtStagedDoc v;
        v.hdr = *(const MtDocHdr*)p;
        v.R = (const MtRow*)(p + sizeof(MtDocHdr));
        v.blk = (const MtBlk*)(v.R + v.hdr.rowTop);
        v.pset = (const MtPSet*)(v.blk + v.hdr.blkTop);
        v.text = (const uint16_t*)(v.pset + v.hdr.psetTop);     // psetTop: rewritten to the staged count
        return v;
    }
};
