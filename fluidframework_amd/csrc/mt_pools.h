// mt_pools.h — the two inventories the host layer loops over (host code only): the eight
// per-document capacities and the device arrays of MtState.  A new capacity or pool is one
// line here (and its member in the struct the device reads); create, resize, checkpoint,
// restore, the byte counts and destroy follow from the tables.
#pragma once
#include <stddef.h>
#include <string.h>
#include "mt_replay.h"
#include "mt_pack.h"

// The offset fields of MtDocLayout, and the elements a document of capacities y takes of each
// pool (in the offset fields).
static unsigned long long MtDocLayout::*const MT_LY_OFF[9] = {&MtDocLayout::row, &MtDocLayout::blk, &MtDocLayout::heap,
    &MtDocLayout::win, &MtDocLayout::anc, &MtDocLayout::text, &MtDocLayout::pset, &MtDocLayout::mid, &MtDocLayout::regr};
static MtDocLayout mt_slice(const MtDocLayout& y) {
    MtDocLayout s{};
    s.row = y.rowCap; s.blk = y.blkCap; s.heap = (unsigned long long)y.heapCap + 1; s.win = y.winCap;
    s.anc = (unsigned long long)y.winCap * MT_MAXH; s.text = 2ull * y.textCap; s.pset = y.psetCap; s.mid = y.midCap;
    s.regr = 2ull * y.regCap;
    return s;
}

// The device arrays of MtState (in its order) and the layout table: where the pointer is, the
// element size, the count (a MtDocLayout offset field: uid and udelta are laid out as the window
// is, uanc as anc; or null and a per-document constant), the member's name and the name the
// growth messages use, and whether mt_checkpoint shadows it (not uid, udelta and uanc; the layout
// table's shadow is mt_ctx::ck_layout, on the host).
struct MtPoolDesc { size_t at, esz; unsigned long long MtDocLayout::*n; uint32_t perDoc; const char *field, *name; bool ck; };
#define MT_POOL(member, T, n, perDoc, name, ck) {offsetof(MtState, member), sizeof(T), n, perDoc, #member, name, ck}
static const MtPoolDesc MT_POOLS[] = {
    MT_POOL(rows, MtRow, &MtDocLayout::row, 0, "rows", true),
    MT_POOL(blk, MtBlk, &MtDocLayout::blk, 0, "blocks", true),
    MT_POOL(heap, MtHeapE, &MtDocLayout::heap, 0, "heap", true),
    MT_POOL(win, int, &MtDocLayout::win, 0, "window", true),
    MT_POOL(uid, int, &MtDocLayout::win, 0, "window", false),
    MT_POOL(udelta, int, &MtDocLayout::win, 0, "window", false),
    MT_POOL(uanc, int, &MtDocLayout::anc, 0, "window", false),
    MT_POOL(text, uint16_t, &MtDocLayout::text, 0, "text", true),
    MT_POOL(pset, MtPSet, &MtDocLayout::pset, 0, "property sets", true),
    MT_POOL(hdr, MtDocHdr, nullptr, 1, "headers", true),
    MT_POOL(hold, int, nullptr, MT_RFL, "recycled rows", true),
    MT_POOL(ovx, MtOvx, nullptr, MT_OVX_CAP, "overlap lists", true),
    MT_POOL(mid, int, &MtDocLayout::mid, 0, "markers", true),
    MT_POOL(reg, MtReg, nullptr, MT_REG_CAP, "registers", true),
    MT_POOL(regr, int, &MtDocLayout::regr, 0, "register rows", true),
    MT_POOL(layout, MtDocLayout, nullptr, 1, "layout", false),
};
#undef MT_POOL
enum { MT_NPOOLS = sizeof(MT_POOLS) / sizeof(MT_POOLS[0]) };
static void* mt_pool_get(const MtState& S, const MtPoolDesc& d) { void* p; memcpy(&p, (const char*)&S + d.at, sizeof p); return p; }
static void mt_pool_set(MtState& S, const MtPoolDesc& d, void* p) { memcpy((char*)&S + d.at, &p, sizeof p); }
// Bytes of pool d holding t elements (per offset field) for D documents, and of all of them.
static uint64_t mt_pool_bytes(const MtPoolDesc& d, const MtDocLayout& t, size_t D) {
    return d.esz * (uint64_t)(d.n ? t.*d.n : (unsigned long long)d.perDoc * D);
}
static uint64_t mt_pool_bytes_of(const MtDocLayout& t, size_t D) {
    uint64_t b = 0;
    for (const MtPoolDesc& d : MT_POOLS) b += mt_pool_bytes(d, t, D);
    return b;
}

// The per-document capacities: the mt_limits member, the MtDocLayout capacity, what the
// document holds of it (MtOcc), the name messages use, the limit, the largest-capacity member
// of MtState (null: the device needs none), the MT_GROW_* slot of the capacities autogrow can
// raise (-1: sized by mt_docs_resize only), and the offset field and element size of the
// slice a relocation copies.  (In the order mt_docs_resize reports a capacity below holdings.)
struct MtCapDesc {
    uint32_t mt_limits::*lim; uint32_t MtDocLayout::*cap; uint32_t MtOcc::*occ; const char* name; uint32_t max;
    uint32_t MtState::*most; int grow; unsigned long long MtDocLayout::*off; size_t esz;
};
static const MtCapDesc MT_CAPS[8] = {
    {&mt_limits::rows_per_doc, &MtDocLayout::rowCap, &MtOcc::rows, "rows", 1u << 30, &MtState::rowCap, MT_GROW_ROWS, &MtDocLayout::row, sizeof(MtRow)},
    {&mt_limits::blocks_per_doc, &MtDocLayout::blkCap, &MtOcc::blks, "blocks", 1u << 30, &MtState::blkCap, MT_GROW_BLKS, &MtDocLayout::blk, sizeof(MtBlk)},
    {&mt_limits::text_per_doc, &MtDocLayout::textCap, &MtOcc::text, "text", 1u << 30, &MtState::textCap, MT_GROW_TEXT, &MtDocLayout::text, 2},
    {&mt_limits::propsets_per_doc, &MtDocLayout::psetCap, &MtOcc::psets, "property sets", 1u << 30, &MtState::psetCap, MT_GROW_PSET, &MtDocLayout::pset, sizeof(MtPSet)},
    {&mt_limits::heap_per_doc, &MtDocLayout::heapCap, &MtOcc::heap, "heap", 1u << 30, &MtState::heapCap, MT_GROW_HEAP, &MtDocLayout::heap, sizeof(MtHeapE)},
    {&mt_limits::window_per_doc, &MtDocLayout::winCap, &MtOcc::win, "window", 1u << 26, &MtState::winCap, MT_GROW_WIN, &MtDocLayout::win, 4},
    {&mt_limits::markers_per_doc, &MtDocLayout::midCap, &MtOcc::mids, "markers", 1u << 30, nullptr, -1, &MtDocLayout::mid, 4},
    {&mt_limits::register_rows_per_doc, &MtDocLayout::regCap, &MtOcc::regs, "register rows", 1u << 24, nullptr, -1, &MtDocLayout::regr, 4},
};
