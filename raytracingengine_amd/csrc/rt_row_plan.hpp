// rt_row_plan.hpp — which image rows a render call produces (the row set of rt_render_opts) and
// how a multi-GPU frame deals them over its ranks (rt_multi.cpp).  Row arithmetic and nothing
// else: plain C++, no HIP, no call into the library, so the host test
// (tests/row_plan/plan_main.cpp) compiles it alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "rt_capi.h"

namespace rtamd {

// The blocks of a row set in the order the render packs them: rows [row_begin, row_end), or with
// row_cycle > 1 the row_block-row blocks starting at row_begin + k*row_cycle*row_block inside it.
//   for (RowBlocks b(o, height); !b.done(); b.next())  — image rows [b.y, b.y + b.rows()) are the
//   packed rows [b.packed, b.packed + b.rows()); after the loop b.packed is the row count.
struct RowBlocks {
    uint64_t y, end, block, stride;
    uint32_t packed = 0;
    RowBlocks(const rt_render_opts& o, uint32_t height)
        : y(o.row_begin), end(o.row_end ? std::min(o.row_end, height) : height) {
        const bool cyclic = o.row_cycle > 1 && o.row_block != 0;
        block = cyclic ? o.row_block : (end > y ? end - y : 0);
        stride = cyclic ? static_cast<uint64_t>(o.row_block) * o.row_cycle : block;
    }
    bool done() const { return y >= end; }
    uint32_t rows() const { return static_cast<uint32_t>(std::min(block, end - y)); }
    void next() {
        packed += rows();
        y += stride;
    }
};

// Rows a render call produces.
inline uint32_t rendered_rows(const rt_render_opts& o, uint32_t height) {
    RowBlocks b(o, height);
    while (!b.done()) b.next();
    return b.packed;
}

constexpr uint32_t kDefaultBlock = 16;  // rows per block of a multi-GPU split without row_block

// Slot s of a V-slot block-cyclic split in blocks of b rows: base with that row set.
inline void slot_opts(const rt_render_opts& base, uint32_t b, int V, int s, rt_render_opts& o) {
    o = base;
    o.row_begin = static_cast<uint32_t>(s) * b;
    o.row_block = static_cast<uint16_t>(b);
    o.row_cycle = static_cast<uint16_t>(V);
}

// The first slot of a rank when rank 0 owns `weight` slots and every other rank one.  kOffByOne
// exists for the host test's mutant only.
template <bool kOffByOne = false>
inline int first_slot_of(int rank, int weight) {
    return rank == 0 ? 0 : weight + rank - 1 + (kOffByOne ? 1 : 0);
}

// One rank's share of a frame of n ranks.  The frame's rows are dealt block-cyclically over
// V = weight + n − 1 row sets ("slots"); rank 0 owns slots [0, weight), rank r ≥ 1 slot
// weight + r − 1 (weight 1: slot r).  One rank: a contiguous full frame.  Every rank pads a
// frame's rows to max_rows, so a slot of a batch has the same extent on every rank and rank 0's
// receive buffer is [slots][nframes][max_rows] rows per output.
struct Plan {
    rt_render_opts opts;  // the first slot's
    uint32_t block = 0, rows = 0, max_rows = 0;
    int n = 1, weight = 1;
    int slots = 1, first_slot = 0, nslots = 1;
    uint32_t slot_rows[64];  // rows of each of this rank's slots

    bool weighted() const { return weight > 1; }
    // the (first) slot rank r owns
    int slot_of(int r) const { return first_slot_of(r, weight); }
    // opts of this rank's j-th slot
    rt_render_opts slot(int j) const {
        rt_render_opts o = opts;
        if (n > 1) slot_opts(opts, block, slots, first_slot + j, o);
        return o;
    }
    // pixels of one slot of a batch: frame f's packed rows start max_rows rows after frame f − 1's
    size_t slot_px(uint32_t width, int nframes) const {
        return static_cast<size_t>(nframes) * max_rows * width;
    }
    // bytes a rank sends per output of bpp bytes per pixel: one slot of the batch
    size_t send_bytes(uint32_t width, int nframes, size_t bpp) const {
        return slot_px(width, nframes) * bpp;
    }
    // where slot s of the batch sits in rank 0's receive buffer, and the buffer's bytes
    size_t recv_offset(int s, uint32_t width, int nframes, size_t bpp) const {
        return static_cast<size_t>(s) * send_bytes(width, nframes, bpp);
    }
    size_t recv_bytes(uint32_t width, int nframes, size_t bpp) const {
        return recv_offset(slots, width, nframes, bpp);
    }
};

// The plan of `rank` of n for a frame of H rows.  o: the caller's resolved opts; of its row set
// only row_block is read (0: kDefaultBlock).  False, with pl untouched, when o selects rows of
// its own: multi-GPU frames render the whole image.
template <bool kOffByOne = false>
inline bool make_plan(uint32_t H, rt_render_opts o, int n, int rank, int weight, Plan& pl) {
    if (o.row_begin != 0 || (o.row_end != 0 && o.row_end != H) || o.row_cycle > 1) return false;
    o.row_end = H;
    pl.n = n;
    pl.weight = n == 1 ? 1 : weight;
    pl.slots = pl.weight + n - 1;
    pl.first_slot = first_slot_of<kOffByOne>(rank, pl.weight);
    pl.nslots = rank == 0 ? pl.weight : 1;
    if (n == 1) {
        o.row_block = o.row_cycle = 0;
        pl.opts = o;
        pl.block = H;
        pl.rows = pl.max_rows = pl.slot_rows[0] = rendered_rows(o, H);
        return true;
    }
    pl.block = o.row_block ? o.row_block : kDefaultBlock;
    auto rows_of = [&](int s) {
        rt_render_opts q;
        slot_opts(o, pl.block, pl.slots, s, q);
        return rendered_rows(q, H);
    };
    slot_opts(o, pl.block, pl.slots, pl.first_slot, pl.opts);
    pl.rows = pl.max_rows = 0;
    for (int j = 0; j < pl.nslots; ++j) pl.rows += pl.slot_rows[j] = rows_of(pl.first_slot + j);
    for (int s = 0; s < pl.slots; ++s) pl.max_rows = std::max(pl.max_rows, rows_of(s));
    return true;
}

}  // namespace rtamd
