// depth_block.hpp -- the arithmetic of the per-base read depth (rsem-bam2wig, rsem-bam2readdepth): depth.hip
// runs it on the device, tests/depth_check.cpp runs the same source on the host -- the tile body on tests/simt_emu.hpp.
//
// The contract (wiggle.cpp:16-37): depth[b] is a FOLD -- start from the value passed in, add the weight of every block that covers
// base b, in the order of the blocks.  A double sum depends on the order of its additions, so nothing here may reorder them: no
// floating-point atomics, no difference array with a prefix sum, no tree.
//
// The bases of a call are cut into tiles of kTile.  Every block becomes one entry per tile it touches, (tile, block index), in
// block order; a STABLE sort on the tile alone groups the entries by tile and keeps the blocks' order inside every tile; one
// workgroup per touched tile then walks its entries in that order, one lane per two bases, and does the fold in a register.
#pragma once
#include <cstdint>

#include "simt_macros.hpp"

#ifdef __HIPCC__
#define RSEM_DEPTH_FN __host__ __device__ inline  // depth.hip: its host side cuts the batches with the same functions
#else
#define RSEM_DEPTH_FN inline
#endif

namespace rsem_depth {

constexpr int kTileThreads = 256;                    // lanes of a workgroup (four waves of 64)
constexpr int kLaneBases = 2;                        // bases per lane: tid and tid + 256 of the tile, both coalesced
constexpr int kTile = kTileThreads * kLaneBases;     // bases per tile
constexpr int kChunk = 256;                          // entries staged in LDS at a time (one per lane): 4 KiB
constexpr uint64_t kDefaultBatchItems = 1ull << 26;  // 28 bytes of device memory per item and 28 per block
constexpr uint64_t kMaxBatchEntries = 0x7fffffffull;  // the library's sort and scans count in int

// the tiles the block [start, start + len) touches (start + len does not overflow: checked at the entry point)
RSEM_DEPTH_FN uint64_t first_tile(uint64_t start) { return start / kTile; }
RSEM_DEPTH_FN uint64_t tiles_of(uint64_t start, uint32_t len) { return len ? (start + len - 1) / kTile - start / kTile + 1 : 0; }
// what a block counts against the item budget of a batch: its entries, and 1 where it has none (the blocks of a batch are bounded too)
RSEM_DEPTH_FN uint64_t items_of(uint64_t start, uint32_t len) { return len ? tiles_of(start, len) : 1; }

// bits of the largest tile id of n_tiles tiles (the radix sort looks at no more)
RSEM_DEPTH_FN int tile_bits(uint64_t n_tiles) {
    uint64_t m = n_tiles ? n_tiles - 1 : 0;
    int b = 0;
    while (m) { b++; m >>= 1; }
    return b ? b : 1;
}

// Batches: whole blocks in their order, as many as stay within `budget` items; a block above the budget is a batch of its own.
// Returns the end (exclusive) of the batch that starts at block lo, its items and its entries.
RSEM_DEPTH_FN uint64_t batch_end(const uint64_t* start, const uint32_t* len, uint64_t n_blocks, uint64_t lo, uint64_t budget, uint64_t& items,
                                 uint64_t& entries) {
    items = entries = 0;
    uint64_t b = lo;
    while (b < n_blocks) {
        const uint64_t it = items_of(start[b], len[b]);
        if (items > 0 && items + it > budget) break;
        items += it;
        entries += tiles_of(start[b], len[b]);
        b++;
    }
    return b;
}

// what a lane needs of an entry inside its tile: the covered bases [lo, lo + cnt) relative to the tile's first base, the weight
struct TileEntry {
    uint32_t lo, cnt;
    double w;
};

RSEM_DEPTH_FN TileEntry clip_to_tile(uint64_t tile_base, uint64_t start, uint32_t len, double w) {
    const uint64_t end = start + len, tile_end = tile_base + kTile;
    TileEntry e;
    e.lo = start > tile_base ? (uint32_t)(start - tile_base) : 0u;
    e.cnt = (uint32_t)((end < tile_end ? end : tile_end) - tile_base) - e.lo;
    e.w = w;
    return e;
}

// One workgroup, one touched tile: the tile's ne entries are blk_of[e0 .. e0 + ne), block indices in block order.  Every lane loads
// its two bases, walks the entries in order -- kChunk at a time staged in `stage` (LDS, kChunk entries), every lane reading the same
// entry at the same time: a broadcast read, no bank conflict -- and adds the weight where the entry covers the base.  The add is
// under the condition, not a multiply by 0 or 1 and not an add of 0.0: -0.0 + 0.0 is +0.0.
RSEM_DEVFN void accumulate_tile(uint64_t tile, uint32_t e0, uint32_t ne, const uint32_t* blk_of, const uint64_t* start, const uint32_t* len,
                                const double* w, double* depth, uint64_t n_bases, TileEntry* stage) {
    const int tid = RSEM_TIDX;
    const uint64_t tile_base = tile * kTile;
    const uint64_t b0 = tile_base + (uint64_t)tid, b1 = b0 + kTileThreads;
    const uint32_t p0 = (uint32_t)tid, p1 = p0 + kTileThreads;
    double a0 = b0 < n_bases ? depth[b0] : 0.0;
    double a1 = b1 < n_bases ? depth[b1] : 0.0;
    for (uint32_t c = 0; c < ne; c += kChunk) {
        const uint32_t m = ne - c < (uint32_t)kChunk ? ne - c : (uint32_t)kChunk;
        RSEM_SYNC();  // every lane is done with the chunk before
        if ((uint32_t)tid < m) {
            const uint32_t b = blk_of[e0 + c + (uint32_t)tid];
            stage[tid] = clip_to_tile(tile_base, start[b], len[b], w[b]);
        }
        RSEM_SYNC();
        for (uint32_t j = 0; j < m; j++) {
            const TileEntry e = stage[j];
            if (p0 - e.lo < e.cnt) a0 += e.w;
            if (p1 - e.lo < e.cnt) a1 += e.w;
        }
    }
    if (b0 < n_bases) depth[b0] = a0;
    if (b1 < n_bases) depth[b1] = a1;
}

}  // namespace rsem_depth
