// depth.hip -- per-base read depth on MI355X (rsem-bam2wig, rsem-bam2readdepth).  Replaces the loop of
// wiggle.cpp:16-37, `read_depth[pos] += w` once per aligned base on one thread: depth[b] is the fold, in block order, of the weights
// of the blocks that cover base b (depth_block.hpp), bit for bit.
//
// A batch of blocks goes through
//   k_count         the tiles every block touches;
//   hipcub::DeviceScan::ExclusiveSum     where the block's entries start: the entry list is in block order;
//   k_expand        one entry (tile, block index) per (block, tile) pair;
//   hipcub::DeviceRadixSort::SortPairs   the library's STABLE radix sort on the tile alone, over the bits the tile ids have: inside a
//                   tile the entries stay in block order;
//   hipcub::DeviceRunLengthEncode::Encode, hipcub::DeviceScan::ExclusiveSum     the touched tiles and where their entries start;
//   k_accumulate    one workgroup per touched tile: accumulate_tile of depth_block.hpp.
// No atomics anywhere: a base belongs to one lane of one workgroup of a launch, and the launches of a stream run one after the other.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "depth_block.hpp"
#include "stage_util.hpp"

namespace {

using namespace rsem_depth;
using rsem::blocks256;

// cnt has n + 1 elements: the scan's last output is the number of entries
__global__ void __launch_bounds__(256) k_count(const uint64_t* __restrict__ start, const uint32_t* __restrict__ len, uint32_t n, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    cnt[i] = i < n ? (uint32_t)tiles_of(start[i], len[i]) : 0u;
}

__global__ void __launch_bounds__(256) k_expand(const uint64_t* __restrict__ start, const uint32_t* __restrict__ len, uint32_t n,
                                                 const uint32_t* __restrict__ off, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = off[i], m = off[i + 1] - o;
    const uint32_t t0 = (uint32_t)first_tile(start[i]);
    for (uint32_t j = 0; j < m; j++) {
        keys[o + j] = t0 + j;
        vals[o + j] = i;
    }
}

__global__ void __launch_bounds__(kTileThreads) k_accumulate(const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ seg_off,
                                                             const uint32_t* __restrict__ blk_of, const uint64_t* __restrict__ start,
                                                             const uint32_t* __restrict__ len, const double* __restrict__ w, double* depth,
                                                             uint64_t n_bases) {
    __shared__ TileEntry stage[kChunk];
    const uint32_t e0 = seg_off[blockIdx.x];
    accumulate_tile(tiles[blockIdx.x], e0, seg_off[blockIdx.x + 1] - e0, blk_of, start, len, w, depth, n_bases, stage);
}

struct Batch { uint64_t lo, hi, entries; };

int run(int device, uint64_t n_bases, const std::vector<Batch>& batches, uint64_t max_blocks, uint64_t max_entries, const uint64_t* start,
        const uint32_t* len, const double* w, double* depth, rsem_depth_info* info) {
    const uint64_t n_tiles = (n_bases + kTile - 1) / kTile;
    const int bits = tile_bits(n_tiles);

    RSEM_HIP_TRY(hipSetDevice(device));
    rsem::StageQueue q;
    RSEM_HIP_TRY(q.create());
    hipStream_t st = q.st;

    // the library's temporary storage for the largest batch
    size_t tmp_bytes = 0;
    {
        size_t t_sort = 0, t_scan_b = 0, t_scan_e = 0, t_rle = 0;
        hipcub::DoubleBuffer<uint32_t> qk(nullptr, nullptr), qv(nullptr, nullptr);
        RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, qk, qv, (int)max_entries, 0, bits, st));
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(max_blocks + 1), st));
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan_e, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(max_entries + 1), st));
        RSEM_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, t_rle, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                           (uint32_t*)nullptr, (int)max_entries, st));
        tmp_bytes = std::max(std::max(t_sort, t_rle), std::max(t_scan_b, t_scan_e));
    }
    const size_t need = (size_t)n_bases * 8 + (size_t)(max_blocks + 1) * 28 + (size_t)(max_entries + 1) * 28 + tmp_bytes + 64;
    size_t free_b = 0, total_b = 0;
    RSEM_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        rsem::set_last_error("rsem_depth_accumulate: %llu bases and batches of up to %llu blocks and %llu entries take %zu bytes of device memory, "
                             "%zu are free", (unsigned long long)n_bases, (unsigned long long)max_blocks, (unsigned long long)max_entries, need, free_b);
        return RSEM_ERR_NOMEM;
    }
    rsem::DevMem mem;
    double *d_depth = nullptr, *d_w = nullptr;
    uint64_t* d_start = nullptr;
    uint32_t *d_len = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_keys[2] = {nullptr, nullptr}, *d_vals[2] = {nullptr, nullptr};
    uint32_t *d_tiles = nullptr, *d_runs = nullptr, *d_seg = nullptr, *d_nruns = nullptr;
    uint8_t* d_tmp = nullptr;
    RSEM_HIP_TRY(mem.alloc(&d_depth, (size_t)n_bases));
    RSEM_HIP_TRY(mem.alloc(&d_start, (size_t)max_blocks));
    RSEM_HIP_TRY(mem.alloc(&d_len, (size_t)max_blocks));
    RSEM_HIP_TRY(mem.alloc(&d_w, (size_t)max_blocks));
    RSEM_HIP_TRY(mem.alloc(&d_cnt, (size_t)max_blocks + 1));
    RSEM_HIP_TRY(mem.alloc(&d_off, (size_t)max_blocks + 1));
    for (int h = 0; h < 2; h++) {
        RSEM_HIP_TRY(mem.alloc(&d_keys[h], (size_t)max_entries));
        RSEM_HIP_TRY(mem.alloc(&d_vals[h], (size_t)max_entries));
    }
    RSEM_HIP_TRY(mem.alloc(&d_tiles, (size_t)max_entries));
    RSEM_HIP_TRY(mem.alloc(&d_runs, (size_t)max_entries + 1));
    RSEM_HIP_TRY(mem.alloc(&d_seg, (size_t)max_entries + 1));
    RSEM_HIP_TRY(mem.alloc(&d_nruns, 1));
    RSEM_HIP_TRY(mem.alloc(&d_tmp, tmp_bytes));

    double upload_ms = 0, kernel_ms = 0;
    RSEM_HIP_TRY(q.upload_begin());
    RSEM_HIP_TRY(hipMemcpyAsync(d_depth, depth, (size_t)n_bases * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(q.upload_end());
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (int rc = q.add_upload_lap(upload_ms)) return rc;

    uint64_t n_entries = 0, n_touched = 0;
    int32_t n_launches = 0;
    for (const Batch& b : batches) {
        if (!b.entries) continue;  // blocks without a base
        const uint32_t n = (uint32_t)(b.hi - b.lo), ne = (uint32_t)b.entries;
        RSEM_HIP_TRY(q.upload_begin());
        RSEM_HIP_TRY(hipMemcpyAsync(d_start, start + b.lo, (size_t)n * 8, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_len, len + b.lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_w, w + b.lo, (size_t)n * 8, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(q.upload_end());
        hipLaunchKernelGGL(k_count, dim3(blocks256((uint64_t)n + 1)), dim3(256), 0, st, d_start, d_len, n, d_cnt);
        size_t tb = tmp_bytes;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_cnt, d_off, (int)(n + 1), st));
        // the blocks' counts must add up to what the host cut the batch by before anything is written behind their offsets
        uint32_t counted = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&counted, d_off + n, 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (counted != ne) {
            rsem::set_last_error("rsem_depth_accumulate: blocks %llu .. %llu have %u entries on the device, %u were expected", (unsigned long long)b.lo,
                                 (unsigned long long)b.hi, counted, ne);
            return RSEM_ERR_STATE;
        }
        hipLaunchKernelGGL(k_expand, dim3(blocks256(n)), dim3(256), 0, st, d_start, d_len, n, d_off, d_keys[0], d_vals[0]);
        tb = tmp_bytes;
        hipcub::DoubleBuffer<uint32_t> bk(d_keys[0], d_keys[1]), bv(d_vals[0], d_vals[1]);
        RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, bk, bv, (int)ne, 0, bits, st));
        tb = tmp_bytes;
        RSEM_HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(d_tmp, tb, bk.Current(), d_tiles, d_runs, d_nruns, (int)ne, st));
        uint32_t nruns = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&nruns, d_nruns, 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (nruns < 1 || nruns > ne || (uint64_t)nruns > n_tiles) {
            rsem::set_last_error("rsem_depth_accumulate: %u touched tiles among %u entries and %llu tiles", nruns, ne, (unsigned long long)n_tiles);
            return RSEM_ERR_STATE;
        }
        tb = tmp_bytes;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_runs, d_seg, (int)(nruns + 1), st));  // (its last output does not read d_runs[nruns])
        hipLaunchKernelGGL(k_accumulate, dim3(nruns), dim3(kTileThreads), 0, st, d_tiles, d_seg, bv.Current(), d_start, d_len, d_w, d_depth, n_bases);
        RSEM_HIP_TRY(q.kernels_end());
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (int rc = q.add_laps(upload_ms, kernel_ms)) return rc;
        n_entries += ne;
        n_touched += nruns;
        n_launches += 7;
    }
    RSEM_HIP_TRY(hipMemcpyAsync(depth, d_depth, (size_t)n_bases * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (info) {
        info->n_entries = n_entries;
        info->n_tiles_touched = n_touched;
        info->n_launches = n_launches;
        info->device_bytes = mem.bytes;
        info->upload_ms = upload_ms;
        info->kernel_ms = kernel_ms;
    }
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_depth_accumulate(int device, uint64_t n_bases, uint64_t n_blocks, const uint64_t* start, const uint32_t* len, const double* w,
                                     double* depth, rsem_depth_info* info) {
    RSEM_REQUIRE(device >= 0, "rsem_depth_accumulate: device must not be negative");
    RSEM_REQUIRE(n_blocks == 0 || (start && len && w), "rsem_depth_accumulate: start, len and w must not be NULL");
    RSEM_REQUIRE(n_bases == 0 || depth, "rsem_depth_accumulate: depth must not be NULL");
    for (uint64_t i = 0; i < n_blocks; i++) {
        uint64_t end;
        if (__builtin_add_overflow(start[i], (uint64_t)len[i], &end) || end > n_bases) {
            rsem::set_last_error("rsem_depth_accumulate: block %llu, %u bases from %llu on, runs past the %llu bases", (unsigned long long)i, len[i],
                                 (unsigned long long)start[i], (unsigned long long)n_bases);
            return RSEM_ERR_INVALID;
        }
    }
    uint64_t budget = kDefaultBatchItems;
    if (int rc = rsem::env_whole("RSEM_DEPTH_BATCH_ITEMS", 1, LLONG_MAX, &budget)) return rc;  // a test and measurement knob, read at call time
    if (info) {
        memset(info, 0, sizeof(*info));
        info->batch_items = budget;
    }
    if (n_blocks == 0 || n_bases == 0) return RSEM_OK;  // nothing to add: depth stays as it is, no device needed
    RSEM_REQUIRE((n_bases + kTile - 1) / kTile <= 0xffffffffull, "rsem_depth_accumulate: more than 2^32 tiles of bases in one call (the tile ids are 32-bit)");

    std::vector<Batch> batches;
    uint64_t max_blocks = 0, max_entries = 0, all_entries = 0;
    for (uint64_t lo = 0; lo < n_blocks;) {
        uint64_t items, entries;
        const uint64_t hi = batch_end(start, len, n_blocks, lo, budget, items, entries);
        if (entries > kMaxBatchEntries || hi - lo > kMaxBatchEntries) {
            rsem::set_last_error("rsem_depth_accumulate: a batch of %llu blocks and %llu entries (2^31 - 1 at most)", (unsigned long long)(hi - lo),
                                 (unsigned long long)entries);
            return RSEM_ERR_INVALID;
        }
        batches.push_back({lo, hi, entries});
        max_blocks = std::max(max_blocks, hi - lo);
        max_entries = std::max(max_entries, entries);
        all_entries += entries;
        lo = hi;
    }
    if (info) info->n_batches = (int32_t)batches.size();
    if (all_entries == 0) return RSEM_OK;  // blocks of no bases only
    return run(device, n_bases, batches, max_blocks, max_entries, start, len, w, depth, info);
}
