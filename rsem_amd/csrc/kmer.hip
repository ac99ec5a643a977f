// kmer.hip -- shared k-mers of the reference's transcripts on MI355X (rsem-for-ebseq-calculate-clustering-info; DESIGN.md
// section 10).  Replaces the sort-and-count of EBSeq/calcClusteringInfo.cpp:101-130: for every transcript the number of k-mer
// start positions whose k-mer also occurs in at least one other transcript.  Integer arithmetic throughout (kmer_block.hpp).
//
//   k_tile<HIST|COUNT|EMIT>  a workgroup stages 2048 codes plus a halo of k - 1 in LDS; a lane takes 8 consecutive starts, finds
//                   the separators in front of them and rolls the key of the LAST chunk (and the bucket of the first bases) along.
//                   HIST adds to the bucket histogram, COUNT counts the starts of the batch's buckets per tile, EMIT writes
//                   (key, position) behind the tile's offset, in position order.
//   hipcub::DeviceRadixSort::SortPairs   the library's stable radix sort, once per chunk, last chunk first, over the bits the
//                   chunk's keys can have; between two sorts k_gather builds the next chunk's keys for the current order.
//   k_heads         head flags (the k-mer differs from its predecessor's) and the transcript of every element;
//   hipcub::DeviceScan::InclusiveSum     the group index of every element;
//   k_flags         a group is shared where two neighbours inside it differ in transcript (whatever the order of equal k-mers);
//   k_count         every element of a shared group adds to its transcript's 32-bit counter: runs of equal transcript inside a
//                   wave are added once, by their first lane.
// The only atomics are integer adds: nothing depends on their order.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "kmer_block.hpp"
#include "stage_util.hpp"

namespace {

using namespace rsem_kmer;
using rsem::blocks256;

constexpr int kTileThreads = 256;
constexpr int kPerLane = kLaneStarts;
constexpr int kTile = kTileThreads * kPerLane;  // starts per workgroup
constexpr int kMaxK = 32768;                    // the halo of a tile stays within 32 KiB of LDS
constexpr uint64_t kMaxBatchItems = 0x7fffffffull;  // the indices inside a batch are 32-bit

enum { kHist = 0, kCount = 1, kEmit = 2 };

struct TileArgs {
    const uint8_t* sep;  // the separated codes; readable up to (number of tiles) * kTile + k + 32 bytes, separators behind the end
    int k, pb;           // pb = bucket_bases(k)
    int last_off, last_len;  // the last chunk: its first base inside the k-mer and its length
    uint32_t b_lo, b_hi;     // the batch: buckets [b_lo, b_hi)
    unsigned long long* hist;
    uint32_t* tile_cnt;
    const uint32_t* tile_off;
    uint64_t* keys;
    void* vals;
};

// exclusive prefix of v over the workgroup's lanes; total = the sum over all of them
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t* wave_sums, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int w = 0; w < kTileThreads / 64; w++) {
        const uint32_t s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + inc - v;
}

template <int MODE, class ValT>
__global__ void __launch_bounds__(kTileThreads) k_tile(TileArgs a) {
    extern __shared__ uint4 stage4[];
    __shared__ uint32_t wave_sums[kTileThreads / 64];
    const uint8_t* s = (const uint8_t*)stage4;
    const int tid = threadIdx.x, k = a.k;
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    const int nvec = (kTile + k - 1 + 15) / 16;
    for (int q = tid; q < nvec; q += kTileThreads) stage4[q] = *(const uint4*)(a.sep + base + (uint64_t)16 * q);
    __syncthreads();

    const int p0 = tid * kPerLane;
    uint64_t keys[kPerLane];
    uint32_t sel = 0;  // bit j: start p0 + j is a k-mer of this batch
    uint32_t run_bucket = 0, run = 0;
    lane_starts(s, p0, k, a.last_off, a.last_len, a.pb, [&](int j, bool valid, uint64_t key, uint32_t bucket) {
        if (MODE == kHist) {  // runs of one bucket (poly(A), N runs) are added once
            if (valid && run && bucket == run_bucket) run++;
            else {
                if (run) atomicAdd(a.hist + run_bucket, (unsigned long long)run);
                run = valid ? 1 : 0;
                run_bucket = bucket;
            }
        } else {
            if (valid && bucket >= a.b_lo && bucket < a.b_hi) sel |= 1u << j;
            keys[j] = key;
        }
    });
    if (MODE == kHist) {
        if (run) atomicAdd(a.hist + run_bucket, (unsigned long long)run);
        return;
    }
    uint32_t total;
    const uint32_t rank = block_exclusive((uint32_t)__builtin_popcount(sel), wave_sums, total);
    if (MODE == kCount) {
        if (tid == 0) a.tile_cnt[blockIdx.x] = total;
        return;
    }
    uint32_t o = a.tile_off[blockIdx.x] + rank;
    ValT* vals = (ValT*)a.vals;
    for (int j = 0; j < kPerLane; j++)
        if (sel >> j & 1) {
            a.keys[o] = keys[j];
            vals[o] = (ValT)(base + p0 + j);
            o++;
        }
}

// the keys of the chunk at bases [off, off + len) for the elements in their current order
template <class ValT>
__global__ void __launch_bounds__(256) k_gather(const uint8_t* __restrict__ sep, const ValT* __restrict__ vals, uint32_t n, int off, int len,
                                                 uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    keys[i] = encode(sep + (uint64_t)vals[i] + off, len);
}

template <class ValT>
__global__ void __launch_bounds__(256) k_heads(const uint8_t* __restrict__ sep, const uint64_t* __restrict__ soff, int32_t M, int k,
                                                const uint64_t* __restrict__ keys, const ValT* __restrict__ vals, uint32_t n,
                                                uint32_t* __restrict__ heads, int32_t* __restrict__ tids) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = vals[i];
    tids[i] = find_transcript(soff, M, p);
    heads[i] = i == 0 || is_head(sep, k, keys[i], keys[i - 1], p, (uint64_t)vals[i - 1]);
}

// gid = inclusive sum of the head flags: group g holds the elements with gid = g + 1
__global__ void __launch_bounds__(256) k_flags(const uint32_t* __restrict__ gid, const int32_t* __restrict__ tids, uint32_t n,
                                                uint8_t* __restrict__ shared_group) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0 || i >= n) return;
    if (gid[i] == gid[i - 1] && tids[i] != tids[i - 1]) shared_group[gid[i] - 1] = 1;  // every writer writes the same value
}

__global__ void __launch_bounds__(256) k_count(const uint32_t* __restrict__ gid, const int32_t* __restrict__ tids, uint32_t n,
                                                const uint8_t* __restrict__ shared_group, uint32_t* __restrict__ shared) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    // a whole wave stays together for the ballot; lanes behind the end and elements of unshared groups carry -1
    const int32_t t = (i < n && shared_group[gid[i] - 1]) ? tids[i] : -1;
    const int32_t before = __shfl_up(t, 1);
    const uint64_t boundary = __ballot(lane == 0 || before != t);
    if (t >= 0 && (boundary >> lane & 1)) atomicAdd(shared + t, (uint32_t)run_length(boundary, lane, 64));
}

template <class ValT>
int run(int device, int32_t M, const uint64_t* seq_off, const uint8_t* codes, int32_t k, uint64_t n_kmers, uint64_t budget_env,
        uint32_t* shared, rsem_kmer_info* info) {
    const uint64_t L = seq_off[M], Ls = L + (uint64_t)M;
    const uint64_t ntiles = (Ls + kTile - 1) / kTile;
    const size_t sep_bytes = (size_t)ntiles * kTile + (size_t)k + 32;
    const int nC = n_chunks(k), pb = bucket_bases(k);
    const uint32_t nbuckets = (uint32_t)pow5(pb);

    // the separated codes and the transcripts' starts among them
    std::vector<uint8_t> sep((size_t)Ls);
    std::vector<uint64_t> soff((size_t)M + 1);
    for (int32_t t = 0; t < M; t++) {
        soff[t] = seq_off[t] + (uint64_t)t;
        const size_t len = (size_t)(seq_off[t + 1] - seq_off[t]);
        if (len) memcpy(sep.data() + soff[t], codes + seq_off[t], len);
        sep[soff[t] + len] = kSep;
    }
    soff[M] = Ls;

    RSEM_HIP_TRY(hipSetDevice(device));
    rsem::StageQueue q;
    RSEM_HIP_TRY(q.create());
    hipStream_t st = q.st;
    rsem::DevMem mem;
    uint8_t* d_sep = nullptr;
    uint64_t* d_soff = nullptr;
    uint32_t *d_shared = nullptr, *d_tile_cnt = nullptr, *d_tile_off = nullptr;
    RSEM_HIP_TRY(mem.alloc(&d_sep, sep_bytes));
    RSEM_HIP_TRY(mem.alloc(&d_soff, (size_t)M + 1));
    RSEM_HIP_TRY(mem.alloc(&d_shared, (size_t)M));
    RSEM_HIP_TRY(mem.alloc(&d_tile_cnt, (size_t)ntiles + 1));
    RSEM_HIP_TRY(mem.alloc(&d_tile_off, (size_t)ntiles + 1));

    RSEM_HIP_TRY(q.upload_begin());
    RSEM_HIP_TRY(hipMemsetAsync(d_sep, kSep, sep_bytes, st));
    RSEM_HIP_TRY(hipMemcpyAsync(d_sep, sep.data(), (size_t)Ls, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(d_soff, soff.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(d_shared, 0, (size_t)M * 4, st));
    RSEM_HIP_TRY(hipMemsetAsync(d_tile_cnt, 0, ((size_t)ntiles + 1) * 4, st));
    RSEM_HIP_TRY(q.upload_end());
    RSEM_HIP_TRY(hipStreamSynchronize(st));

    // what fits: keys and values, each twice -- the two halves the library's sort goes back and forth between (its DoubleBuffer
    // form: no third copy in its temporary storage); everything behind the sort lives in the half the last sort left free
    const size_t per_item = 2 * sizeof(uint64_t) + 2 * sizeof(ValT);
    size_t free_b = 0, total_b = 0;
    RSEM_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = std::max<size_t>(free_b / 16, (size_t)256 << 20) + (size_t)nbuckets * 8;
    const size_t usable = free_b > margin ? free_b - margin : 0;
    // the library's temporary storage for n items (sort, scans): asked of the library, and taken off what the halves may use
    auto library_bytes = [&](uint64_t n, size_t& bytes) -> int {
        size_t tmp_sort = 0, tmp_scan = 0, tmp_tiles = 0;
        hipcub::DoubleBuffer<uint64_t> qk(nullptr, nullptr);
        hipcub::DoubleBuffer<ValT> qv(nullptr, nullptr);
        RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, qk, qv, (int)n, 0, 63, st));
        RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp_scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, st));
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_tiles, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(ntiles + 1), st));
        bytes = std::max(tmp_sort, std::max(tmp_scan, tmp_tiles));
        return RSEM_OK;
    };
    uint64_t capacity = std::min<uint64_t>(usable / per_item, kMaxBatchItems);
    if (capacity) {
        size_t at_most = 0;
        if (int rc = library_bytes(capacity, at_most)) return rc;
        capacity = usable > at_most ? std::min<uint64_t>((usable - at_most) / per_item, kMaxBatchItems) : 0;
    }
    const uint64_t budget = budget_env ? budget_env : capacity;

    TileArgs ta;
    ta.sep = d_sep; ta.k = k; ta.pb = pb;
    ta.last_off = (nC - 1) * kChunkBases; ta.last_len = chunk_len(k, nC - 1);
    ta.b_lo = 0; ta.b_hi = nbuckets;
    ta.hist = nullptr; ta.tile_cnt = d_tile_cnt; ta.tile_off = d_tile_off; ta.keys = nullptr; ta.vals = nullptr;
    const size_t lds = (size_t)((kTile + k - 1 + 15) / 16) * 16;

    // the batches: everything at once where it fits, whole buckets of the first bases otherwise
    struct Batch { uint32_t lo, hi; uint64_t items; };
    std::vector<Batch> batches;
    if (n_kmers <= budget) {
        batches.push_back({0, nbuckets, n_kmers});
    } else {
        unsigned long long* d_hist = nullptr;
        RSEM_HIP_TRY(mem.alloc(&d_hist, (size_t)nbuckets));
        RSEM_HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)nbuckets * 8, st));
        ta.hist = d_hist;
        hipLaunchKernelGGL((k_tile<kHist, ValT>), dim3((unsigned)ntiles), dim3(kTileThreads), lds, st, ta);
        std::vector<unsigned long long> hist(nbuckets);
        RSEM_HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, (size_t)nbuckets * 8, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        for (uint32_t lo = 0; lo < nbuckets;) {
            uint64_t items;
            const uint32_t hi = batch_end(hist, nbuckets, lo, budget, items);
            if (items) batches.push_back({lo, hi, items});
            lo = hi;
        }
    }
    uint64_t max_items = 0;
    for (const Batch& b : batches) max_items = std::max(max_items, b.items);
    uint64_t *d_keys[2] = {nullptr, nullptr};
    ValT* d_vals[2] = {nullptr, nullptr};
    uint8_t* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    if (max_items <= kMaxBatchItems)
        if (int rc = library_bytes(max_items, tmp_bytes)) return rc;
    if (max_items > capacity || (size_t)max_items * per_item + tmp_bytes > usable) {
        rsem::set_last_error("rsem_kmer_shared_counts: a batch of %llu %d-mers (%zu bytes each and %zu of the library's) does not fit the device: "
                             "%zu bytes are free, %zu of them usable, at most %llu k-mers a batch%s", (unsigned long long)max_items, k, per_item,
                             tmp_bytes, free_b, usable, (unsigned long long)capacity,
                             batches.size() > 1 ? " (the k-mers that share their first bases stay in one batch)" : "");
        return RSEM_ERR_NOMEM;
    }
    for (int h = 0; h < 2; h++) {
        RSEM_HIP_TRY(mem.alloc(&d_keys[h], (size_t)max_items));
        RSEM_HIP_TRY(mem.alloc(&d_vals[h], (size_t)max_items));
    }
    RSEM_HIP_TRY(mem.alloc(&d_tmp, tmp_bytes));

    uint64_t n_groups = 0;
    for (const Batch& b : batches) {
        const uint32_t n = (uint32_t)b.items;
        int cur = 0;
        ta.b_lo = b.lo; ta.b_hi = b.hi; ta.keys = d_keys[0]; ta.vals = d_vals[0];
        hipLaunchKernelGGL((k_tile<kCount, ValT>), dim3((unsigned)ntiles), dim3(kTileThreads), lds, st, ta);
        size_t tb = tmp_bytes;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_tile_cnt, d_tile_off, (int)(ntiles + 1), st));
        // the tiles' counts must add up to the batch before anything is written behind their offsets
        uint32_t counted = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&counted, d_tile_off + ntiles, 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (counted != n) {
            rsem::set_last_error("rsem_kmer_shared_counts: the tiles of buckets %u .. %u hold %u %d-mers, %u were expected", b.lo, b.hi, counted, k, n);
            return RSEM_ERR_STATE;
        }
        hipLaunchKernelGGL((k_tile<kEmit, ValT>), dim3((unsigned)ntiles), dim3(kTileThreads), lds, st, ta);
        for (int c = nC - 1; c >= 0; c--) {
            if (c < nC - 1)
                hipLaunchKernelGGL((k_gather<ValT>), dim3(blocks256(n)), dim3(256), 0, st, d_sep, d_vals[cur], n, c * kChunkBases, chunk_len(k, c), d_keys[cur]);
            tb = tmp_bytes;
            hipcub::DoubleBuffer<uint64_t> bk(d_keys[cur], d_keys[cur ^ 1]);
            hipcub::DoubleBuffer<ValT> bv(d_vals[cur], d_vals[cur ^ 1]);
            RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, bk, bv, (int)n, 0, key_bits(chunk_len(k, c)), st));
            if (bk.Current() != d_keys[cur]) cur ^= 1;  // the library says in which half the sorted list ended up
        }
        // the halves the sorted list is not in: head flags and group indices in the keys' (4 + 4 bytes per element), the transcripts in
        // the values'; the groups' flags take the place of the head flags once those are summed
        uint32_t* d_heads = (uint32_t*)d_keys[cur ^ 1];
        uint32_t* d_gid = d_heads + n;
        int32_t* d_tids = (int32_t*)d_vals[cur ^ 1];
        uint8_t* d_group = (uint8_t*)d_heads;
        hipLaunchKernelGGL((k_heads<ValT>), dim3(blocks256(n)), dim3(256), 0, st, d_sep, d_soff, M, k, d_keys[cur], d_vals[cur], n, d_heads, d_tids);
        tb = tmp_bytes;
        RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tb, d_heads, d_gid, (int)n, st));
        RSEM_HIP_TRY(hipMemsetAsync(d_group, 0, (size_t)n, st));
        hipLaunchKernelGGL(k_flags, dim3(blocks256(n)), dim3(256), 0, st, d_gid, d_tids, n, d_group);
        hipLaunchKernelGGL(k_count, dim3(blocks256(n)), dim3(256), 0, st, d_gid, d_tids, n, d_group, d_shared);
        uint32_t groups = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&groups, d_gid + (n - 1), 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        n_groups += groups;
    }
    RSEM_HIP_TRY(q.kernels_end());
    RSEM_HIP_TRY(hipMemcpyAsync(shared, d_shared, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (info) {
        double up = 0, kern = 0;
        if (int rc = q.add_laps(up, kern)) return rc;
        info->n_groups = n_groups;
        info->n_batches = (int32_t)batches.size();
        info->batch_items = budget;
        info->max_batch_items = max_items;
        info->batch_bytes = (uint64_t)max_items * per_item + tmp_bytes;
        info->upload_ms = up;
        info->kernel_ms = kern;
    }
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_kmer_shared_counts(int device, int32_t M, const uint64_t* seq_off, const uint8_t* codes, int32_t k, uint32_t* shared,
                                       rsem_kmer_info* info) {
    RSEM_REQUIRE(device >= 0 && M >= 0 && seq_off && shared, "rsem_kmer_shared_counts: device and M must not be negative, seq_off and shared not NULL");
    RSEM_REQUIRE(k >= 1, "rsem_kmer_shared_counts: k must be at least 1");
    RSEM_REQUIRE(seq_off[0] == 0, "rsem_kmer_shared_counts: seq_off[0] must be 0");
    uint64_t n_kmers = 0, longest = 0;
    for (int32_t t = 0; t < M; t++) {
        RSEM_REQUIRE(seq_off[t + 1] >= seq_off[t], "rsem_kmer_shared_counts: seq_off must not decrease");
        const uint64_t len = seq_off[t + 1] - seq_off[t];
        RSEM_REQUIRE(len < (1ull << 32), "rsem_kmer_shared_counts: a transcript of 2^32 bases or more (the counters are 32-bit)");
        longest = std::max(longest, len);
        if (len >= (uint64_t)k) n_kmers += len - (uint64_t)k + 1;
    }
    const uint64_t L = seq_off[M];
    RSEM_REQUIRE(L == 0 || codes, "rsem_kmer_shared_counts: codes must not be NULL");
    uint8_t seen = 0;
    for (uint64_t i = 0; i < L; i++) seen |= (uint8_t)(codes[i] > 4);
    RSEM_REQUIRE(!seen, "rsem_kmer_shared_counts: codes must be 0 .. 4 (A C G T N)");
    uint64_t budget_env = 0;
    if (int rc = rsem::env_whole("RSEM_KMER_BATCH_ITEMS", 1, LLONG_MAX, &budget_env)) return rc;  // a test and measurement knob, read at call time
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_kmers = n_kmers;
        info->n_chunks = n_chunks(k);
    }
    for (int32_t t = 0; t < M; t++) shared[t] = 0;
    if (n_kmers == 0) return RSEM_OK;  // no transcript is as long as k: nothing to sort
    if (k > kMaxK) {
        rsem::set_last_error("rsem_kmer_shared_counts: k = %d with transcripts of up to %llu bases: k above %d is not supported (a tile's halo of "
                             "k - 1 codes is kept in LDS)", k, (unsigned long long)longest, kMaxK);
        return RSEM_ERR_INVALID;
    }
    // 32-bit positions as sort values while the separated codes (one separator behind every transcript) allow it
    const char* wide = getenv("RSEM_KMER_WIDE_VALUES");  // a test knob: the 64-bit positions on an input of any size
    if (wide && strcmp(wide, "0") && strcmp(wide, "1")) {
        rsem::set_last_error("RSEM_KMER_WIDE_VALUES = '%s': 0 or 1 is expected", wide);
        return RSEM_ERR_INVALID;
    }
    if (L + (uint64_t)M <= 0xffffffffull && !(wide && wide[0] == '1')) return run<uint32_t>(device, M, seq_off, codes, k, n_kmers, budget_env, shared, info);
    return run<uint64_t>(device, M, seq_off, codes, k, n_kmers, budget_env, shared, info);
}
