// pairscan.hip -- the reordering of rsem-scan-for-paired-end-reads on MI355X.  Replaces the loop of
// scanForPairedEndReads.cpp:78-126: the sequential walk that cuts a name-grouped file into groups, the four vectors of a paired group,
// std::sort with less_than (:39-51) and the pops from the back (:98-115).  The arithmetic is in pairscan_block.hpp.
//
// rsem_pairscan_reorder: a batch of whole runs of equal canonical names goes through
//   k_pairscan_mark     a lane per record: the cut of its name against the record before (hard / soft start), its class words;
//   hipcub::DeviceScan::InclusiveScan    RunCount: paired starts counted from the run's first record;
//   hipcub::DeviceScan::ExclusiveSum     twice: both | partial_1 << 32 and partial_2 | unknown << 32 before every record;
//   k_pairscan_open     a lane per record: does it open a group;
//   hipcub::DeviceScan::InclusiveSum     group ordinals;
//   k_pairscan_goff     a lane per record: a group's first record goes into goff;
//   k_pairscan_place    a lane per record: single-end, partial and unknown records to their places, `both` records behind their group's
//                       start in file order, the group's verdict; the wave's smallest (group << 8 | code) goes into the verdict word;
//   hipcub::DeviceScan::ExclusiveSum     the groups to sort, by a wave | by a workgroup << 32;
//   k_pairscan_lists    a lane per record: the two lists;
//   k_pairscan_rank     a wave per group of up to 64 `both` records, a workgroup per longer one: the stable rank of every record.
// The verdict word is the only word with more than one writer: a 64-bit vector atomicMin per wave that has a failing group.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "pairscan_block.hpp"
#include "stage_util.hpp"

using namespace rsem_pairk;

namespace {

using rsem::blocks256;
using Buf = rsem::GrowBuf<2>;  // a device buffer that only grows

enum { B_NOFF, B_NAMES, B_FLAG, B_TID, B_POS, B_MPOS, B_MARK, B_RUN, B_WA, B_WB, B_CA, B_CB, B_OPEN, B_ORD, B_GOFF, B_PERM, B_BOTH, B_SW, B_SWS, B_SMALL, B_LARGE, B_TMP,
       B_COUNT };

}  // namespace

struct rsem_pairscan {
    int device = 0;
    bool on_device = false, ended = false;
    unsigned long long* d_verdict = nullptr;
    rsem::StageQueue q;
    Buf buf[B_COUNT];
    size_t device_bytes = 0;
    std::mutex mu;
};

namespace {

__global__ void __launch_bounds__(256) k_pairscan_mark(Recs R, uint32_t* __restrict__ mark, uint64_t* __restrict__ wa, uint64_t* __restrict__ wb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i < R.n) {
        const uint32_t c = class_of(R.flag[i]);
        mark[i] = mark_record(R, i);
        wa[i] = class_word_a(c);
        wb[i] = class_word_b(c);
    } else if (i == R.n) {  // the sums' last output is the totals
        wa[i] = 0ull;
        wb[i] = 0ull;
    }
}

__global__ void __launch_bounds__(256) k_pairscan_open(int64_t n, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ run, uint32_t* __restrict__ open) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i < n) open[i] = opens_group(mark[i], run[i]);
}

__global__ void __launch_bounds__(256) k_pairscan_goff(int64_t n, const uint32_t* __restrict__ open, const uint32_t* __restrict__ ord, uint32_t* __restrict__ goff) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i < n && open[i]) goff[ord[i] - 1u] = (uint32_t)i;
    if (i == n - 1) goff[ord[i]] = (uint32_t)n;
}

__global__ void __launch_bounds__(256) k_pairscan_place(Recs R, Scans S, const uint32_t* __restrict__ goff, uint64_t group_base, uint32_t rec_base, uint32_t* __restrict__ perm,
                                                         uint32_t* __restrict__ both_src, uint64_t* __restrict__ sort_word, unsigned long long* verdict) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i == R.n) sort_word[i] = 0ull;
    place_body(i < R.n, i, R, S, goff, group_base, rec_base, perm, both_src, sort_word, verdict);
}

__global__ void __launch_bounds__(256) k_pairscan_lists(int64_t n, const uint64_t* __restrict__ sort_word, const uint64_t* __restrict__ sws, const uint32_t* __restrict__ ord,
                                                         uint32_t* __restrict__ small, uint32_t* __restrict__ large) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i >= n || !sort_word[i]) return;
    if (sort_word[i] & 0xffffffffull) small[sws[i] & 0xffffffffull] = ord[i] - 1u;
    else large[sws[i] >> 32] = ord[i] - 1u;
}

__global__ void __launch_bounds__(kGroupThreads) k_pairscan_rank(Recs R, uint32_t n_small, uint32_t nb_small, const uint32_t* __restrict__ small,
                                                                  const uint32_t* __restrict__ large, const uint32_t* __restrict__ goff, const uint64_t* __restrict__ ca,
                                                                  const uint32_t* __restrict__ both_src, uint32_t rec_base, uint32_t* __restrict__ perm) {
    __shared__ Key stage[kGroupThreads];
    const int tid = RSEM_TIDX;
    if (blockIdx.x < nb_small) {
        const int wv = tid >> 6;
        const uint32_t idx = blockIdx.x * 4u + (uint32_t)wv;
        if (idx >= n_small) return;
        const uint32_t g = small[idx], g0 = goff[g];
        rank_group<kWave>(g0, (uint32_t)((ca[goff[g + 1]] - ca[g0]) & 0xffffffffull), tid & 63, R, both_src, stage + wv * kWave, rec_base, perm);
    } else {
        const uint32_t g = large[blockIdx.x - nb_small], g0 = goff[g];
        rank_group<kGroupThreads>(g0, (uint32_t)((ca[goff[g + 1]] - ca[g0]) & 0xffffffffull), tid, R, both_src, stage, rec_base, perm);
    }
}

// RSEM_PAIRSCAN_BATCH_ITEMS, read at every call
int read_budget(uint64_t& budget) {
    budget = kDefaultBatchItems;
    return rsem::env_whole("RSEM_PAIRSCAN_BATCH_ITEMS", 1, LLONG_MAX, &budget);
}

int to_device(rsem_pairscan* h) {
    RSEM_HIP_TRY(hipSetDevice(h->device));
    if (h->on_device) return RSEM_OK;
    RSEM_HIP_TRY(h->q.create());
    RSEM_HIP_TRY(hipMalloc((void**)&h->d_verdict, 8));
    h->device_bytes += 8;
    h->on_device = true;
    return RSEM_OK;
}

struct Call {
    const uint64_t* name_off;
    const uint8_t* names;
    const uint32_t* flag;
    const int32_t *tid, *pos, *mpos;
    uint32_t* perm_out;
};

// the records [lo, lo + n) of the call: one batch.  word: the verdict word so far (kNoVerdict: nothing failed)
int run_batch(rsem_pairscan* h, const Call& c, uint64_t lo, uint64_t n, uint64_t group_base, unsigned long long& word, uint64_t& n_groups, uint64_t& n_sorted,
              int64_t& fail_record, rsem_pairscan_verdict* v, double& upload_ms, double& kernel_ms) {
    const uint64_t nb = c.name_off[lo + n] - c.name_off[lo];
    size_t t1 = 0, t2 = 0, t3 = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, t1, (const uint32_t*)nullptr, (uint32_t*)nullptr, RunCount(), (int)n, h->q.st));
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n + 1), h->q.st));
    RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, t3, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, h->q.st));
    const size_t w4 = (size_t)(n + 1) * 4, w8 = (size_t)(n + 1) * 8;
    const size_t need[B_COUNT] = {w8, (size_t)nb, w4, w4, w4, w4, w4, w4, w8, w8, w8, w8, w4, w4, w4, w4, w4, w8, w8, w4, w4, std::max(t1, std::max(t2, t3))};
    for (int b = 0; b < B_COUNT; b++) RSEM_HIP_TRY(h->buf[b].need(std::max<size_t>(need[b], 8), h->device_bytes));
    auto U64 = [&](int b) { return h->buf[b].as<uint64_t>(); };
    auto U32 = [&](int b) { return h->buf[b].as<uint32_t>(); };
    auto I32 = [&](int b) { return h->buf[b].as<int32_t>(); };
    hipStream_t st = h->q.st;
    RSEM_HIP_TRY(h->q.upload_begin());
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_NOFF), c.name_off + lo, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_NAMES].p, c.names + c.name_off[lo], (size_t)nb, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U32(B_FLAG), c.flag + lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_TID), c.tid + lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_POS), c.pos + lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_MPOS), c.mpos + lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(h->q.upload_end());

    const Recs R{U64(B_NOFF), h->buf[B_NAMES].as<uint8_t>(), c.name_off[lo], U32(B_FLAG), I32(B_TID), I32(B_POS), I32(B_MPOS), (int64_t)n};
    const Scans S{U32(B_ORD), U64(B_CA), U64(B_CB)};
    hipLaunchKernelGGL(k_pairscan_mark, dim3(blocks256(n + 1)), dim3(256), 0, st, R, U32(B_MARK), U64(B_WA), U64(B_WB));
    size_t tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveScan(h->buf[B_TMP].p, tb, U32(B_MARK), U32(B_RUN), RunCount(), (int)n, st));
    tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U64(B_WA), U64(B_CA), (int)(n + 1), st));
    tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U64(B_WB), U64(B_CB), (int)(n + 1), st));
    hipLaunchKernelGGL(k_pairscan_open, dim3(blocks256(n)), dim3(256), 0, st, (int64_t)n, U32(B_MARK), U32(B_RUN), U32(B_OPEN));
    tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(h->buf[B_TMP].p, tb, U32(B_OPEN), U32(B_ORD), (int)n, st));
    hipLaunchKernelGGL(k_pairscan_goff, dim3(blocks256(n)), dim3(256), 0, st, (int64_t)n, U32(B_OPEN), U32(B_ORD), U32(B_GOFF));
    hipLaunchKernelGGL(k_pairscan_place, dim3(blocks256(n + 1)), dim3(256), 0, st, R, S, U32(B_GOFF), group_base, (uint32_t)lo, U32(B_PERM), U32(B_BOTH), U64(B_SW),
                       h->d_verdict);
    tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U64(B_SW), U64(B_SWS), (int)(n + 1), st));
    hipLaunchKernelGGL(k_pairscan_lists, dim3(blocks256(n)), dim3(256), 0, st, (int64_t)n, U64(B_SW), U64(B_SWS), U32(B_ORD), U32(B_SMALL), U32(B_LARGE));
    uint64_t to_sort = 0;
    uint32_t ng = 0;
    RSEM_HIP_TRY(hipMemcpyAsync(&to_sort, U64(B_SWS) + n, 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(&ng, U32(B_ORD) + (n - 1), 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(&word, h->d_verdict, 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    v->n_launches += 10;
    const uint32_t n_small = (uint32_t)(to_sort & 0xffffffffull), n_large = (uint32_t)(to_sort >> 32), nb_small = (n_small + 3) / 4;
    if (ng < 1 || ng > n || (uint64_t)n_small + n_large > ng) {  // what the lists were sized for
        rsem::set_last_error("rsem_pairscan_reorder: %u groups, %u and %u of them to sort, in a batch of %llu records", ng, n_small, n_large, (unsigned long long)n);
        return RSEM_ERR_STATE;
    }
    if (word == kNoVerdict && n_small + n_large) {
        hipLaunchKernelGGL(k_pairscan_rank, dim3(nb_small + n_large), dim3(kGroupThreads), 0, st, R, n_small, nb_small, U32(B_SMALL), U32(B_LARGE), U32(B_GOFF), U64(B_CA),
                           U32(B_BOTH), (uint32_t)lo, U32(B_PERM));
        v->n_launches += 1;
    }
    RSEM_HIP_TRY(h->q.kernels_end());
    if (word == kNoVerdict) RSEM_HIP_TRY(hipMemcpyAsync(c.perm_out + lo, U32(B_PERM), (size_t)n * 4, hipMemcpyDeviceToHost, st));
    else {
        const uint64_t fg = word >> 8;
        if (fg < group_base || fg >= group_base + ng) { rsem::set_last_error("rsem_pairscan_reorder: failing group %llu outside its batch", (unsigned long long)fg); return RSEM_ERR_STATE; }
        uint32_t first = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&first, U32(B_GOFF) + (fg - group_base), 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        fail_record = (int64_t)(lo + first);
    }
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    n_groups += ng;
    n_sorted += (uint64_t)n_small + n_large;
    return h->q.add_laps(upload_ms, kernel_ms);
}

}  // namespace

extern "C" int rsem_pairscan_create(rsem_pairscan** out, int device) {
    RSEM_REQUIRE(out, "rsem_pairscan_create: out must not be NULL");
    *out = nullptr;
    RSEM_REQUIRE(device >= 0, "rsem_pairscan_create: device must not be negative");
    rsem_pairscan* h = new rsem_pairscan();
    h->device = device;
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_pairscan_destroy(rsem_pairscan* h) {
    if (!h) return;
    if (h->on_device) {
        (void)hipSetDevice(h->device);
        if (h->d_verdict) (void)hipFree(h->d_verdict);
        for (Buf& b : h->buf) b.release(h->device_bytes);
        h->q.release();
    }
    delete h;
}

extern "C" int rsem_pairscan_reorder(rsem_pairscan* h, int64_t n_records, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, const int32_t* tid,
                                     const int32_t* pos, const int32_t* mpos, int32_t last, uint32_t* perm_out, rsem_pairscan_verdict* v) {
    RSEM_REQUIRE(h, "rsem_pairscan_reorder: the handle must not be NULL");
    RSEM_REQUIRE(v, "rsem_pairscan_reorder: the verdict must not be NULL");
    RSEM_REQUIRE(n_records >= 0, "rsem_pairscan_reorder: n_records must not be negative");
    RSEM_REQUIRE(n_records < (1ll << 32), "rsem_pairscan_reorder: 2^32 records or more in one call");
    RSEM_REQUIRE(n_records == 0 || perm_out, "rsem_pairscan_reorder: perm_out must not be NULL");
    RSEM_REQUIRE(n_records == 0 || (name_off && names && flag && tid && pos && mpos), "rsem_pairscan_reorder: the per-record arrays must not be NULL");
    uint64_t budget;
    if (int rc = read_budget(budget)) return rc;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->ended) { rsem::set_last_error("rsem_pairscan_reorder: the call before this one was the last"); return RSEM_ERR_STATE; }
    memset(v, 0, sizeof(*v));
    v->group = -1;
    v->group_record = -1;
    v->batch_items = budget;
    v->n_records = (uint64_t)n_records;
    v->device_bytes = h->device_bytes;
    if (n_records == 0) { h->ended = last != 0; return RSEM_OK; }  // nothing to order: no device needed
    RSEM_REQUIRE(name_off[0] == 0, "rsem_pairscan_reorder: name_off must start at 0");
    for (int64_t i = 0; i < n_records; i++)
        if (name_off[i + 1] <= name_off[i] || name_off[i + 1] - name_off[i] > kMaxName) {
            rsem::set_last_error("rsem_pairscan_reorder: record %lld: a name of 1 to %u bytes is expected (name_off must ascend)", (long long)i, kMaxName);
            return RSEM_ERR_INVALID;
        }
    if (int rc = to_device(h)) return rc;
    const Call c{name_off, names, flag, tid, pos, mpos, perm_out};
    const Recs all{name_off, names, 0, flag, tid, pos, mpos, n_records};
    unsigned long long word = kNoVerdict;
    RSEM_HIP_TRY(hipMemcpy(h->d_verdict, &word, 8, hipMemcpyHostToDevice));
    uint64_t n_groups = 0, n_sorted = 0;
    int64_t fail_record = -1;
    double upload_ms = 0, kernel_ms = 0;
    for (uint64_t lo = 0; lo < (uint64_t)n_records && word == kNoVerdict;) {
        const uint64_t hi = batch_end(all, lo, budget);
        if (hi - lo > 0x3fffffffull) { rsem::set_last_error("rsem_pairscan_reorder: a batch of %llu records (2^30 - 1 at most)", (unsigned long long)(hi - lo)); return RSEM_ERR_INVALID; }
        if (int rc = run_batch(h, c, lo, hi - lo, n_groups, word, n_groups, n_sorted, fail_record, v, upload_ms, kernel_ms)) return rc;
        v->n_batches++;
        lo = hi;
    }
    v->n_groups = n_groups;
    v->n_sorted_groups = n_sorted;
    v->device_bytes = h->device_bytes;
    v->upload_ms = upload_ms;
    v->kernel_ms = kernel_ms;
    if (word != kNoVerdict) {
        v->code = (int32_t)(word & 0xffu);
        v->group = (int64_t)(word >> 8);
        v->group_record = fail_record;
    } else h->ended = last != 0;
    return RSEM_OK;
}
