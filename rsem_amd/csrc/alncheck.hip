// alncheck.hip -- the checks of rsem-sam-validator and rsem-get-unique on MI355X.  Replaces the loop of
// samValidator.cpp:82-183 with check_read (:26-59) and its std::set<std::string> of read names, and output() of getUnique.cpp:25-30
// with the grouping of :55-65.  The checks themselves are in alncheck_block.hpp.
//
// rsem_alncheck_push: a batch of whole units goes through
//   k_alncheck_unit     a lane per unit: its own checks, the cut of its name, the name's hash, whether it opens a group, its lengths
//                       against the unit before; the wave's smallest failing (unit << 8 | code) goes into the verdict word;
//   hipcub::DeviceScan::ExclusiveSum     over (1 << 40 | name length) of the opening units: group ordinal and name offset at once;
//   k_alncheck_gather   a lane per unit: an opening unit's name goes behind the resident names;
//   hipcub::DeviceRadixSort::SortPairs   the batch's groups by hash (stable: ties stay in group order) -- the batch's resident run;
//   k_alncheck_lookup   a lane per group: its hash bisected in every earlier run and looked for beside it in its own, every
//                       candidate settled by its bytes; NOT_GROUPED goes into the verdict word the same way.
// The verdict word is the only word with more than one writer: a 64-bit vector atomicMin per wave that has a failing unit.
// rsem_alncheck_unique: k_unique_start, hipcub::DeviceScan::InclusiveSum, k_unique_keep (every keep byte has one writer).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "alncheck_block.hpp"
#include "stage_util.hpp"

using namespace rsem_alnk;

namespace {

using rsem::blocks256;
using Buf = rsem::GrowBuf<2>;  // a device buffer that only grows; keep: what it holds stays (the resident arrays)

enum { B_NOFF, B_NAMES, B_FLAG, B_TID, B_POS, B_ISIZE, B_LQ, B_COFF, B_CIGAR, B_DETAIL, B_HASH, B_OPEN, B_SCAN, B_GHASH, B_GUNIT, B_SUNIT, B_UREF, B_RUNOFF, B_TMP,
       B_COUNT };

}  // namespace

struct rsem_alncheck {
    int device = 0;
    std::vector<uint32_t> target_len;
    bool on_device = false, refused = false, ended = false;
    int paired = -1;  // fixed by the first record of the first push
    void* d_tlen = nullptr;
    Carry* d_carry[2] = {nullptr, nullptr};
    int carry_cur = 0;
    unsigned long long* d_verdict = nullptr;
    rsem::StageQueue q;
    Buf buf[B_COUNT];
    Buf res_hash, res_ref, res_names;   // the closed and open groups of the file so far: 16 bytes a group and the names' bytes
    uint64_t n_groups = 0, names_used = 0;
    std::vector<uint64_t> run_off{0};   // the sorted runs of res_hash / res_ref, one a batch that opened a group
    size_t device_bytes = 0;
    std::mutex mu;
};

namespace {

__global__ void __launch_bounds__(256) k_alncheck_unit(Recs R, int paired, const uint32_t* __restrict__ target_len, const Carry* __restrict__ before,
                                                        Carry* __restrict__ after, int64_t n_units, int hash_bits, uint64_t unit_base, UnitArrays A,
                                                        unsigned long long* verdict) {
    const int64_t u = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (u == n_units) A.open[u] = 0ull;  // the scan's last output is the totals
    unit_body(u < n_units, u, R, paired, target_len, before, after, n_units, hash_bits, unit_base, A, verdict);
}

__global__ void __launch_bounds__(256) k_alncheck_gather(Recs R, int mates, int64_t n_units, const uint64_t* __restrict__ open, const uint64_t* __restrict__ scan,
                                                          const uint64_t* __restrict__ hash, uint64_t names_used, uint8_t* __restrict__ res_names,
                                                          uint64_t* __restrict__ g_hash, uint32_t* __restrict__ g_unit, uint64_t* __restrict__ u_ref) {
    const int64_t u = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (u < n_units) gather_unit(u, R, mates, open, scan, hash, names_used, res_names, g_hash, g_unit, u_ref);
}

__global__ void __launch_bounds__(256) k_alncheck_lookup(uint64_t n_g, Resident S, const uint32_t* __restrict__ sorted_unit, const uint64_t* __restrict__ u_ref,
                                                          uint32_t* __restrict__ unit_detail, uint64_t unit_base, unsigned long long* verdict) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + (uint64_t)RSEM_TIDX;
    lookup_body(p < n_g, p, S, sorted_unit, u_ref, unit_detail, unit_base, verdict);
}

__global__ void __launch_bounds__(256) k_unique_start(Recs R, uint32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i < R.n) start[i] = unique_start(R, i);
}

__global__ void __launch_bounds__(256) k_unique_keep(int64_t n, const uint32_t* __restrict__ incl, const uint32_t* __restrict__ flag, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (i < n) keep[i] = unique_keep(incl, flag, n, i);
}

// RSEM_ALNCHECK_BATCH_ITEMS and RSEM_ALNCHECK_HASH_BITS, read at every call
int read_knobs(uint64_t& budget, int& hash_bits) {
    budget = kDefaultBatchItems;
    uint64_t bits = 64;
    if (int rc = rsem::env_whole("RSEM_ALNCHECK_BATCH_ITEMS", 1, LLONG_MAX, &budget)) return rc;
    if (int rc = rsem::env_whole("RSEM_ALNCHECK_HASH_BITS", 1, 64, &bits)) return rc;
    hash_bits = (int)bits;
    return RSEM_OK;
}

// what both entry points ask of the names
int check_names(const char* who, int64_t n, const uint64_t* name_off, const uint8_t* names) {
    if (name_off[0] != 0) { rsem::set_last_error("%s: name_off must start at 0", who); return RSEM_ERR_INVALID; }
    for (int64_t i = 0; i < n; i++) {
        if (name_off[i + 1] <= name_off[i] || name_off[i + 1] - name_off[i] > kMaxName) {
            rsem::set_last_error("%s: record %lld: a name of 1 to %u bytes is expected (name_off must ascend)", who, (long long)i, kMaxName);
            return RSEM_ERR_INVALID;
        }
        if (names[name_off[i]] == 0 || is_space(names[name_off[i]])) {
            rsem::set_last_error("%s: record %lld: its name starts with white space: the name the reference compares is empty (it asserts there)", who, (long long)i);
            return RSEM_ERR_INVALID;
        }
    }
    return RSEM_OK;
}

int to_device(rsem_alncheck* h) {
    RSEM_HIP_TRY(hipSetDevice(h->device));
    if (h->on_device) return RSEM_OK;
    RSEM_HIP_TRY(h->q.create());
    const size_t tb = std::max<size_t>(h->target_len.size() * 4, 8);
    RSEM_HIP_TRY(hipMalloc(&h->d_tlen, tb));
    h->device_bytes += tb;
    if (!h->target_len.empty()) RSEM_HIP_TRY(hipMemcpy(h->d_tlen, h->target_len.data(), h->target_len.size() * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {
        RSEM_HIP_TRY(hipMalloc((void**)&h->d_carry[k], sizeof(Carry)));
        RSEM_HIP_TRY(hipMemset(h->d_carry[k], 0, sizeof(Carry)));
        h->device_bytes += sizeof(Carry);
    }
    RSEM_HIP_TRY(hipMalloc((void**)&h->d_verdict, 8));
    h->device_bytes += 8;
    h->on_device = true;
    return RSEM_OK;
}

struct PushCall {
    const uint64_t* name_off;
    const uint8_t* names;
    const uint32_t* flag;
    const int32_t *tid, *pos, *isize, *lq;
    const uint64_t* cigar_off;
    const uint32_t* cigar;
};

// the records [lo, lo + nrec) of the push: one batch.  Returns the verdict word (kNoVerdict: nothing failed so far) and, for a
// failing unit of this batch, its detail word.
int run_batch(rsem_alncheck* h, const PushCall& c, uint64_t lo, uint64_t nrec, int hash_bits, unsigned long long& word, uint32_t& fail_detail, uint64_t& opened,
              rsem_alncheck_verdict* v, double& upload_ms, double& kernel_ms) {
    const int mates = h->paired ? 2 : 1;
    const uint64_t nu = (nrec + (uint64_t)mates - 1) / (uint64_t)mates, unit_base = lo / (uint64_t)mates;
    const uint64_t nb = c.name_off[lo + nrec] - c.name_off[lo], nw = c.cigar_off[lo + nrec] - c.cigar_off[lo];
    size_t t_scan = 0, t_sort = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(nu + 1), h->q.st));
    RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nu, 0,
                                                    hash_bits, h->q.st));
    const size_t need[B_COUNT] = {(size_t)(nrec + 1) * 8, (size_t)nb, (size_t)nrec * 4, (size_t)nrec * 4, (size_t)nrec * 4, (size_t)nrec * 4, (size_t)nrec * 4, (size_t)(nrec + 1) * 8,
                                  (size_t)nw * 4, (size_t)nu * 4, (size_t)nu * 8, (size_t)(nu + 1) * 8, (size_t)(nu + 1) * 8, (size_t)nu * 8, (size_t)nu * 4, (size_t)nu * 4,
                                  (size_t)nu * 8, (h->run_off.size() + 1) * 8, std::max(t_scan, t_sort)};
    for (int b = 0; b < B_COUNT; b++) RSEM_HIP_TRY(h->buf[b].need(std::max<size_t>(need[b], 8), h->device_bytes));
    // the resident arrays take the batch's groups and names at most: they grow here, or the push fails with everything kept
    hipError_t e1 = h->res_hash.need((size_t)(h->n_groups + nu) * 8, h->device_bytes, (size_t)h->n_groups * 8);
    if (e1 == hipSuccess) e1 = h->res_ref.need((size_t)(h->n_groups + nu) * 8, h->device_bytes, (size_t)h->n_groups * 8);
    if (e1 == hipSuccess) e1 = h->res_names.need((size_t)(h->names_used + nb), h->device_bytes, (size_t)h->names_used);
    if (e1 != hipSuccess) {
        (void)hipGetLastError();
        rsem::set_last_error("rsem_alncheck_push: the names of %llu groups (%llu bytes) and %llu more do not fit the device: %s",
                             (unsigned long long)h->n_groups, (unsigned long long)h->names_used, (unsigned long long)nu, hipGetErrorString(e1));
        return e1 == hipErrorOutOfMemory ? RSEM_ERR_NOMEM : RSEM_ERR_HIP;
    }
    auto U64 = [&](int b) { return h->buf[b].as<uint64_t>(); };
    auto U32 = [&](int b) { return h->buf[b].as<uint32_t>(); };
    auto I32 = [&](int b) { return h->buf[b].as<int32_t>(); };
    hipStream_t st = h->q.st;
    RSEM_HIP_TRY(h->q.upload_begin());
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_NOFF), c.name_off + lo, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_NAMES].p, c.names + c.name_off[lo], (size_t)nb, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U32(B_FLAG), c.flag + lo, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_TID), c.tid + lo, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_POS), c.pos + lo, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_ISIZE), c.isize + lo, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_LQ), c.lq + lo, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_COFF), c.cigar_off + lo, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, st));
    if (nw) RSEM_HIP_TRY(hipMemcpyAsync(U32(B_CIGAR), c.cigar + c.cigar_off[lo], (size_t)nw * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_RUNOFF), h->run_off.data(), h->run_off.size() * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(h->q.upload_end());

    const Recs R{U64(B_NOFF), h->buf[B_NAMES].as<uint8_t>(), c.name_off[lo], U32(B_FLAG), I32(B_TID), I32(B_POS), I32(B_ISIZE), I32(B_LQ), U64(B_COFF), U32(B_CIGAR),
                 c.cigar_off[lo], (int64_t)nrec};
    const UnitArrays A{U32(B_DETAIL), U64(B_HASH), U64(B_OPEN)};
    Carry *before = h->d_carry[h->carry_cur], *after = h->d_carry[h->carry_cur ^ 1];
    hipLaunchKernelGGL(k_alncheck_unit, dim3(blocks256(nu + 1)), dim3(256), 0, st, R, h->paired, (const uint32_t*)h->d_tlen, before, after, (int64_t)nu, hash_bits,
                       unit_base, A, h->d_verdict);
    size_t tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U64(B_OPEN), U64(B_SCAN), (int)(nu + 1), st));
    hipLaunchKernelGGL(k_alncheck_gather, dim3(blocks256(nu)), dim3(256), 0, st, R, mates, (int64_t)nu, U64(B_OPEN), U64(B_SCAN), U64(B_HASH), h->names_used,
                       h->res_names.as<uint8_t>(), U64(B_GHASH), U32(B_GUNIT), U64(B_UREF));
    uint64_t totals = 0;
    RSEM_HIP_TRY(hipMemcpyAsync(&totals, U64(B_SCAN) + nu, 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    const uint64_t ng = totals >> 40, name_bytes = totals & ((1ull << 40) - 1ull);
    if (ng > nu || name_bytes > nb) {  // what the resident arrays were sized for
        rsem::set_last_error("rsem_alncheck_push: %llu groups with %llu name bytes on the device, %llu and %llu at most were expected", (unsigned long long)ng,
                             (unsigned long long)name_bytes, (unsigned long long)nu, (unsigned long long)nb);
        return RSEM_ERR_STATE;
    }
    v->n_launches += 3;
    if (ng) {
        tb = h->buf[B_TMP].cap;
        RSEM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(h->buf[B_TMP].p, tb, U64(B_GHASH), h->res_hash.as<uint64_t>() + h->n_groups, U32(B_GUNIT), U32(B_SUNIT), (int)ng, 0,
                                                        hash_bits, st));
        const Resident S{h->res_hash.as<uint64_t>(), h->res_ref.as<uint64_t>(), h->res_names.as<uint8_t>(), U64(B_RUNOFF), (uint32_t)(h->run_off.size() - 1)};
        hipLaunchKernelGGL(k_alncheck_lookup, dim3(blocks256(ng)), dim3(256), 0, st, ng, S, U32(B_SUNIT), U64(B_UREF), U32(B_DETAIL), unit_base, h->d_verdict);
        v->n_launches += 2;
    }
    RSEM_HIP_TRY(h->q.kernels_end());
    RSEM_HIP_TRY(hipMemcpyAsync(&word, h->d_verdict, 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (word != kNoVerdict) {
        const uint64_t fu = word >> 8;
        if (fu < unit_base || fu >= unit_base + nu) { rsem::set_last_error("rsem_alncheck_push: failing unit %llu outside its batch", (unsigned long long)fu); return RSEM_ERR_STATE; }
        RSEM_HIP_TRY(hipMemcpy(&fail_detail, U32(B_DETAIL) + (fu - unit_base), 4, hipMemcpyDeviceToHost));
    } else {
        h->n_groups += ng;
        h->names_used += name_bytes;
        if (ng) h->run_off.push_back(h->n_groups);
        h->carry_cur ^= 1;
        opened += ng;
    }
    return h->q.add_laps(upload_ms, kernel_ms);
}

}  // namespace

extern "C" int rsem_alncheck_create(rsem_alncheck** out, int device, int32_t n_targets, const uint32_t* target_len) {
    RSEM_REQUIRE(out, "rsem_alncheck_create: out must not be NULL");
    *out = nullptr;
    RSEM_REQUIRE(device >= 0, "rsem_alncheck_create: device must not be negative");
    RSEM_REQUIRE(n_targets >= 0, "rsem_alncheck_create: n_targets must not be negative");
    RSEM_REQUIRE(n_targets == 0 || target_len, "rsem_alncheck_create: target_len must not be NULL");
    rsem_alncheck* h = new rsem_alncheck();
    h->device = device;
    h->target_len.assign(target_len, target_len + n_targets);
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_alncheck_destroy(rsem_alncheck* h) {
    if (!h) return;
    if (h->on_device) {
        (void)hipSetDevice(h->device);
        for (void* p : {h->d_tlen, (void*)h->d_carry[0], (void*)h->d_carry[1], (void*)h->d_verdict})
            if (p) (void)hipFree(p);
        for (Buf* b : {&h->res_hash, &h->res_ref, &h->res_names}) b->release(h->device_bytes);
        for (Buf& b : h->buf) b.release(h->device_bytes);
        h->q.release();
    }
    delete h;
}

extern "C" int rsem_alncheck_push(rsem_alncheck* h, int64_t n_records, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, const int32_t* tid,
                                  const int32_t* pos, const int32_t* isize, const int32_t* l_qseq, const uint64_t* cigar_off, const uint32_t* cigar, int32_t last,
                                  rsem_alncheck_verdict* v) {
    RSEM_REQUIRE(h, "rsem_alncheck_push: the handle must not be NULL");
    RSEM_REQUIRE(v, "rsem_alncheck_push: the verdict must not be NULL");
    RSEM_REQUIRE(n_records >= 0, "rsem_alncheck_push: n_records must not be negative");
    RSEM_REQUIRE(n_records < (1ll << 40), "rsem_alncheck_push: 2^40 records or more in one push");
    RSEM_REQUIRE(n_records == 0 || (name_off && names && flag && tid && pos && isize && l_qseq && cigar_off), "rsem_alncheck_push: the per-record arrays must not be NULL");
    uint64_t budget;
    int hash_bits;
    if (int rc = read_knobs(budget, hash_bits)) return rc;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->refused) { rsem::set_last_error("rsem_alncheck_push: a verdict has been returned for this handle: it takes no more records"); return RSEM_ERR_STATE; }
    if (h->ended) { rsem::set_last_error("rsem_alncheck_push: the push before this one was the last"); return RSEM_ERR_STATE; }
    memset(v, 0, sizeof(*v));
    v->unit_record = -1;
    v->batch_items = budget;
    v->n_records = (uint64_t)n_records;
    v->paired = h->paired;
    v->device_bytes = h->device_bytes;
    if (n_records == 0) { h->ended = last != 0; return RSEM_OK; }  // nothing to check: no device needed
    if (int rc = check_names("rsem_alncheck_push", n_records, name_off, names)) return rc;
    RSEM_REQUIRE(cigar_off[0] == 0, "rsem_alncheck_push: cigar_off must start at 0");
    const int32_t n_targets = (int32_t)h->target_len.size();
    for (int64_t i = 0; i < n_records; i++) {
        if (cigar_off[i + 1] < cigar_off[i] || cigar_off[i + 1] - cigar_off[i] > 65535) {
            rsem::set_last_error("rsem_alncheck_push: record %lld: cigar_off must not descend, 65535 operations at most", (long long)i);
            return RSEM_ERR_INVALID;
        }
        if (l_qseq[i] < 1) { rsem::set_last_error("rsem_alncheck_push: record %lld: l_qseq %d (the reference asserts l_qseq > 0)", (long long)i, l_qseq[i]); return RSEM_ERR_INVALID; }
        if (!(flag[i] & 4u) && (tid[i] < 0 || tid[i] >= n_targets)) {
            rsem::set_last_error("rsem_alncheck_push: record %lld is mapped to reference %d of %d", (long long)i, tid[i], n_targets);
            return RSEM_ERR_INVALID;
        }
    }
    RSEM_REQUIRE(cigar_off[n_records] == 0 || cigar, "rsem_alncheck_push: cigar must not be NULL");
    const int paired = h->paired >= 0 ? h->paired : (int)(flag[0] & 1u);
    RSEM_REQUIRE(!paired || last || !(n_records & 1), "rsem_alncheck_push: a push of paired-end records holds whole units (an even number) unless it is the last");
    h->paired = paired;
    v->paired = paired;
    if (int rc = to_device(h)) return rc;
    const int mates = paired ? 2 : 1;
    const PushCall c{name_off, names, flag, tid, pos, isize, l_qseq, cigar_off, cigar};
    unsigned long long word = kNoVerdict;
    RSEM_HIP_TRY(hipMemcpy(h->d_verdict, &word, 8, hipMemcpyHostToDevice));
    uint32_t fail_detail = 0;
    uint64_t opened = 0;
    double upload_ms = 0, kernel_ms = 0;
    int rc = RSEM_OK;
    for (uint64_t lo = 0; lo < (uint64_t)n_records && word == kNoVerdict;) {
        const uint64_t take = batch_records((uint64_t)n_records - lo, budget, mates);
        if (take > 0x3fffffffull) { rsem::set_last_error("rsem_alncheck_push: a batch of %llu records (2^30 - 1 at most)", (unsigned long long)take); rc = RSEM_ERR_INVALID; break; }
        if ((rc = run_batch(h, c, lo, take, hash_bits, word, fail_detail, opened, v, upload_ms, kernel_ms)) != RSEM_OK) break;
        v->n_batches++;
        lo += take;
    }
    if (rc != RSEM_OK) { h->refused = true; return rc; }  // (the handle's state is behind the records it has seen)
    const uint64_t n_units = ((uint64_t)n_records + (uint64_t)mates - 1) / (uint64_t)mates;
    v->n_units = n_units;
    v->n_groups = opened;
    v->resident_groups = h->n_groups;
    v->resident_name_bytes = h->names_used;
    v->device_bytes = h->device_bytes;
    v->upload_ms = upload_ms;
    v->kernel_ms = kernel_ms;
    if (word != kNoVerdict) {
        h->refused = true;
        v->code = (int32_t)(fail_detail & 0xffu);
        v->mate = (int32_t)((fail_detail >> 8) & 0xffu);
        v->cigar_op = fail_detail >> 16;
        v->units_ok = word >> 8;
        v->unit_record = (int64_t)((word >> 8) * (uint64_t)mates);
        if ((uint32_t)v->code != (uint32_t)(word & 0xffu)) { rsem::set_last_error("rsem_alncheck_push: the verdict word and the unit's detail disagree"); return RSEM_ERR_STATE; }
    } else {
        v->units_ok = n_units;
        h->ended = last != 0;
    }
    return RSEM_OK;
}

extern "C" int rsem_alncheck_unique(int device, int64_t n_records, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, uint8_t* keep,
                                    rsem_alncheck_info* info) {
    RSEM_REQUIRE(device >= 0, "rsem_alncheck_unique: device must not be negative");
    RSEM_REQUIRE(n_records >= 0, "rsem_alncheck_unique: n_records must not be negative");
    RSEM_REQUIRE(n_records < (1ll << 40), "rsem_alncheck_unique: 2^40 records or more in one call");
    RSEM_REQUIRE(n_records == 0 || (name_off && names && flag && keep), "rsem_alncheck_unique: the per-record arrays must not be NULL");
    uint64_t budget;
    int hash_bits;
    if (int rc = read_knobs(budget, hash_bits)) return rc;
    if (info) { memset(info, 0, sizeof(*info)); info->batch_items = budget; info->n_records = (uint64_t)n_records; }
    if (n_records == 0) return RSEM_OK;
    if (int rc = check_names("rsem_alncheck_unique", n_records, name_off, names)) return rc;
    // batches of whole groups: the end moves behind the group it would cut (the host looks at the names at the cut only)
    std::vector<std::pair<uint64_t, uint64_t>> batches;
    uint64_t largest = 0, largest_bytes = 0;
    for (uint64_t lo = 0; lo < (uint64_t)n_records;) {
        uint64_t hi = std::min<uint64_t>((uint64_t)n_records, lo + budget);
        while (hi < (uint64_t)n_records && name_off[hi + 1] - name_off[hi] == name_off[hi] - name_off[hi - 1] &&
               !memcmp(names + name_off[hi], names + name_off[hi - 1], name_off[hi] - name_off[hi - 1])) hi++;
        if (hi - lo > 0x3fffffffull) { rsem::set_last_error("rsem_alncheck_unique: a batch of %llu records (2^30 - 1 at most)", (unsigned long long)(hi - lo)); return RSEM_ERR_INVALID; }
        batches.push_back({lo, hi});
        largest = std::max(largest, hi - lo);
        largest_bytes = std::max(largest_bytes, name_off[hi] - name_off[lo]);
        lo = hi;
    }
    RSEM_HIP_TRY(hipSetDevice(device));
    rsem::StageQueue q;
    RSEM_HIP_TRY(q.create());
    hipStream_t st = q.st;
    size_t t_scan = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, t_scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)largest, st));
    rsem::DevMem mem;
    uint64_t* d_noff = nullptr;
    uint8_t *d_names = nullptr, *d_keep = nullptr, *d_tmp = nullptr;
    uint32_t *d_flag = nullptr, *d_start = nullptr, *d_incl = nullptr;
    RSEM_HIP_TRY(mem.alloc(&d_noff, (size_t)largest + 1));
    RSEM_HIP_TRY(mem.alloc(&d_names, (size_t)largest_bytes + 8));
    RSEM_HIP_TRY(mem.alloc(&d_flag, (size_t)largest));
    RSEM_HIP_TRY(mem.alloc(&d_start, (size_t)largest));
    RSEM_HIP_TRY(mem.alloc(&d_incl, (size_t)largest));
    RSEM_HIP_TRY(mem.alloc(&d_keep, (size_t)largest + 8));
    RSEM_HIP_TRY(mem.alloc(&d_tmp, t_scan + 8));
    double upload_ms = 0, kernel_ms = 0;
    uint64_t n_groups = 0, n_kept = 0;
    for (const auto& b : batches) {
        const uint64_t lo = b.first, n = b.second - b.first, nb = name_off[b.second] - name_off[lo];
        RSEM_HIP_TRY(q.upload_begin());
        RSEM_HIP_TRY(hipMemcpyAsync(d_noff, name_off + lo, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_names, names + name_off[lo], (size_t)nb, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_flag, flag + lo, (size_t)n * 4, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(q.upload_end());
        const Recs R{d_noff, d_names, name_off[lo], d_flag, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, (int64_t)n};
        hipLaunchKernelGGL(k_unique_start, dim3(blocks256(n)), dim3(256), 0, st, R, d_start);
        size_t tb = t_scan + 8;
        RSEM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(d_tmp, tb, (const uint32_t*)d_start, d_incl, (int)n, st));
        hipLaunchKernelGGL(k_unique_keep, dim3(blocks256(n)), dim3(256), 0, st, (int64_t)n, (const uint32_t*)d_incl, (const uint32_t*)d_flag, d_keep);
        RSEM_HIP_TRY(q.kernels_end());
        uint32_t groups = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(keep + lo, d_keep, (size_t)n, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(&groups, d_incl + (n - 1), 4, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (int rc = q.add_laps(upload_ms, kernel_ms)) return rc;
        n_groups += groups;
        for (uint64_t i = lo; i < b.second; i++) n_kept += keep[i];
    }
    if (info) {
        info->n_groups = n_groups;
        info->n_kept = n_kept;
        info->n_batches = (int32_t)batches.size();
        info->n_launches = 3 * (int32_t)batches.size();
        info->device_bytes = mem.bytes;
        info->upload_ms = upload_ms;
        info->kernel_ms = kernel_ms;
    }
    return RSEM_OK;
}
