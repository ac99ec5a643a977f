// refseq.hip -- FASTA bodies -> bases and segments of bases -> sequences on MI355X (rsem-extract-reference-transcripts,
// rsem-synthesis-reference-transcripts, rsem-preref).  Replaces the getline / check / += loops of
// extractRef.cpp:336-349, synthesisRef.cpp:175-188 and Refs.h:96-102, Transcript::extractSeq (Transcript.h:90-117), the two
// policies' convert and the poly-A append of RefSeq.h:23-28.  The bodies are in refseq_block.hpp.
//
// rsem_refseq_load     k_refseq_count (a wave a tile: kept bytes, first bad byte per record)
//                      hipcub::DeviceScan::ExclusiveSum over the tiles' counts
//                      k_refseq_write (the same masks again, the bytes to their places)
// rsem_refseq_gather   k_refseq_gather (a wave a span of the cumulative length, bisection to its first segment)
// No kernel waits for another workgroup; the only atomic is the minimum over a record's bad bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "refseq_block.hpp"
#include "stage_util.hpp"

using namespace rsem_refseqk;

namespace {

using Buf = rsem::GrowBuf<8>;  // a device buffer that only grows

enum { B_RAW, B_BASES, B_LO, B_HI, B_KEEP, B_BAD, B_BASE, B_END, B_COUNT_T, B_START_T, B_TMP, B_CUM, B_SRC, B_DST, B_FLAGS, B_N };

}  // namespace

struct rsem_refseq {
    int device = 0;
    uint64_t store_bytes = 0, store_pad = 0;
    bool on_device = false;
    void* d_store = nullptr;  // the allocation: store_pad + store_bytes (+ 16)
    rsem::StageQueue q;
    Buf buf[B_N];
    size_t device_bytes = 0;
    // the batch that is resident
    int64_t res_first = 0, res_n = 0;
    std::vector<uint64_t> res_base, res_bases;  // per resident record: where its bases start, how many
    rsem_refseq_info info{};
    std::mutex mu;
};

namespace {

__global__ void __launch_bounds__(kThreads) k_refseq_count(Batch B, uint64_t n_tiles, uint64_t* __restrict__ count, uint64_t* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * 4u + (uint64_t)(RSEM_TIDX >> 6);
    if (t >= n_tiles) return;  // (a whole wave)
    load_count(B, t, RSEM_TIDX & 63, count, bad);
}

__global__ void __launch_bounds__(kThreads) k_refseq_write(Batch B, uint64_t n_tiles, const uint64_t* __restrict__ start, uint8_t* __restrict__ out,
                                                            uint64_t* __restrict__ base, uint64_t* __restrict__ end) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[4][kStage];
    const uint64_t t = (uint64_t)blockIdx.x * 4u + (uint64_t)(RSEM_TIDX >> 6);
    if (t >= n_tiles) return;
    load_write(B, t, RSEM_TIDX & 63, start, out, stage[RSEM_TIDX >> 6], base, end);
}

__global__ void __launch_bounds__(kThreads) k_refseq_gather(Segments S, const uint8_t* __restrict__ bases, uint8_t* __restrict__ store) {
    const uint64_t c0 = ((uint64_t)blockIdx.x * 4u + (uint64_t)(RSEM_TIDX >> 6)) * kSpan;
    gather_span(S, c0, c0 + kSpan, RSEM_TIDX & 63, bases, store);
}

__global__ void k_refseq_loaded() {}

int env_u64(const char* name, uint64_t lo, uint64_t multiple, const char* what, bool* set, uint64_t* v) {
    *set = false;
    const char* e = getenv(name);
    if (!e) return RSEM_OK;
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end || errno || e[0] == '-' || e[0] == '+' || e[0] == ' ' || x < lo || (multiple && x % multiple)) {
        rsem::set_last_error("%s = '%s': %s is expected", name, e, what);
        return RSEM_ERR_INVALID;
    }
    *set = true;
    *v = x;
    return RSEM_OK;
}

int to_device(rsem_refseq* h) {
    RSEM_HIP_TRY(hipSetDevice(h->device));
    if (h->on_device) return RSEM_OK;
    RSEM_HIP_TRY(h->q.create());
    const size_t bytes = (size_t)(h->store_pad + h->store_bytes + 16);
    RSEM_HIP_TRY(hipMalloc(&h->d_store, bytes));
    h->device_bytes += bytes;
    // the runtime loads this translation unit's code object at its first launch (tens of milliseconds): paid here, not inside the first batch's kernel time
    hipLaunchKernelGGL(k_refseq_loaded, dim3(1), dim3(1), 0, h->q.st);
    RSEM_HIP_TRY(hipStreamSynchronize(h->q.st));
    h->on_device = true;
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_refseq_create(rsem_refseq** out, int device, uint64_t store_bytes) {
    RSEM_REQUIRE(out, "rsem_refseq_create: out must not be NULL");
    *out = nullptr;
    RSEM_REQUIRE(device >= 0, "rsem_refseq_create: device must not be negative");
    RSEM_REQUIRE(store_bytes < (1ull << 46), "rsem_refseq_create: a store of 2^46 bytes or more");
    bool set;
    uint64_t pad = 0;
    if (int rc = env_u64("RSEM_REFSEQ_STORE_PAD", 0, 16, "a whole number of bytes, a multiple of 16,", &set, &pad)) return rc;
    RSEM_REQUIRE(pad < (1ull << 40), "RSEM_REFSEQ_STORE_PAD: 2^40 bytes or more");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) {
        rsem::set_last_error("rsem_refseq_create: no device %d", device);
        return RSEM_ERR_NODEVICE;
    }
    rsem_refseq* h = new rsem_refseq();
    h->device = device;
    h->store_bytes = store_bytes;
    h->store_pad = pad;
    h->info.store_pad = pad;
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_refseq_destroy(rsem_refseq* h) {
    if (!h) return;
    if (h->on_device) {
        (void)hipSetDevice(h->device);
        if (h->d_store) (void)hipFree(h->d_store);
        for (Buf& b : h->buf) b.release(h->device_bytes);
        h->q.release();
    }
    delete h;
}

extern "C" int rsem_refseq_load(rsem_refseq* h, int32_t mode, const uint8_t* raw, int64_t n_records, const uint64_t* body_lo, const uint64_t* body_hi,
                                const uint8_t* keep, int64_t first, int64_t* n_taken, uint64_t* n_bases, int64_t* bad) {
    RSEM_REQUIRE(h, "rsem_refseq_load: the handle must not be NULL");
    RSEM_REQUIRE(mode == (int32_t)kModeRaw || mode == (int32_t)kModeChecked, "rsem_refseq_load: mode must be 0 (raw) or 1 (checked)");
    RSEM_REQUIRE(n_records >= 1 && n_records < (1ll << 31), "rsem_refseq_load: 1 to 2^31 - 1 records are expected");
    RSEM_REQUIRE(first >= 0 && first < n_records, "rsem_refseq_load: first must be a record of the call");
    RSEM_REQUIRE(raw && body_lo && body_hi && n_taken && n_bases && bad, "rsem_refseq_load: the arrays must not be NULL");
    uint64_t budget = 0;
    bool set;
    if (int rc = env_u64("RSEM_REFSEQ_BATCH_BYTES", 1, 0, "a whole number from 1 on", &set, &budget)) return rc;  // read at every call
    std::lock_guard<std::mutex> lock(h->mu);
    if (int rc = to_device(h)) return rc;
    if (!set) {  // a quarter of what is free: the raw bytes, the bases and their slack must fit beside what later batches' transcripts need
        size_t fr = 0, tot = 0;
        RSEM_HIP_TRY(hipMemGetInfo(&fr, &tot));
        budget = std::max<uint64_t>((uint64_t)(fr + h->buf[B_RAW].cap + h->buf[B_BASES].cap) / 4, 1u << 20);
    }
    const int64_t last = (int64_t)batch_end(body_lo, body_hi, (uint64_t)n_records, (uint64_t)first, budget);
    const uint32_t n = (uint32_t)(last - first);
    for (int64_t r = first; r < last; r++) {
        if (body_hi[r] < body_lo[r] || (r > first && body_lo[r] < body_hi[r - 1])) {
            rsem::set_last_error("rsem_refseq_load: record %lld: the bodies must ascend and lie apart", (long long)r);
            return RSEM_ERR_INVALID;
        }
    }
    // a record of more than 2^31 - 1 bases is refused before anything is uploaded: its line ends are counted only where its raw length asks for it
    uint64_t kept_raw = 0;
    for (int64_t r = first; r < last; r++) {
        const uint64_t len = body_hi[r] - body_lo[r];
        if (keep && !keep[r]) continue;
        kept_raw += len;
        if (len <= kMaxBases) continue;
        uint64_t nl = 0;
        for (const uint8_t *p = raw + body_lo[r], *e = raw + body_hi[r]; (p = (const uint8_t*)memchr(p, '\n', (size_t)(e - p))) != nullptr; p++) nl++;
        if (len - nl > kMaxBases) {
            rsem::set_last_error("rsem_refseq_load: record %lld has %llu bases: 2^31 - 1 at most (the reference's coordinates are int)", (long long)r,
                                 (unsigned long long)(len - nl));
            return RSEM_ERR_INVALID;
        }
    }
    const uint64_t origin = body_lo[first] & ~15ull, raw_len = body_hi[last - 1] - origin;
    const uint64_t n_tiles = (raw_len + kTile - 1) / kTile;
    RSEM_REQUIRE(n_tiles < (1ull << 31) - 8, "rsem_refseq_load: a batch of 2^43 bytes or more");
    h->res_first = first;
    h->res_n = 0;  // nothing is resident until this load is through
    std::vector<uint64_t> lo(n), hi(n), none(n, kNone);
    std::vector<uint8_t> kp(n);
    for (uint32_t i = 0; i < n; i++) { lo[i] = body_lo[first + i] - origin; hi[i] = body_hi[first + i] - origin; kp[i] = keep ? keep[first + i] != 0 : 1; }

    size_t tmp_bytes = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n_tiles + 1), h->q.st));
    const size_t need[B_TMP + 1] = {(size_t)raw_len + 32, (size_t)kept_raw + 2 * kPad + 16, (size_t)n * 8, (size_t)n * 8, (size_t)n + 8, (size_t)n * 8, (size_t)n * 8,
                                    (size_t)n * 8, (size_t)(n_tiles + 1) * 8, (size_t)(n_tiles + 1) * 8, tmp_bytes};
    for (int b = 0; b <= B_TMP; b++) RSEM_HIP_TRY(h->buf[b].need(need[b], h->device_bytes));
    auto U64 = [&](int b) { return h->buf[b].as<uint64_t>(); };
    hipStream_t st = h->q.st;
    RSEM_HIP_TRY(h->q.upload_begin());
    if (raw_len) RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_RAW].p, raw + origin, (size_t)raw_len, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_LO), lo.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_HI), hi.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_KEEP].p, kp.data(), (size_t)n, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U64(B_BAD), none.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(U64(B_BASE), 0, (size_t)n * 8, st));
    RSEM_HIP_TRY(hipMemsetAsync(U64(B_END), 0, (size_t)n * 8, st));
    RSEM_HIP_TRY(hipMemsetAsync(U64(B_COUNT_T) + n_tiles, 0, 8, st));
    RSEM_HIP_TRY(h->q.upload_end());
    const Batch B{h->buf[B_RAW].as<uint8_t>(), raw_len, n, U64(B_LO), U64(B_HI), h->buf[B_KEEP].as<uint8_t>(), (uint32_t)mode};
    uint8_t* bases = h->buf[B_BASES].as<uint8_t>() + kPad;
    std::vector<uint64_t> base(n), end(n), bd(n);
    uint64_t total = 0;
    if (n_tiles) {
        const uint32_t blocks = (uint32_t)((n_tiles + 3) / 4);
        hipLaunchKernelGGL(k_refseq_count, dim3(blocks), dim3(kThreads), 0, st, B, n_tiles, U64(B_COUNT_T), U64(B_BAD));
        size_t tb = h->buf[B_TMP].cap;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U64(B_COUNT_T), U64(B_START_T), (int)(n_tiles + 1), st));
        // the bases must fit what was allocated for them before a byte of them is written
        RSEM_HIP_TRY(hipMemcpyAsync(&total, U64(B_START_T) + n_tiles, 8, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        if (total > kept_raw) {
            rsem::set_last_error("rsem_refseq_load: %llu bases on the device, %llu at most were expected", (unsigned long long)total, (unsigned long long)kept_raw);
            return RSEM_ERR_STATE;
        }
        hipLaunchKernelGGL(k_refseq_write, dim3(blocks), dim3(kThreads), 0, st, B, n_tiles, U64(B_START_T), bases, U64(B_BASE), U64(B_END));
        h->info.n_launches += 3;
    }
    RSEM_HIP_TRY(h->q.kernels_end());
    RSEM_HIP_TRY(hipMemcpyAsync(base.data(), U64(B_BASE), (size_t)n * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(end.data(), U64(B_END), (size_t)n * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(bd.data(), U64(B_BAD), (size_t)n * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    h->res_base.assign(n, 0);
    h->res_bases.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (end[i] < base[i] || end[i] > total) {
            rsem::set_last_error("rsem_refseq_load: record %lld: bases %llu .. %llu of %llu", (long long)(first + i), (unsigned long long)base[i],
                                 (unsigned long long)end[i], (unsigned long long)total);
            return RSEM_ERR_STATE;
        }
        h->res_base[i] = base[i];
        h->res_bases[i] = n_bases[first + i] = end[i] - base[i];
        bad[first + i] = bd[i] == kNone ? -1 : (int64_t)(bd[i] + origin);
        if (n_bases[first + i] > kMaxBases) {
            rsem::set_last_error("rsem_refseq_load: record %lld has %llu bases: 2^31 - 1 at most", (long long)(first + i), (unsigned long long)n_bases[first + i]);
            return RSEM_ERR_INVALID;
        }
    }
    h->res_n = n;
    *n_taken = n;
    if (int rc = h->q.add_laps(h->info.upload_ms, h->info.kernel_ms)) return rc;
    h->info.n_batches += 1;
    h->info.n_records += n;
    h->info.raw_bytes += raw_len;
    h->info.n_bases += total;
    h->info.batch_bytes = budget;
    h->info.device_bytes = h->device_bytes;
    return RSEM_OK;
}

extern "C" int rsem_refseq_gather(rsem_refseq* h, int64_t n_segments, const int64_t* src, const uint32_t* first_base, const uint32_t* len, const uint64_t* dst,
                                  const uint32_t* flags) {
    RSEM_REQUIRE(h, "rsem_refseq_gather: the handle must not be NULL");
    RSEM_REQUIRE(n_segments >= 0 && n_segments < (1ll << 40), "rsem_refseq_gather: 0 to 2^40 - 1 segments are expected");
    if (n_segments == 0) return RSEM_OK;
    RSEM_REQUIRE(src && first_base && len && dst && flags, "rsem_refseq_gather: the arrays must not be NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    const size_t n = (size_t)n_segments;
    std::vector<uint64_t> cum(n + 1), sa(n);
    cum[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (flags[i] & ~(uint32_t)kFlagAll) { rsem::set_last_error("rsem_refseq_gather: segment %zu: flags %u", i, flags[i]); return RSEM_ERR_INVALID; }
        if (len[i] < 1 || len[i] > kMaxBases) { rsem::set_last_error("rsem_refseq_gather: segment %zu: 1 to 2^31 - 1 bases are expected", i); return RSEM_ERR_INVALID; }
        if (dst[i] > h->store_bytes || len[i] > h->store_bytes - dst[i]) {
            rsem::set_last_error("rsem_refseq_gather: segment %zu: bytes %llu + %u of a store of %llu", i, (unsigned long long)dst[i], len[i], (unsigned long long)h->store_bytes);
            return RSEM_ERR_INVALID;
        }
        if (i && dst[i] < dst[i - 1] + len[i - 1]) {  // one writer a byte: the segments ascend in the store and lie apart
            rsem::set_last_error("rsem_refseq_gather: segment %zu: the destinations must ascend and lie apart", i);
            return RSEM_ERR_INVALID;
        }
        if (flags[i] & kFlagFill) sa[i] = 0;
        else {
            const int64_t r = src[i] - h->res_first;
            if (r < 0 || r >= h->res_n) { rsem::set_last_error("rsem_refseq_gather: segment %zu: record %lld is not loaded", i, (long long)src[i]); return RSEM_ERR_INVALID; }
            if ((uint64_t)first_base[i] + len[i] > h->res_bases[(size_t)r]) {
                rsem::set_last_error("rsem_refseq_gather: segment %zu: bases %u + %u of record %lld, which has %llu", i, first_base[i], len[i], (long long)src[i],
                                     (unsigned long long)h->res_bases[(size_t)r]);
                return RSEM_ERR_INVALID;
            }
            sa[i] = h->res_base[(size_t)r] + first_base[i];
        }
        cum[i + 1] = cum[i] + len[i];
    }
    if (int rc = to_device(h)) return rc;
    const size_t need[4] = {(n + 1) * 8, n * 8, n * 8, n * 4};
    for (int b = 0; b < 4; b++) RSEM_HIP_TRY(h->buf[B_CUM + b].need(need[b], h->device_bytes));
    RSEM_HIP_TRY(h->buf[B_BASES].need(2 * kPad + 16, h->device_bytes));  // (fills alone: no load came before)
    hipStream_t st = h->q.st;
    RSEM_HIP_TRY(h->q.upload_begin());
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_CUM].p, cum.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_SRC].p, sa.data(), n * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_DST].p, dst, n * 8, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(h->buf[B_FLAGS].p, flags, n * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(h->q.upload_end());
    const Segments S{(uint64_t)n, h->buf[B_CUM].as<uint64_t>(), h->buf[B_SRC].as<uint64_t>(), h->buf[B_DST].as<uint64_t>(), h->buf[B_FLAGS].as<uint32_t>()};
    const uint64_t blocks = (cum[n] + kGroupSpan - 1) / kGroupSpan;
    RSEM_REQUIRE(blocks < (1ull << 31), "rsem_refseq_gather: 2^45 bytes or more in one call");
    hipLaunchKernelGGL(k_refseq_gather, dim3((uint32_t)blocks), dim3(kThreads), 0, st, S, h->buf[B_BASES].as<uint8_t>() + kPad, (uint8_t*)h->d_store + h->store_pad);
    RSEM_HIP_TRY(h->q.kernels_end());
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (int rc = h->q.add_laps(h->info.upload_ms, h->info.kernel_ms)) return rc;
    h->info.n_launches += 1;
    h->info.n_segments += n;
    h->info.gathered_bytes += cum[n];
    h->info.device_bytes = h->device_bytes;
    return RSEM_OK;
}

extern "C" int rsem_refseq_download(rsem_refseq* h, uint64_t offset, uint64_t bytes, uint8_t* out) {
    RSEM_REQUIRE(h, "rsem_refseq_download: the handle must not be NULL");
    RSEM_REQUIRE(offset <= h->store_bytes && bytes <= h->store_bytes - offset, "rsem_refseq_download: outside the store");
    if (bytes == 0) return RSEM_OK;
    RSEM_REQUIRE(out, "rsem_refseq_download: out must not be NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    if (int rc = to_device(h)) return rc;
    RSEM_HIP_TRY(h->q.upload_begin());  // (the first lap, around a copy the other way)
    RSEM_HIP_TRY(hipMemcpyAsync(out, (const uint8_t*)h->d_store + h->store_pad + offset, (size_t)bytes, hipMemcpyDeviceToHost, h->q.st));
    RSEM_HIP_TRY(h->q.upload_end());
    RSEM_HIP_TRY(hipStreamSynchronize(h->q.st));
    return h->q.add_upload_lap(h->info.download_ms);
}

extern "C" int rsem_refseq_get_info(rsem_refseq* h, rsem_refseq_info* info) {
    RSEM_REQUIRE(h && info, "rsem_refseq_get_info: the handle and info must not be NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    *info = h->info;
    return RSEM_OK;
}
