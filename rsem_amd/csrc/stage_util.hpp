// stage_util.hpp -- the host-side scaffolding the batch stages share (kmer, depth, gmap, refseq, alncheck, pairscan, simulate, ci,
// gibbs_diag): device memory that is released on every path, buffers that grow, a stream with the three
// events around a batch's upload and its kernels, the whole-number knobs.  Nothing here launches a kernel.
#pragma once
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <vector>

#include "common.hpp"

namespace rsem {

struct DevMem {  // frees what it owns on scope exit
    std::vector<void*> ptrs;
    size_t bytes = 0;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t alloc(T** p, size_t n) {
        const size_t b = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = hipMalloc((void**)p, b);
        if (e == hipSuccess) { ptrs.push_back(*p); bytes += b; }
        return e;
    }
};
struct EventGuard {  // events / streams released on every exit path
    hipEvent_t e = nullptr;
    ~EventGuard() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
};
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreate(&s); }
};

// A device buffer that only grows, by bytes / SlackDiv + 256 more than is asked; total: the owner's count of device bytes.
// keep = 0 (scratch): the old block is freed first, and on failure the buffer is empty.  keep > 0 (resident arrays): the first keep
// bytes move to the new block before the old one is freed, and on failure nothing has changed.
template <unsigned SlackDiv>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t bytes, size_t& total, size_t keep = 0) {
        if (bytes <= cap) return hipSuccess;
        const size_t want = bytes + bytes / SlackDiv + 256;
        const bool carry = keep && p;
        if (!carry) release(total);
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;  // (carry: what was there is still there)
        if (carry) {
            e = hipMemcpy(q, p, keep, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { (void)hipFree(q); return e; }
            release(total);
        }
        p = q; cap = want; total += want;
        return hipSuccess;
    }
    void release(size_t& total) {
        if (p) { (void)hipFree(p); total -= cap; }
        p = nullptr; cap = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

// A stage's stream and the events ea, eb, ec: the upload of a batch lies between the first two, its kernels between the last two.
struct StageQueue {
    hipStream_t st = nullptr;
    hipEvent_t ea = nullptr, eb = nullptr, ec = nullptr;
    StageQueue() = default;
    StageQueue(const StageQueue&) = delete;
    StageQueue& operator=(const StageQueue&) = delete;
    ~StageQueue() { release(); }
    hipError_t create() {
        hipError_t e = hipStreamCreate(&st);
        for (hipEvent_t* ev : {&ea, &eb, &ec})
            if (e == hipSuccess) e = hipEventCreate(ev);
        return e;
    }
    void release() {  // (on the device that create() ran on)
        for (hipEvent_t* ev : {&ea, &eb, &ec}) {
            if (*ev) (void)hipEventDestroy(*ev);
            *ev = nullptr;
        }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
    hipError_t upload_begin() { return hipEventRecord(ea, st); }
    hipError_t upload_end() { return hipEventRecord(eb, st); }
    hipError_t kernels_end() { return hipEventRecord(ec, st); }
    // once the stream has passed the events: the milliseconds between them, added
    int add_upload_lap(double& upload_ms) {
        float ms = 0;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, ea, eb));
        upload_ms += ms;
        return RSEM_OK;
    }
    int add_laps(double& upload_ms, double& kernel_ms) {
        if (int rc = add_upload_lap(upload_ms)) return rc;
        float ms = 0;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, eb, ec));
        kernel_ms += ms;
        return RSEM_OK;
    }
};

// A knob that holds a whole number from lo to hi, read when it is called.  Unset: *value stays as it is.  Anything but such a
// number is an error, not silently the default -- a value strtoll clamps to the ends of long long (ERANGE) too.
inline int env_whole(const char* name, long long lo, long long hi, uint64_t* value) {
    const char* e = getenv(name);
    if (!e) return RSEM_OK;
    char* end = nullptr;
    errno = 0;
    const long long v = strtoll(e, &end, 10);
    if (end == e || *end || errno == ERANGE || v < lo || v > hi) {
        if (hi == LLONG_MAX) set_last_error("%s = '%s': a whole number from %lld on is expected", name, e, lo);
        else set_last_error("%s = '%s': a whole number from %lld to %lld is expected", name, e, lo, hi);
        return RSEM_ERR_INVALID;
    }
    *value = (uint64_t)v;
    return RSEM_OK;
}

}  // namespace rsem
