// ci.hip -- credibility intervals on MI355X (rsem-calculate-credibility-intervals).
//
// Reference: calcCI.cpp.  Phase I (sample_theta_from_c, :93-164): for each of nCV Gibbs count vectors, nSpC draws
// theta ~ Dirichlet(c + pseudoC) (independent gammas / mw), TPM as float + the mean effective length l_bar of the
// draw, transposed through a temporary file (Buffer.h) into M rows of nSamples floats.  Phase II (calcCI_batch,
// :286-388): per transcript sort the row, shortest interval with >= confidence mass + coefficient of quartile
// variation (calcCI, :216-284), for TPM and for FPKM = 1e3 / l_bar[k] * TPM[k]; per gene (and, allele-specific,
// per transcript) the same on the float sums of its members' rows.
//
// Here the M x nSamples matrix lives in HBM (C2: 50 k x 50 k floats = 10 GB of 288 GB), is produced directly in
// row-per-transcript order and never touches a file:
//   k_ci_draw       lane = sample, loop over a chunk of transcripts: y = Gamma(c_j + pseudoC) / (mw_j eel_j) as float
//                   into Y[j][s] (coalesced along s), per-sample normaliser T_s and sum(y eel) accumulated in
//                   registers, two double atomics per lane per chunk.  (theta's own normaliser cancels in TPM.)
//   k_ci_keys_*     rows (or float sums of member rows) scaled to TPM / FPKM into a key batch
//   hipcub segmented radix sort of the batch (one segment per row)
//   k_ci_intervals  one thread per sorted row runs the reference's two-pointer scan verbatim (ties included)
// RNG: Philox4x32-10 counters (seed, sample, transcript) -- a different stream than the reference's per-thread
// MT19937 + boost gamma (whose output depends on -p); the interval stage is bit-identical given the same row.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "rng.hpp"
#include "stage_util.hpp"

namespace {

using rsem::kEpsilon;
using rsem::DevMem;
using rsem::EventGuard;
using rsem::Philox;
using rsem::StreamGuard;

constexpr int kBlock = 256;
constexpr uint32_t kDrawTag = 0x43495331u;  // 'CIS1'

// y[j][s] for transcripts j in this block's chunk, samples s = lane
__global__ void __launch_bounds__(64) k_ci_draw(int32_t M, int32_t nS, int32_t nSpC, int32_t chunk, const int32_t* __restrict__ cvecs,
                                                  const double* __restrict__ w, const double* __restrict__ eel, double pseudoC,
                                                  Philox ph, float* __restrict__ Y, double* __restrict__ T, double* __restrict__ L) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nS) return;
    const int j0 = 1 + blockIdx.y * chunk, j1 = min(M + 1, j0 + chunk);
    const int32_t* cv = cvecs + (size_t)(s / nSpC) * (size_t)(M + 1);
    double t = 0.0, l = 0.0;
    for (int j = j0; j < j1; j++) {
        const double wj = w[j];
        const int c = cv[j];
        float y = 0.0f;
        if (wj > 0.0 && c >= 0) y = (float)(rsem::gamma_draw_bulk(ph, (uint32_t)s, (uint32_t)j, kDrawTag, (double)c + pseudoC) * wj);
        Y[(size_t)(j - 1) * nS + s] = y;
        t += (double)y;
        l += (double)y * eel[j];
    }
    atomicAdd(T + s, t);
    atomicAdd(L + s, l);
}

// sc[s] = 1e6 / T_s ; lbar[s] = (float)(L_s / T_s)   (calcCI.cpp:143-148)
// A draw whose normaliser is below EPSILON (every transcript with weight drew zero) has no TPM: the reference stops at
// assert(sum >= EPSILON) (calcCI.cpp:143); here the flag makes the call fail instead of letting 1e3 / 0 * 0 = NaN rows through.
__global__ void k_ci_scales(int32_t nS, const double* __restrict__ T, const double* __restrict__ L, double* sc, float* lbar, int* bad) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nS) return;
    const double t = T[s];
    if (!(t >= kEpsilon)) *bad = 1;
    sc[s] = t >= kEpsilon ? 1e6 / t : 0.0;
    lbar[s] = t >= kEpsilon ? (float)(L[s] / t) : 0.0f;
}

__device__ inline float tpm_of(float y, double sc) { return (float)((double)y * sc); }
__device__ inline float fpkm_of(float tpm, float lbar) { return (float)(1e3 / (double)lbar * (double)tpm); }  // calcCI.cpp:345

// keys[r][s] = TPM or FPKM sample s of row row0 + r
__global__ void k_ci_keys_rows(int32_t nS, const float* __restrict__ Y, const double* __restrict__ sc, const float* __restrict__ lbar,
                               int64_t row0, int64_t nrows, bool fpkm, float* __restrict__ keys) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * nS) return;
    const size_t r = (size_t)(idx / nS);
    const int s = (int)(idx - (int64_t)r * nS);
    float v = tpm_of(Y[(size_t)(row0 + r) * nS + s], sc[s]);
    if (fpkm) v = fpkm_of(v, lbar[s]);
    keys[r * nS + s] = v;
}

// keys[g][s] = float sum over the group's member rows, in order (calcCI.cpp:346-351)
__global__ void k_ci_keys_groups(int32_t nS, const float* __restrict__ Y, const double* __restrict__ sc, const float* __restrict__ lbar,
                                 const int32_t* __restrict__ gb, const int32_t* __restrict__ ge, int64_t ngroups, bool fpkm,
                                 float* __restrict__ keys) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ngroups * nS) return;
    const size_t g = (size_t)(idx / nS);
    const int s = (int)(idx - (int64_t)g * nS);
    const double scs = sc[s];
    const float lb = lbar[s];
    float acc = 0.0f;
    for (int j = gb[g]; j < ge[g]; j++) {  // member rows are sids gb..ge-1, stored at row sid-1
        float v = tpm_of(Y[(size_t)(j - 1) * nS + s], scs);
        if (fpkm) v = fpkm_of(v, lb);
        acc += v;
    }
    keys[g * nS + s] = acc;
}

// plain rows (tests / the sampling-only entry point): tpm[j][s] in place of y
__global__ void k_ci_finish_rows(int32_t nS, int64_t nrows, float* __restrict__ Y, const double* __restrict__ sc) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * nS) return;
    const size_t r = (size_t)(idx / nS);
    const int s = (int)(idx - (int64_t)r * nS);
    Y[r * nS + s] = tpm_of(Y[r * nS + s], sc[s]);
}

// Interval + quartile statistics of one sorted row; one thread per row.  Same results as calcCI (calcCI.cpp:216-284),
// written around runs of equal values: with t = the number of samples allowed outside, start from the lowest upper
// end (always the LAST index of a run) that leaves <= t samples above it, then slide the lower end up run by run,
// re-extending the upper end by whole runs whenever more than t samples fall outside; the first strictly shortest
// [x[lo], x[hi]] wins.  Quartiles are Tukey's hinges.
__device__ inline int run_last(const float* x, int n, int i) {   // last index of the run of equal values containing i
    while (i < n - 1 && x[i + 1] == x[i]) ++i;
    return i;
}
__device__ inline int run_first(const float* x, int i) {         // first index of that run
    while (i > 0 && x[i - 1] == x[i]) --i;
    return i;
}

__global__ void k_ci_intervals(int64_t nrows, int32_t n, const float* __restrict__ sorted, double confidence,
                               float* __restrict__ lb_out, float* __restrict__ ub_out, float* __restrict__ cqv_out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const float* x = sorted + (size_t)r * n;
    const int allowed = n - ((int)(confidence * n - 1e-8) + 1);  // samples that may lie outside the interval

    // upper end: walk down over whole runs while the samples above still fit into `allowed`
    int hi = n - 1;
    for (;;) {
        const int below = run_first(x, hi) - 1;  // last index of the next lower run, -1 if none
        if (below < 0 || n - 1 - below > allowed) break;
        hi = below;
    }
    int outside = n - 1 - hi;

    float best_lo = -1e30f, best_hi = 1e30f;
    for (int lo = 0; lo <= allowed;) {
        if (x[hi] - x[lo] < best_hi - best_lo) { best_lo = x[lo]; best_hi = x[hi]; }
        const int next = run_last(x, n, lo) + 1;  // first index of the next higher run
        if (next <= allowed) {
            outside += next - lo;
            while (outside > allowed && hi < n - 1) {  // take back whole runs at the top
                const int up = run_last(x, n, hi + 1);
                outside -= up - hi;
                hi = up;
            }
        }
        lo = next;
    }

    const int q = n / 4, rem = n % 4;
    float q1, q3;
    if (rem == 0) {
        q1 = (float)((double)(x[q - 1] + x[q]) / 2.0);  // float add, then halved in double, as the reference
        q3 = (float)((double)(x[3 * q - 1] + x[3 * q]) / 2.0);
    } else if (rem == 3) {
        q1 = (float)((double)(x[q] + x[q + 1]) / 2.0);
        q3 = (float)((double)(x[3 * q + 1] + x[3 * q + 2]) / 2.0);
    } else {
        q1 = x[q];
        q3 = x[3 * q];
    }
    lb_out[r] = best_lo;
    ub_out[r] = best_hi;
    cqv_out[r] = (q3 - q1 > 0.0f) ? (q3 - q1) / (q3 + q1) : 0.0f;  // float division
}

__global__ void k_ci_offsets(int64_t n, int32_t nS, int* off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) off[i] = (int)(i * nS);
}

// sorts `nrows` rows held in d_keys (device, nrows x nS) and writes their intervals to the host arrays at [out0 ...)
struct RowSorter {
    int32_t nS = 0;
    int64_t cap_rows = 0;
    float* d_sorted = nullptr;
    int* d_off = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    float *d_lb = nullptr, *d_ub = nullptr, *d_cqv = nullptr;
    DevMem mem;
    hipStream_t st = nullptr;
    double sort_ms = 0.0, interval_ms = 0.0;
    uint64_t n_keys = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;

    int init(int32_t nSamples, int64_t rows, hipStream_t stream) {
        nS = nSamples; cap_rows = rows; st = stream;
        RSEM_HIP_TRY(mem.alloc(&d_sorted, (size_t)rows * nS));
        RSEM_HIP_TRY(mem.alloc(&d_off, (size_t)rows + 1));
        RSEM_HIP_TRY(mem.alloc(&d_lb, (size_t)rows));
        RSEM_HIP_TRY(mem.alloc(&d_ub, (size_t)rows));
        RSEM_HIP_TRY(mem.alloc(&d_cqv, (size_t)rows));
        hipLaunchKernelGGL(k_ci_offsets, dim3(rsem::ceil_div(rows + 1, kBlock)), dim3(kBlock), 0, st, rows, nS, d_off);
        RSEM_HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tmp_bytes, (const float*)nullptr, d_sorted, (int)(rows * nS),
                                                               (int)rows, d_off, d_off + 1, 0, 32, st));
        RSEM_HIP_TRY(mem.alloc((char**)&d_tmp, tmp_bytes));
        RSEM_HIP_TRY(hipEventCreate(&e0)); RSEM_HIP_TRY(hipEventCreate(&e1)); RSEM_HIP_TRY(hipEventCreate(&e2));
        return RSEM_OK;
    }
    ~RowSorter() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (e2) (void)hipEventDestroy(e2);
    }
    int run(const float* d_keys, int64_t nrows, double confidence, float* lb, float* ub, float* cqv) {
        if (nrows == 0) return RSEM_OK;
        RSEM_HIP_TRY(hipEventRecord(e0, st));
        RSEM_HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(d_tmp, tmp_bytes, d_keys, d_sorted, (int)(nrows * nS), (int)nrows, d_off,
                                                               d_off + 1, 0, 32, st));
        RSEM_HIP_TRY(hipEventRecord(e1, st));
        hipLaunchKernelGGL(k_ci_intervals, dim3(rsem::ceil_div(nrows, 64)), dim3(64), 0, st, nrows, nS, d_sorted, confidence, d_lb, d_ub,
                           d_cqv);
        RSEM_HIP_TRY(hipEventRecord(e2, st));
        RSEM_HIP_TRY(hipMemcpyAsync(lb, d_lb, sizeof(float) * nrows, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(ub, d_ub, sizeof(float) * nrows, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(cqv, d_cqv, sizeof(float) * nrows, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        float a = 0, b = 0;
        RSEM_HIP_TRY(hipEventElapsedTime(&a, e0, e1));
        RSEM_HIP_TRY(hipEventElapsedTime(&b, e1, e2));
        sort_ms += a; interval_ms += b;
        n_keys += (uint64_t)nrows * nS;
        return RSEM_OK;
    }
};

// R = rows per batch of the segmented sort: int offsets, 4 GB of keys.  RSEM_CI_BATCH_KEYS (test knob, read at every call): the
// most keys a batch may hold instead of 2^30, a whole number from nS to 2^30 -- anything else is an error, not silently the default.
int batch_rows(int32_t nS, int64_t total, int64_t& R) {
    int64_t keys = (int64_t)1 << 30;
    if (const char* e = getenv("RSEM_CI_BATCH_KEYS")) {
        char* end = nullptr;
        const unsigned long long v = (e[0] >= '0' && e[0] <= '9') ? strtoull(e, &end, 10) : 0;
        RSEM_REQUIRE(end && end != e && *end == '\0' && end - e <= 10 && v >= (unsigned long long)nS && v <= (1ull << 30),
                     "RSEM_CI_BATCH_KEYS must be a whole number from nSamples to 2^30 (1073741824)");
        keys = (int64_t)v;
    }
    const int64_t cap = std::max<int64_t>(1, keys / nS);
    R = std::max<int64_t>(1, std::min(total, cap));
    return RSEM_OK;
}

struct Sampler {  // Y (M x nS, unnormalised), scale and l_bar per sample, on the device
    DevMem mem;
    float* d_Y = nullptr;
    double* d_sc = nullptr;
    float* d_lbar = nullptr;
    double sample_ms = 0.0;
    int run(int32_t M, int32_t nCV, int32_t nSpC, const int32_t* cvecs, const double* eel, const double* mw, double pseudoC,
            uint64_t seed, hipStream_t st) {
        const int32_t nS = nCV * nSpC;
        std::vector<double> w((size_t)M + 1, 0.0);
        for (int j = 1; j <= M; j++)
            if (eel[j] >= kEpsilon && mw[j] >= kEpsilon) w[j] = 1.0 / (mw[j] * eel[j]);  // calcCI.cpp:131,137-141
        int32_t* d_cv; double *d_w, *d_eel, *d_T, *d_L;
        int* d_bad;
        RSEM_HIP_TRY(mem.alloc(&d_bad, 1));
        RSEM_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), st));
        RSEM_HIP_TRY(mem.alloc(&d_Y, (size_t)M * nS));
        RSEM_HIP_TRY(mem.alloc(&d_sc, (size_t)nS));
        RSEM_HIP_TRY(mem.alloc(&d_lbar, (size_t)nS));
        RSEM_HIP_TRY(mem.alloc(&d_cv, (size_t)nCV * (M + 1)));
        RSEM_HIP_TRY(mem.alloc(&d_w, (size_t)M + 1));
        RSEM_HIP_TRY(mem.alloc(&d_eel, (size_t)M + 1));
        RSEM_HIP_TRY(mem.alloc(&d_T, (size_t)nS));
        RSEM_HIP_TRY(mem.alloc(&d_L, (size_t)nS));
        RSEM_HIP_TRY(hipMemcpyAsync(d_cv, cvecs, sizeof(int32_t) * (size_t)nCV * (M + 1), hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_w, w.data(), sizeof(double) * ((size_t)M + 1), hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(d_eel, eel, sizeof(double) * ((size_t)M + 1), hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemsetAsync(d_T, 0, sizeof(double) * nS, st));
        RSEM_HIP_TRY(hipMemsetAsync(d_L, 0, sizeof(double) * nS, st));
        EventGuard g0, g1;
        RSEM_HIP_TRY(g0.create()); RSEM_HIP_TRY(g1.create());
        hipEvent_t e0 = g0.e, e1 = g1.e;
        RSEM_HIP_TRY(hipEventRecord(e0, st));
        // enough (sample block, transcript chunk) waves to fill 256 CUs several times over
        const int sblocks = rsem::ceil_div(nS, 64);
        int nchunks = std::max(1, std::min<int>(M, (256 * 4 * 8 + sblocks - 1) / sblocks));
        const int chunk = (M + nchunks - 1) / nchunks;
        nchunks = (M + chunk - 1) / chunk;
        Philox ph{(uint32_t)seed, (uint32_t)(seed >> 32) ^ 0x52534349u};  // 'RSCI'
        hipLaunchKernelGGL(k_ci_draw, dim3(sblocks, nchunks), dim3(64), 0, st, M, nS, nSpC, chunk, d_cv, d_w, d_eel, pseudoC, ph, d_Y,
                           d_T, d_L);
        hipLaunchKernelGGL(k_ci_scales, dim3(rsem::ceil_div(nS, kBlock)), dim3(kBlock), 0, st, nS, d_T, d_L, d_sc, d_lbar, d_bad);
        RSEM_HIP_TRY(hipEventRecord(e1, st));
        int h_bad = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        float ms = 0;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        sample_ms = ms;
        if (h_bad) {
            rsem::set_last_error("a sampled expression vector sums to less than EPSILON (no transcript with weight and effective length): no TPM can be formed");
            return RSEM_ERR_INVALID;
        }
        return RSEM_OK;
    }
};

int check_common(int32_t M, int32_t nCV, int32_t nSpC) {
    RSEM_REQUIRE(M > 0 && nCV > 0 && nSpC > 0, "M, nCV and nSpC must be positive");
    RSEM_REQUIRE((int64_t)nCV * nSpC < ((int64_t)1 << 30), "nCV * nSpC too large");
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_ci_intervals(int device, int64_t nrows, int32_t nSamples, const float* rows, double confidence, float* lb,
                                 float* ub, float* cqv) {
    RSEM_REQUIRE(nrows >= 0 && nSamples > 0 && rows && lb && ub && cqv, "bad arguments");
    RSEM_REQUIRE(confidence > 0.0 && confidence <= 1.0, "confidence must be in (0, 1]");
    int64_t R = 0;
    int rc = batch_rows(nSamples, std::max<int64_t>(nrows, 1), R);
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(hipSetDevice(device));
    StreamGuard sg;
    RSEM_HIP_TRY(sg.create());
    hipStream_t st = sg.s;
    {
        RowSorter sorter;
        DevMem mem;
        float* d_keys = nullptr;
        rc = sorter.init(nSamples, R, st);
        if (rc == RSEM_OK && mem.alloc(&d_keys, (size_t)R * nSamples) != hipSuccess) { rsem::set_last_error("out of device memory"); rc = RSEM_ERR_NOMEM; }
        for (int64_t r0 = 0; rc == RSEM_OK && r0 < nrows; r0 += R) {
            const int64_t n = std::min(R, nrows - r0);
            if (hipMemcpyAsync(d_keys, rows + (size_t)r0 * nSamples, sizeof(float) * (size_t)n * nSamples, hipMemcpyHostToDevice, st) != hipSuccess) {
                rsem::set_last_error("upload failed"); rc = RSEM_ERR_HIP; break;
            }
            rc = sorter.run(d_keys, n, confidence, lb + r0, ub + r0, cqv + r0);
        }
    }
    return rc;
}

extern "C" int rsem_ci_sample(int device, int32_t M, int32_t nCV, int32_t nSpC, const int32_t* cvecs, const double* eel,
                              const double* mw, double pseudoC, uint64_t seed, float* tpm_samples, float* l_bars) {
    int rc = check_common(M, nCV, nSpC);
    if (rc != RSEM_OK) return rc;
    RSEM_REQUIRE(cvecs && eel && mw && tpm_samples && l_bars, "null argument");
    RSEM_HIP_TRY(hipSetDevice(device));
    StreamGuard sg;
    RSEM_HIP_TRY(sg.create());
    hipStream_t st = sg.s;
    const int32_t nS = nCV * nSpC;
    {
        Sampler S;
        rc = S.run(M, nCV, nSpC, cvecs, eel, mw, pseudoC, seed, st);
        if (rc == RSEM_OK) {
            hipLaunchKernelGGL(k_ci_finish_rows, dim3(rsem::ceil_div((uint64_t)M * nS, kBlock)), dim3(kBlock), 0, st, nS, (int64_t)M, S.d_Y, S.d_sc);
            if (hipMemcpyAsync(tpm_samples, S.d_Y, sizeof(float) * (size_t)M * nS, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(l_bars, S.d_lbar, sizeof(float) * nS, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) {
                rsem::set_last_error("download failed"); rc = RSEM_ERR_HIP;
            }
        }
    }
    return rc;
}

namespace {

// Everything behind the sampling stage (calcCI.cpp:286-388): per transcript, per gene and -- for an allele-specific reference --
// per transcript over its alleles: sort the row's samples, shortest interval, quartile statistics; TPM and FPKM.  S holds the
// samples on the device (Y: M x nS; TPM of sample s = (float)(Y * sc[s])).
int ci_after_sampling(Sampler& S, int32_t M, int32_t nS, double confidence, int32_t m, const int32_t* gene_starts, int32_t m_trans,
                      const int32_t* trans_starts, float* tpm_ci, float* fpkm_ci, float* gene_tpm_ci, float* gene_fpkm_ci, float* iso_tpm_ci,
                      float* iso_fpkm_ci, hipStream_t st, RowSorter& sorter) {
    const bool allele = trans_starts != nullptr;
    DevMem mem;
    float* d_keys = nullptr;
    int32_t *d_gb = nullptr, *d_ge = nullptr;
    int64_t R = 0;
    int rc = batch_rows(nS, M, R);
    if (rc != RSEM_OK) return rc;
    rc = sorter.init(nS, R, st);
    if (rc == RSEM_OK && (mem.alloc(&d_keys, (size_t)R * nS) != hipSuccess || mem.alloc(&d_gb, (size_t)R) != hipSuccess ||
                          mem.alloc(&d_ge, (size_t)R) != hipSuccess)) {
        rsem::set_last_error("out of device memory"); rc = RSEM_ERR_NOMEM;
    }
    // per transcript (calcCI.cpp:343-354)
    for (int pass = 0; rc == RSEM_OK && pass < 2; pass++) {
        float* out = pass ? fpkm_ci : tpm_ci;
        for (int64_t r0 = 0; rc == RSEM_OK && r0 < M; r0 += R) {
            const int64_t n = std::min<int64_t>(R, M - r0);
            hipLaunchKernelGGL(k_ci_keys_rows, dim3(rsem::ceil_div((uint64_t)n * nS, kBlock)), dim3(kBlock), 0, st, nS, S.d_Y, S.d_sc,
                               S.d_lbar, r0, n, pass == 1, d_keys);
            rc = sorter.run(d_keys, n, confidence, out + r0, out + (size_t)M + r0, out + 2 * (size_t)M + r0);
        }
    }
    // groups: genes, and transcripts of an allele-specific reference.  Single-member groups copy their member's
    // interval (calcCI.cpp:356-363, 330-337); the others sort the float sums of their members' rows.
    auto groups = [&](int32_t ng, const int32_t* starts, float* out_t, float* out_f) -> int {
        std::vector<int32_t> multi;
        for (int g = 0; g < ng; g++) {
            const int b = starts[g], e = starts[g + 1];
            if (e - b > 1) multi.push_back(g);
            else if (e - b == 1)
                for (int k = 0; k < 3; k++) {
                    out_t[(size_t)k * ng + g] = tpm_ci[(size_t)k * M + b - 1];
                    out_f[(size_t)k * ng + g] = fpkm_ci[(size_t)k * M + b - 1];
                }
            else
                for (int k = 0; k < 3; k++) out_t[(size_t)k * ng + g] = out_f[(size_t)k * ng + g] = 0.0f;
        }
        std::vector<int32_t> gb, ge;
        std::vector<float> lb, ub, cq;
        for (size_t i0 = 0; i0 < multi.size(); i0 += (size_t)R) {
            const size_t n = std::min<size_t>((size_t)R, multi.size() - i0);
            gb.resize(n); ge.resize(n); lb.resize(n); ub.resize(n); cq.resize(n);
            for (size_t i = 0; i < n; i++) { gb[i] = starts[multi[i0 + i]]; ge[i] = starts[multi[i0 + i] + 1]; }
            RSEM_HIP_TRY(hipMemcpyAsync(d_gb, gb.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
            RSEM_HIP_TRY(hipMemcpyAsync(d_ge, ge.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
            for (int pass = 0; pass < 2; pass++) {
                hipLaunchKernelGGL(k_ci_keys_groups, dim3(rsem::ceil_div((uint64_t)n * nS, kBlock)), dim3(kBlock), 0, st, nS, S.d_Y, S.d_sc,
                                   S.d_lbar, d_gb, d_ge, (int64_t)n, pass == 1, d_keys);
                int r = sorter.run(d_keys, (int64_t)n, confidence, lb.data(), ub.data(), cq.data());
                if (r != RSEM_OK) return r;
                float* out = pass ? out_f : out_t;
                for (size_t i = 0; i < n; i++) {
                    const int g = multi[i0 + i];
                    out[g] = lb[i]; out[(size_t)ng + g] = ub[i]; out[2 * (size_t)ng + g] = cq[i];
                }
            }
        }
        return RSEM_OK;
    };
    if (rc == RSEM_OK) rc = groups(m, gene_starts, gene_tpm_ci, gene_fpkm_ci);
    if (rc == RSEM_OK && allele) rc = groups(m_trans, trans_starts, iso_tpm_ci, iso_fpkm_ci);
    return rc;
}

int ci_check_groups(int32_t M, const int32_t* gene_starts, int32_t m, const int32_t* trans_starts, int32_t m_trans, double confidence,
                    const float* iso_tpm_ci, const float* iso_fpkm_ci) {
    RSEM_REQUIRE(m > 0 && gene_starts[0] == 1 && gene_starts[m] == M + 1, "gene_starts must run from 1 to M+1");
    RSEM_REQUIRE(confidence > 0.0 && confidence <= 1.0, "confidence must be in (0, 1]");
    if (trans_starts) RSEM_REQUIRE(m_trans > 0 && iso_tpm_ci && iso_fpkm_ci && trans_starts[0] == 1 && trans_starts[m_trans] == M + 1, "bad trans_starts");
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_ci_calculate(int device, int32_t M, int32_t nCV, int32_t nSpC, const int32_t* cvecs, const double* eel,
                                 const double* mw, double pseudoC, uint64_t seed, double confidence, int32_t m,
                                 const int32_t* gene_starts, int32_t m_trans, const int32_t* trans_starts, float* tpm_ci,
                                 float* fpkm_ci, float* gene_tpm_ci, float* gene_fpkm_ci, float* iso_tpm_ci, float* iso_fpkm_ci,
                                 rsem_ci_profile* prof) {
    int rc = check_common(M, nCV, nSpC);
    if (rc != RSEM_OK) return rc;
    RSEM_REQUIRE(cvecs && eel && mw && gene_starts && tpm_ci && fpkm_ci && gene_tpm_ci && gene_fpkm_ci, "null argument");
    rc = ci_check_groups(M, gene_starts, m, trans_starts, m_trans, confidence, iso_tpm_ci, iso_fpkm_ci);
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(hipSetDevice(device));
    StreamGuard sg;
    RSEM_HIP_TRY(sg.create());
    hipStream_t st = sg.s;
    const int32_t nS = nCV * nSpC;
    EventGuard gt0, gt1;
    RSEM_HIP_TRY(gt0.create()); RSEM_HIP_TRY(gt1.create());
    hipEvent_t t0 = gt0.e, t1 = gt1.e;
    RSEM_HIP_TRY(hipEventRecord(t0, st));
    {
        Sampler S;
        RowSorter sorter;
        rc = S.run(M, nCV, nSpC, cvecs, eel, mw, pseudoC, seed, st);
        if (rc == RSEM_OK)
            rc = ci_after_sampling(S, M, nS, confidence, m, gene_starts, m_trans, trans_starts, tpm_ci, fpkm_ci, gene_tpm_ci, gene_fpkm_ci, iso_tpm_ci,
                                   iso_fpkm_ci, st, sorter);
        if (rc == RSEM_OK) {
            hipError_t e = hipEventRecord(t1, st);
            if (e == hipSuccess) e = hipEventSynchronize(t1);
            float ms = 0;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
            if (e != hipSuccess) { rsem::set_last_error("event timing failed"); rc = RSEM_ERR_HIP; }
            if (prof) {
                prof->sample_ms = S.sample_ms; prof->sort_ms = sorter.sort_ms; prof->interval_ms = sorter.interval_ms; prof->total_ms = ms;
                prof->n_draws = (uint64_t)M * nS; prof->n_keys_sorted = sorter.n_keys;
            }
        }
    }
    return rc;
}

extern "C" int rsem_ci_calculate_samples(int device, int32_t M, int32_t nSamples, const float* tpm_samples, const float* l_bars, double confidence,
                                         int32_t m, const int32_t* gene_starts, int32_t m_trans, const int32_t* trans_starts, float* tpm_ci,
                                         float* fpkm_ci, float* gene_tpm_ci, float* gene_fpkm_ci, float* iso_tpm_ci, float* iso_fpkm_ci,
                                         rsem_ci_profile* prof) {
    RSEM_REQUIRE(M > 0 && nSamples > 0 && nSamples < (1 << 30), "M and nSamples must be positive (nSamples < 2^30)");
    RSEM_REQUIRE(tpm_samples && l_bars && gene_starts && tpm_ci && fpkm_ci && gene_tpm_ci && gene_fpkm_ci, "null argument");
    int rc = ci_check_groups(M, gene_starts, m, trans_starts, m_trans, confidence, iso_tpm_ci, iso_fpkm_ci);
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(hipSetDevice(device));
    StreamGuard sg;
    RSEM_HIP_TRY(sg.create());
    hipStream_t st = sg.s;
    const int32_t nS = nSamples;
    EventGuard gt0, gt1;
    RSEM_HIP_TRY(gt0.create()); RSEM_HIP_TRY(gt1.create());
    RSEM_HIP_TRY(hipEventRecord(gt0.e, st));
    {
        Sampler S;  // filled from the caller's samples: Y = the TPM values themselves, every scale 1
        RowSorter sorter;
        RSEM_HIP_TRY(S.mem.alloc(&S.d_Y, (size_t)M * nS));
        RSEM_HIP_TRY(S.mem.alloc(&S.d_sc, (size_t)nS));
        RSEM_HIP_TRY(S.mem.alloc(&S.d_lbar, (size_t)nS));
        std::vector<double> ones((size_t)nS, 1.0);
        RSEM_HIP_TRY(hipMemcpyAsync(S.d_Y, tpm_samples, sizeof(float) * (size_t)M * nS, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(S.d_sc, ones.data(), sizeof(double) * nS, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipMemcpyAsync(S.d_lbar, l_bars, sizeof(float) * nS, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));  // (`ones` is a local)
        rc = ci_after_sampling(S, M, nS, confidence, m, gene_starts, m_trans, trans_starts, tpm_ci, fpkm_ci, gene_tpm_ci, gene_fpkm_ci, iso_tpm_ci,
                               iso_fpkm_ci, st, sorter);
        if (rc == RSEM_OK) {
            hipError_t e = hipEventRecord(gt1.e, st);
            if (e == hipSuccess) e = hipEventSynchronize(gt1.e);
            float ms = 0;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, gt0.e, gt1.e);
            if (e != hipSuccess) { rsem::set_last_error("event timing failed"); rc = RSEM_ERR_HIP; }
            if (prof) {
                prof->sample_ms = 0.0; prof->sort_ms = sorter.sort_ms; prof->interval_ms = sorter.interval_ms; prof->total_ms = ms;
                prof->n_draws = 0; prof->n_keys_sorted = sorter.n_keys;
            }
        }
    }
    return rc;
}

// rsem_hip_preload (status.hip): the first launch of a translation unit makes the runtime load its code object
namespace { __global__ void k_preload_ci() {} }
namespace rsem { void preload_ci() { hipLaunchKernelGGL(k_preload_ci, dim3(1), dim3(1), 0, nullptr); (void)hipGetLastError(); } }
