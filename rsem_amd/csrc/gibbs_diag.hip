// gibbs_diag.hip -- convergence diagnostics of the Gibbs stage on MI355X (rsem-run-gibbs --diagnostics).
//
// The reference has no counterpart: it writes the count vectors (Gibbs.cpp:257-262) and says nothing about whether its chains
// agree.  Input are those count vectors, nchains blocks of nsamples[k] x (M+1) int32.  Every chain gives its last n' rows, cut in
// two: m = 2 nchains sequences of n values per transcript.  Per transcript: mean, posterior sd, split-R-hat, effective sample
// size by Geyer's initial monotone sequence, and the last lag the sum took (the definition: gibbs_diag_math.hpp).
//
//   k_diag_short    lane = transcript, blockIdx.y = sequence.  A workgroup stages its 128 columns x up to 128 samples in LDS with
//                   16-byte loads (the rows are uploaded with a pitch of a multiple of 128 ints) and every lane walks its own
//                   column: int64 sums of the values shifted by the sequence's first one, for the lags 1 .. L0 + 2.
//   k_diag_finish   lane = transcript: combines the m sequences, runs Geyer's rule over the lags <= L0 + 2 and either writes the
//                   answer (its lag is <= L0) or appends the transcript to the long list (the one atomic: an integer counter,
//                   whose order enters nothing).
//   k_diag_long     one wave per listed transcript, its series in LDS (or read from global memory past the LDS budget): lanes
//                   take lags in groups of 64, after each group the wave continues Geyer's rule, from k = 0, uniformly.
//   k_diag_summary  a fixed tree in two levels (up to 256 workgroups, then one).
// No floating-point atomics; nothing depends on scheduling.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "simt_macros.hpp"
#include "gibbs_diag_math.hpp"
#include "stage_util.hpp"

namespace {

using namespace rsem_diag;

constexpr int kTileCols = 128;       // columns of a workgroup of k_diag_short = its threads
constexpr int kTileRows = 128;       // samples it holds in LDS at a time (64 KiB); longer sequences go in chunks that overlap by the lags
constexpr int kDefaultL0 = 15;
constexpr int kMaxL0 = 63;
constexpr size_t kLongLdsBytes = 32 << 10;  // series of one transcript that k_diag_long keeps in LDS (five of its one-wave workgroups per CU)

// The sums of all sequences: field f of sequence j for column c at part[((j * F) + f) * Mp + c], F = 2 + 2 Lc:
// f = 0: s1, 1: s2, 2 .. Lc+1: c_1 .. c_Lc, Lc+2 .. 2Lc+1: e_1 .. e_Lc.
struct Layout {
    const int32_t* data;  // row j * n + s = sample s of sequence j, Mp ints per row
    int64_t* part;
    int64_t Mp;
    int32_t n, m, Lc, M1;
    __device__ __host__ int F() const { return 2 + 2 * Lc; }
};

__global__ void __launch_bounds__(kTileCols) k_diag_short(Layout L, int rows_lds) {
    extern __shared__ int4 tile4[];
    int32_t* tile = (int32_t*)tile4;
    const int tid = threadIdx.x, j = blockIdx.y;
    const int64_t col0 = (int64_t)blockIdx.x * kTileCols, col = col0 + tid;
    const int n = L.n, Lc = L.Lc;
    const int32_t* seq = L.data + (size_t)j * n * L.Mp;
    const int32_t x0 = seq[col];
    int64_t* out = L.part + (size_t)j * L.F() * L.Mp + col;
    const int step = rows_lds >= n ? n : rows_lds - Lc;
    for (int s0 = 0; s0 < n; s0 += step) {
        const int nrows = min(rows_lds, n - s0), own = min(step, n - s0);
        __syncthreads();
        for (int idx = tid; idx < nrows * (kTileCols / 4); idx += kTileCols) {
            const int r = idx / (kTileCols / 4), q = idx % (kTileCols / 4);
            tile4[idx] = *(const int4*)(seq + (size_t)(s0 + r) * L.Mp + col0 + 4 * q);
        }
        __syncthreads();
        // from here a lane touches its own column only
        for (int r = 0; r < nrows; r++) tile[r * kTileCols + tid] -= x0;
        int64_t s1 = 0, s2 = 0;
        for (int r = 0; r < own; r++) {
            const int32_t y = tile[r * kTileCols + tid];
            s1 += y;
            s2 += (int64_t)y * y;
        }
        if (s0 == 0) { out[0] = s1; out[L.Mp] = s2; }
        else { out[0] += s1; out[L.Mp] += s2; }
        for (int t = 1; t <= Lc; t++) {
            const int cnt = min(own, n - t - s0);  // rows r of this chunk with s0 + r + t < n
            int64_t acc = 0;
            for (int r = 0; r < cnt; r++) acc += (int64_t)tile[r * kTileCols + tid] * tile[(r + t) * kTileCols + tid];
            int64_t* o = out + (size_t)(1 + t) * L.Mp;
            if (s0 == 0) *o = acc; else *o += acc;
        }
    }
    int64_t a = 0, z = 0;
    for (int t = 1; t <= Lc; t++) {
        a += seq[(size_t)(t - 1) * L.Mp + col] - x0;
        z += seq[(size_t)(n - t) * L.Mp + col] - x0;
        out[(size_t)(1 + Lc + t) * L.Mp] = a + z;
    }
}

struct SeqGlobal {
    Layout L;
    int64_t col;
    __device__ void operator()(int j, int64_t& x0, int64_t& s1, int64_t& s2) const {
        x0 = L.data[(size_t)j * L.n * L.Mp + col];
        const int64_t* p = L.part + (size_t)j * L.F() * L.Mp + col;
        s1 = p[0];
        s2 = p[L.Mp];
    }
};
struct LagGlobal {
    Layout L;
    int64_t col;
    __device__ void operator()(int j, int t, int64_t& c_t, int64_t& e_t) const {
        const int64_t* p = L.part + (size_t)j * L.F() * L.Mp + col;
        c_t = p[(size_t)(1 + t) * L.Mp];
        e_t = p[(size_t)(1 + L.Lc + t) * L.Mp];
    }
};

__global__ void __launch_bounds__(256) k_diag_finish(Layout L, int L0, double* __restrict__ mean, double* __restrict__ sd,
                                                      double* __restrict__ rhat, double* __restrict__ ess, int32_t* __restrict__ lag,
                                                      int32_t* __restrict__ long_list, int32_t* long_count) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= L.M1) return;
    const Result r = gd_evaluate(L.n, L.m, L0, SeqGlobal{L, col}, LagGlobal{L, col});
    mean[col] = r.mean;
    sd[col] = r.sd;
    rhat[col] = r.rhat;
    if (r.is_long) {
        long_list[atomicAdd(long_count, 1)] = (int32_t)col;
        if (col == 0) long_count[1] = 1;  // the noise column is worked on like the others and left out of the summary
    } else {
        ess[col] = r.ess;
        lag[col] = r.lag;
    }
}

template <bool kLds>
__global__ void __launch_bounds__(64) k_diag_long(Layout L, const int32_t* __restrict__ long_list, double* __restrict__ ess,
                                                    int32_t* __restrict__ lag) {
    extern __shared__ int4 series4[];
    __shared__ double rho_s[64];
    int32_t* xs = (int32_t*)series4;
    const int lane = threadIdx.x, n = L.n, m = L.m;
    const int64_t col = long_list[blockIdx.x];
    if (kLds) {
        for (int i = lane; i < m * n; i += 64) xs[i] = L.data[(size_t)i * L.Mp + col];
        __syncthreads();
    }
    auto X = [&](int j, int s) -> int32_t { return kLds ? xs[j * n + s] : L.data[((size_t)j * n + s) * L.Mp + col]; };
    const SeqGlobal seq{L, col};
    const Moments mo = gd_moments(n, m, seq);
    Geyer g;
    gd_geyer_init(g);
    bool stopped = false;
    for (int base = 0; base <= n - 1 && !stopped; base += 64) {
        const int t = base + lane;
        double rho = 0.0;
        if (t == 0) rho = 1.0;
        else if (t <= n - 1) {
            double gs = 0.0;
            for (int j = 0; j < m; j++) {
                int64_t x0, s1, s2, c_t = 0, e_t = 0;
                seq(j, x0, s1, s2);
                const int32_t x0i = (int32_t)x0;
                for (int s = 0; s < n - t; s++) c_t += (int64_t)(X(j, s) - x0i) * (X(j, s + t) - x0i);
                for (int s = 0; s < t; s++) e_t += (int64_t)(X(j, s) - x0i) + (X(j, n - 1 - s) - x0i);
                gs += gd_gamma(n, t, s1, c_t, e_t);
            }
            rho = gd_rho(mo.W, gs / (double)m, mo.varp);
        }
        rho_s[lane] = rho;
        __syncthreads();
        for (int p = 0; p < 32; p++) {  // the same in every lane
            const int k = (base >> 1) + p;
            if (2 * k + 1 > n - 1 || !gd_geyer_take(g, k, rho_s[2 * p], rho_s[2 * p + 1])) { stopped = true; break; }
        }
        __syncthreads();
    }
    if (lane == 0) {
        ess[col] = gd_ess((int64_t)m * n, g);
        lag[col] = g.lag;
    }
}

struct Best {
    double max_rhat, min_ess;
    int32_t max_id, min_id, n_defined, n_1p01, n_1p1;
};
__device__ inline void best_join(Best& a, const Best& b) {  // ties: the smaller id
    if (b.max_id && (!a.max_id || b.max_rhat > a.max_rhat || (b.max_rhat == a.max_rhat && b.max_id < a.max_id))) { a.max_rhat = b.max_rhat; a.max_id = b.max_id; }
    if (b.min_id && (!a.min_id || b.min_ess < a.min_ess || (b.min_ess == a.min_ess && b.min_id < a.min_id))) { a.min_ess = b.min_ess; a.min_id = b.min_id; }
    a.n_defined += b.n_defined;
    a.n_1p01 += b.n_1p01;
    a.n_1p1 += b.n_1p1;
}

// ids 1 .. M; max_rhat over the finite values, min_ess over the values that are not NaN; the two counts include rhat = +inf.
// Two levels of the same fixed tree: every workgroup reduces its ids (grid-strided) into part[blockIdx.x], then one workgroup
// reduces the parts (src = part, n = the number of parts).  best_join is exact, commutative and associative.
constexpr int kSummaryBlocks = 256;
__device__ inline void best_tree(Best* sh, Best b, Best* out) {
    sh[threadIdx.x] = b;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) best_join(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}
__global__ void __launch_bounds__(256) k_diag_summary(int32_t M, const double* __restrict__ rhat, const double* __restrict__ ess, Best* part) {
    __shared__ Best sh[256];
    Best b{0.0, 0.0, 0, 0, 0, 0, 0};
    for (int64_t i = 1 + (int64_t)blockIdx.x * 256 + threadIdx.x; i <= M; i += (int64_t)gridDim.x * 256) {
        const double r = rhat[i], e = ess[i];
        const int32_t id = (int32_t)i;
        Best c{r, e, isfinite(r) ? id : 0, isnan(e) ? 0 : id, isfinite(r) ? 1 : 0, r > 1.01 ? 1 : 0, r > 1.1 ? 1 : 0};
        best_join(b, c);
    }
    best_tree(sh, b, part + blockIdx.x);
}
__global__ void __launch_bounds__(256) k_diag_summary_parts(int nparts, const Best* __restrict__ part, Best* out) {
    __shared__ Best sh[256];
    Best b{0.0, 0.0, 0, 0, 0, 0, 0};
    if ((int)threadIdx.x < nparts) b = part[threadIdx.x];
    best_tree(sh, b, out);
}

}  // namespace

extern "C" int rsem_gibbs_diagnose(int device, int32_t M, int nchains, const int32_t* nsamples, const int32_t* const* count_vectors,
                                   double* mean, double* sd, double* rhat, double* ess, int32_t* lag, rsem_gibbs_diag_summary* summary) {
    RSEM_REQUIRE(device >= 0 && M > 0 && nchains > 0 && nsamples && count_vectors, "rsem_gibbs_diagnose: device, M, nchains must not be negative, nsamples and count_vectors not NULL");
    RSEM_REQUIRE(nchains < 32768, "rsem_gibbs_diagnose: at most 32767 chains");
    int32_t nmin = nsamples[0];
    for (int k = 0; k < nchains; k++) {
        RSEM_REQUIRE(nsamples[k] >= 0, "rsem_gibbs_diagnose: negative nsamples");
        RSEM_REQUIRE(count_vectors[k], "rsem_gibbs_diagnose: a count-vector block is NULL");
        nmin = std::min(nmin, nsamples[k]);
    }
    const int32_t nused = 2 * (nmin / 2), n = nused / 2, m = 2 * nchains;
    if (n < 2) {
        rsem::set_last_error("rsem_gibbs_diagnose: the shortest chain has %d samples: its halves have %d, and at least 2 are needed", nmin, n);
        return RSEM_ERR_INVALID;
    }
    int L0 = kDefaultL0;
    if (const char* e = getenv("RSEM_GIBBS_DIAG_L0")) {  // a test and measurement knob, read at call time
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end || v < 1 || v > kMaxL0 || v % 2 == 0) {
            rsem::set_last_error("RSEM_GIBBS_DIAG_L0 = '%s': an odd number in 1 .. %d is expected", e, kMaxL0);
            return RSEM_ERR_INVALID;
        }
        L0 = (int)v;
    }
    Layout L;
    L.n = n; L.m = m; L.M1 = M + 1;
    L.Lc = std::min(L0 + 2, n - 1);
    L.Mp = ((int64_t)M + 1 + kTileCols - 1) / kTileCols * kTileCols;
    const size_t data_ints = (size_t)m * n * L.Mp, part_words = (size_t)m * L.F() * L.Mp;
    const size_t need = data_ints * 4 + part_words * 8 + (size_t)L.Mp * (4 * 8 + 4 + 4) + (1 << 20);

    RSEM_HIP_TRY(hipSetDevice(device));
    size_t free_b = 0, total_b = 0;
    RSEM_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        rsem::set_last_error("rsem_gibbs_diagnose: %d sequences of %d samples x %d transcripts need %zu bytes on the device (%zu of count vectors, "
                             "%zu of sums), %zu are free", m, n, M + 1, need, data_ints * 4, part_words * 8, free_b);
        return RSEM_ERR_NOMEM;
    }
    rsem::StageQueue q;
    RSEM_HIP_TRY(q.create());
    hipStream_t st = q.st;
    rsem::DevMem mem;
    int32_t *d_data = nullptr, *d_lag = nullptr, *d_list = nullptr, *d_count = nullptr;
    int64_t* d_part = nullptr;
    double *d_mean = nullptr, *d_sd = nullptr, *d_rhat = nullptr, *d_ess = nullptr;
    Best* d_best = nullptr;
    RSEM_HIP_TRY(mem.alloc(&d_data, data_ints));
    RSEM_HIP_TRY(mem.alloc(&d_part, part_words));
    RSEM_HIP_TRY(mem.alloc(&d_mean, (size_t)L.Mp)); RSEM_HIP_TRY(mem.alloc(&d_sd, (size_t)L.Mp));
    RSEM_HIP_TRY(mem.alloc(&d_rhat, (size_t)L.Mp)); RSEM_HIP_TRY(mem.alloc(&d_ess, (size_t)L.Mp));
    RSEM_HIP_TRY(mem.alloc(&d_lag, (size_t)L.Mp)); RSEM_HIP_TRY(mem.alloc(&d_list, (size_t)L.Mp));
    RSEM_HIP_TRY(mem.alloc(&d_count, 2)); RSEM_HIP_TRY(mem.alloc(&d_best, 1 + kSummaryBlocks));
    L.data = d_data; L.part = d_part;

    // upload: the last n' rows of every chain, each row at a pitch of Mp ints (a multiple of 16 bytes; the columns behind M are zero)
    RSEM_HIP_TRY(q.upload_begin());
    RSEM_HIP_TRY(hipMemsetAsync(d_data, 0, data_ints * 4, st));
    RSEM_HIP_TRY(hipMemsetAsync(d_count, 0, 2 * sizeof(int32_t), st));
    for (int k = 0; k < nchains; k++) {
        const int32_t* src = count_vectors[k] + (size_t)(nsamples[k] - nused) * ((size_t)M + 1);
        RSEM_HIP_TRY(hipMemcpy2DAsync(d_data + (size_t)k * nused * L.Mp, (size_t)L.Mp * 4, src, ((size_t)M + 1) * 4, ((size_t)M + 1) * 4, (size_t)nused,
                                      hipMemcpyHostToDevice, st));
    }
    RSEM_HIP_TRY(q.upload_end());

    const int rows_lds = std::min(n, kTileRows);
    hipLaunchKernelGGL(k_diag_short, dim3((unsigned)(L.Mp / kTileCols), (unsigned)m), dim3(kTileCols), (size_t)rows_lds * kTileCols * 4, st, L, rows_lds);
    hipLaunchKernelGGL(k_diag_finish, dim3(rsem::ceil_div((uint64_t)M + 1, 256)), dim3(256), 0, st, L, L0, d_mean, d_sd, d_rhat, d_ess, d_lag, d_list, d_count);
    int32_t counts[2] = {0, 0};
    RSEM_HIP_TRY(hipMemcpyAsync(counts, d_count, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    const int32_t n_long = counts[0];
    if (n_long > 0) {
        const size_t series = ((size_t)m * n * 4 + 15) / 16 * 16;
        if (series <= kLongLdsBytes) {
            hipLaunchKernelGGL(k_diag_long<true>, dim3((unsigned)n_long), dim3(64), series, st, L, d_list, d_ess, d_lag);
        } else {
            hipLaunchKernelGGL(k_diag_long<false>, dim3((unsigned)n_long), dim3(64), 0, st, L, d_list, d_ess, d_lag);
        }
    }
    const int sum_blocks = std::min(kSummaryBlocks, rsem::ceil_div((uint64_t)M, 256));
    hipLaunchKernelGGL(k_diag_summary, dim3(sum_blocks), dim3(256), 0, st, M, d_rhat, d_ess, d_best + 1);
    hipLaunchKernelGGL(k_diag_summary_parts, dim3(1), dim3(256), 0, st, sum_blocks, d_best + 1, d_best);
    RSEM_HIP_TRY(q.kernels_end());
    Best best;
    RSEM_HIP_TRY(hipMemcpyAsync(&best, d_best, sizeof(Best), hipMemcpyDeviceToHost, st));
    const size_t M1 = (size_t)M + 1;
    if (mean) RSEM_HIP_TRY(hipMemcpyAsync(mean, d_mean, M1 * 8, hipMemcpyDeviceToHost, st));
    if (sd) RSEM_HIP_TRY(hipMemcpyAsync(sd, d_sd, M1 * 8, hipMemcpyDeviceToHost, st));
    if (rhat) RSEM_HIP_TRY(hipMemcpyAsync(rhat, d_rhat, M1 * 8, hipMemcpyDeviceToHost, st));
    if (ess) RSEM_HIP_TRY(hipMemcpyAsync(ess, d_ess, M1 * 8, hipMemcpyDeviceToHost, st));
    if (lag) RSEM_HIP_TRY(hipMemcpyAsync(lag, d_lag, M1 * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (summary) {
        double up = 0, kern = 0;
        if (int rc = q.add_laps(up, kern)) return rc;
        summary->n_used = nused; summary->sequences = m; summary->n_defined = best.n_defined;
        summary->max_rhat_id = best.max_id; summary->min_ess_id = best.min_id;
        summary->n_rhat_gt_1p01 = best.n_1p01; summary->n_rhat_gt_1p1 = best.n_1p1; summary->n_long = n_long - counts[1];
        summary->max_rhat = best.max_id ? best.max_rhat : NAN;
        summary->min_ess = best.min_id ? best.min_ess : NAN;
        summary->upload_ms = up; summary->kernel_ms = kern;
    }
    return RSEM_OK;
}
