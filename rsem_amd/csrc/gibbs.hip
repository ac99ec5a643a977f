// gibbs.hip -- rsem-run-gibbs's sampler on MI355X (gfx950).  C ABI: include/rsem_hip.h.
//
// The reference chain (Gibbs.cpp:265-353) is a collapsed Gibbs sampler: reads are visited strictly
// in order, each visit removes the read from `counts`, draws its transcript with probability
// proportional to (counts[sid] + alpha) * conprb, and adds it back.  `counts` is loop-carried from
// read to read (and nearly every read carries the noise transcript 0), so a chain has no
// read-level parallelism.  Two device samplers are provided:
//
//   RSEM_GIBBS_EXACT     the reference chain itself: same visiting order, same left-to-right
//                        cumulative sums, MT19937 + u = mt()*2^-32 (sampling.h:50-65), hence the
//                        same integer count vectors bit for bit.  A team of workgroups per chain:
//                        tiles of 256 reads resolved in LDS, W tiles of a window at once, the moves
//                        between them settled through the team's tables (gibbs_exact_team.hpp).
//   RSEM_GIBBS_PARALLEL  the data-augmentation (uncollapsed) Gibbs sampler for the same posterior:
//                        theta | z ~ Dirichlet(counts + alpha) (one Gamma draw per transcript,
//                        Marsaglia-Tsang, Philox4x32-10 counter RNG), then all z_i | theta drawn
//                        independently in parallel over the sliced layout of sell_layout.hpp --
//                        an E-step-shaped, HBM-bound sweep (8 B per alignment inside runs of
//                        identical reads).  It is a different Markov chain with the same
//                        stationary distribution; it mixes more slowly per sweep on weakly
//                        identified isoform pairs, which `thin` (extra sweeps per counted round)
//                        compensates.  Results are deterministic for a fixed seed.
//
// Per kept sample (Gibbs.cpp:313-346): theta = (counts + alpha) / totc, polishTheta,
// calcExpressionValues (WriteResults.h:55-104) and the running sums -- on the device.
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <cerrno>
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <string>

#include <cstdlib>

#include "comm_internal.hpp"
#include "rng.hpp"
#include "sell_layout.hpp"

namespace {

using rsem::kEpsilon;

using rsem::Philox;
using rsem::u53;
using rsem::gamma_draw;

// g[i] = Gamma(counts[i] + alpha_i) (unnormalised Dirichlet draw); omitted transcripts (counts < 0) get 0
// ... and the counts are re-armed for the z pass that follows (init_counts: 0, or -1 for omitted transcripts; the noise
// bin starts at N0), which saves the separate reset launch of every sweep
__global__ void k_sample_theta(int32_t M, int32_t* __restrict__ counts, const double* __restrict__ alpha,
                               double pseudoC, Philox ph, uint32_t sweep, double* g, const int32_t* __restrict__ init_counts,
                               int32_t n0) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M) return;
    int c = counts[i];
    g[i] = (c < 0) ? 0.0 : gamma_draw(ph, (uint32_t)i, sweep, (double)c + (alpha ? alpha[i] : pseudoC));
    counts[i] = init_counts[i] + (i == 0 ? n0 : 0);
}

__global__ void k_fill_double(int32_t n, double v, double* g) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = v;
}

// waves per SIMD the sweep kernel is compiled for (its register budget): 4 = what it needs unconstrained (100 VGPRs)
#ifndef RSEM_GIBBS_MIN_WAVES
#define RSEM_GIBBS_MIN_WAVES 4  /* 5 (95 VGPRs, 2 spilled) measured the same: profiles/r03d_exact_sweep_bench.log */
#endif
constexpr int kGWindow = 2048;  // sids per workgroup window (g values: 16 KB, int counts: 8 KB of LDS)
static_assert(kGWindow == kLayoutWindow, "the layout sorts reads apart and sizes windows for the sweep's LDS window (sell_layout.hpp)");

// the per-wave body of the sweep kernel (also run on the CPU by tests/gibbs_emu.cpp)
#include "gibbs_block.hpp"


__global__ __launch_bounds__(kBlock, RSEM_GIBBS_MIN_WAVES) void k_sample_z_lane(
    const Shape* __restrict__ shapes, const Unit* __restrict__ units, uint32_t T, int M,
    const double* __restrict__ g, const double* __restrict__ scp, const int32_t* __restrict__ ssid,
    const double* __restrict__ sncp, const unsigned long long* __restrict__ masks, Philox ph, uint32_t sweep,
    int32_t* counts
    ) {
    __shared__ double g_win[kGWindow];
    __shared__ int cnt_win[kGWindow];
    __shared__ int s_noise;
    const Unit U = units[blockIdx.x];
    if (threadIdx.x == 0) s_noise = 0;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int noise = 0;
    {
        const Shape S = U.S;
        const uint32_t u_end = S.slice_base + U.slice_begin + U.n_slices;
        const uint32_t s_begin = S.slice_base + U.slice_begin + (uint32_t)w * U.per_wave;
        const uint32_t s_end = min(u_end, s_begin + U.per_wave);
        const double g0 = g[0];
#define RSEM_GIBBS_BLOCK(KK, FF) gibbs_block<KK, FF>(S, T, s_begin, s_end, lane, U.base, U.span, g, g0, g_win, cnt_win, scp, ssid, sncp, masks, ph, sweep, counts, noise, M)
        if (s_begin < u_end) switch (S.K + (U.pad[0] != 0 ? 4 : 0)) {  // (uniform over the workgroup)
            case 1: RSEM_GIBBS_BLOCK(1, false); break;
            case 2: RSEM_GIBBS_BLOCK(2, false); break;
            case 3: RSEM_GIBBS_BLOCK(3, false); break;
            case 4: RSEM_GIBBS_BLOCK(4, false); break;
            case 5: RSEM_GIBBS_BLOCK(1, true); break;
            case 6: RSEM_GIBBS_BLOCK(2, true); break;
            case 7: RSEM_GIBBS_BLOCK(3, true); break;
            default: RSEM_GIBBS_BLOCK(4, true); break;
#undef RSEM_GIBBS_BLOCK
        } else stage_gwindows(U.base, U.span, M, g, g_win, cnt_win);
    }
    for (int d = 32; d >= 1; d >>= 1) noise += __shfl_xor(noise, d);
    if (lane == 0 && noise) atomicAdd(&s_noise, noise);
    __syncthreads();
    for (int i = threadIdx.x; i < U.span; i += blockDim.x) {
        const int v = cnt_win[i];
        if (v != 0) atomicAdd(&counts[U.base + i], v);
    }
    if (threadIdx.x == 0 && s_noise) atomicAdd(&counts[0], s_noise);
}

// reads with > 256 alignments (not in the sliced layout): a WAVE per read over the caller's CSR.  The read is walked in chunks of 64
// alignments, lane = alignment: an inclusive scan inside the chunk (shuffles), the chunks one after the other -- once for the total,
// once more for the first alignment whose running sum passes the target (the same scan, so the two passes agree to the bit and the
// target always lands on an alignment).  (A thread per read was 2 x 2 000 dependent round trips for a read of 2 000 alignments: the
// cliff profiles/r05z_long_rows.log shows for the E step.)  The pick is a pick from the same distribution as before, not the same
// pick: the partial sums are formed in another order.
__global__ __launch_bounds__(kBlock) void k_sample_z_long(uint32_t n_rows, const uint32_t* __restrict__ row_list, uint32_t row_id_base,
                                                           const uint64_t* __restrict__ row_ptr, const int32_t* __restrict__ sid,
                                                           const double* __restrict__ cp, const double* __restrict__ ncp,
                                                           const double* __restrict__ g, Philox ph, uint32_t sweep, int32_t* counts) {
    const int lane = threadIdx.x & 63;
    const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // (wave-uniform)
    if (t >= n_rows) return;
    const uint32_t i = row_list[t];
    const uint64_t fr = row_ptr[i], to = row_ptr[i + 1];
    const double f0 = g[0] * ncp[i];
    auto chunk_scan = [&](uint64_t j0, double& f, int& s) -> double {  // inclusive scan of the chunk's weights; returns this lane's prefix
        const uint64_t j = j0 + (uint64_t)lane;
        s = j < to ? sid[j] : 0;
        f = j < to ? g[s] * cp[j] : 0.0;
        double p = f;
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_up(p, d);
            if (lane >= d) p += o;
        }
        return p;
    };
    double total = f0;
    for (uint64_t j0 = fr; j0 < to; j0 += 64) {
        double f;
        int s;
        const double p = chunk_scan(j0, f, s);
        total += __shfl(p, 63);
    }
    if (!(total > 0.0)) return;
    uint32_t r[4];
    ph.gen(row_id_base + t, sweep, 0x5a5a5a5au, 0u, r);
    double target = u53(r[0], r[1]) * total;
    if (target >= total) target = total * (1.0 - 1.1102230246251565e-16);
    int pick = 0;
    if (!(target < f0)) {
        double run = f0;
        int last = 0;
        bool found = false;
        for (uint64_t j0 = fr; j0 < to && !found; j0 += 64) {  // (wave-uniform: found comes from a ballot)
            double f;
            int s;
            const double p = chunk_scan(j0, f, s);
            const unsigned long long hit = __ballot(target < run + p);
            const unsigned long long pos = __ballot(f > 0.0);
            if (hit) {
                pick = __shfl(s, __builtin_ctzll(hit));
                found = true;
            } else {
                if (pos) last = __shfl(s, 63 - __builtin_clzll(pos));
                run += __shfl(p, 63);
            }
        }
        if (!found) pick = last;
    }
    if (lane == 0) atomicAdd(&counts[pick], 1);
}

// ---- EXACT mode: the reference chain (Gibbs.cpp:297-311), a team of workgroups per chain ------------------------------
//
// The chain is sequential from read to read only through `counts`, and one visit changes at most two of its entries
// (counts[z_old]--, counts[z_new]++).  The kernel therefore draws tiles of consecutive reads speculatively against the counts as
// they were before the tile and settles, in file order, the draws that a move of an earlier read of the tile (or of the window
// of tiles the team took together) actually touches -- with the SAME random numbers.  The fixed point is the sequential chain:
// same visiting order, same left-to-right cumulative sums, same MT19937 stream (read r takes the r-th output), hence the same
// integer count vectors bit for bit (tests/test_gibbs_gpu.py, tests/test_cli_gpu.py against the reference's own countvectors
// files; the kernel body on the CPU emulator: tests/test_gibbs_exact_team_emu_cpu.py).  gibbs_exact_team.hpp over
// gibbs_exact_wg.hpp, compiled twice: the uniform pseudo count, and --prior (per-transcript pseudo counts) in namespace gx_prior.

struct MtState { uint32_t mt[624]; int idx; };  // a chain's generator between launches (= GxMtState of the headers)

#include "gibbs_exact_team.hpp"
#define RSEM_GX_PRIOR 1
namespace gx_prior {
#include "gibbs_exact_team.hpp"
}
#undef RSEM_GX_PRIOR
static_assert(sizeof(GxMtState) == sizeof(MtState) && sizeof(gx_prior::GxMtState) == sizeof(MtState), "one layout of a chain's generator");
static_assert(sizeof(TeamArgs) == sizeof(gx_prior::TeamArgs) && sizeof(XSlot) == sizeof(gx_prior::XSlot) && sizeof(XTeamCtl) == sizeof(gx_prior::XTeamCtl),
              "the host fills the uniform pass's records for either kernel");

// ---- per-sample statistics (Gibbs.cpp:313-346, WriteResults.h:55-104) ---------------------------
//
// theta_i = (counts_i + alpha_i) / totc, polishTheta, calcExpressionValues.  Written out, with
//   t_i = theta_i / mw_i  (0 when i >= 1 and (mw_i < EPS or eel_i < EPS)),  S1 = sum_i t_i,
//   S2 = sum_{i >= 1, eel_i >= EPS} t_i,  S3 = sum_{i >= 1, eel_i >= EPS} t_i / eel_i:
//   frac_i = t_i / S1 / denom with denom = S2 / S1 (1 when < EPS); fpkm_i = frac_i * 1e9 / eel_i;
//   tpm_i = fpkm_i / denom2 * 1e6 with denom2 = sum fpkm (1 when < EPS).
// Pass A leaves one (S1, S2, S3) partial per workgroup and chain, pass B folds them in a fixed order and adds the
// sample to the chain's accumulators (and copies the count vector out), so the result does not depend on scheduling.

constexpr int kStatMaxBlocks = 64;

__device__ inline double stat_t(int i, int c, const double* __restrict__ alpha, double pseudoC, double totc,
                                const double* __restrict__ eel, const double* __restrict__ mw) {
    double th = (c < 0) ? 0.0 : ((double)c + (alpha ? alpha[i] : pseudoC)) / totc;
    if (i > 0 && (mw[i] < kEpsilon || eel[i] < kEpsilon)) return 0.0;
    return th / mw[i];
}

__device__ inline double block_sum_256(double v) {  // fixed tree
    __shared__ double red[kBlock / 64];
    __syncthreads();
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < kBlock / 64; i++) t += red[i];
    return t;
}

// grid (nblk, chains); chain c takes part while kept < nsamples[c]
__global__ __launch_bounds__(kBlock) void k_gibbs_stats_a(int32_t M, const int32_t* __restrict__ counts_base, uint64_t stride_c,
                                                           int chain0, const int32_t* __restrict__ nsamples, int kept,
                                                           const double* __restrict__ alpha, double pseudoC, double totc,
                                                           const double* __restrict__ eel, const double* __restrict__ mw,
                                                           double* partials) {
    const int chain = chain0 + blockIdx.y;
    if (kept >= nsamples[chain]) return;
    const int32_t* counts = counts_base + (uint64_t)chain * stride_c;
    const int n = M + 1, nb = gridDim.x;
    const int per = (n + nb - 1) / nb;
    const int lo = blockIdx.x * per, hi = min(n, lo + per);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const double t = stat_t(i, counts[i], alpha, pseudoC, totc, eel, mw);
        s1 += t;
        if (i >= 1 && eel[i] >= kEpsilon) { s2 += t; s3 += t / eel[i]; }
    }
    s1 = block_sum_256(s1);
    s2 = block_sum_256(s2);
    s3 = block_sum_256(s3);
    if (threadIdx.x == 0) {
        double* p = partials + ((uint64_t)chain * kStatMaxBlocks + blockIdx.x) * 3;
        p[0] = s1; p[1] = s2; p[2] = s3;
    }
}

__global__ __launch_bounds__(kBlock) void k_gibbs_stats_b(int32_t M, const int32_t* __restrict__ counts_base, uint64_t stride_c,
                                                           int chain0, const int32_t* __restrict__ nsamples, int kept,
                                                           const double* __restrict__ alpha, double pseudoC, double totc,
                                                           const double* __restrict__ eel, const double* __restrict__ mw,
                                                           const double* __restrict__ partials, double* acc_base,
                                                           int32_t* cv_base, const uint64_t* __restrict__ cv_off) {
    const int chain = chain0 + blockIdx.y;
    if (kept >= nsamples[chain]) return;
    const int32_t* counts = counts_base + (uint64_t)chain * stride_c;
    const int n = M + 1, nb = gridDim.x;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int b = 0; b < nb; b++) {
        const double* p = partials + ((uint64_t)chain * kStatMaxBlocks + b) * 3;
        s1 += p[0]; s2 += p[1]; s3 += p[2];
    }
    double denom = s2 / s1;
    if (denom < kEpsilon) denom = 1.0;
    double denom2 = (s3 / s1 / denom) * 1e9;
    if (denom2 < kEpsilon) denom2 = 1.0;
    double* pme_c = acc_base + (uint64_t)chain * 4 * n;
    double* pve_c = pme_c + n;
    double* pme_tpm = pve_c + n;
    double* pme_fpkm = pme_tpm + n;
    int32_t* cv = cv_base ? cv_base + cv_off[chain] + (uint64_t)kept * n : nullptr;
    const int per = (n + nb - 1) / nb;
    const int lo = blockIdx.x * per, hi = min(n, lo + per);
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const int ci = counts[i];
        double fp = 0.0;
        if (i >= 1 && eel[i] >= kEpsilon) fp = (stat_t(i, ci, alpha, pseudoC, totc, eel, mw) / s1 / denom) * 1e9 / eel[i];
        const double c = (double)ci;
        pme_c[i] += c;
        pve_c[i] += c * c;
        pme_fpkm[i] += fp;
        pme_tpm[i] += (i >= 1) ? fp / denom2 * 1e6 : 0.0;
        if (cv) cv[i] = ci;
    }
}

// squared per-group count sums (genes, or transcripts over alleles): grid (ceil(m/256), chains)
__global__ void k_gibbs_group_stats(int32_t m, const int32_t* __restrict__ grp, const int32_t* __restrict__ counts_base,
                                    uint64_t stride_c, int chain0, const int32_t* __restrict__ nsamples, int kept,
                                    double* acc_base) {
    const int chain = chain0 + blockIdx.y;
    if (kept >= nsamples[chain]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t* counts = counts_base + (uint64_t)chain * stride_c;
    double c = 0.0;
    for (int j = grp[i]; j < grp[i + 1]; j++) c += (double)counts[j];
    acc_base[(uint64_t)chain * m + i] += c * c;
}

// per-chain state for the start of a run
__global__ void k_reset_chains(int32_t M, const int32_t* __restrict__ init_counts, int32_t n0, int32_t* counts_base,
                               uint64_t stride_c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= M) counts_base[(uint64_t)blockIdx.y * stride_c + i] = init_counts[i] + (i == 0 ? n0 : 0);
}

// out[i] = sum over chains, in chain order (release(), Gibbs.cpp:372-388)
__global__ void k_sum_chains(uint64_t n, int nchains, uint64_t stride, const double* __restrict__ acc_base, double* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < nchains; c++) s += acc_base[(uint64_t)c * stride + i];
    out[i] = s;
}

void host_mt_seed(MtState& g, uint32_t seed) {  // boost::random::mt19937 seeding
    g.mt[0] = seed;
    for (int i = 1; i < 624; i++) g.mt[i] = 1812433253u * (g.mt[i - 1] ^ (g.mt[i - 1] >> 30)) + (uint32_t)i;
    g.idx = 624;
}

uint32_t host_mt_next(MtState& g) {
    if (g.idx >= 624) {
        for (int k = 0; k < 624; k++) {
            uint32_t y = (g.mt[k] & 0x80000000u) | (g.mt[(k + 1) % 624] & 0x7fffffffu);
            g.mt[k] = g.mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        g.idx = 0;
    }
    uint32_t y = g.mt[g.idx++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

}  // namespace

struct rsem_gibbs_ctx {
    int device = 0;
    int32_t M = 0, m = 0;
    uint64_t N1 = 0, nitems = 0, nhits = 0, N0 = 0;
    double pseudoC = 1.0, totc = 0.0;
    hipStream_t stream = nullptr;
    int n_cus = 256;
    rsem_comm* comm = nullptr;  // not owned: chain sums are reduced to rank 0 when set
    // items exactly as given (noise column inline): EXACT mode
    uint64_t* d_irp = nullptr;
    int32_t* d_isid = nullptr;
    double* d_icp = nullptr;
    uint32_t n_tiles = 0;
    std::vector<uint32_t> h_tiles;       // first read of every tile (+ N1), gx_build_tiles; host: the windows of k_gibbs_exact_team
    std::vector<uint64_t> h_tile_items;  // ... and its first item (row_ptr[h_tiles[t]])            are cut from them per team size
    int team_W = 0;                      // the team size d_slots was built for (0: none yet)
    void* d_slots = nullptr;             // XSlot[n_win][team_W]
    uint32_t n_win = 0;
    // PARALLEL mode, built on the device at its first use: noise split out + the sliced layout
    bool have_parallel = false;
    uint64_t* d_row_ptr = nullptr;
    int32_t* d_sid = nullptr;
    double* d_cp = nullptr;
    double* d_ncp = nullptr;
    SellLayout L;
    double* d_scp = nullptr;
    double* d_sncp = nullptr;
    Unit* d_units = nullptr;
    std::vector<Unit> h_units;  // host copy of d_units (rsem_gibbs_debug_units)
    uint32_t n_units = 0;
    double* d_g = nullptr;
    // shared by all chains
    int32_t* d_init_counts = nullptr;
    double* d_alpha = nullptr;
    double* d_eel = nullptr;
    double* d_mw = nullptr;
    int32_t* d_grp = nullptr;
    // allele-specific: transcript groups over alleles
    int32_t m_trans = 0;
    int32_t* d_ta = nullptr;
    std::vector<double> last_pve_c_trans;
};

namespace {

// device memory / events released on every exit path of a run
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T* as() const { return (T*)p; }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 8)); }
};
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// noise column (sid 0) of every read summed into ncp, the other items counted: thread per read
__global__ void k_split_count(uint64_t N1, int32_t M, const uint64_t* __restrict__ irp, const int32_t* __restrict__ isid,
                              const double* __restrict__ icp, uint64_t* nh, double* ncp, int* err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N1) return;
    const uint64_t fr = irp[i], to = irp[i + 1];
    if (to <= fr) { *err = (to < fr) ? 1 : 3; nh[i] = 0; ncp[i] = 0.0; return; }
    uint64_t n = 0;
    double nc = 0.0;
    for (uint64_t j = fr; j < to; j++) {
        const int s = isid[j];
        if (s < 0 || s > M) { *err = 2; continue; }
        if (s == 0) nc += icp[j];
        else ++n;
    }
    nh[i] = n;
    ncp[i] = nc;
}

__global__ void k_split_fill(uint64_t N1, const uint64_t* __restrict__ irp, const int32_t* __restrict__ isid,
                             const double* __restrict__ icp, const uint64_t* __restrict__ rp, int32_t* sid, double* cp) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N1) return;
    uint64_t o = rp[i];
    for (uint64_t j = irp[i]; j < irp[i + 1]; j++) {
        const int s = isid[j];
        if (s > 0) { sid[o] = s; cp[o] = icp[j]; ++o; }
    }
}

// items CSR sanity (the EXACT kernels index counts[] with these ids): thread per read
__global__ void k_check_items(uint64_t N1, int32_t M, const uint64_t* __restrict__ irp, const int32_t* __restrict__ isid, int* err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N1) return;
    const uint64_t fr = irp[i], to = irp[i + 1];
    if (to < fr) { *err = 1; return; }
    if (to == fr) { *err = 3; return; }
    for (uint64_t j = fr; j < to; j++)
        if (isid[j] < 0 || isid[j] > M) *err = 2;
}

int items_error(int code) {
    rsem::set_last_error(code == 1 ? "row_ptr is not monotone" : code == 2 ? "sid outside 0..M" : "a read without any item cannot be sampled");
    return RSEM_ERR_INVALID;
}

// PARALLEL mode's structures, all built on the device from the items CSR
int ensure_parallel_layout(rsem_gibbs_ctx* c) {
    if (c->have_parallel) return RSEM_OK;
    uint32_t forced_T = 0;  // measurement / test knob: slices per block (0: chosen from the size of the input, sell_build)
    if (const char* e = getenv("RSEM_GIBBS_LAYOUT_T")) {
        // (4..256 only: the layout itself never chooses T < 8, and T < 4 takes unit paths that no test runs the sampler on.
        // Anything else is an error, not silently the default.)
        char* end = nullptr;
        const unsigned long v = strtoul(e, &end, 10);
        RSEM_REQUIRE(end != e && *end == '\0' && v >= 4 && v <= 256, "RSEM_GIBBS_LAYOUT_T must be a whole number in 4..256");
        forced_T = (uint32_t)v;
    }
    hipStream_t st = c->stream;
    const uint64_t N1 = c->N1;
    DevBuf nh, err, tmp;
    RSEM_HIP_TRY(nh.alloc(sizeof(uint64_t) * (N1 + 1)));
    RSEM_HIP_TRY(err.alloc(sizeof(int)));
    RSEM_HIP_TRY(hipMemsetAsync(err.p, 0, sizeof(int), st));
    RSEM_HIP_TRY(hipMemsetAsync(nh.p, 0, sizeof(uint64_t) * (N1 + 1), st));
    RSEM_HIP_TRY(dmalloc(&c->d_row_ptr, N1 + 1));
    RSEM_HIP_TRY(dmalloc(&c->d_ncp, N1));
    if (N1) {
        hipLaunchKernelGGL(k_split_count, dim3(rsem::ceil_div(N1, kBlock)), dim3(kBlock), 0, st, N1, c->M, c->d_irp, c->d_isid, c->d_icp,
                           nh.as<uint64_t>(), c->d_ncp, err.as<int>());
        RSEM_HIP_TRY(hipGetLastError());
    }
    size_t tb = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, nh.as<uint64_t>(), c->d_row_ptr, N1 + 1, st));
    RSEM_HIP_TRY(tmp.alloc(tb));
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, nh.as<uint64_t>(), c->d_row_ptr, N1 + 1, st));
    uint64_t nhits = 0;
    int h_err = 0;
    RSEM_HIP_TRY(hipMemcpyAsync(&nhits, c->d_row_ptr + N1, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(&h_err, err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (h_err) return items_error(h_err);
    c->nhits = nhits;
    RSEM_HIP_TRY(dmalloc(&c->d_sid, nhits));
    RSEM_HIP_TRY(dmalloc(&c->d_cp, nhits));
    if (N1) {
        hipLaunchKernelGGL(k_split_fill, dim3(rsem::ceil_div(N1, kBlock)), dim3(kBlock), 0, st, N1, c->d_irp, c->d_isid, c->d_icp,
                           c->d_row_ptr, c->d_sid, c->d_cp);
        RSEM_HIP_TRY(hipGetLastError());
    }
    std::vector<Unit> units;
    int rc = sell_build_refined(c->L, st, N1, c->M, c->d_row_ptr, c->d_sid, (uint32_t)c->n_cus * 4 * 6 * 5 / 2, forced_T, nullptr, 0, kGWindow, units,
                                &c->d_units);  // (Unit::pad[0]: ids outside the unit's window)
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(dmalloc(&c->d_scp, c->L.n_planes * 64));
    RSEM_HIP_TRY(dmalloc(&c->d_sncp, (size_t)c->L.n_slots));
    rc = sell_fill_values(c->L, st, c->d_row_ptr, c->d_cp, c->d_ncp, c->d_scp, c->d_sncp);
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    c->n_units = (uint32_t)units.size();
    c->h_units = units;
    RSEM_HIP_TRY(dmalloc(&c->d_g, (size_t)c->M + 1));
    if (c->L.n_long_rows == 0) {  // the split CSR was only needed to build the slices
        hipFree(c->d_sid); hipFree(c->d_cp); hipFree(c->d_row_ptr); hipFree(c->d_ncp);
        c->d_sid = nullptr; c->d_cp = nullptr; c->d_row_ptr = nullptr; c->d_ncp = nullptr;
    }
    c->have_parallel = true;
    return RSEM_OK;
}

// grp / ta: the starts of consecutive groups over the ids 1..M.  k_gibbs_group_stats walks counts[] from one start to the next, so
// an array that does not run from 1 to M + 1 without ever decreasing would make it read outside the count vector.
int check_group_starts(int32_t M, int32_t n, const int32_t* starts, const char* what) {
    bool ok = starts[0] == 1 && starts[n] == M + 1;
    for (int32_t i = 0; ok && i < n; i++) ok = starts[i] <= starts[i + 1];
    if (!ok) {
        rsem::set_last_error("%s must start at 1, end at M + 1 and never decrease", what);
        return RSEM_ERR_INVALID;
    }
    return RSEM_OK;
}

constexpr int kMaxTeamDevices = 64;
std::atomic<int> g_team_busy[kMaxTeamDevices];  // team runs in flight per device (zero-initialised)

}  // namespace

extern "C" {

int rsem_gibbs_chain_seeds(uint32_t seed, int nchains, uint32_t* out) {
    RSEM_REQUIRE(out && nchains >= 0, "bad argument");
    MtState g;
    host_mt_seed(g, seed);
    int n = 0;
    while (n < nchains) {  // sampling.h:26-38: skip seeds already handed out
        uint32_t s = host_mt_next(g);
        bool dup = false;
        for (int i = 0; i < n; i++) if (out[i] == s) { dup = true; break; }
        if (!dup) out[n++] = s;
    }
    return RSEM_OK;
}

int rsem_gibbs_destroy(rsem_gibbs_ctx* c) {
    if (!c) return RSEM_OK;
    (void)hipSetDevice(c->device);
    hipFree(c->d_irp); hipFree(c->d_isid); hipFree(c->d_icp); hipFree(c->d_slots); hipFree(c->d_row_ptr); hipFree(c->d_sid);
    hipFree(c->d_cp); hipFree(c->d_ncp); sell_free(c->L); hipFree(c->d_scp); hipFree(c->d_sncp);
    hipFree(c->d_init_counts); hipFree(c->d_g); hipFree(c->d_alpha);
    hipFree(c->d_eel); hipFree(c->d_mw); hipFree(c->d_grp);
    hipFree(c->d_units); hipFree(c->d_ta);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RSEM_OK;
}

int rsem_gibbs_set_allele_groups(rsem_gibbs_ctx* c, int32_t m_trans, const int32_t* ta) {
    RSEM_REQUIRE(c && ta && m_trans >= 1, "bad argument");
    if (int rc = check_group_starts(c->M, m_trans, ta, "ta (the transcripts' first alleles)")) return rc;
    RSEM_HIP_TRY(hipSetDevice(c->device));
    hipFree(c->d_ta);
    c->d_ta = nullptr;
    c->m_trans = 0;
    RSEM_HIP_TRY(dmalloc(&c->d_ta, (size_t)m_trans + 1));
    RSEM_HIP_TRY(hipMemcpy(c->d_ta, ta, sizeof(int32_t) * ((size_t)m_trans + 1), hipMemcpyHostToDevice));
    c->m_trans = m_trans;
    return RSEM_OK;
}

int rsem_gibbs_get_pve_c_trans(rsem_gibbs_ctx* c, double* out) {
    RSEM_REQUIRE(c && out, "NULL argument");
    if (!c->m_trans || (int32_t)c->last_pve_c_trans.size() != c->m_trans) {
        rsem::set_last_error("allele groups were never set, or no chain has run since");
        return RSEM_ERR_STATE;
    }
    memcpy(out, c->last_pve_c_trans.data(), sizeof(double) * c->m_trans);
    return RSEM_OK;
}

int rsem_gibbs_set_comm(rsem_gibbs_ctx* c, rsem_comm* comm) {
    RSEM_REQUIRE(c != nullptr, "NULL argument");
    c->comm = comm;
    return RSEM_OK;
}

int rsem_gibbs_debug_order(rsem_gibbs_ctx* c, uint32_t* order, uint8_t* lg, uint32_t* n_sell_rows) {
    RSEM_REQUIRE(c && order && lg && n_sell_rows, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_parallel_layout(c);
    if (rc != RSEM_OK) return rc;
    const SellLayout& L = c->L;
    RSEM_REQUIRE((uint64_t)L.n_sell_rows + L.n_long_rows == c->N1, "the layout does not hold every read");
    if (c->N1) {
        RSEM_HIP_TRY(hipMemcpyAsync(order, L.d_order, sizeof(uint32_t) * c->N1, hipMemcpyDeviceToHost, c->stream));
        RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (uint64_t p = 0; p < c->N1; p++) lg[p] = RSEM_GIBBS_ORDER_LONG;
    for (int s = 0; s < L.n_shapes; s++) {
        const Shape& S = L.h_shapes[s];
        for (uint64_t p = S.row_base; p < (uint64_t)S.row_base + S.n_rows && p < L.n_sell_rows; p++) lg[p] = (uint8_t)S.lg;
    }
    *n_sell_rows = L.n_sell_rows;
    return RSEM_OK;
}

int rsem_gibbs_debug_units(rsem_gibbs_ctx* c, uint32_t* T, uint32_t* n_units_io, uint32_t* out) {
    RSEM_REQUIRE(c && T && n_units_io, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_parallel_layout(c);
    if (rc != RSEM_OK) return rc;
    *T = c->L.T;
    const uint32_t cap = *n_units_io;
    *n_units_io = (uint32_t)c->h_units.size();
    if (!out) return RSEM_OK;
    RSEM_REQUIRE(cap >= c->h_units.size(), "out holds fewer units than the layout has");
    for (size_t u = 0; u < c->h_units.size(); u++) {
        const Unit& U = c->h_units[u];
        uint32_t* o = out + 6 * u;
        o[0] = U.slice_begin; o[1] = U.n_slices; o[2] = U.per_wave; o[3] = U.pad[0] != 0; o[4] = (uint32_t)U.S.lg; o[5] = (uint32_t)U.S.K;
    }
    return RSEM_OK;
}

int rsem_gibbs_debug_unit_windows(rsem_gibbs_ctx* c, uint32_t* n_units_io, int32_t* out) {
    RSEM_REQUIRE(c && n_units_io, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_parallel_layout(c);
    if (rc != RSEM_OK) return rc;
    const uint32_t cap = *n_units_io;
    *n_units_io = (uint32_t)c->h_units.size();
    if (!out) return RSEM_OK;
    RSEM_REQUIRE(cap >= c->h_units.size(), "out holds fewer units than the layout has");
    for (size_t u = 0; u < c->h_units.size(); u++) {
        out[2 * u] = c->h_units[u].base;
        out[2 * u + 1] = c->h_units[u].span;
    }
    return RSEM_OK;
}

int rsem_gibbs_create(rsem_gibbs_ctx** out, int device, int32_t M, uint64_t N1, uint64_t nitems, const uint64_t* row_ptr,
                      const int32_t* sid, const double* conprb, const int32_t* init_counts, const double* alpha,
                      double pseudoC, double totc, uint64_t N0, const double* eel, const double* mw, int32_t m,
                      const int32_t* grp) {
    RSEM_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RSEM_REQUIRE(M >= 1 && m >= 1, "M and m must be >= 1");
    RSEM_REQUIRE(row_ptr && sid && conprb && init_counts && eel && mw && grp, "NULL argument");
    RSEM_REQUIRE(N1 < 0xfffffff0ull, "N1 too large for one chain context");
    RSEM_REQUIRE(row_ptr[0] == 0 && row_ptr[N1] == nitems, "row_ptr[0] != 0 or row_ptr[N1] != nitems");
    RSEM_REQUIRE(N0 < 0x7fffffffull, "N0 does not fit the reference's int counts");
    if (int rc = check_group_starts(M, m, grp, "grp (the genes' first transcripts)")) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        rsem::set_last_error("no HIP device %d (have %d)", device, ndev);
        return RSEM_ERR_NODEVICE;
    }
    RSEM_HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    RSEM_HIP_TRY(hipGetDeviceProperties(&prop, device));
    rsem_gibbs_ctx* c = new (std::nothrow) rsem_gibbs_ctx();
    if (!c) return RSEM_ERR_NOMEM;
    c->device = device; c->M = M; c->m = m; c->N1 = N1; c->nitems = nitems; c->N0 = N0;
    c->pseudoC = pseudoC; c->totc = totc;
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
#define G_TRY(expr)                                                                                     \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            rsem::set_last_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));  \
            rsem_gibbs_destroy(c);                                                                      \
            return _e == hipErrorOutOfMemory ? RSEM_ERR_NOMEM : RSEM_ERR_HIP;                           \
        }                                                                                               \
    } while (0)
    G_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    hipStream_t st = c->stream;
    const size_t nM = (size_t)M + 1;
    G_TRY(dmalloc(&c->d_irp, N1 + 1)); G_TRY(dmalloc(&c->d_isid, nitems)); G_TRY(dmalloc(&c->d_icp, nitems));
    G_TRY(dmalloc(&c->d_init_counts, nM)); G_TRY(dmalloc(&c->d_eel, nM)); G_TRY(dmalloc(&c->d_mw, nM));
    G_TRY(dmalloc(&c->d_grp, (size_t)m + 1));
    G_TRY(hipMemcpyAsync(c->d_irp, row_ptr, sizeof(uint64_t) * (N1 + 1), hipMemcpyHostToDevice, st));
    if (nitems) {
        G_TRY(hipMemcpyAsync(c->d_isid, sid, sizeof(int32_t) * nitems, hipMemcpyHostToDevice, st));
        G_TRY(hipMemcpyAsync(c->d_icp, conprb, sizeof(double) * nitems, hipMemcpyHostToDevice, st));
    }
    G_TRY(hipMemcpyAsync(c->d_init_counts, init_counts, sizeof(int32_t) * nM, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(c->d_eel, eel, sizeof(double) * nM, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(c->d_mw, mw, sizeof(double) * nM, hipMemcpyHostToDevice, st));
    G_TRY(hipMemcpyAsync(c->d_grp, grp, sizeof(int32_t) * ((size_t)m + 1), hipMemcpyHostToDevice, st));
    if (alpha) {
        G_TRY(dmalloc(&c->d_alpha, nM));
        G_TRY(hipMemcpyAsync(c->d_alpha, alpha, sizeof(double) * nM, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> tiles;  // (outlives the asynchronous copy: the stream is synchronised below)
    for (uint64_t i = 0; i < N1; i++)
        if (row_ptr[i + 1] < row_ptr[i]) {
            rsem::set_last_error("row_ptr decreases at read %llu", (unsigned long long)i);
            rsem_gibbs_destroy(c);
            return RSEM_ERR_INVALID;
        }
    uint64_t soft_cap = 0;  // measurement knob: tiles closed at fewer items than LDS holds (gx_build_tiles)
    if (const char* e = getenv("RSEM_GX_TILE_ITEMS")) soft_cap = strtoull(e, nullptr, 10);
    if (alpha) gx_prior::gx_build_tiles(N1, row_ptr, tiles, soft_cap);  // (--prior: tiles of 3072 items)
    else gx_build_tiles(N1, row_ptr, tiles, soft_cap);
    c->n_tiles = (uint32_t)tiles.size() - 1;
    std::vector<uint64_t> tile_items(tiles.size());
    for (size_t i = 0; i < tiles.size(); i++) tile_items[i] = row_ptr[tiles[i]];
    c->h_tiles = tiles;
    c->h_tile_items = tile_items;
    // the ids index counts[] on the device: check them there (the host copy is not walked)
    int* d_err = nullptr;
    int h_err = 0;
    G_TRY(dmalloc(&d_err, 1));
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(int), st);
    if (e == hipSuccess && N1) {
        hipLaunchKernelGGL(k_check_items, dim3(rsem::ceil_div(N1, kBlock)), dim3(kBlock), 0, st, N1, M, c->d_irp, c->d_isid, d_err);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_err);
    G_TRY(e);
#undef G_TRY
    if (h_err) { rsem_gibbs_destroy(c); return items_error(h_err); }
    *out = c;
    return RSEM_OK;
}

int rsem_gibbs_run_chains(rsem_gibbs_ctx* c, int mode, int nchains, const uint32_t* seeds, int burnin, const int32_t* nsamples,
                          int gap, int thin, int32_t* const* count_vectors, double* pme_c, double* pve_c, double* pme_tpm,
                          double* pme_fpkm, double* pve_c_genes, double* pve_c_trans, rsem_gibbs_profile* prof) {
    RSEM_REQUIRE(c && seeds && nsamples && pme_c && pve_c && pme_tpm && pme_fpkm && pve_c_genes, "NULL argument");
    RSEM_REQUIRE(mode == RSEM_GIBBS_EXACT || mode == RSEM_GIBBS_PARALLEL, "unknown mode");
    RSEM_REQUIRE(nchains >= 1 && nchains <= 65535, "nchains out of range");
    RSEM_REQUIRE(burnin >= 0 && gap >= 1, "bad chain parameters");
    int max_ns = 0;
    uint64_t cv_total = 0;
    std::vector<uint64_t> cv_off(nchains, 0);
    std::vector<int32_t> last_round(nchains, 0);
    for (int k = 0; k < nchains; k++) {
        RSEM_REQUIRE(nsamples[k] >= 1, "every chain must keep at least one sample");
        max_ns = std::max(max_ns, (int)nsamples[k]);
        cv_off[k] = cv_total;
        cv_total += (uint64_t)nsamples[k] * ((uint64_t)c->M + 1);
        last_round[k] = burnin + 1 + (nsamples[k] - 1) * gap;
    }
    if (thin < 1) thin = 1;
    RSEM_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (mode == RSEM_GIBBS_PARALLEL) {
        int rc = ensure_parallel_layout(c);
        if (rc != RSEM_OK) return rc;
    }
    const size_t nM = (size_t)c->M + 1;
    const int gM = rsem::ceil_div(nM, kBlock);
    const uint64_t stride_c = nM, stride_z = c->N1;
    const bool exact = mode == RSEM_GIBBS_EXACT;
    const size_t m = (size_t)c->m, mt = (size_t)c->m_trans;
    // per-chain state; out = [pme_c | pve_c | pme_tpm | pme_fpkm | pve_c_genes | pve_c_trans] summed over the chains
    const size_t n_out = 4 * nM + m + mt;
    DevBuf counts, z, mts, acc, acc_g, acc_t, partials, d_ns, d_last, d_cvoff, cv, outb;
    RSEM_HIP_TRY(counts.alloc(sizeof(int32_t) * nM * nchains));
    if (exact) RSEM_HIP_TRY(z.alloc(sizeof(int32_t) * c->N1 * nchains));
    if (exact) RSEM_HIP_TRY(mts.alloc(sizeof(MtState) * nchains * 2));  // (two buffers: see k_gibbs_exact_team)
    RSEM_HIP_TRY(acc.alloc(sizeof(double) * 4 * nM * nchains));
    RSEM_HIP_TRY(acc_g.alloc(sizeof(double) * m * nchains));
    RSEM_HIP_TRY(acc_t.alloc(sizeof(double) * mt * nchains));
    RSEM_HIP_TRY(partials.alloc(sizeof(double) * 3 * kStatMaxBlocks * nchains));
    RSEM_HIP_TRY(d_ns.alloc(sizeof(int32_t) * nchains));
    RSEM_HIP_TRY(d_last.alloc(sizeof(int32_t) * nchains));
    RSEM_HIP_TRY(d_cvoff.alloc(sizeof(uint64_t) * nchains));
    RSEM_HIP_TRY(outb.alloc(sizeof(double) * n_out));
    if (count_vectors) RSEM_HIP_TRY(cv.alloc(sizeof(int32_t) * cv_total));
    EventPair ev;
    RSEM_HIP_TRY(hipEventCreate(&ev.a));
    RSEM_HIP_TRY(hipEventCreate(&ev.b));
    RSEM_HIP_TRY(hipMemsetAsync(acc.p, 0, sizeof(double) * 4 * nM * nchains, st));
    RSEM_HIP_TRY(hipMemsetAsync(acc_g.p, 0, sizeof(double) * m * nchains, st));
    if (mt) RSEM_HIP_TRY(hipMemsetAsync(acc_t.p, 0, sizeof(double) * mt * nchains, st));
    RSEM_HIP_TRY(hipMemcpyAsync(d_ns.p, nsamples, sizeof(int32_t) * nchains, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(d_last.p, last_round.data(), sizeof(int32_t) * nchains, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(d_cvoff.p, cv_off.data(), sizeof(uint64_t) * nchains, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_reset_chains, dim3(gM, nchains), dim3(kBlock), 0, st, c->M, c->d_init_counts, (int32_t)c->N0,
                       counts.as<int32_t>(), stride_c);
    RSEM_HIP_TRY(hipGetLastError());
    const int nblk = std::max(1, std::min(kStatMaxBlocks, rsem::ceil_div(nM, 2048)));

    // statistics of the `kept`-th sample of chains [chain0, chain0 + n)
    auto keep_sample = [&](int kept, int chain0, int n) -> int {
        hipLaunchKernelGGL(k_gibbs_stats_a, dim3(nblk, n), dim3(kBlock), 0, st, c->M, counts.as<int32_t>(), stride_c, chain0,
                           d_ns.as<int32_t>(), kept, c->d_alpha, c->pseudoC, c->totc, c->d_eel, c->d_mw, partials.as<double>());
        hipLaunchKernelGGL(k_gibbs_stats_b, dim3(nblk, n), dim3(kBlock), 0, st, c->M, counts.as<int32_t>(), stride_c, chain0,
                           d_ns.as<int32_t>(), kept, c->d_alpha, c->pseudoC, c->totc, c->d_eel, c->d_mw, partials.as<double>(),
                           acc.as<double>(), count_vectors ? cv.as<int32_t>() : nullptr, d_cvoff.as<uint64_t>());
        hipLaunchKernelGGL(k_gibbs_group_stats, dim3(rsem::ceil_div(m, kBlock), n), dim3(kBlock), 0, st, c->m, c->d_grp,
                           counts.as<int32_t>(), stride_c, chain0, d_ns.as<int32_t>(), kept, acc_g.as<double>());
        if (mt)
            hipLaunchKernelGGL(k_gibbs_group_stats, dim3(rsem::ceil_div(mt, kBlock), n), dim3(kBlock), 0, st, c->m_trans, c->d_ta,
                               counts.as<int32_t>(), stride_c, chain0, d_ns.as<int32_t>(), kept, acc_t.as<double>());
        RSEM_HIP_TRY(hipGetLastError());
        return RSEM_OK;
    };

    long long sweeps = 0;
    int team_used = 0;  // EXACT: workgroups per chain
    RSEM_HIP_TRY(hipEventRecord(ev.a, st));
    // EXACT.  force_one: one workgroup per chain whatever the device has to spare.  aborted: a team gave up at a barrier (a workgroup
    // of it was not running: another tenant's kernels held the compute units) -- nothing of the run is kept.
    auto exact_run = [&](bool force_one, bool& aborted) -> int {
        // all chains advance together, a team of workgroups each (Gibbs.cpp:207-254: the reference's threads)
        std::vector<MtState> h(nchains);
        for (int k = 0; k < nchains; k++) host_mt_seed(h[k], seeds[k]);
        RSEM_HIP_TRY(hipMemcpyAsync(mts.p, h.data(), sizeof(MtState) * nchains, hipMemcpyHostToDevice, st));
        DevBuf prof_buf;  // RSEM_GX_PROFILE builds: the workgroup kernel's phase cycles
        RSEM_HIP_TRY(prof_buf.alloc(16 * sizeof(unsigned long long)));
        RSEM_HIP_TRY(hipMemsetAsync(prof_buf.p, 0, 16 * sizeof(unsigned long long), st));
        // The team kernel: W workgroups per chain (gibbs_exact_team.hpp) when the device has compute units to spare for them --
        // W = compute units / chains of this call, at most kXTeamMax; RSEM_GX_TEAM=<W> overrules (1: one workgroup per chain).
        // A cooperative launch: the team barrier needs every workgroup resident, and the runtime refuses a grid that is not.
        // One team run per device and process at a time: two cooperative grids that each want every compute unit cannot both be
        // resident (contexts of two host threads sharing a GPU -- the LOCAL communicator of the tests -- take one workgroup per
        // chain for whichever comes second).
        // ... and per device across the processes of this host: an advisory lock on a file named after the GPU's PCI address, held for
        // the run (released by close, also when the process dies).  Best effort: where the file cannot be made the run goes ahead.
        struct TeamLease {
            int dev = -1, fd = -1;
            bool mine = false;
            hipStream_t st = nullptr;
            void take(int d, hipStream_t stream) {
                if (d < 0 || d >= kMaxTeamDevices) return;
                dev = d;
                st = stream;
                mine = g_team_busy[d].fetch_add(1) == 0;
                if (!mine) { g_team_busy[d].fetch_sub(1); return; }
                char bus[64] = {0};
                if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, d) != hipSuccess) { (void)hipGetLastError(); return; }
                for (char* q = bus; *q; ++q) if (*q == ':' || *q == '.' || *q == '/') *q = '_';
                const std::string path = std::string("/tmp/rsem_hip_team_") + bus + ".lock";
                // Whoever makes the file opens it to every user of the host (the umask is not asked); a user who may not write it --
                // another user's file from before this rule, or a sticky /tmp with fs.protected_regular -- locks it through a
                // read-only descriptor (flock does not care).  Never through a link somebody planted.
                fd = ::open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
                if (fd >= 0) (void)::fchmod(fd, 0666);
                else if (errno == EACCES || errno == EPERM || errno == EROFS) fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC | O_NOFOLLOW);
                // no descriptor: nobody can tell whether another process runs its teams on this GPU -- one workgroup per chain, which
                // always makes progress; same when the lock is taken
                if (fd < 0 || ::flock(fd, LOCK_EX | LOCK_NB) != 0) drop();
            }
            void drop() {  // (also as soon as the run turns out to use one workgroup per chain: the next context need not)
                if (fd >= 0) ::close(fd);
                fd = -1;
                if (mine) g_team_busy[dev].fetch_sub(1);
                mine = false;
            }
            ~TeamLease() {
                // an error path may leave team launches queued: they must have left the GPU before the next team run is let in
                if (mine && st) (void)hipStreamSynchronize(st);
                drop();
            }
        } lease;
        const bool prior = c->d_alpha != nullptr;  // --prior: the pass of the two headers compiled in namespace gx_prior
        int W = 1;
        const bool oversubscribe = getenv("RSEM_GX_TEST_OVERSUBSCRIBE") != nullptr;  // tests/test_gibbs_gpu.py: a team that CANNOT be resident
        if (!force_one) lease.take(c->device, st);
        if (lease.mine) {
            W = std::max(1, std::min(kXTeamMax, c->n_cus / std::max(1, nchains)));
            if (W < 8) W = 1;  // with every compute unit busy, teams of 4 advance a chain no faster than one workgroup (profiles/r05b_c3_64chains.log)
            if (const char* e = getenv("RSEM_GX_TEAM")) W = std::max(1, std::min(kXTeamMax, atoi(e)));
            W = (int)std::min<uint64_t>((uint64_t)W, std::max<uint64_t>(1, c->n_tiles));
            int coop = 0, per_cu = 0;
            (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device);
            hipError_t oe = prior ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gx_prior::k_gibbs_exact_team<false>, kXThr, 0)
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_gibbs_exact_team<false>, kXThr, 0);
            if (oe != hipSuccess) per_cu = 0;
            (void)hipGetLastError();
            if (!coop || per_cu < 1) W = 1;
            else if (!oversubscribe) W = std::min(W, std::max(1, per_cu * c->n_cus / std::max(1, nchains)));
        }
        if (W == 1) lease.drop();
        DevBuf t_ctl, t_net, t_gnet, t_ref;
        TeamArgs ta{};  // (the same bytes for either pass: see the static_asserts behind the includes)
        {
            if (c->team_W != W) {  // the windows of this team size (W = 1: a window per tile)
                std::vector<unsigned char> bytes;
                size_t n_slots;
                if (prior) {
                    std::vector<gx_prior::XSlot> slots;
                    gx_prior::gx_build_windows(W, c->h_tiles, c->h_tile_items, slots);
                    n_slots = slots.size();
                    bytes.assign((const unsigned char*)slots.data(), (const unsigned char*)slots.data() + sizeof(gx_prior::XSlot) * n_slots);
                } else {
                    std::vector<XSlot> slots;
                    gx_build_windows(W, c->h_tiles, c->h_tile_items, slots);
                    n_slots = slots.size();
                    bytes.assign((const unsigned char*)slots.data(), (const unsigned char*)slots.data() + sizeof(XSlot) * n_slots);
                }
                if (c->d_slots) { (void)hipFree(c->d_slots); c->d_slots = nullptr; }
                RSEM_HIP_TRY(hipMalloc(&c->d_slots, std::max<size_t>(bytes.size(), 8)));
                RSEM_HIP_TRY(hipMemcpy(c->d_slots, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
                c->n_win = (uint32_t)(n_slots / (size_t)W);
                c->team_W = W;
            }
            ta.W = W;
            ta.nchains = nchains;
            ta.nw = (uint32_t)(((W + 15) / 16) * 16 / 2);
            ta.slots = (const XSlot*)c->d_slots;
            ta.n_win = c->n_win;
            ta.N1 = c->N1;
            ta.M = c->M;
            if (const char* e = getenv("RSEM_GX_SPIN_LIMIT")) ta.spin_limit = strtoull(e, nullptr, 10);  // ticks of 10 ns; tests
        }
        if (W > 1) {  // what the workgroups of a team tell each other through
            const size_t rows = 2 * ((size_t)c->M + 2);  // (both copies of each table: XTeam)
            RSEM_HIP_TRY(t_ctl.alloc(sizeof(XTeamCtl) * nchains));
            RSEM_HIP_TRY(t_net.alloc(sizeof(uint32_t) * rows * ta.nw * nchains));
            RSEM_HIP_TRY(t_gnet.alloc(sizeof(uint32_t) * rows * 2 * nchains));
            RSEM_HIP_TRY(t_ref.alloc(sizeof(int32_t) * rows * nchains));
            RSEM_HIP_TRY(hipMemsetAsync(t_ctl.p, 0, sizeof(XTeamCtl) * nchains, st));
            RSEM_HIP_TRY(hipMemsetAsync(t_net.p, 0x80, sizeof(uint32_t) * rows * ta.nw * nchains, st));  // every cell at kXBias
            RSEM_HIP_TRY(hipMemsetAsync(t_gnet.p, 0x80, sizeof(uint32_t) * rows * 2 * nchains, st));
            RSEM_HIP_TRY(hipMemsetAsync(t_ref.p, 0, sizeof(int32_t) * rows * nchains, st));
            ta.ctl = t_ctl.as<XTeamCtl>();
            ta.net = t_net.as<uint32_t>();
            ta.gnet = t_gnet.as<uint32_t>();
            ta.ref = t_ref.as<int32_t>();
            if (getenv("RSEM_GX_VERBOSE")) fprintf(stderr, "[gibbs exact] teams of %d workgroups per chain, %u windows per sweep\n", W, c->n_win);
        }
        team_used = W;
        int mt_flip = 0;  // which half of mts holds the chains' generators
        hipError_t team_err = hipSuccess;
        auto sweep_team = [&](bool init, int round) {
            const uint64_t* a_rp = c->d_irp;
            const int32_t* a_sid = c->d_isid;
            const double* a_cp = c->d_icp;
            int32_t* a_counts = counts.as<int32_t>();
            int32_t* a_z = z.as<int32_t>();
            double a_pc = c->pseudoC;
            const double* a_alpha = c->d_alpha;
            const MtState* a_in = mts.as<MtState>() + (size_t)mt_flip * nchains;
            MtState* a_out = mts.as<MtState>() + (size_t)(mt_flip ^ 1) * nchains;
            const int32_t* a_last = d_last.as<int32_t>();
            int a_round = round;
            uint64_t a_sc = stride_c, a_sz = stride_z;
            unsigned long long* a_prof = (RSEM_GX_PROFILE && !init) ? prof_buf.as<unsigned long long>() : (unsigned long long*)nullptr;
            void* args[] = {&ta, &a_rp, &a_sid, &a_cp, &a_counts, &a_z, &a_pc, &a_alpha, &a_in, &a_out, &a_last, &a_round, &a_sc, &a_sz, &a_prof};
            const void* fn = prior ? (init ? (const void*)gx_prior::k_gibbs_exact_team<true> : (const void*)gx_prior::k_gibbs_exact_team<false>)
                                   : (init ? (const void*)k_gibbs_exact_team<true> : (const void*)k_gibbs_exact_team<false>);
            // a team needs all its workgroups resident: a cooperative launch (the runtime refuses a grid that is not); one workgroup
            // per chain waits for nobody and may be any number of chains
            hipError_t e = W > 1 && !oversubscribe ? hipLaunchCooperativeKernel(fn, dim3((unsigned)(nchains * W)), dim3(kXThr), args, 0, st)
                         : W > 1 ? hipLaunchKernel(fn, dim3((unsigned)(nchains * W)), dim3(kXThr), args, 0, st)
                                 : hipLaunchKernel(fn, dim3((unsigned)nchains), dim3(kXThr), args, 0, st);
            if (e != hipSuccess && team_err == hipSuccess) team_err = e;
            mt_flip ^= 1;
        };
        auto sweep = [&](bool init, int round) { sweep_team(init, round); };
        sweep(true, 0);  // initial state: z_i ~ conprb (Gibbs.cpp:281-291)
        RSEM_HIP_TRY(hipGetLastError());
        RSEM_HIP_TRY(hipStreamSynchronize(st));  // h must outlive the copy
        const int rounds = burnin + 1 + (max_ns - 1) * gap;
        for (int round = 1; round <= rounds; round++) {
            sweep(false, round);
            RSEM_HIP_TRY(hipGetLastError());
            ++sweeps;
            if (round > burnin && (round - burnin - 1) % gap == 0) {
                int rc = keep_sample((round - burnin - 1) / gap, 0, nchains);
                if (rc != RSEM_OK) return rc;
            }
        }
        if (team_err != hipSuccess) {
            rsem::set_last_error("k_gibbs_exact_team: launch of %d x %d workgroups failed: %s", nchains, W, hipGetErrorString(team_err));
            return RSEM_ERR_HIP;
        }
        if (W > 1) {
            std::vector<XTeamCtl> hc(nchains);
            RSEM_HIP_TRY(hipMemcpyAsync(hc.data(), t_ctl.p, sizeof(XTeamCtl) * nchains, hipMemcpyDeviceToHost, st));
            RSEM_HIP_TRY(hipStreamSynchronize(st));
            for (int k = 0; k < nchains; k++)
                if (hc[k].abort) {
                    rsem::set_last_error("k_gibbs_exact_team: chain %d's team of %d workgroups gave up waiting at a team barrier (a workgroup of the team "
                                         "was not running: is another program using GPU %d?)", k, W, c->device);
                    aborted = true;
                    return RSEM_ERR_HIP;
                }
            if (getenv("RSEM_GX_VERBOSE")) {
                unsigned long long nb = 0;
                for (int k = 0; k < nchains; k++) nb += hc[k].epoch;
                fprintf(stderr, "[gibbs exact] %.2f team barriers per window\n", (double)nb / std::max(1.0, (double)nchains * (double)c->n_win * (double)sweeps));
            }
        }
        if (RSEM_GX_PROFILE) {
            unsigned long long h[16];
            RSEM_HIP_TRY(hipMemcpyAsync(h, prof_buf.p, sizeof(h), hipMemcpyDeviceToHost, st));
            RSEM_HIP_TRY(hipStreamSynchronize(st));
            const double tiles = h[7] ? (double)h[7] : 1.0;
            fprintf(stderr, "[gibbs exact team] shader-clock cycles per tile: stage %.0f | own flags %.0f | rng + gather %.0f | first draw %.0f | rounds %.0f (%.2f scans) | "
                            "redraw + clean-up %.0f | publish %.0f | team barrier %.0f | cross look-ups %.0f | commit + barrier %.0f ; phases %.2f ; tiles %.0f\n",
                    h[0] / tiles, h[1] / tiles, h[2] / tiles, h[3] / tiles, h[4] / tiles, h[8] / tiles, h[11] / tiles, h[5] / tiles, h[6] / tiles, h[10] / tiles,
                    h[13] / tiles, h[9] / tiles, tiles);
        }
        return RSEM_OK;
    };
    if (exact) {
        bool aborted = false;
        int rc = exact_run(false, aborted);
        if (rc != RSEM_OK && aborted && !getenv("RSEM_GX_NO_FALLBACK")) {
            // The chain's integers do not depend on the team size: start the run over with one workgroup per chain, which waits
            // for nobody.  (What the teams did is lost; the caller gets the same result, later.)
            fprintf(stderr, "rsem_gibbs_run_chains: %s -- starting the run over with one workgroup per chain\n", rsem_hip_last_error());
            RSEM_HIP_TRY(hipStreamSynchronize(st));
            RSEM_HIP_TRY(hipMemsetAsync(acc.p, 0, sizeof(double) * 4 * nM * nchains, st));
            RSEM_HIP_TRY(hipMemsetAsync(acc_g.p, 0, sizeof(double) * m * nchains, st));
            if (mt) RSEM_HIP_TRY(hipMemsetAsync(acc_t.p, 0, sizeof(double) * mt * nchains, st));
            hipLaunchKernelGGL(k_reset_chains, dim3(gM, nchains), dim3(kBlock), 0, st, c->M, c->d_init_counts, (int32_t)c->N0,
                               counts.as<int32_t>(), stride_c);
            RSEM_HIP_TRY(hipGetLastError());
            sweeps = 0;
            RSEM_HIP_TRY(hipEventRecord(ev.a, st));
            aborted = false;
            rc = exact_run(true, aborted);
        }
        if (rc != RSEM_OK) return rc;
    } else {
        // one chain after the other: a sweep of this sampler fills the GPU by itself
        for (int k = 0; k < nchains; k++) {
            Philox ph{seeds[k], 0x52534547u};  // 'RSEG'
            uint32_t sweep_no = 0;
            int32_t* ck = counts.as<int32_t>() + (size_t)k * stride_c;
            auto parallel_z = [&](uint32_t sw) -> int {
                if (c->n_units)
                    hipLaunchKernelGGL(k_sample_z_lane, dim3(c->n_units), dim3(kBlock), 0, st, c->L.d_shapes, c->d_units, c->L.T, c->M,
                                       c->d_g, c->d_scp, c->L.d_ssid, c->d_sncp, c->L.d_masks, ph, sw, ck
                                       );
                if (c->L.n_long_rows)
                    hipLaunchKernelGGL(k_sample_z_long, dim3(rsem::ceil_div(c->L.n_long_rows, kBlock / 64)), dim3(kBlock), 0, st,
                                       c->L.n_long_rows, c->L.d_order + c->L.n_sell_rows, c->L.n_sell_rows, c->d_row_ptr, c->d_sid,
                                       c->d_cp, c->d_ncp, c->d_g, ph, sw, ck);
                RSEM_HIP_TRY(hipGetLastError());
                return RSEM_OK;
            };
            // initial state: z_i ~ conprb (Gibbs.cpp:281-291) = a z pass with all weights 1
            hipLaunchKernelGGL(k_fill_double, dim3(gM), dim3(kBlock), 0, st, (int32_t)nM, 1.0, c->d_g);
            int rc = parallel_z(sweep_no++);
            if (rc != RSEM_OK) return rc;
            int kept = 0;
            for (int round = 1; round <= last_round[k]; round++) {
                for (int t = 0; t < thin; t++) {
                    hipLaunchKernelGGL(k_sample_theta, dim3(gM), dim3(kBlock), 0, st, c->M, ck, c->d_alpha, c->pseudoC, ph, sweep_no,
                                       c->d_g, c->d_init_counts, (int32_t)c->N0);
                    rc = parallel_z(sweep_no++);
                    if (rc != RSEM_OK) return rc;
                    ++sweeps;
                }
                if (round > burnin && (round - burnin - 1) % gap == 0) {
                    rc = keep_sample(kept++, k, 1);
                    if (rc != RSEM_OK) return rc;
                }
            }
        }
    }
    RSEM_HIP_TRY(hipEventRecord(ev.b, st));
    // release() part 1 (Gibbs.cpp:372-388): the chains' sums, in chain order; across GPUs: one reduce to rank 0
    double* o = outb.as<double>();
    hipLaunchKernelGGL(k_sum_chains, dim3(rsem::ceil_div(4 * nM, kBlock)), dim3(kBlock), 0, st, (uint64_t)(4 * nM), nchains,
                       (uint64_t)(4 * nM), acc.as<double>(), o);
    hipLaunchKernelGGL(k_sum_chains, dim3(rsem::ceil_div(m, kBlock)), dim3(kBlock), 0, st, (uint64_t)m, nchains, (uint64_t)m,
                       acc_g.as<double>(), o + 4 * nM);
    if (mt)
        hipLaunchKernelGGL(k_sum_chains, dim3(rsem::ceil_div(mt, kBlock)), dim3(kBlock), 0, st, (uint64_t)mt, nchains, (uint64_t)mt,
                           acc_t.as<double>(), o + 4 * nM + m);
    RSEM_HIP_TRY(hipGetLastError());
    EventPair evr;
    const bool reduce = rsem::comm_active(c->comm);
    if (reduce) {
        RSEM_HIP_TRY(hipEventCreate(&evr.a));
        RSEM_HIP_TRY(hipEventCreate(&evr.b));
        RSEM_HIP_TRY(hipEventRecord(evr.a, st));
        int rc = rsem::comm_reduce_sum_f64(c->comm, o, n_out, 0, st);
        if (rc != RSEM_OK) return rc;
        RSEM_HIP_TRY(hipEventRecord(evr.b, st));
    }
    RSEM_HIP_TRY(hipMemcpyAsync(pme_c, o, sizeof(double) * nM, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(pve_c, o + nM, sizeof(double) * nM, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(pme_tpm, o + 2 * nM, sizeof(double) * nM, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(pme_fpkm, o + 3 * nM, sizeof(double) * nM, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(pve_c_genes, o + 4 * nM, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    c->last_pve_c_trans.assign(mt, 0.0);
    if (mt) RSEM_HIP_TRY(hipMemcpyAsync(c->last_pve_c_trans.data(), o + 4 * nM + m, sizeof(double) * mt, hipMemcpyDeviceToHost, st));
    if (count_vectors)
        for (int k = 0; k < nchains; k++)
            if (count_vectors[k])
                RSEM_HIP_TRY(hipMemcpyAsync(count_vectors[k], cv.as<int32_t>() + cv_off[k], sizeof(int32_t) * (size_t)nsamples[k] * nM,
                                            hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (mt && pve_c_trans) memcpy(pve_c_trans, c->last_pve_c_trans.data(), sizeof(double) * mt);
    if (prof) {
        float ms = 0.f;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        prof->total_ms = ms;
        prof->sweeps = sweeps;
        prof->sweep_ms = sweeps ? ms / (double)sweeps : 0.0;
        prof->chains = nchains;
        prof->team = team_used;
        prof->reduce_ms = 0.0;
        if (reduce) {
            float rms = 0.f;
            RSEM_HIP_TRY(hipEventElapsedTime(&rms, evr.a, evr.b));
            prof->reduce_ms = rms;
        }
    }
    return RSEM_OK;
}

int rsem_gibbs_run(rsem_gibbs_ctx* c, int mode, uint32_t seed, int burnin, int nsamples, int gap, int thin,
                   int32_t* count_vectors, double* pme_c, double* pve_c, double* pme_tpm, double* pme_fpkm,
                   double* pve_c_genes, double* sweep_ms) {
    RSEM_REQUIRE(nsamples >= 1, "bad chain parameters");
    const int32_t ns = nsamples;
    int32_t* cvs[1] = {count_vectors};
    rsem_gibbs_profile prof;
    int rc = rsem_gibbs_run_chains(c, mode, 1, &seed, burnin, &ns, gap, thin, count_vectors ? cvs : nullptr, pme_c, pve_c, pme_tpm,
                                   pme_fpkm, pve_c_genes, nullptr, &prof);
    if (rc == RSEM_OK && sweep_ms) *sweep_ms = prof.sweep_ms;
    return rc;
}

}  // extern "C"

// rsem_hip_preload (status.hip): the first launch of a translation unit makes the runtime load its code object
namespace { __global__ void k_preload_gibbs() {} }
namespace rsem { void preload_gibbs() { hipLaunchKernelGGL(k_preload_gibbs, dim3(1), dim3(1), 0, nullptr); (void)hipGetLastError(); } }
