// em.hip -- rsem-run-em's E step / M step on MI355X (gfx950).  C ABI: include/rsem_hip.h.
//
// What the reference does per round (EM.cpp:199-236, 385-413): for every read i, f_j =
// theta[sid_j] * conprb_j over its alignments (plus the noise term theta[0] * ncp_i), each clamped
// to 0 below 1e-300; if the row sum is >= 1e-300 the normalised fractions are added to
// counts[sid_j]; then theta = counts / sum(counts) and two convergence statistics.
//
// Device design (this file is the product; the CPU restatement lives in oracle/ and is never
// linked here):
//   * the CSR is uploaded once, then re-laid-out ON THE DEVICE into a "sliced" layout: reads are
//     radix-sorted by (shape, min sid, hash of the sid tuple) so that reads hitting the same
//     transcript set become neighbours, and are packed 64/G to a 64-lane slice with G = 1..64 lanes
//     per read and K <= 4 planes of 64 entries; lane l of plane k holds alignment k*G + (l % G) of
//     read l / G.  Every global load of the hot loop is therefore a fully coalesced 256 B (sid) or
//     512 B (conprb) wave access, whatever the row length (1..256 alignments per read).
//   * per-read normaliser: xor-shuffle reduction over the G lanes of a read;
//   * per-transcript counts (k_estep_lane): inside a block of slices a lane follows consecutive
//     sorted reads; while their sid tuple does not change it keeps the partial counts in registers and
//     skips the sid planes; on a change it spills into a 2048-entry LDS count window, which leaves the
//     workgroup as one device atomic per touched sid;
//   * optional Q32 value planes (rsem_em_set_option "value_bits" 32): 4 B per alignment instead of 8 for
//     the reads that qualify (sell_layout.hpp), the rest stay F64 in shapes of their own;
//   * the noise bin (touched by every read) never sees a per-read atomic: per-lane register, block
//     reduction, one atomic per workgroup into one of kTotSlots slots beside the counts; a second set
//     of slots counts the reads with a non-zero normaliser, so that sum(counts) is known exactly
//     (N0 + that count) without a reduction: ONE totals protocol for every entry point;
//   * M step + convergence statistics run on the device (k_mstep_fast, or the closers inside the
//     lane kernel); no kernel waits on another workgroup; a `done` word set by the last closer to
//     arrive freezes theta at exactly the reference's stopping round while the host only polls it
//     every few rounds (no per-round host sync);
//   * the units of the layout stand in up to three groups (compact / a few ids outside their window / split rows), and the three EM
//     loops of rsem_em_run (kernel sequence, statistics on a second stream, one launch per round) deal them to launches each in its
//     own way: unit_groups.hpp is where that dealing is written down; launch_lane below is the one launch site of the lane kernel.
// MFMA is not used: ~2 flops per 12 bytes, the bound is HBM bandwidth.
#include <climits>
#include <cstdlib>
#include <cmath>
#include <type_traits>

#include "comm_internal.hpp"
#include "em_internal.hpp"
#include "upload.hpp"
#include "sell_layout.hpp"
#include "unit_groups.hpp"

namespace {

using rsem::kEpsilon;
using rsem::LanePlan;
using rsem::Loop;

constexpr int kMaxTimedRounds = 4096;
constexpr int kWindow = 2048;        // doubles of LDS count window per workgroup (16 KB)
static_assert(kWindow == kLayoutWindow, "the layout sorts reads apart and sizes windows for the E step's LDS window (sell_layout.hpp)");

constexpr int kTotSlots = 64;  // addresses per device-wide total (E-step workgroups add round-robin)


// ---- E step ----------------------------------------------------------------------------------

// wave_sum and the per-wave body of the LANE kernel (also run on the CPU by tests/estep_emu.cpp)
#include "estep_block.hpp"
// Ctrl, HostMirror and the closer of a round (also run on the CPU by tests/round_close_emu.cpp)
#include "round_close.hpp"

// the workgroup's share of the two device-wide totals: tot[0] += v (noise fraction), tot[1] += u (reads with a non-zero
// normaliser: an integer count, so its total is exact in any order)
__device__ inline void block_add_totals(double v, double u, double* tot) {
    __shared__ double red3[2 * (kBlock / 64)];
    v = wave_sum(v);
    u = wave_sum(u);
    if ((threadIdx.x & 63) == 0) { red3[threadIdx.x >> 6] = v; red3[kBlock / 64 + (threadIdx.x >> 6)] = u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, tu = 0.0;
        for (int i = 0; i < kBlock / 64; i++) { t += red3[i]; tu += red3[kBlock / 64 + i]; }
        const int slot = blockIdx.x & (kTotSlots - 1);  // kTotSlots addresses per total: a single hot address serialises the whole launch behind it
        if (t != 0.0) unsafeAtomicAdd(&tot[slot], t);
        if (tu != 0.0) unsafeAtomicAdd(&tot[kTotSlots + slot], tu);
    }
}

// The reads the sliced layout does not take (more than 256 alignments: a Trinity-shaped tail), a WAVE per read: the lanes stride
// over the read's alignments (coalesced 4- and 8-byte loads), the normaliser is a wave sum, the fractions go to counts[] by
// atomics.  Until round 5 these reads went through k_estep_csr, a thread per read: ONE read of 2 000 alignments walked by one
// thread is 2 000 dependent round trips -- 100 such reads among 10 M took the E step of configs[1] from 0.12 to 1.99 ms
// (profiles/r05z_long_rows.log).  Summation order within a read differs from the thread's (a tree over lanes), like the lane
// kernel's.
__global__ __launch_bounds__(kBlock) void k_estep_long(uint64_t n_rows, const uint32_t* __restrict__ row_list, const uint64_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ sid, const double* __restrict__ cp, const double* __restrict__ ncp,
                                                        const double* __restrict__ theta, double* counts, const Ctrl* ctrl, double* totals) {
    if (ctrl && ctrl->done) return;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    double noise = 0.0, neff = 0.0;
    const double th0 = theta[0];
    for (uint64_t t = wave; t < n_rows; t += n_waves) {  // (wave-uniform)
        const uint64_t i = row_list[t];
        const uint64_t fr = row_ptr[i], to = row_ptr[i + 1];
        double f0 = th0 * ncp[i];
        if (f0 < kEpsilon) f0 = 0.0;
        double part = 0.0;
        for (uint64_t j = fr + lane; j < to; j += 64) {
            double f = theta[sid[j]] * cp[j];
            if (f < kEpsilon) f = 0.0;
            part += f;
        }
        const double sum = wave_sum(part) + f0;
        if (sum >= kEpsilon) {
            if (lane == 0) { noise += f0 / sum; neff += 1.0; }
            for (uint64_t j = fr + lane; j < to; j += 64) {  // (the read's lines are in the L2 from the first pass)
                const int s = sid[j];
                double f = theta[s] * cp[j];
                if (f < kEpsilon) f = 0.0;
                f /= sum;
                if (f != 0.0) unsafeAtomicAdd(&counts[s], f);
            }
        }
    }
    block_add_totals(noise, neff, totals);
}

// Posterior weight of every alignment in file order (calcExpectedWeights, EM.cpp:237-243): w[j] = f_j / sum_i and
// w_noise[i]; rows whose normaliser is < 1e-300 get zeros.  Thread per read over the caller's CSR, no atomics: the
// counts of the same round come from the main E-step kernel, this pass only serves the consumers that need the
// weights themselves (the model statistics of rounds 1-10, the transcript BAM).
__global__ __launch_bounds__(kBlock) void k_weights_csr(uint64_t N1, const uint64_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ sid, const double* __restrict__ cp,
                                                         const double* __restrict__ ncp, const double* __restrict__ theta,
                                                         double* __restrict__ w, double* __restrict__ w_noise) {
    const double th0 = theta[0];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N1; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t fr = row_ptr[i], to = row_ptr[i + 1];
        double f0 = th0 * ncp[i];
        if (f0 < kEpsilon) f0 = 0.0;
        double sum = f0;
        for (uint64_t j = fr; j < to; j++) {
            double f = theta[sid[j]] * cp[j];
            if (f < kEpsilon) f = 0.0;
            sum += f;
        }
        const bool ok = sum >= kEpsilon;
        w_noise[i] = ok ? f0 / sum : 0.0;
        for (uint64_t j = fr; j < to; j++) {
            double f = theta[sid[j]] * cp[j];
            if (f < kEpsilon) f = 0.0;
            w[j] = ok ? f / sum : 0.0;
        }
    }
}

// segmented sum of v over lanes {g, g+G, g+2G, ...} keyed by `key`; returns true on the tail lane
// of each run, whose v then holds the run total.
__device__ inline bool seg_reduce(int key, double& v, int lane, int lg) {
    const int G = 1 << lg;
    int kprev = __shfl_up(key, G);
    int knext = __shfl_down(key, G);
    int flag = (lane < G) || (kprev != key);
    for (int d = G; d < 64; d <<= 1) {
        if (__ballot(!flag) == 0ull) break;  // every lane has reached the head of its run: the remaining steps would add nothing
        double ov = __shfl_up(v, d);
        int of = __shfl_up(flag, d);
        if (lane >= d && !flag) { v += ov; flag = of; }
    }
    return (lane + G >= 64) || (knext != key);
}

// ---- split rows: the two passes around the lane kernel (sell_layout.hpp: sell_build_far) ----------------------------------------
// Before: the far part of every split read's normaliser, sum over its far alignments of theta[sid] * conprb (each clamped
// like every term of EM.cpp:212-219).  Thread per read: a split read has a handful of far alignments.
constexpr int kRowsumCap = 512;  // far entries of a wave's 64 row slots staged in LDS (4 KB per wave: room for 32 waves per CU); beyond that the slots walk global memory
template <bool kBatched>
__global__ __launch_bounds__(kBlock) void k_far_rowsum(uint32_t n_xs, const uint64_t* __restrict__ far_ptr, const int32_t* __restrict__ far_sid,
                                                        const double* __restrict__ far_cp, const double* __restrict__ theta, double* __restrict__ extra,
                                                        const Ctrl* ctrl) {
    if (ctrl->done) return;
    // A wave = 64 consecutive row slots = one contiguous run of far entries (they are kept in slot order).  The run is read
    // with coalesced loads -- lane i takes entries i, i + 64, ... --, every entry's term theta[sid] * conprb (clamped like
    // every term of EM.cpp:212-219) goes to LDS, and each lane then adds up its own slot's terms from there.  (With every
    // lane reading its own slot's entries straight from global memory the loads of a wave were 48 bytes apart: 0.29 ms for
    // 37 M entries at configs[1]'s size, profiles/r04g_call.log.)
    // kBatched: the wave issues the loads of 4 x 64 entries, then their 4 x 64 theta gathers, then writes the terms -- two
    // dependent trips to memory per 256 entries instead of two per 64 --, and waits for nobody but itself: its LDS row is its
    // own, and the LDS serves a wave's instructions in order.
    __shared__ double s_term[kBlock / 64][kRowsumCap];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t xs = blockIdx.x * blockDim.x + threadIdx.x;  // row slot - x_slot_base
    const bool in = xs < n_xs;
    const uint64_t e0 = far_ptr[in ? xs : n_xs], e1 = far_ptr[in ? xs + 1 : n_xs];
    const uint64_t E0 = __shfl(e0, 0), E1 = __shfl(e1, 63);
    const uint64_t n = E1 - E0;
    const bool staged = n <= (uint64_t)kRowsumCap;
    if (staged) {
        if (kBatched) {
            constexpr int kB = 4;
            for (uint32_t k0 = 0; k0 < (uint32_t)n; k0 += 64 * kB) {  // (uniform over the wave)
                int sd[kB];
                double cv[kB], th[kB];
#pragma unroll
                for (int u = 0; u < kB; u++) {
                    // (an entry past the end reads the last one instead: a load under a condition becomes a branch and a
                    // wait per load)
                    const uint32_t k = min(k0 + (uint32_t)(u * 64 + lane), (uint32_t)n - 1u);
                    sd[u] = far_sid[E0 + k];
                    cv[u] = stream_load(&far_cp[E0 + k]);
                }
#pragma unroll
                for (int u = 0; u < kB; u++) th[u] = theta[sd[u]];
#pragma unroll
                for (int u = 0; u < kB; u++) {
                    const uint32_t k = min(k0 + (uint32_t)(u * 64 + lane), (uint32_t)n - 1u);  // (past the end: the last entry's own term once more)
                    double f = th[u] * cv[u];
                    if (f < kEpsilon) f = 0.0;
                    s_term[w][k] = f;
                }
            }
        } else {
            for (uint64_t k = (uint64_t)lane; k < n; k += 64) {
                double f = theta[far_sid[E0 + k]] * stream_load(&far_cp[E0 + k]);
                if (f < kEpsilon) f = 0.0;
                s_term[w][k] = f;
            }
        }
    }
    if (kBatched) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
    if (!in) return;
    double sum = 0.0;
    if (staged) {
        for (uint64_t e = e0; e < e1; e++) sum += s_term[w][e - E0];
    } else {
        for (uint64_t e = e0; e < e1; e++) {
            double f = theta[far_sid[e]] * far_cp[e];
            if (f < kEpsilon) f = 0.0;
            sum += f;
        }
    }
    extra[xs] = sum;
}
// After: the far alignments' fractions, theta[sid] * conprb / normaliser of their read (inv[], left by the lane kernel), added
// to counts[sid] in transcript order: consecutive entries of one id are summed by a segmented shuffle reduction, one atomic
// per id and wave -- the transposed (CSC) pass instead of a global atomic per alignment.  A wave takes 4 x 64 consecutive
// entries per step and issues all their loads, then all their gathers, before it reduces.
// kXcd: workgroup b runs on XCD b % 8 (observed, MI355X_MICROARCH.md "Workgroup dispatch"; only speed depends on it), so the
// workgroups are renumbered to give every XCD one contiguous eighth of the entries: the block of row slots whose reciprocals
// its waves gather is then in ONE L2 at a time instead of every block in flight in all eight.
template <bool kXcd>
__global__ __launch_bounds__(kBlock) void k_far_colsum(uint64_t n_far, const int32_t* __restrict__ csc_sid, const double* __restrict__ csc_cp,
                                                        const uint32_t* __restrict__ csc_slot, uint32_t slot_base, const double* __restrict__ theta,
                                                        const double* __restrict__ inv, double* counts, const Ctrl* ctrl) {
    if (ctrl->done) return;
    const int lane = threadIdx.x & 63;
    uint32_t wg = blockIdx.x;
    if (kXcd) {
        const uint32_t x = blockIdx.x & 7, i = blockIdx.x >> 3, q = gridDim.x >> 3, r = gridDim.x & 7;
        wg = x * q + (x < r ? x : r) + i;  // XCD x takes workgroups [x q + min(x, r), ...): q + (x < r) of them
    }
    const uint64_t wave = ((uint64_t)wg * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    constexpr int kU = 4;
    for (uint64_t b = wave * (64 * kU); b < n_far; b += n_waves * (64 * kU)) {  // (uniform over the wave)
        int key[kU], past[kU];
        double cv[kU];
        uint32_t sl[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            // (an entry past the end reads the last one instead and is keyed -1: a load under a condition becomes a branch and
            // a wait per load)
            const uint64_t i = b + (uint64_t)(u * 64 + lane), ic = i < n_far ? i : n_far - 1;
            past[u] = -(int)(i >= n_far);
            key[u] = csc_sid[ic];
            cv[u] = stream_load(&csc_cp[ic]);
            sl[u] = csc_slot[ic];
        }
        __builtin_amdgcn_sched_barrier(0);  // (every load above is issued before the first one is waited for)
#pragma unroll
        for (int u = 0; u < kU; u++) key[u] |= past[u];
        double th[kU], iv[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {
            th[u] = theta[key[u] > 0 ? key[u] : 0];
            iv[u] = inv[sl[u] - slot_base];
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            double f = th[u] * cv[u];
            if (f < kEpsilon) f = 0.0;
            double v = key[u] > 0 ? f * iv[u] : 0.0;
            const bool tail = seg_reduce(key[u], v, lane, 0);
            if (tail && key[u] > 0 && v != 0.0) unsafeAtomicAdd(&counts[key[u]], v);
        }
    }
}

// (k_estep_lane below; its per-wave body is estep_block.hpp, included above.)
// The one-kernel round (kSolo, rsem_em_run's default loop): besides their E-step work for round r, some workgroups close
// a slice of round r-1 -- convergence statistics of theta_{r-1} (buffer `theta`) against theta_{r-2} (buffer `prev`),
// EM.cpp:400-416 -- and clears that slice of `prev`, which is the buffer round r+1 accumulates into.  The last closer
// to arrive applies the stop rule, writes the round's line to the host mirror and clears prev's totals (every other
// closer has read them by then).  No M-step kernel, no second stream: a round IS this launch.
struct SoloArgs {
    double* prev = nullptr;     // [counts | totals] of round r-2
    Ctrl* ctrl = nullptr;
    HostMirror* mirror = nullptr;
    int stat_round = 0;         // r-1, or 0 when there is no finished round to close yet
    int min_round = 0, max_round = 0;
};

// Closing is latency (dependent trips to memory, one returning atomic on a word every closer hits), not bandwidth.
// Measured: done at the END of every workgroup it kept the workgroup's LDS and wave slots idle for that long and cost
// 18 % (configs[2]) to 90 % (configs[1]) of the E step; done by 1024 neighbouring workgroups their ~2000 same-line
// atomics queued up behind each other (+40 us on either config).  So: kCloseMax workgroups spread evenly over the
// launch order close a slice each in their PROLOGUE, the whole workgroup taking part, one pair of atomics per closer.
constexpr int kCloseMax = 128;
__device__ inline void solo_close_round(const SoloArgs& A, int M, double N0, const double* __restrict__ cur, CloseScratch* scratch) {
    const int n_close = min((int)gridDim.x, kCloseMax);
    const int stride = (int)gridDim.x / n_close;
    const int rel = (int)blockIdx.x - stride / 2;
    if (rel < 0 || rel % stride != 0 || rel / stride >= n_close) return;  // (uniform over the workgroup)
    const int me = rel / stride;
    const int lane = threadIdx.x & 63;
    const int n = M + 1;
    const int per = (n + n_close - 1) / n_close;
    SliceWalk walk;
    walk.load(me * per, min(n, me * per + per), kBlock, cur, A.prev);
    const double extra_c = wave_sum(cur[n + lane]) + N0, sum_c = wave_sum(cur[n + kTotSlots + lane]) + N0;
    const double extra_p = wave_sum(A.prev[n + lane]) + N0, sum_p = wave_sum(A.prev[n + kTotSlots + lane]) + N0;
    CloseAcc acc;
    walk.each(cur, A.prev, [&](int i, double craw, double praw) {
        const double c = craw + (i == 0 ? extra_c : 0.0);
        A.prev[i] = 0.0;
        acc.add(c, c / sum_c, (praw + (i == 0 ? extra_p : 0.0)) / sum_p);
    });
    close_reduce(acc, scratch);
    if (threadIdx.x == 0 && close_arrive(A.ctrl, A.mirror, me, n_close, acc, A.stat_round, A.min_round, A.max_round))
        for (int k = 0; k < 2 * kTotSlots; k++) A.prev[n + k] = 0.0;  // the last closer: every other one has read them
}

// theta and counts of the round the one-kernel loop stopped at, from the buffer that round accumulated (EM.cpp:392-398)
__global__ __launch_bounds__(kBlock) void k_solo_finish(int32_t M, double N0, const double* __restrict__ buf, double* theta, double* counts_last) {
    const int n = M + 1;
    const int lane = threadIdx.x & 63;
    const double extra0 = wave_sum(buf[n + lane]) + N0, sum = wave_sum(buf[n + kTotSlots + lane]) + N0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double c = buf[i] + (i == 0 ? extra0 : 0.0);
        counts_last[i] = c;
        theta[i] = c / sum;
    }
}

// kFC: `theta` holds the previous round's raw counts, tsrc its totals (see ThetaSrc)
#ifndef RSEM_FQ_DEPTH
#define RSEM_FQ_DEPTH 3
#endif
constexpr int kFarQDepth = RSEM_FQ_DEPTH;  // register sets of the far-queue loop: loads two slices ahead, theta of far ids one slice ahead
// kFQ: the launch over the units with ids outside their window (Unit::pad[0]; unit_groups.hpp deals them to a launch of their own): partial
// counts for such ids queue up in LDS per wave (FarQueue, estep_block.hpp) -- 18 KB more per workgroup, three workgroups per CU
// instead of four, which is why the compact units are not launched with it.
template <bool kFC, bool kSolo = false, bool kFQ = false>
__global__ __launch_bounds__(kBlock) void k_estep_lane(
    const Shape* __restrict__ shapes, const Unit* __restrict__ units, uint32_t T, int M,
    const double* __restrict__ theta, const double* __restrict__ tsrc, double N0, const unsigned char* __restrict__ sval,
    const int16_t* __restrict__ sexp, const int32_t* __restrict__ ssid, const double* __restrict__ sncp,
    const unsigned long long* __restrict__ masks, double* counts, double* totals, const Ctrl* ctrl,
    unsigned long long* trace, SoloArgs solo = SoloArgs(), XArgs xa = XArgs(), StartList sl = StartList()) {
    if (ctrl->done) return;
    if (trace && threadIdx.x == 0) trace[2 * blockIdx.x] = wall_clock64();  // rsem_em_debug_trace only
    __shared__ double th_win[kWindow];
    __shared__ double cnt_win[kWindow];
    __shared__ int fq_sid[kFQ ? (kBlock / 64) * kFarQCap : 1];
    __shared__ double fq_val[kFQ ? (kBlock / 64) * kFarQCap : 1];
    __shared__ int fq_n[kBlock / 64];
    const Unit U = units[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave index, as a scalar
    FarQueue fq;
    if (kFQ) {
        fq.sid = fq_sid + w * kFarQCap;
        fq.val = fq_val + w * kFarQCap;
        fq.n = fq_n + w;
        if (lane == 0) fq_n[w] = 0;
    }
    __shared__ CloseScratch close_lds;
    if (kSolo && solo.stat_round > 0) solo_close_round(solo, M, N0, theta, &close_lds);
    double noise = 0.0, neff = 0.0;
    {
        const Shape& G = U.S;
        Shape S;
        S.plane_base = G.plane_base;
        S.slice_base = G.slice_base;
        S.n_slices = G.n_slices;
        S.row_base = 0;
        S.n_rows = 0;
        S.slot_base = G.slot_base;
        S.K = G.K;
        S.lg = G.lg;
        S.fmt = G.fmt;
        S.val_base = G.val_base;
        S.cut = G.cut;
        S.reserved = 0;
        const uint32_t u_end = S.slice_base + U.slice_begin + U.n_slices;
        const uint32_t s_begin = S.slice_base + U.slice_begin + (uint32_t)w * U.per_wave;
        const uint32_t s_end = min(u_end, s_begin + U.per_wave);
#define RSEM_ESTEP_BLOCK(KK, QQ, FF, XX) \
    estep_block<KK, kFC, QQ, (QQ ? kQ32Depth[KK - 1] : kF64Depth[KK - 1]), FF, XX>(S, s_begin, s_end, lane, U.base, U.span, theta, tsrc, N0, th_win, cnt_win, sval, sexp, ssid, sncp, masks, counts, noise, neff, M, xa, FarQueue(), sl)
        // (uniform over the workgroup)  split rows (F64X) only exist where theta is a plain array: the loops that read theta
        // out of the previous round's counts (kFC) are not taken for a layout with split rows (loop_wanted)
#define RSEM_ESTEP_BLOCK_FQ(KK, QQ, XX) \
    estep_block<KK, kFC, QQ, kFarQDepth, true, XX, true>(S, s_begin, s_end, lane, U.base, U.span, theta, tsrc, N0, th_win, cnt_win, sval, sexp, ssid, sncp, masks, counts, noise, neff, M, xa, fq)
        const int code = (S.K - 1) | ((S.fmt == kFmtQ32 ? 1 : 0) << 2) | ((U.pad[0] != 0 ? 1 : 0) << 3) | (((!kFC && S.fmt == kFmtF64X) ? 1 : 0) << 4);
        if constexpr (kFQ) {
            // (every unit of this launch takes the loop with the far path and the queue: a unit without ids outside never uses either)
            if (s_begin < u_end) switch ((code & 7) | ((code >> 4) << 3)) {
                case 0: RSEM_ESTEP_BLOCK_FQ(1, false, false); break;
                case 1: RSEM_ESTEP_BLOCK_FQ(2, false, false); break;
                case 2: RSEM_ESTEP_BLOCK_FQ(3, false, false); break;
                case 3: RSEM_ESTEP_BLOCK_FQ(4, false, false); break;
                case 4: RSEM_ESTEP_BLOCK_FQ(1, true, false); break;
                case 5: RSEM_ESTEP_BLOCK_FQ(2, true, false); break;
                case 6: RSEM_ESTEP_BLOCK_FQ(3, true, false); break;
                case 7: RSEM_ESTEP_BLOCK_FQ(4, true, false); break;
                default:
                    if constexpr (!kFC) switch (code & 3) {
                        case 0: RSEM_ESTEP_BLOCK_FQ(1, false, true); break;
                        case 1: RSEM_ESTEP_BLOCK_FQ(2, false, true); break;
                        case 2: RSEM_ESTEP_BLOCK_FQ(3, false, true); break;
                        default: RSEM_ESTEP_BLOCK_FQ(4, false, true); break;
                    }
                    break;
            } else {
                const ThetaSrc th = theta_src<kFC>(theta, tsrc, N0, lane);
                stage_windows<kFC>(U.base, U.span, M, th, th_win, cnt_win);
            }
        } else
        if (s_begin < u_end) switch (code) {
            case 0: RSEM_ESTEP_BLOCK(1, false, false, false); break;
            case 1: RSEM_ESTEP_BLOCK(2, false, false, false); break;
            case 2: RSEM_ESTEP_BLOCK(3, false, false, false); break;
            case 3: RSEM_ESTEP_BLOCK(4, false, false, false); break;
            case 4: RSEM_ESTEP_BLOCK(1, true, false, false); break;
            case 5: RSEM_ESTEP_BLOCK(2, true, false, false); break;
            case 6: RSEM_ESTEP_BLOCK(3, true, false, false); break;
            case 7: RSEM_ESTEP_BLOCK(4, true, false, false); break;
            case 8: RSEM_ESTEP_BLOCK(1, false, true, false); break;
            case 9: RSEM_ESTEP_BLOCK(2, false, true, false); break;
            case 10: RSEM_ESTEP_BLOCK(3, false, true, false); break;
            case 11: RSEM_ESTEP_BLOCK(4, false, true, false); break;
            case 12: RSEM_ESTEP_BLOCK(1, true, true, false); break;
            case 13: RSEM_ESTEP_BLOCK(2, true, true, false); break;
            case 14: RSEM_ESTEP_BLOCK(3, true, true, false); break;
            case 15: RSEM_ESTEP_BLOCK(4, true, true, false); break;
            default:
                if constexpr (!kFC) switch (code & 11) {
                    case 0: RSEM_ESTEP_BLOCK(1, false, false, true); break;
                    case 1: RSEM_ESTEP_BLOCK(2, false, false, true); break;
                    case 2: RSEM_ESTEP_BLOCK(3, false, false, true); break;
                    case 3: RSEM_ESTEP_BLOCK(4, false, false, true); break;
                    case 8: RSEM_ESTEP_BLOCK(1, false, true, true); break;
                    case 9: RSEM_ESTEP_BLOCK(2, false, true, true); break;
                    case 10: RSEM_ESTEP_BLOCK(3, false, true, true); break;
                    default: RSEM_ESTEP_BLOCK(4, false, true, true); break;
                }
                break;
#undef RSEM_ESTEP_BLOCK
#undef RSEM_ESTEP_BLOCK_FQ
        } else {
            const ThetaSrc th = theta_src<kFC>(theta, tsrc, N0, lane);
            stage_windows<kFC>(U.base, U.span, M, th, th_win, cnt_win);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < U.span; i += blockDim.x) {
        const double v = cnt_win[i];
        if (v != 0.0) unsafeAtomicAdd(&counts[U.base + i], v);
    }
    block_add_totals(noise, neff, totals);
    if (trace && threadIdx.x == 0) trace[2 * blockIdx.x + 1] = wall_clock64();
}

// ---- M step ----------------------------------------------------------------------------------

constexpr int kMstepBlocks = 64;  // workgroups of k_mstep_fast at the most (mstep_fast_grid)
static_assert(kCloseMax <= kSumSlots && kMstepBlocks <= kSumSlots, "every closer has a slot for its share of the sum");

// M step without a grid-wide reduction.  Every read whose normaliser is >= EPSILON contributes fractions that sum to
// one, so sum(counts) (EM.cpp:395) = N0 + (number of such reads), which the E-step workgroups count on the side
// (one atomic per E-step workgroup into one of kTotSlots slots; exact, the addends are integers), like the noise
// fraction (a second set of slots).  No reduction, no barrier before theta = counts / sum.
// kFused (the fused loop of rsem_em_run): counts / totals of this round are LEFT IN PLACE -- the next E step reads theta
// out of them (ThetaSrc) and is already running beside this kernel -- and the buffer that round r-1 left (`spent`,
// counts then totals, read for the last time by this round's E step) is cleared for round r+2 instead.
template <bool kFused>
__global__ __launch_bounds__(kBlock) void k_mstep_fast(int32_t M, double N0, double* counts, double* totals,
                                                        const double* __restrict__ theta_old, double* theta_new,
                                                        double* counts_last, Ctrl* ctrl, int round, int min_round, int max_round,
                                                        HostMirror* mirror, double* spent) {
    if (ctrl->done) return;
    const int n = M + 1;
    const int nb = gridDim.x;
    const int per = (n + nb - 1) / nb;
    const int lo = blockIdx.x * per, hi = min(n, lo + per);
    // wave 0: lanes 0..63 fetch the slots of both totals (fixed summation order)
    __shared__ double s_totals[2];
    if (threadIdx.x < 64) {
        double a = __hip_atomic_load(&totals[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double b = __hip_atomic_load(&totals[kTotSlots + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = wave_sum(a);
        b = wave_sum(b);
        if (threadIdx.x == 0) { s_totals[0] = a; s_totals[1] = b; }
    }
    // this workgroup's slice of counts / theta_old is requested first, so it arrives while the partials are reduced
    SliceWalk walk;
    walk.load(lo, hi, (int)blockDim.x, counts, theta_old);
    __shared__ CloseScratch close_lds;
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = 0;
    __syncthreads();
    const double extra0 = s_totals[0] + N0;  // counts[0] += noise + N0 (EM.cpp:392)
    const double sum = s_totals[1] + N0;
    CloseAcc acc;
    if (kFused && blockIdx.x == 0 && threadIdx.x < 2 * kTotSlots) spent[n + threadIdx.x] = 0.0;
    walk.each(counts, theta_old, [&](int i, double craw, double old) {
        const double c = craw + (i == 0 ? extra0 : 0.0);
        const double th = c / sum;
        theta_new[i] = th;
        counts_last[i] = c;
        if (kFused) spent[i] = 0.0;
        else counts[i] = 0.0;
        acc.add(c, th, old);
    });
    close_reduce(acc, &close_lds);
    // (the slots' floating-point sum of the counts is for the ROUND line only: theta divides by the exact `sum` above)
    if (threadIdx.x == 0 && close_arrive(ctrl, mirror, (int)blockIdx.x, nb, acc, round, min_round, max_round)) s_last = 1;
    __syncthreads();
    // the last workgroup to arrive clears the totals for the next round: every workgroup has read them by now
    if (!kFused && s_last && threadIdx.x < 2 * kTotSlots) __hip_atomic_store(&totals[threadIdx.x], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ---- ctx -------------------------------------------------------------------------------------

struct rsem_em_ctx {
    int device = 0;
    int32_t M = 0;
    uint64_t N1 = 0, nnz = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    // caller-order CSR
    uint64_t* d_row_ptr = nullptr;
    int32_t* d_sid = nullptr;
    double* d_cp = nullptr;
    double* d_ncp = nullptr;
    bool have_values = false;
    // sliced layout
    SellLayout L;
    unsigned char* d_sval = nullptr;  // value planes: F64 or Q32 per shape (sell_layout.hpp)
    double* d_sncp = nullptr;
    int16_t* d_sexp = nullptr;        // per-slot exponents of the Q32 reads (only with value_bits = 32)
    int* d_fill_err = nullptr;
    int value_bits = 64;              // 64: every read F64; 32: Q32 where a read qualifies
    int value_range_bits = 8;         // a read qualifies when its non-zero values span less than 2^this
    int short_last_plane = 1;         // reads whose last value plane is a quarter or more empty take a short class (sell_shape.hpp: Shape::cut)
    int short_min_units = kShortClassMinUnits;  // ... where the class fills this many units (short_classes_worth_it)
    int sid_start_list = 1;           // the launches without far queue take a new tuple's ids from the start list (sell_layout.hpp); 0: from the id planes
    SidTraffic sid_traffic;           // what those launches then load of ids (partition_units: it follows the unit table)
    bool layout_has_q32 = false;      // the current layout was built with Q32 shapes (from the then-current values)
    bool layout_ok = false;           // false between free_layout and a build_layout that went through (a failed rebuild)
    // the lane kernel's work list (dealt to its launches by unit_groups.hpp)
    Unit* d_units = nullptr;
    std::vector<Unit> h_units;
    uint64_t long_nnz = 0;  // alignments of the reads left in the CSR
    uint32_t* d_rank = nullptr;  // caller row -> sorted row (inverse of L.d_order), built on first use (em_planes_view)
    double *d_xextra = nullptr, *d_xinv = nullptr;  // split rows: far part of the normaliser / its reciprocal, per row slot from L.x_slot_base
    int split_rows = 1;          // lay reads with ids outside their window out as split rows (option "split_rows")
    int split_policy = 1;        // 1: the reads that are mostly outside their window split; 2: every read with an id outside
    uint32_t n_far_units = 0;               // units with an id outside their LDS window (Unit::pad[0])
    unsigned long long n_stray_reads = 0;   // reads the second layout pass sorted apart (sell_build_refined)
    int tune_passes_left = 1;               // measured-lifetime reordering of the units, done on first use
    uint32_t n_units = 0;
    // Split rows: the units of the F64X shapes stand behind the others in d_units, [n_units_main, n_units), and run BESIDE them -- on
    // stream_x: k_far_rowsum -> their lane launch -> k_far_colsum, a chain of passes bound by the L2's request rate and by their own
    // round trips, while the compact units stream from HBM on the context's stream (launch_estep).
    uint32_t n_units_main = 0;
    // ... and inside [0, n_units_main) the units with ids outside their window stand behind the compact ones, [n_units_compact,
    // n_units_main): they are launched with the far-queue instantiation (k_estep_lane<.., kFQ = true>), beside the compact units on
    // stream_x.  far_queue = 0 (option / RSEM_HIP_FAR_QUEUE=0): one launch over all of them as until round 5.
    uint32_t n_units_compact = 0;
    uint32_t n_units_queued = 0;  // main units that qualify for the far-queue launch, whether or not it is taken (partition_units)
    int far_queue = 1;
    hipStream_t stream_x = nullptr;
    hipEvent_t ev_x_fork = nullptr, ev_x_join = nullptr;
    int x_overlap = 0;            // (measured: +4 % on configs[2] with 10 % cross-gene reads split, -4 % at configs[1]'s size without genes)
    // EM state
    double* d_theta[2] = {nullptr, nullptr};
    double* d_red3 = nullptr;     // three buffers of [counts (M+1) | totals (2 * kTotSlots)] (the fused loop rotates them)
    double* d_red = nullptr;      // = d_red3: [counts | totals] in one buffer, so that one all-reduce covers both
    double* d_counts = nullptr;   // = d_red
    double* d_counts_last = nullptr;
    double* d_totals = nullptr;   // = d_red + M + 1: kTotSlots slots of the noise fraction, then of the reads with a non-zero normaliser
    double* d_w = nullptr;        // expected-weights scratch (nnz), lazily allocated
    double* d_wn = nullptr;
    Ctrl* d_ctrl = nullptr;
    int grid_long = 0;
    uint32_t forced_T = 0;
    int check_every = 64;
    int n_cus = 256;
    std::vector<hipEvent_t> events;
    HostMirror* mirror = nullptr;  // pinned host memory, written by the M-step kernel
    hipEvent_t lag_ev[2] = {nullptr, nullptr};
    hipStream_t stream2 = nullptr;  // fused loop: the statistics kernel of round r runs here, beside the E step of round r+1
    hipEvent_t ev_e[4] = {nullptr, nullptr, nullptr, nullptr}, ev_s[4] = {nullptr, nullptr, nullptr, nullptr};
    rsem_comm* comm = nullptr;     // not owned; rows sharded over its ranks when set
    // Option "release_csr": d_sid / d_cp (12 bytes per alignment, the caller-order half of the device memory) are freed while only
    // the theta-only rounds run -- they stream the sliced layout alone -- and read back from the planes (k_unfill_sell, the same
    // doubles) by whatever needs them next: the weights pass, new values, a rebuild of the layout, a model context's view.
    bool csr_released = false;
    int views_out = 0;             // model contexts holding d_sid / d_cp (em_device_view .. em_view_release)
    rsem_em_progress_fn progress = nullptr;
    void* progress_user = nullptr;
};

namespace {

// (field by field: a copy of a Unit need not keep the 4 padding bytes in front of its Shape)
bool same_unit(const Unit& a, const Unit& b) {
    return a.shape == b.shape && a.slice_begin == b.slice_begin && a.n_slices == b.n_slices && a.per_wave == b.per_wave && a.base == b.base &&
           a.span == b.span && a.pad[0] == b.pad[0] && a.pad[1] == b.pad[1] && !memcmp(&a.S, &b.S, sizeof(Shape));
}

// The unit table in the three groups of unit_groups.hpp: the units of the split rows' shapes behind all the others, and the queued
// main units behind the compact ones where they get a launch of their own (every part keeps its order); host and device copy.
int partition_units(rsem_em_ctx* c) {
    auto is_main = [](const Unit& u) { return u.S.fmt != kFmtF64X; };
    const auto mid = std::stable_partition(c->h_units.begin(), c->h_units.end(), is_main);
    c->n_units_main = (uint32_t)(mid - c->h_units.begin());
    auto queued = [](const Unit& u) { return rsem::unit_queued(u.pad[0], u.pad[1], u.n_slices); };
    c->n_units_queued = (uint32_t)std::count_if(c->h_units.begin(), mid, queued);
    c->n_units_compact = c->n_units_main;
    if (rsem::far_group_adopted(c->far_queue != 0, c->n_units_queued, c->n_units_main))
        c->n_units_compact = (uint32_t)(std::stable_partition(c->h_units.begin(), mid, [&](const Unit& u) { return !queued(u); }) - c->h_units.begin());
    // the device copy follows every time, so that a unit's index means the same unit on both sides (tune_unit_order reads the
    // trace in device order)
    if (c->n_units)
        RSEM_HIP_TRY(hipMemcpyAsync(c->d_units, c->h_units.data(), sizeof(Unit) * c->n_units, hipMemcpyHostToDevice, c->stream));
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    c->sid_traffic = SidTraffic();
    if (c->L.d_start_list) {
        const bool far = c->far_queue != 0 && c->n_units_compact < c->n_units_main;  // (the far-queue launch of the PLAIN loop: unit_groups.hpp)
        return sell_count_sid_traffic(c->L, c->d_units, c->n_units, far ? c->n_units_compact : 0u, far ? c->n_units_main : 0u, c->stream, c->sid_traffic);
    }
    return RSEM_OK;
}

// the start list as the launches are handed it: none for the far-queue launch, none with option "sid_start_list" 0
bool start_list_on(const rsem_em_ctx* c) { return c->sid_start_list != 0 && c->L.d_start_list != nullptr; }
// bytes of ids one E step loads (rsem_em_get_info "sid_plane_bytes_loaded")
uint64_t sid_bytes_loaded(const rsem_em_ctx* c) {
    if (!start_list_on(c)) return c->L.n_sid_planes_loaded * 256;
    const SidTraffic& t = c->sid_traffic;
    return 256 * (t.first_planes + t.marked_planes) + 4 * (t.list_entries + t.list_slices);
}

// ---- the lane kernel's launches ---------------------------------------------------------------------------------------------------------
// What varies between the launches of k_estep_lane; everything else the kernel is handed comes from the context.
struct LaneIO {
    const double* theta = nullptr;   // theta, or (FUSED / SOLO: kFC) the previous round's raw counts ...
    const double* tsrc = nullptr;    // ... and their totals
    double N0 = 0.0;
    double* counts = nullptr;
    double* totals = nullptr;        // the two device-wide totals beside the counts
    unsigned long long* trace = nullptr;  // per-workgroup timestamps, two per unit (tune_unit_order, rsem_em_debug_trace)
    SoloArgs solo;                   // SOLO: the round the closers close (handed to the launch that carries them, no other)
    XArgs xa;                        // PLAIN: the split rows' side arrays
};

// The instantiation a loop takes for its far-queue launch and for its other launches.
using LaneKernel = decltype(&k_estep_lane<false, false, false>);
LaneKernel lane_kernel(Loop loop, bool far_queue) {
    if (loop == Loop::PLAIN) return far_queue ? k_estep_lane<false, false, true> : k_estep_lane<false, false, false>;
    if (far_queue) return k_estep_lane<true, false, true>;
    return loop == Loop::SOLO ? k_estep_lane<true, true, false> : k_estep_lane<true, false, false>;
}

// THE launch of the lane kernel over units [u0, u1): the only place that spells out its argument list.
void launch_lane(rsem_em_ctx* c, Loop loop, bool far_queue, uint32_t u0, uint32_t u1, hipStream_t s, const LaneIO& io) {
    if (u1 <= u0) return;
    const bool closes = loop == Loop::SOLO && !far_queue;
    StartList sl;
    if (!far_queue && start_list_on(c)) { sl.list = c->L.d_start_list; sl.off = c->L.d_start_off; }
    hipLaunchKernelGGL(lane_kernel(loop, far_queue), dim3(u1 - u0), dim3(kBlock), 0, s, c->L.d_shapes, c->d_units + u0, c->L.T, c->M, io.theta, io.tsrc,
                       io.N0, (const unsigned char*)c->d_sval, (const int16_t*)c->d_sexp, c->L.d_ssid, c->d_sncp, c->L.d_masks, io.counts,
                       io.totals, (const Ctrl*)c->d_ctrl, io.trace ? io.trace + 2 * (size_t)u0 : nullptr,
                       closes ? io.solo : SoloArgs(), io.xa, sl);
}

LanePlan plan_lanes(const rsem_em_ctx* c, Loop loop) {
    rsem::UnitGroups g;
    g.n = c->n_units; g.n_main = c->n_units_main; g.n_compact = c->n_units_compact;
    g.far_queue = c->far_queue != 0; g.x_overlap = c->x_overlap != 0; g.split_rows = c->L.n_x_rows != 0; g.stream_x = c->stream_x != nullptr;
    return rsem::plan_lane_launches(g, loop);
}
void launch_planned(rsem_em_ctx* c, const LanePlan& plan, Loop loop, hipStream_t st, const LaneIO& io) {
    for (int i = 0; i < plan.n; i++) launch_lane(c, loop, plan.at[i].far_queue, plan.at[i].u0, plan.at[i].u1, plan.at[i].second ? c->stream_x : st, io);
}
// the second stream (stream_x) beside the caller's: it starts behind what the caller's holds, and the caller's waits for it
int fork_x(rsem_em_ctx* c, hipStream_t st) {
    RSEM_HIP_TRY(hipEventRecord(c->ev_x_fork, st));
    RSEM_HIP_TRY(hipStreamWaitEvent(c->stream_x, c->ev_x_fork, 0));
    return RSEM_OK;
}
int join_x(rsem_em_ctx* c, hipStream_t st) {
    RSEM_HIP_TRY(hipEventRecord(c->ev_x_join, c->stream_x));
    RSEM_HIP_TRY(hipStreamWaitEvent(st, c->ev_x_join, 0));
    return RSEM_OK;
}

// One E step from a plain theta array (the PLAIN loop and every entry point that runs a single step): the lane launches of
// unit_groups.hpp between the split rows' two side passes, then the reads left in the CSR.  totals: where the workgroups add the two
// device-wide totals.
int launch_estep(rsem_em_ctx* c, const double* d_theta, double* d_counts, hipStream_t st, double* d_totals, unsigned long long* d_trace = nullptr) {
    const Ctrl* ctrl = c->d_ctrl;
    const LanePlan plan = plan_lanes(c, Loop::PLAIN);
    hipStream_t sx = plan.x_second ? c->stream_x : st;  // the split rows' chain: rowsum -> their lane launch -> colsum
    LaneIO io;
    io.theta = d_theta; io.counts = d_counts; io.totals = d_totals; io.trace = d_trace;
    if (plan.fork_join) { int rc = fork_x(c, st); if (rc != RSEM_OK) return rc; }
    if (c->L.n_x_rows) {  // split rows: the far part of their normalisers first
        io.xa.extra = c->d_xextra; io.xa.inv = c->d_xinv; io.xa.slot_base = c->L.x_slot_base;
        static const bool batched = !(getenv("RSEM_HIP_ROWSUM_BATCHED") && atoi(getenv("RSEM_HIP_ROWSUM_BATCHED")) == 0);  // measurement knob
        hipLaunchKernelGGL(batched ? k_far_rowsum<true> : k_far_rowsum<false>, dim3(rsem::ceil_div(c->L.n_x_slots, kBlock)), dim3(kBlock), 0, sx, c->L.n_x_slots,
                           (const uint64_t*)c->L.d_far_ptr, (const int32_t*)c->L.d_far_sid, (const double*)c->L.d_far_cp, d_theta, c->d_xextra, ctrl);
    }
    launch_planned(c, plan, Loop::PLAIN, st, io);
    if (c->L.n_far) {  // ... and their far alignments' fractions afterwards, in transcript order
        // one step of 4 x 64 entries per wave: the pass is a chain of dependent trips (entries -> theta, reciprocal -> shuffles ->
        // atomic), and more waves in flight hide more of it than a loop per wave (8 / 16 / 32 workgroups per CU: 335 / 326 /
        // 312 us at configs[1]'s size without gene structure, the whole grid 294: profiles/r04l_call.log)
        const int grid = std::max(1, rsem::ceil_div(c->L.n_far, kBlock * 4));
        static const bool xcd = !(getenv("RSEM_HIP_COLSUM_XCD") && atoi(getenv("RSEM_HIP_COLSUM_XCD")) == 0);  // measurement knob
        hipLaunchKernelGGL(xcd ? k_far_colsum<true> : k_far_colsum<false>, dim3(grid), dim3(kBlock), 0, sx, c->L.n_far, (const int32_t*)c->L.d_csc_sid,
                           (const double*)c->L.d_csc_cp, (const uint32_t*)c->L.d_csc_slot, c->L.x_slot_base, d_theta, (const double*)c->d_xinv, d_counts, ctrl);
    }
    if (plan.fork_join) {
        RSEM_HIP_TRY(hipGetLastError());
        int rc = join_x(c, st);
        if (rc != RSEM_OK) return rc;
    }
    RSEM_HIP_TRY(hipGetLastError());
    if (c->L.n_long_rows) {
        hipLaunchKernelGGL(k_estep_long, dim3(c->grid_long), dim3(kBlock), 0, st, (uint64_t)c->L.n_long_rows,
                           (const uint32_t*)(c->L.d_order + c->L.n_sell_rows), (const uint64_t*)c->d_row_ptr, (const int32_t*)c->d_sid, (const double*)c->d_cp,
                           (const double*)c->d_ncp, d_theta, d_counts, ctrl, d_totals);
        RSEM_HIP_TRY(hipGetLastError());
    }
    return RSEM_OK;
}

int launch_weights(rsem_em_ctx* c, const double* d_theta, hipStream_t st) {
    const int grid = std::max(1, std::min<int>(c->n_cus * 16, rsem::ceil_div(c->N1, kBlock)));
    hipLaunchKernelGGL(k_weights_csr, dim3(grid), dim3(kBlock), 0, st, c->N1, c->d_row_ptr, c->d_sid, c->d_cp, c->d_ncp, d_theta,
                       c->d_w, c->d_wn);
    RSEM_HIP_TRY(hipGetLastError());
    return RSEM_OK;
}

// workgroups of k_mstep_fast (either instantiation)
int mstep_fast_grid(const rsem_em_ctx* c) {
    return std::max(1, std::min(kMstepBlocks, rsem::ceil_div((uint64_t)c->M + 1, kBlock * 2)));
}

// One plain round: the E step from th_old into the context's [counts | totals], their sum over the shards where `comm` is given
// (EM.cpp:385-389: counts and the two totals in one all-reduce), then k_mstep_fast<false>, which writes th_new, counts_last and the
// round's line and leaves the scratch clear.  timed: two events around the E step, or nullptr.
int plain_round(rsem_em_ctx* c, const double* th_old, double* th_new, double N0, int round, int min_round, int max_round, HostMirror* mirror,
                rsem_comm* comm, const hipEvent_t* timed) {
    hipStream_t st = c->stream;
    if (timed) RSEM_HIP_TRY(hipEventRecord(timed[0], st));
    int rc = launch_estep(c, th_old, c->d_counts, st, c->d_totals);
    if (rc != RSEM_OK) return rc;
    if (timed) RSEM_HIP_TRY(hipEventRecord(timed[1], st));
    if (comm && (rc = rsem::comm_allreduce_sum_f64(comm, c->d_red, (size_t)c->M + 1 + 2 * kTotSlots, st)) != RSEM_OK) return rc;
    hipLaunchKernelGGL(k_mstep_fast<false>, dim3(mstep_fast_grid(c)), dim3(kBlock), 0, st, c->M, N0, c->d_counts, c->d_totals, th_old, th_new,
                       c->d_counts_last, c->d_ctrl, round, min_round, max_round, mirror, (double*)nullptr);
    RSEM_HIP_TRY(hipGetLastError());
    return RSEM_OK;
}

// What every entry point that runs an E step starts with.
int estep_ready(const rsem_em_ctx* c) {
    if (!c->have_values) { rsem::set_last_error("CSR values were never set"); return RSEM_ERR_STATE; }
    if (!c->layout_ok) { rsem::set_last_error("the device layout could not be rebuilt after the last change of values / options"); return RSEM_ERR_STATE; }
    RSEM_HIP_TRY(hipSetDevice(c->device));
    return RSEM_OK;
}

// The [counts | totals] scratch, clear: how every entry point finds it and leaves it.
hipError_t clear_scratch(rsem_em_ctx* c) {
    return hipMemsetAsync(c->d_red, 0, sizeof(double) * ((size_t)c->M + 1 + 2 * kTotSlots), c->stream);
}

int build_layout(rsem_em_ctx* c);
void free_layout(rsem_em_ctx* c);

// alignments of the reads that stay in the CSR (> 256 alignments): their bytes are part of a launch's physical traffic
__global__ void k_sum_row_lengths(uint32_t n, const uint32_t* __restrict__ rows, const uint64_t* __restrict__ row_ptr, unsigned long long* out) {
    unsigned long long v = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v += row_ptr[rows[i] + 1] - row_ptr[rows[i]];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

int release_csr(rsem_em_ctx* c) {
    if (c->csr_released) return RSEM_OK;
    const char* why = nullptr;
    if (!c->layout_ok || !c->have_values) why = "there is no layout with values yet";
    else if (c->layout_has_q32 || c->value_bits == 32) why = "Q32 planes hold rounded values";
    else if (c->L.n_x_rows) why = "split rows keep part of their alignments outside the planes";
    else if (c->L.n_long_rows) why = "reads with more than 256 alignments live in the CSR alone";
    else if (c->views_out > 0) why = "a model context still holds the arrays";
    if (why) { rsem::set_last_error("release_csr: %s", why); return RSEM_ERR_STATE; }
    RSEM_HIP_TRY(hipSetDevice(c->device));
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_sid); c->d_sid = nullptr;
    (void)hipFree(c->d_cp); c->d_cp = nullptr;
    c->csr_released = true;
    return RSEM_OK;
}

int ensure_csr(rsem_em_ctx* c) {
    if (!c->csr_released) return RSEM_OK;
    RSEM_HIP_TRY(hipSetDevice(c->device));
    RSEM_HIP_TRY(dmalloc(&c->d_sid, c->nnz));
    if (hipError_t e = dmalloc(&c->d_cp, c->nnz); e != hipSuccess) {  // (all or nothing: the next call starts from "released")
        (void)hipFree(c->d_sid);
        c->d_sid = nullptr;
        RSEM_HIP_TRY(e);
    }
    if (c->L.n_sell_rows)
        hipLaunchKernelGGL(k_unfill_sell, dim3(rsem::ceil_div(c->L.n_sell_rows, kBlock)), dim3(kBlock), 0, c->stream, c->L.d_shapes, c->L.n_shapes, c->L.T,
                           c->L.n_sell_rows, (const uint32_t*)c->L.d_order, (const uint64_t*)c->d_row_ptr, (const int32_t*)c->L.d_ssid,
                           (const unsigned char*)c->d_sval, c->d_sid, c->d_cp);
    RSEM_HIP_TRY(hipGetLastError());
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));  // whoever is handed the arrays next may read them on another stream
    c->csr_released = false;
    return RSEM_OK;
}

int write_values(rsem_em_ctx* c) {
    if (c->d_fill_err) RSEM_HIP_TRY(hipMemsetAsync(c->d_fill_err, 0, sizeof(int), c->stream));
    int rc = sell_fill_values(c->L, c->stream, c->d_row_ptr, c->d_cp, c->d_ncp, c->d_sval, c->d_sncp, c->d_sexp, c->d_fill_err, c->d_sid);
    if (rc != RSEM_OK) return rc;
    if (c->layout_has_q32) {  // a Q32 shape was handed a read that no longer qualifies: cannot happen after a rebuild
        int h = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&h, c->d_fill_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        if (h) { rsem::set_last_error("Q32 planes: a read's values left the range its format was chosen for"); return RSEM_ERR_STATE; }
    }
    return RSEM_OK;
}

// The caller-order values changed.  F64 layout: rewrite the planes.  With value_bits = 32 the format of a read depends
// on its values, so the layout is rebuilt from them (the rounds that change the values every time -- rounds 1-11 of
// rsem-run-em -- run with value_bits = 64 and switch afterwards).
int fill_values(rsem_em_ctx* c) {
    if (c->value_bits == 32 || c->layout_has_q32) {
        free_layout(c);
        return build_layout(c);
    }
    return write_values(c);
}

void free_layout(rsem_em_ctx* c) {
    sell_free(c->L);
    hipFree(c->d_rank); hipFree(c->d_xextra); hipFree(c->d_xinv);
    c->d_rank = nullptr; c->d_xextra = nullptr; c->d_xinv = nullptr;
    hipFree(c->d_sval); hipFree(c->d_sncp); hipFree(c->d_sexp); hipFree(c->d_fill_err); hipFree(c->d_units);
    c->d_sval = nullptr; c->d_sncp = nullptr; c->d_sexp = nullptr; c->d_fill_err = nullptr; c->d_units = nullptr;
    c->h_units.clear();
    c->n_units = 0;
    c->layout_has_q32 = false;
    c->layout_ok = false;
}

int build_layout(rsem_em_ctx* c) {
    // one block per wave, ~2.5 blocks per wave slot (6 waves/SIMD) for load balance
    const uint32_t target_waves = (uint32_t)c->n_cus * 4 * 6 * 5 / 2;
    const bool q32 = c->value_bits == 32 && c->have_values;
    std::vector<Unit> units;
    // (not together with Q32 planes: which reads take that format is a documented function of their values alone)
    int split = c->split_rows && !q32;
    // (measurement knobs, applied to this build alone: the options keep what the caller set)
    int short_on = c->short_last_plane, short_min_units = c->short_min_units;
    if (const char* e = getenv("RSEM_HIP_SHORT_LAST_PLANE")) short_on = atoi(e) != 0;               // 0 = every plane full
    if (const char* e = getenv("RSEM_HIP_SHORT_MIN_UNITS")) short_min_units = std::max(1, atoi(e));  // the class threshold
    if (const char* e = getenv("RSEM_HIP_SPLIT")) split = split && atoi(e) != 0;  // measurement knob: 0 = reads that leave their window stay whole
    // which reads split: those that are mostly outside their window (1), or every read with an id outside (2)
    if (split) split = c->split_policy;
    if (const char* e = getenv("RSEM_HIP_SPLIT_POLICY")) { if (split) split = !strcmp(e, "all") ? 2 : 1; }  // measurement knob
    int rc = sell_build_refined(c->L, c->stream, c->N1, c->M, c->d_row_ptr, c->d_sid, target_waves, c->forced_T,
                                q32 ? c->d_cp : nullptr, c->value_range_bits, kWindow, units, &c->d_units, &c->n_stray_reads, split,
                                short_on ? short_min_units : 0, true);
    if (rc != RSEM_OK) return rc;
    if (c->L.n_x_rows) {
        const size_t nxs = (size_t)c->L.n_x_slots;
        RSEM_HIP_TRY(dmalloc(&c->d_xextra, nxs));
        RSEM_HIP_TRY(dmalloc(&c->d_xinv, nxs));
        RSEM_HIP_TRY(hipMemsetAsync(c->d_xextra, 0, sizeof(double) * std::max<size_t>(nxs, 1), c->stream));
        RSEM_HIP_TRY(hipMemsetAsync(c->d_xinv, 0, sizeof(double) * std::max<size_t>(nxs, 1), c->stream));
    }
    c->layout_has_q32 = q32;
    RSEM_HIP_TRY(hipMalloc((void**)&c->d_sval, std::max<uint64_t>(c->L.val_bytes, 1)));
    RSEM_HIP_TRY(dmalloc(&c->d_sncp, (size_t)c->L.n_slots));
    if (q32) {
        RSEM_HIP_TRY(dmalloc(&c->d_sexp, (size_t)c->L.n_slots));
        RSEM_HIP_TRY(dmalloc(&c->d_fill_err, 1));
    }
    RSEM_HIP_TRY(hipMemsetAsync(c->d_sval, 0, c->L.val_bytes, c->stream));
    RSEM_HIP_TRY(hipMemsetAsync(c->d_sncp, 0, sizeof(double) * c->L.n_slots, c->stream));
    if (c->have_values) {
        rc = write_values(c);
        if (rc != RSEM_OK) return rc;
    }
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_units = (uint32_t)units.size();
    c->h_units = units;
    if (const char* e = getenv("RSEM_HIP_X_OVERLAP")) c->x_overlap = atoi(e);  // measurement knob: 1 = the split rows' chain on its own stream
    if (const char* e = getenv("RSEM_HIP_FAR_QUEUE")) c->far_queue = atoi(e);  // measurement knob: 0 = one launch, global atomics in the far units' loop
    rc = partition_units(c);
    if (rc != RSEM_OK) return rc;
    if ((c->L.n_x_rows || c->n_units_compact < c->n_units_main) && !c->stream_x) {
        RSEM_HIP_TRY(hipStreamCreateWithFlags(&c->stream_x, hipStreamNonBlocking));
        RSEM_HIP_TRY(hipEventCreateWithFlags(&c->ev_x_fork, hipEventDisableTiming));
        RSEM_HIP_TRY(hipEventCreateWithFlags(&c->ev_x_join, hipEventDisableTiming));
    }
    c->tune_passes_left = 1;
    if (const char* e = getenv("RSEM_HIP_TUNE")) c->tune_passes_left = atoi(e);  // tuning knob: 0 disables
    c->n_far_units = 0;
    for (const Unit& u : c->h_units) c->n_far_units += u.pad[0] != 0;
    c->grid_long = std::max(1, std::min<int>(c->n_cus * 8, rsem::ceil_div(c->L.n_long_rows, kBlock / 64)));  // (k_estep_long: a wave per read)
    c->long_nnz = 0;
    if (c->L.n_long_rows) {
        unsigned long long* d_n = (unsigned long long*)c->d_totals;  // (a slot that is clear between E steps: cleared again below)
        hipLaunchKernelGGL(k_sum_row_lengths, dim3(c->grid_long), dim3(kBlock), 0, c->stream, c->L.n_long_rows, c->L.d_order + c->L.n_sell_rows,
                           c->d_row_ptr, d_n);
        RSEM_HIP_TRY(hipGetLastError());
        unsigned long long h = 0;
        RSEM_HIP_TRY(hipMemcpyAsync(&h, d_n, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        RSEM_HIP_TRY(hipMemsetAsync(c->d_totals, 0, sizeof(double), c->stream));
        RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        c->long_nnz = h;
    }
    c->layout_ok = true;
    return RSEM_OK;
}

// an option the layout was built from changed: build it again from the CSR
int rebuild_layout(rsem_em_ctx* c) {
    RSEM_HIP_TRY(hipSetDevice(c->device));
    free_layout(c);
    return build_layout(c);
}

}  // namespace

extern "C" {

int rsem_em_create(rsem_em_ctx** out, int device, int32_t M, uint64_t N1, uint64_t nnz, const uint64_t* row_ptr,
                   const int32_t* sid, const double* conprb, const double* ncp) {
    RSEM_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RSEM_REQUIRE(M >= 1, "M must be >= 1");
    RSEM_REQUIRE(row_ptr != nullptr && (sid != nullptr || nnz == 0), "row_ptr / sid is NULL");
    RSEM_REQUIRE(N1 < 0xfffffff0ull, "N1 too large for one shard (max 2^32-16 reads)");
    RSEM_REQUIRE(row_ptr[0] == 0 && row_ptr[N1] == nnz, "row_ptr[0] != 0 or row_ptr[N1] != nnz");
    RSEM_REQUIRE((conprb == nullptr) == (ncp == nullptr), "conprb and ncp must be given together");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        rsem::set_last_error("no HIP device %d (have %d)", device, ndev);
        return RSEM_ERR_NODEVICE;
    }
    RSEM_HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    RSEM_HIP_TRY(hipGetDeviceProperties(&prop, device));
    rsem_em_ctx* c = new (std::nothrow) rsem_em_ctx();
    if (!c) return RSEM_ERR_NOMEM;
    c->device = device;
    c->M = M;
    c->N1 = N1;
    c->nnz = nnz;
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int rc = RSEM_OK;
    auto fail = [&](int code) { rsem_em_destroy(c); return code; };
#define TRY_OR_FAIL(expr)                                                                               \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            rsem::set_last_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));  \
            return fail(_e == hipErrorOutOfMemory ? RSEM_ERR_NOMEM : RSEM_ERR_HIP);                     \
        }                                                                                               \
    } while (0)
    TRY_OR_FAIL(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    TRY_OR_FAIL(dmalloc(&c->d_row_ptr, N1 + 1));
    TRY_OR_FAIL(dmalloc(&c->d_sid, nnz));
    TRY_OR_FAIL(dmalloc(&c->d_cp, nnz));
    TRY_OR_FAIL(dmalloc(&c->d_ncp, N1));
    // the big arrays go through pinned staging (upload.hpp)
    if ((rc = rsem::staged_h2d(c->d_row_ptr, row_ptr, sizeof(uint64_t) * (N1 + 1), c->stream)) != RSEM_OK) return fail(rc);
    if ((rc = rsem::staged_h2d(c->d_sid, sid, sizeof(int32_t) * nnz, c->stream)) != RSEM_OK) return fail(rc);
    if (conprb) {
        if ((rc = rsem::staged_h2d(c->d_cp, conprb, sizeof(double) * nnz, c->stream)) != RSEM_OK) return fail(rc);
        if ((rc = rsem::staged_h2d(c->d_ncp, ncp, sizeof(double) * N1, c->stream)) != RSEM_OK) return fail(rc);
        c->have_values = true;
    }
    for (int i = 0; i < 2; i++) TRY_OR_FAIL(dmalloc(&c->d_theta[i], (size_t)M + 1));
    TRY_OR_FAIL(dmalloc(&c->d_red3, 3 * ((size_t)M + 1 + 2 * kTotSlots)));
    c->d_red = c->d_red3;
    c->d_counts = c->d_red;
    c->d_totals = c->d_red + (size_t)M + 1;
    TRY_OR_FAIL(dmalloc(&c->d_counts_last, (size_t)M + 1));
    TRY_OR_FAIL(hipMemsetAsync(c->d_totals, 0, sizeof(double) * 2 * kTotSlots, c->stream));
    TRY_OR_FAIL(hipHostMalloc((void**)&c->mirror, sizeof(HostMirror), hipHostMallocDefault));
    memset(c->mirror, 0, sizeof(HostMirror));
    for (int i = 0; i < 2; i++) TRY_OR_FAIL(hipEventCreateWithFlags(&c->lag_ev[i], hipEventDisableTiming));
    {   // the statistics kernels are tiny and sit on the next round's critical path: highest priority, so that they are
        // dispatched as soon as workgroup slots free up instead of behind the E step's thousands of workgroups
        int least = 0, greatest = 0;
        TRY_OR_FAIL(hipDeviceGetStreamPriorityRange(&least, &greatest));
        TRY_OR_FAIL(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, greatest));
    }
    for (int i = 0; i < 4; i++) {
        TRY_OR_FAIL(hipEventCreateWithFlags(&c->ev_e[i], hipEventDisableTiming));
        TRY_OR_FAIL(hipEventCreateWithFlags(&c->ev_s[i], hipEventDisableTiming));
    }
    TRY_OR_FAIL(dmalloc(&c->d_ctrl, 1));
    TRY_OR_FAIL(hipMemsetAsync(c->d_counts, 0, sizeof(double) * ((size_t)M + 1), c->stream));
    TRY_OR_FAIL(hipMemsetAsync(c->d_ctrl, 0, sizeof(Ctrl), c->stream));
    if (const char* e = getenv("RSEM_HIP_T")) c->forced_T = (uint32_t)atoi(e);  // tuning knob: slices per block
    // measurement knob: the option's value at creation, 0 = every marked slice reads its id planes (read here alone: what the caller sets
    // later with rsem_em_set_option holds through every rebuild of the layout)
    if (const char* e = getenv("RSEM_HIP_SID_START_LIST")) c->sid_start_list = atoi(e) != 0;
    rc = build_layout(c);
    if (rc != RSEM_OK) return fail(rc);
    rsem::thread_stager().release();
#undef TRY_OR_FAIL
    *out = c;
    return RSEM_OK;
}

int rsem_em_set_values(rsem_em_ctx* c, const double* conprb, const double* ncp) {
    RSEM_REQUIRE(c && conprb && ncp, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    { int rc0 = ensure_csr(c); if (rc0 != RSEM_OK) return rc0; }
    if (c->nnz) RSEM_HIP_TRY(hipMemcpyAsync(c->d_cp, conprb, sizeof(double) * c->nnz, hipMemcpyHostToDevice, c->stream));
    if (c->N1) RSEM_HIP_TRY(hipMemcpyAsync(c->d_ncp, ncp, sizeof(double) * c->N1, hipMemcpyHostToDevice, c->stream));
    c->have_values = true;
    int rc = fill_values(c);
    if (rc != RSEM_OK) return rc;
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    return RSEM_OK;
}

int rsem_em_get_values(rsem_em_ctx* c, double* conprb, double* ncp) {
    RSEM_REQUIRE(c && conprb && ncp, "NULL argument");
    if (!c->have_values) { rsem::set_last_error("CSR values were never set"); return RSEM_ERR_STATE; }
    RSEM_HIP_TRY(hipSetDevice(c->device));
    { int rc0 = ensure_csr(c); if (rc0 != RSEM_OK) return rc0; }
    if (c->nnz) RSEM_HIP_TRY(hipMemcpyAsync(conprb, c->d_cp, sizeof(double) * c->nnz, hipMemcpyDeviceToHost, c->stream));
    if (c->N1) RSEM_HIP_TRY(hipMemcpyAsync(ncp, c->d_ncp, sizeof(double) * c->N1, hipMemcpyDeviceToHost, c->stream));
    RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    return RSEM_OK;
}

int rsem_em_shard_rows(uint64_t N1, const uint64_t* row_ptr, int world, uint64_t* bounds) {
    RSEM_REQUIRE(row_ptr && bounds && world >= 1, "bad argument");
    // EM.cpp:135-157: thread i reads rows while (rows left > threads left) and (it is the last thread or it holds
    // fewer than nHits / T alignments).  Same boundaries, found by bisection instead of by reading.
    const uint64_t nhT = row_ptr[N1] / (uint64_t)world;
    uint64_t cur = 0;
    bounds[0] = 0;
    for (int i = 0; i < world; i++) {
        const uint64_t left_threads = (uint64_t)(world - i - 1);
        if (i == world - 1) cur = N1;
        else {
            const uint64_t cap = N1 > left_threads ? N1 - left_threads : 0;  // leave one row for every later thread
            const uint64_t target = row_ptr[cur] + nhT;
            uint64_t nxt = (uint64_t)(std::lower_bound(row_ptr + cur, row_ptr + N1 + 1, target) - row_ptr);
            nxt = std::min(nxt, std::max(cap, cur));
            cur = std::max(cur, nxt);
        }
        bounds[i + 1] = cur;
    }
    return RSEM_OK;
}

int rsem_em_set_comm(rsem_em_ctx* c, rsem_comm* comm) {
    RSEM_REQUIRE(c != nullptr, "NULL argument");
    c->comm = comm;
    return RSEM_OK;
}

int rsem_em_set_progress(rsem_em_ctx* c, rsem_em_progress_fn fn, void* user) {
    RSEM_REQUIRE(c != nullptr, "NULL argument");
    c->progress = fn;
    c->progress_user = user;
    return RSEM_OK;
}

int rsem_em_set_option(rsem_em_ctx* c, const char* key, int64_t value) {
    RSEM_REQUIRE(c && key, "NULL argument");
    if (!strcmp(key, "release_csr")) {
        // 1: free the caller-order ids and values (12 B per alignment) until something needs them again (then they are read back
        // from the planes: the same doubles).  Refused -- RSEM_ERR_STATE, nothing changed -- where the planes do not hold everything:
        // Q32 planes, split rows, reads with more than 256 alignments, a live model context.  0: bring them back now.
        RSEM_REQUIRE(value == 0 || value == 1, "release_csr must be 0 or 1");
        return value ? release_csr(c) : ensure_csr(c);
    }
    if (!strcmp(key, "kernel") || !strcmp(key, "split_rows") || !strcmp(key, "split_policy") || !strcmp(key, "value_bits") || !strcmp(key, "value_range_bits")) {
        int rc0 = ensure_csr(c);  // (these may rebuild the layout from the CSR)
        if (rc0 != RSEM_OK) return rc0;
    }
    if (!strcmp(key, "kernel")) {
        RSEM_REQUIRE(value >= RSEM_EM_KERNEL_AUTO && value <= RSEM_EM_KERNEL_LANE, "unknown kernel variant");
        // (the thread-per-read and slice-at-a-time kernels of rounds 1-2 left the product in round 6: the checker is oracle/, not a
        // second kernel in the shipped library)
        RSEM_REQUIRE(value == RSEM_EM_KERNEL_AUTO || value == RSEM_EM_KERNEL_LANE, "kernel variants CSR (1) and SELL (2) were retired: AUTO (0) or LANE (3)");
        return RSEM_OK;  // (both name the one kernel there is)
    }
    if (!strcmp(key, "split_overlap")) {
        RSEM_REQUIRE(value == 0 || value == 1, "split_overlap must be 0 or 1");
        c->x_overlap = (int)value;
        return RSEM_OK;
    }
    if (!strcmp(key, "split_policy")) {
        RSEM_REQUIRE(value == 1 || value == 2, "split_policy must be 1 (reads mostly outside their window) or 2 (every read with an id outside)");
        if (c->split_policy == (int)value) return RSEM_OK;
        c->split_policy = (int)value;
        c->x_overlap = value == 2 ? 1 : 0;
        return rebuild_layout(c);
    }
    if (!strcmp(key, "split_rows")) {
        // 1 (default): a read with transcript ids outside the LDS window of its own gene is laid out as a row of its in-window
        // alignments plus far entries handled by two side passes (k_far_rowsum / k_far_colsum); 0: such reads stay whole and
        // their far ids take global atomics.  Rebuilds the layout.
        RSEM_REQUIRE(value == 0 || value == 1, "split_rows must be 0 or 1");
        if (c->split_rows == (int)value) return RSEM_OK;
        c->split_rows = (int)value;
        return rebuild_layout(c);
    }
    if (!strcmp(key, "value_bits") || !strcmp(key, "value_range_bits")) {
        // Format of the value planes the theta-only E step streams (sell_layout.hpp): 64 = the caller's doubles; 32 = a
        // 32-bit mantissa + per-read exponent for the reads whose non-zero values span < 2^value_range_bits.  Changing it
        // rebuilds the device layout from the current values.
        const bool bits = !strcmp(key, "value_bits");
        if (bits) RSEM_REQUIRE(value == 64 || value == 32, "value_bits must be 64 or 32");
        else RSEM_REQUIRE(value >= 0 && value <= 24, "value_range_bits must be in 0..24");
        int& field = bits ? c->value_bits : c->value_range_bits;
        if (field == (int)value) return RSEM_OK;
        field = (int)value;
        if (c->value_bits == 64 && !c->layout_has_q32) return RSEM_OK;  // nothing built depends on it
        return rebuild_layout(c);
    }
    if (!strcmp(key, "short_last_plane") || !strcmp(key, "short_class_min_units")) {
        // 1 (default): reads whose last value plane is at least a quarter empty are sorted into short classes whose last plane is
        // stored compacted (sell_shape.hpp); 0: every plane holds 64 entries.  short_class_min_units: how many units a class must
        // fill to be taken (a measurement knob; default kShortClassMinUnits).  Either rebuilds the layout.
        const bool sw = !strcmp(key, "short_last_plane");
        if (sw) RSEM_REQUIRE(value == 0 || value == 1, "short_last_plane must be 0 or 1");
        else RSEM_REQUIRE(value >= 1 && value <= 1000000, "short_class_min_units must be in 1..1000000");
        int& field = sw ? c->short_last_plane : c->short_min_units;
        if (field == (int)value) return RSEM_OK;
        field = (int)value;
        if (!sw && !c->short_last_plane) return RSEM_OK;  // nothing built depends on it
        { int rc0 = ensure_csr(c); if (rc0 != RSEM_OK) return rc0; }
        return rebuild_layout(c);
    }
    if (!strcmp(key, "sid_start_list")) {
        // 1 (default): in every slice of a wave but its first, the lanes that start a tuple take its ids from the start list (K * n
        // entries per slice instead of K planes of 64); 0: from the id planes, as the far-queue launch always does.  The list stays
        // built either way: nothing is laid out again.  (RSEM_HIP_SID_START_LIST only gives the value a context is created with: what
        // is set here holds through every later rebuild of the layout.)
        RSEM_REQUIRE(value == 0 || value == 1, "sid_start_list must be 0 or 1");
        c->sid_start_list = (int)value;
        return RSEM_OK;
    }
    if (!strcmp(key, "check_every")) {
        RSEM_REQUIRE(value >= 1 && value <= kHistCap / 4, "check_every out of range");
        c->check_every = (int)value;
        return RSEM_OK;
    }
    rsem::set_last_error("unknown option '%s'", key);
    return RSEM_ERR_INVALID;
}

int rsem_em_get_info(const rsem_em_ctx* c, const char* key, int64_t* value) {
    RSEM_REQUIRE(c && key && value, "NULL argument");
    if (!strcmp(key, "value_bits")) *value = c->value_bits;
    else if (!strcmp(key, "csr_released")) *value = c->csr_released ? 1 : 0;
    else if (!strcmp(key, "csr_bytes")) *value = (int64_t)(12 * c->nnz);                  // d_sid + d_cp: what "release_csr" frees
    else if (!strcmp(key, "value_range_bits")) *value = c->value_range_bits;
    else if (!strcmp(key, "far_units")) *value = c->n_far_units;                        // units with an id outside their LDS window
    else if (!strcmp(key, "units")) *value = c->n_units;
    else if (!strcmp(key, "units_compact")) *value = c->n_units_compact;              // [0, this): units launched without far queue
    else if (!strcmp(key, "units_main")) *value = c->n_units_main;                    // [units_compact, this): far-queue launch; behind: split rows
    else if (!strcmp(key, "units_queued")) *value = c->n_units_queued;                // main units fit for the far queue, adopted or not
    else if (!strcmp(key, "unit_tables_agree")) {  // diagnostic: the device unit table holds the host one's units in the same order
        std::vector<Unit> d(c->n_units);
        if (c->n_units) {
            RSEM_HIP_TRY(hipSetDevice(c->device));
            RSEM_HIP_TRY(hipMemcpyAsync(d.data(), c->d_units, sizeof(Unit) * c->n_units, hipMemcpyDeviceToHost, c->stream));
            RSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        }
        bool same = d.size() == c->h_units.size();
        for (size_t i = 0; same && i < d.size(); i++) same = same_unit(d[i], c->h_units[i]);
        *value = same ? 1 : 0;
    }
    else if (!strcmp(key, "stray_reads")) *value = (int64_t)c->n_stray_reads;             // (a read with two stray ids counts twice)
    else if (!strcmp(key, "reads_q32")) *value = c->L.n_q32_rows;                       // reads held in Q32 planes
    else if (!strcmp(key, "reads_sliced")) *value = c->L.n_sell_rows;                   // reads in the sliced layout
    else if (!strcmp(key, "reads_long")) *value = c->L.n_long_rows;                     // reads left in the CSR
    else if (!strcmp(key, "value_plane_bytes")) *value = (int64_t)c->L.val_bytes;       // incl. padding
    else if (!strcmp(key, "value_plane_entries")) *value = (int64_t)c->L.n_val_entries;  // incl. padding: / alignments in the layout = entries per alignment
    else if (!strcmp(key, "short_last_plane")) *value = c->short_last_plane;
    else if (!strcmp(key, "short_class_min_units")) *value = c->short_min_units;
    else if (!strcmp(key, "short_classes")) *value = (int64_t)__builtin_popcountll(c->L.short_classes);  // classes that passed the threshold
    else if (!strcmp(key, "shapes")) *value = c->L.n_shapes;
    else if (!strcmp(key, "unit_bytes")) *value = (int64_t)sizeof(Unit);                 // one record of the unit table (a part of physical_bytes_per_launch)
    else if (!strcmp(key, "sid_plane_bytes")) *value = (int64_t)(c->L.n_planes * 256);
    else if (!strcmp(key, "slots")) *value = c->L.n_slots;
    else if (!strcmp(key, "sid_plane_bytes_loaded")) *value = (int64_t)sid_bytes_loaded(c);  // ids of the slices where a tuple starts: planes or list entries
    else if (!strcmp(key, "sid_start_list")) *value = c->sid_start_list;
    else if (!strcmp(key, "start_list_entries")) *value = (int64_t)c->L.n_start_entries;     // 0: no list (an empty layout, or 2^32 entries and more)
    else if (!strcmp(key, "start_list_bytes")) *value = (int64_t)(c->L.d_start_list ? 4 * (c->L.n_start_entries + kStartListPad) + 4 * (uint64_t)c->L.n_slices : 0);
    // the terms of sid_plane_bytes_loaded with the list on: 256 * (first + marked) + 4 * (entries + slices)
    else if (!strcmp(key, "sid_first_slice_planes")) *value = (int64_t)c->sid_traffic.first_planes;         // planes of the waves' first slices
    else if (!strcmp(key, "start_list_entries_loaded")) *value = (int64_t)c->sid_traffic.list_entries;      // entries of their later marked slices
    else if (!strcmp(key, "start_list_slices")) *value = (int64_t)c->sid_traffic.list_slices;               // slices whose offset is fetched
    else if (!strcmp(key, "sid_marked_planes_far_queue")) *value = (int64_t)c->sid_traffic.marked_planes;   // planes of the far-queue units' marked slices
    else if (!strcmp(key, "slices")) *value = c->L.n_slices;
    else if (!strcmp(key, "split_rows")) *value = c->L.n_x_rows;    // reads laid out as an in-window row + far entries
    else if (!strcmp(key, "far_entries")) *value = (int64_t)c->L.n_far;
    else if (!strcmp(key, "window_entries")) {  // ids staged in (theta) and flushed from (counts) the LDS windows of all units
        int64_t w = 0;
        for (const Unit& u : c->h_units) w += u.span;
        *value = w;
    } else if (!strcmp(key, "physical_bytes_per_launch")) {
        // What one E-step launch of the LANE kernel moves through HBM by construction of the layout: every value plane,
        // the ids of the slices in which a tuple starts (sid_bytes_loaded: the planes, or with the start list the planes of every
        // wave's first slice, the list entries of its other marked slices and an offset per slice), one noise value (and, Q32, one exponent) per row slot, one
        // mask per slice, the unit table, theta into and counts out of every unit's window, and the CSR entries of the
        // reads with more than 256 alignments.  (Cache hits are not counted: theta of neighbouring units.)
        int64_t w = 0;
        for (const Unit& u : c->h_units) w += u.span;
        const uint64_t long_nnz = c->long_nnz + (c->L.n_long_rows * 4ull) / 3;  // 12 B per alignment + 16 B per read
        // split rows: their far entries once in row order (sid + value, 12 B) and once in column order (sid + value + slot, 16 B),
        // per row slot of the split shapes its far_ptr (8 B) and extra written, read, inv written, read (4 x 8 B; the gathers of
        // inv by the column-order entries stay within a block of slots: cache hits beyond the first)
        const uint64_t far_bytes = 28 * c->L.n_far + 40 * (uint64_t)c->L.n_x_slots;
        *value = (int64_t)(c->L.val_bytes + sid_bytes_loaded(c) + (uint64_t)c->L.n_slots * (8 + (c->layout_has_q32 ? 2 : 0)) +
                           (uint64_t)c->L.n_slices * 8 + (uint64_t)c->n_units * sizeof(Unit) + (uint64_t)w * 16 + 16 * ((uint64_t)c->M + 1)) +
                 (int64_t)(12 * long_nnz + far_bytes);
    }
    else { rsem::set_last_error("unknown info key '%s'", key); return RSEM_ERR_INVALID; }
    return RSEM_OK;
}

// Tuning aid: one E-step launch with per-workgroup start / end timestamps (100 MHz wall clock): out[2u], out[2u+1] for
// unit u in dispatch order; *n_units_io in: capacity (units), out: units written.
int rsem_em_debug_trace(rsem_em_ctx* c, const double* theta, unsigned long long* out, uint32_t* n_units_io) {
    RSEM_REQUIRE(c && theta && out && n_units_io, "NULL argument");
    RSEM_REQUIRE(c->have_values && c->layout_ok, "needs the LANE kernel with values set");
    RSEM_REQUIRE(*n_units_io >= c->n_units, "trace buffer too small");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    RSEM_HIP_TRY(hipMalloc((void**)&d, sizeof(unsigned long long) * 2 * std::max<uint32_t>(c->n_units, 1)));
    RSEM_HIP_TRY(hipMemcpyAsync(c->d_theta[0], theta, sizeof(double) * ((size_t)c->M + 1), hipMemcpyHostToDevice, c->stream));
    RSEM_HIP_TRY(hipMemsetAsync(c->d_ctrl, 0, sizeof(Ctrl), c->stream));
    int rc = RSEM_OK;
    for (int rep = 0; rep < 3 && rc == RSEM_OK; rep++)  // the last repetition is the one reported (caches warm)
        rc = launch_estep(c, c->d_theta[0], c->d_counts, c->stream, c->d_totals, d);
    hipError_t e = hipMemcpyAsync(out, d, sizeof(unsigned long long) * 2 * c->n_units, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)clear_scratch(c);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) { rsem::set_last_error("trace download failed"); return RSEM_ERR_HIP; }
    *n_units_io = c->n_units;
    return rc;
}

// Diagnostic: the split rows' far entries as the two side passes read them (sell_build_far), copied out; nothing in the context changes.
int rsem_em_debug_far(rsem_em_ctx* c, uint32_t* x_slot_base, uint32_t* n_x_slots_io, uint64_t* n_far_io, uint64_t* far_ptr, int32_t* far_sid,
                      uint64_t* far_src, int32_t* csc_sid, uint32_t* csc_slot, uint64_t* csc_src) {
    RSEM_REQUIRE(c && x_slot_base && n_x_slots_io && n_far_io, "NULL argument");
    RSEM_REQUIRE(c->layout_ok, "there is no layout");
    const SellLayout& L = c->L;
    const bool any = L.n_x_rows != 0;  // (no split rows: every size is 0, whatever slots the shape table counted)
    const uint32_t nxs = any ? L.n_x_slots : 0, cap_xs = *n_x_slots_io;
    const uint64_t nf = any ? L.n_far : 0, cap_f = *n_far_io;
    *x_slot_base = any ? L.x_slot_base : 0;
    *n_x_slots_io = nxs;
    *n_far_io = nf;
    if (!far_ptr && !far_sid && !far_src && !csc_sid && !csc_slot && !csc_src) return RSEM_OK;  // first call: the sizes
    RSEM_REQUIRE(far_ptr && far_sid && far_src && csc_sid && csc_slot && csc_src, "all six arrays or none");
    RSEM_REQUIRE(cap_xs >= nxs && cap_f >= nf, "the arrays hold fewer row slots or far entries than the layout has");
    if (!any) { far_ptr[0] = 0; return RSEM_OK; }
    RSEM_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    RSEM_HIP_TRY(hipMemcpyAsync(far_ptr, L.d_far_ptr, sizeof(uint64_t) * ((size_t)nxs + 1), hipMemcpyDeviceToHost, st));
    if (nf) {
        RSEM_HIP_TRY(hipMemcpyAsync(far_sid, L.d_far_sid, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(far_src, L.d_far_src, sizeof(uint64_t) * nf, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(csc_sid, L.d_csc_sid, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(csc_slot, L.d_csc_slot, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(csc_src, L.d_csc_src, sizeof(uint64_t) * nf, hipMemcpyDeviceToHost, st));
    }
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    return RSEM_OK;
}

int rsem_em_destroy(rsem_em_ctx* c) {
    if (!c) return RSEM_OK;
    (void)hipSetDevice(c->device);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    hipFree(c->d_row_ptr); hipFree(c->d_sid); hipFree(c->d_cp); hipFree(c->d_ncp);
    sell_free(c->L); hipFree(c->d_sval); hipFree(c->d_sncp); hipFree(c->d_sexp); hipFree(c->d_fill_err);
    hipFree(c->d_theta[0]); hipFree(c->d_theta[1]); hipFree(c->d_red3);
    for (int i = 0; i < 4; i++) { if (c->ev_e[i]) (void)hipEventDestroy(c->ev_e[i]); if (c->ev_s[i]) (void)hipEventDestroy(c->ev_s[i]); }
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream_x) (void)hipStreamDestroy(c->stream_x);
    if (c->ev_x_fork) (void)hipEventDestroy(c->ev_x_fork);
    if (c->ev_x_join) (void)hipEventDestroy(c->ev_x_join);
    hipFree(c->d_counts_last);
    if (c->mirror) (void)hipHostFree(c->mirror);
    for (int i = 0; i < 2; i++) if (c->lag_ev[i]) (void)hipEventDestroy(c->lag_ev[i]);
    hipFree(c->d_w); hipFree(c->d_wn); hipFree(c->d_ctrl); hipFree(c->d_units);
    if (c->stream && c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RSEM_OK;
}

// Longest-processing-time-first with MEASURED workgroup lifetimes: one traced E-step launch, then the units are
// re-sorted by how long they actually ran (tuple changes, window misses and the sid spread make equal-sized units
// differ 5x), so the launch does not end on a few long-lived workgroups.  Scratch use of [counts | totals]: the
// caller clears them afterwards.
static int tune_unit_order(rsem_em_ctx* c, const double* d_theta) {
    while (c->tune_passes_left > 0) {
        --c->tune_passes_left;
        if (c->n_units < 2048) return RSEM_OK;
        const uint32_t n = c->n_units;
        unsigned long long* d = nullptr;
        RSEM_HIP_TRY(hipMalloc((void**)&d, sizeof(unsigned long long) * 2 * n));
        std::vector<unsigned long long> t(2 * (size_t)n);
        int rc = RSEM_OK;
        for (int rep = 0; rep < 2 && rc == RSEM_OK; rep++)  // second launch: caches and clocks warm
            rc = launch_estep(c, d_theta, c->d_counts, c->stream, c->d_totals, d);
        hipError_t e = hipMemcpyAsync(t.data(), d, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        if (rc != RSEM_OK) return rc;
        if (e != hipSuccess) { rsem::set_last_error("unit tuning: trace download failed"); return RSEM_ERR_HIP; }
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return t[2 * a + 1] - t[2 * a] > t[2 * b + 1] - t[2 * b]; });
        std::vector<Unit> sorted(n);
        for (uint32_t i = 0; i < n; i++) sorted[i] = c->h_units[order[i]];
        c->h_units.swap(sorted);
        rc = partition_units(c);  // (uploads the new order)
        if (rc != RSEM_OK) return rc;
    }
    return RSEM_OK;
}

namespace {
// The fused loop's first round reads theta out of a [counts | totals] buffer like every other round: the caller's theta
// goes in as the counts, with totals chosen so that the round's formula returns it unchanged -- noise + N0 = 0 and
// normaliser total + N0 = 1 (N0 is an integer below 2^31: both sums are exact; x + 0 and x / 1 are exact).
__global__ void k_seed_theta_source(int32_t M, const double* __restrict__ theta, double N0, double* buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = M + 1;
    if (i < n) buf[i] = theta[i];
    if (i < 2 * kTotSlots) buf[n + i] = (i == 0) ? -N0 : (i == kTotSlots ? 1.0 - N0 : 0.0);
}

// The launch after the last round only has that round to close: the closers alone, no E-step work (grid = the number of
// closers: solo_close_round then makes every workgroup one).  Saves one whole E-step launch per rsem_em_run call.
__global__ __launch_bounds__(kBlock) void k_solo_close(int M, const double* __restrict__ cur, double N0, const Ctrl* ctrl, SoloArgs solo) {
    if (ctrl->done) return;
    __shared__ CloseScratch close_lds;
    solo_close_round(solo, M, N0, cur, &close_lds);
}

// Measured (profiles/r02c_em_loops.log, same box, back to back), ms per round on BASELINE configs[2] / configs[1]:
//   plain (E-step kernel, M-step kernel)          1.102 / 0.1393
//   fused (statistics kernel on a second stream)  1.042 / 0.1468   (two stream hand-offs per round)
//   solo  (one launch per round)                  1.051 / 0.1333   (E-step launch itself 1.038 / 0.1322)
// On configs[2] the E step gains 5 % from not starting behind an M-step kernel; on configs[1] the round is so short that
// only the one-launch round wins.  RSEM_EM_FUSED=0 / 1 / 2 forces plain / fused / solo (tests run all three).
// The one-kernel round (SOLO, k_estep_lane<true, true>) needs neither stream hand-off nor M-step kernel and is the default
// whenever the counts need not cross devices between the E step and theta; RSEM_EM_FUSED=2 asks for it explicitly.
// (Loop: unit_groups.hpp, where each loop's dealing of the units to lane launches is written down.)
Loop loop_wanted(const rsem_em_ctx* c, bool sharded) {
    // (split rows take the kernel sequence: their two side passes stand before and after the lane kernel, which then reads
    // theta as a plain array)
    const bool possible = c->L.n_long_rows == 0 && c->n_units > 0 && c->L.n_x_rows == 0;
    if (!possible) return Loop::PLAIN;
    const char* e = getenv("RSEM_EM_FUSED");
    if (e && !strcmp(e, "0")) return Loop::PLAIN;
    if (e && !strcmp(e, "1")) return Loop::FUSED;
    if (e && !strcmp(e, "2") && !sharded) return Loop::SOLO;
    if (!sharded) return Loop::SOLO;
    return 12ull * c->nnz + 16ull * c->N1 >= 2500000000ull ? Loop::FUSED : Loop::PLAIN;
}
}  // namespace

int rsem_em_run(rsem_em_ctx* c, double* theta, double N0, int round0, int min_round, int max_round, int* rounds_done,
                double* counts, double* bChange, int32_t* totNum, rsem_em_profile* prof) {
    RSEM_REQUIRE(c && theta, "NULL argument");
    RSEM_REQUIRE(max_round > round0, "max_round must exceed round0");
    if (int rc0 = estep_ready(c); rc0 != RSEM_OK) return rc0;
    hipStream_t st = c->stream;
    const size_t nb = sizeof(double) * ((size_t)c->M + 1);
    RSEM_HIP_TRY(hipMemcpyAsync(c->d_theta[round0 & 1], theta, nb, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(c->d_ctrl, 0, sizeof(Ctrl), st));
    if (c->tune_passes_left > 0) {
        int trc = tune_unit_order(c, c->d_theta[round0 & 1]);
        if (trc != RSEM_OK) return trc;
    }
    RSEM_HIP_TRY(clear_scratch(c));  // (the tuning launches used it)
    const int timed = prof ? std::min(max_round - round0, kMaxTimedRounds) : 0;
    if (prof) {
        while ((int)c->events.size() < 2 * timed + 2) {
            hipEvent_t e;
            RSEM_HIP_TRY(hipEventCreate(&e));
            c->events.push_back(e);
        }
        RSEM_HIP_TRY(hipEventRecord(c->events[0], st));
    }
    Ctrl h;
    memset(&h, 0, sizeof(h));
    // The host never drains the stream inside the loop.  The last workgroup of every M step writes the round's line and
    // the stop flag into pinned host memory (HostMirror); the host reads them between launches and only waits on the
    // event recorded check_every rounds earlier, so that at most 2 * check_every rounds are in flight.  Launches made
    // after the device set its stop flag return at once (theta is frozen at exactly the reference's stopping round).
    // With a communicator the enqueued collectives must be the same on every rank, so there the decision is taken at
    // fixed rounds from the device flag itself (identical on all ranks: they reduce to the same bits).
    HostMirror* mir = c->mirror;
    mir->done = 0;
    mir->final_round = 0;
    mir->last_round = round0;
    const bool sharded = rsem::comm_active(c->comm);
    int printed = round0, lag = 0;
    auto report = [&](int upto) {  // the reference prints this line after every round (EM.cpp:415)
        if (!c->progress) return;
        for (int q = printed + 1; q <= upto; q++) {
            const RoundStat& rs = mir->hist[(q - 1) % kHistCap];
            c->progress(rs.round, rs.sum, rs.bchange, rs.totNum, c->progress_user);
        }
        printed = std::max(printed, upto);
    };
    // FUSED loop (LANE kernel, no long rows): the E step of round r+1 reads theta straight out of round r's counts and
    // totals (ThetaSrc), so it follows the E step of round r with nothing in between; the statistics / stop-rule kernel of
    // round r (k_mstep_fast<true>) runs beside it on a second stream.  Three [counts | totals] buffers rotate: round r
    // reads buffer (r-1) % 3, accumulates into r % 3; the statistics kernel of round r clears (r-1) % 3 for round r+2,
    // which therefore waits for it (and so also sees its stop flag; the one E step launched past the stopping round only
    // accumulates into a buffer nobody reads).  theta, counts_last and the ROUND lines come from the statistics kernels.
    const Loop loop = loop_wanted(c, sharded);
    const bool fused = loop == Loop::FUSED, solo = loop == Loop::SOLO;
    // The instantiations that take theta out of the previous round's counts (kFC) walk F64X rows as plain F64: no far part, no
    // reciprocal stored.  loop_wanted() does not pick them for a layout with split rows; whoever adds another way here meets this.
    if ((fused || solo) && c->L.n_x_rows) {
        rsem::set_last_error("internal: the fused / one-launch EM loops cannot run a layout with split rows");
        return RSEM_ERR_STATE;
    }
    const size_t R = (size_t)c->M + 1 + 2 * kTotSlots;
    auto buf = [&](int q) { return c->d_red3 + (size_t)(q % 3) * R; };  // the [counts | totals] buffer round q accumulates into
    auto lane_io = [&](int q) {  // round q reads theta out of round q-1's buffer
        LaneIO io;
        io.theta = buf(q - 1); io.tsrc = buf(q - 1) + c->M + 1; io.N0 = N0; io.counts = buf(q); io.totals = buf(q) + c->M + 1;
        return io;
    };
    hipStream_t st2 = c->stream2;
    // SOLO: round r is ONE launch (see SoloArgs); the same three rotating buffers, seeded the same way.  Round q's line and
    // stop decision come out of launch q+1, so the loop issues one launch past max_round (whose own E-step work is unused,
    // like the one launch the device makes past any stopping round).
    const int last_launch = solo ? max_round + 1 : max_round;
    if (fused || solo) {
        RSEM_HIP_TRY(hipMemsetAsync(c->d_red3, 0, sizeof(double) * 3 * R, st));
        hipLaunchKernelGGL(k_seed_theta_source, dim3(rsem::ceil_div((uint64_t)c->M + 1 + 2 * kTotSlots, kBlock)), dim3(kBlock), 0, st, c->M,
                           (const double*)c->d_theta[round0 & 1], N0, buf(round0));
        RSEM_HIP_TRY(hipGetLastError());
    }
    int r = round0;
    while (r < last_launch) {
        ++r;
        const double* th_old = c->d_theta[(r - 1) & 1];
        double* th_new = c->d_theta[r & 1];
        const int ti = r - round0 - 1;
        int rc = RSEM_OK;
        hipStream_t st_stats = st;  // the stream the round's statistics (and with them the stop flag) are produced on
        if (solo) {
            SoloArgs sa;
            sa.prev = buf(r + 1);  // = round r-2's
            sa.ctrl = c->d_ctrl;
            sa.mirror = mir;
            sa.stat_round = r - 1 > round0 ? r - 1 : 0;
            sa.min_round = min_round;
            sa.max_round = max_round;
            if (prof && ti < timed) RSEM_HIP_TRY(hipEventRecord(c->events[2 + 2 * ti], st));
            if (r > max_round) {  // nothing left to accumulate: close round max_round, no E-step work
                if (c->n_units)
                    hipLaunchKernelGGL(k_solo_close, dim3(std::min<uint32_t>(c->n_units, (uint32_t)kCloseMax)), dim3(kBlock), 0, st, c->M, (const double*)buf(r - 1), N0,
                                       (const Ctrl*)c->d_ctrl, sa);
            } else {
                LaneIO io = lane_io(r);
                io.solo = sa;
                const LanePlan plan = plan_lanes(c, Loop::SOLO);
                if (plan.fork_join && (rc = fork_x(c, st)) != RSEM_OK) return rc;
                launch_planned(c, plan, Loop::SOLO, st, io);
                if (plan.fork_join && (rc = join_x(c, st)) != RSEM_OK) return rc;
            }
            RSEM_HIP_TRY(hipGetLastError());
            if (prof && ti < timed) RSEM_HIP_TRY(hipEventRecord(c->events[3 + 2 * ti], st));
        } else if (fused) {
            double* dst = buf(r);
            if (r - round0 >= 3) RSEM_HIP_TRY(hipStreamWaitEvent(st, c->ev_s[(r - 2) & 3], 0));  // dst was cleared by round r-2's statistics
            if (prof && ti < timed) RSEM_HIP_TRY(hipEventRecord(c->events[2 + 2 * ti], st));
            launch_planned(c, plan_lanes(c, Loop::FUSED), Loop::FUSED, st, lane_io(r));
            RSEM_HIP_TRY(hipGetLastError());
            if (prof && ti < timed) RSEM_HIP_TRY(hipEventRecord(c->events[3 + 2 * ti], st));
            if (sharded) {  // EM.cpp:385-389 across shards
                rc = rsem::comm_allreduce_sum_f64(c->comm, dst, R, st);
                if (rc != RSEM_OK) return rc;
            }
            RSEM_HIP_TRY(hipEventRecord(c->ev_e[r & 3], st));
            RSEM_HIP_TRY(hipStreamWaitEvent(st2, c->ev_e[r & 3], 0));
            hipLaunchKernelGGL(k_mstep_fast<true>, dim3(mstep_fast_grid(c)), dim3(kBlock), 0, st2, c->M, N0, dst, dst + c->M + 1, th_old, th_new,
                               c->d_counts_last, c->d_ctrl, r, min_round, max_round, mir, buf(r - 1));
            RSEM_HIP_TRY(hipGetLastError());
            RSEM_HIP_TRY(hipEventRecord(c->ev_s[r & 3], st2));
            st_stats = st2;
        } else {
            rc = plain_round(c, th_old, th_new, N0, r, min_round, max_round, mir, sharded ? c->comm : nullptr,
                             prof && ti < timed ? &c->events[2 + 2 * ti] : nullptr);
            if (rc != RSEM_OK) return rc;
        }
        const bool checkpoint = ((r - round0) % c->check_every == 0) || r == last_launch;
        if (sharded) {
            if (r >= min_round && checkpoint) {
                RSEM_HIP_TRY(hipMemcpyAsync(&h, c->d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st_stats));
                RSEM_HIP_TRY(hipStreamSynchronize(st_stats));
                report(h.done ? h.final_round : r);
                if (h.done) break;
            }
            continue;
        }
        if (checkpoint) {
            RSEM_HIP_TRY(hipEventRecord(c->lag_ev[lag & 1], st_stats));
            if (lag > 0) RSEM_HIP_TRY(hipEventSynchronize(c->lag_ev[(lag - 1) & 1]));
            ++lag;
        }
        const int seen = __atomic_load_n(&mir->last_round, __ATOMIC_ACQUIRE);
        if (c->progress && seen > printed) report(seen);
        if (__atomic_load_n(&mir->done, __ATOMIC_ACQUIRE)) break;
    }
    if (fused) {  // the statistics stream joins the main one
        RSEM_HIP_TRY(hipEventRecord(c->lag_ev[0], st2));
        RSEM_HIP_TRY(hipStreamWaitEvent(st, c->lag_ev[0], 0));
    }
    if (prof) RSEM_HIP_TRY(hipEventRecord(c->events[1], st));
    RSEM_HIP_TRY(hipMemcpyAsync(&h, c->d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (!h.done) { rsem::set_last_error("EM loop ended without the device stop flag"); return RSEM_ERR_STATE; }
    const int fr = h.final_round;
    if (solo) {  // nothing wrote theta or the final counts on the way: they are in the buffer the stopping round accumulated
        hipLaunchKernelGGL(k_solo_finish, dim3(rsem::ceil_div((uint64_t)c->M + 1, kBlock)), dim3(kBlock), 0, st, c->M, N0,
                           (const double*)buf(fr), c->d_theta[fr & 1], c->d_counts_last);
        RSEM_HIP_TRY(hipGetLastError());
    }
    if (fused || solo) RSEM_HIP_TRY(hipMemsetAsync(c->d_red3, 0, sizeof(double) * 3 * R, st));  // leave the shared scratch as the other entry points expect it
    report(fr);
    RSEM_HIP_TRY(hipMemcpyAsync(theta, c->d_theta[fr & 1], nb, hipMemcpyDeviceToHost, st));
    if (counts) RSEM_HIP_TRY(hipMemcpyAsync(counts, c->d_counts_last, nb, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (rounds_done) *rounds_done = fr;
    if (bChange) *bChange = h.last_bchange;
    if (totNum) *totNum = h.last_totNum;
    if (prof) {
        float ms = 0.f;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, c->events[0], c->events[1]));
        prof->total_ms = ms;
        prof->estep_ms_sum = 0.0;
        prof->estep_launches = 0;
        const int executed = fr - round0;
        for (int i = 0; i < std::min(executed, timed); i++) {
            RSEM_HIP_TRY(hipEventElapsedTime(&ms, c->events[2 + 2 * i], c->events[3 + 2 * i]));
            prof->estep_ms_sum += ms;
            prof->estep_launches++;
        }
        prof->rounds = executed;
        prof->algorithmic_bytes_per_round = 12ull * c->nnz + 16ull * c->N1 + 16ull * ((uint64_t)c->M + 1);
    }
    return RSEM_OK;
}

int rsem_em_step(rsem_em_ctx* c, const double* theta, double N0, double* counts, double* theta_new, double* sum,
                 double* bChange, int32_t* totNum) {
    RSEM_REQUIRE(c && theta, "NULL argument");
    if (int rc0 = estep_ready(c); rc0 != RSEM_OK) return rc0;
    hipStream_t st = c->stream;
    const size_t nb = sizeof(double) * ((size_t)c->M + 1);
    RSEM_HIP_TRY(hipMemcpyAsync(c->d_theta[0], theta, nb, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(c->d_ctrl, 0, sizeof(Ctrl), st));
    RSEM_HIP_TRY(clear_scratch(c));
    // round 1 of 1 of the PLAIN loop, this context's reads alone: a caller with several shards adds their counts up itself
    int rc = plain_round(c, c->d_theta[0], c->d_theta[1], N0, 1, 1, 1, nullptr, nullptr, nullptr);
    if (rc != RSEM_OK) return rc;
    Ctrl h;
    RSEM_HIP_TRY(hipMemcpyAsync(&h, c->d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
    if (counts) RSEM_HIP_TRY(hipMemcpyAsync(counts, c->d_counts_last, nb, hipMemcpyDeviceToHost, st));
    if (theta_new) RSEM_HIP_TRY(hipMemcpyAsync(theta_new, c->d_theta[1], nb, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    if (sum) *sum = h.last_sum;
    if (bChange) *bChange = h.last_bchange;
    if (totNum) *totNum = h.last_totNum;
    return RSEM_OK;
}

int rsem_em_expected_weights(rsem_em_ctx* c, const double* theta, double N0, double* counts, double* w, double* w_noise) {
    RSEM_REQUIRE(c && theta, "NULL argument");
    if (int rc0 = estep_ready(c); rc0 != RSEM_OK) return rc0;
    hipStream_t st = c->stream;
    const size_t nb = sizeof(double) * ((size_t)c->M + 1);
    if (w || w_noise) { int rc0 = ensure_csr(c); if (rc0 != RSEM_OK) return rc0; }  // (the weights pass walks the caller-order CSR)
    if ((w || w_noise) && !c->d_w) RSEM_HIP_TRY(dmalloc(&c->d_w, c->nnz));
    if ((w || w_noise) && !c->d_wn) RSEM_HIP_TRY(dmalloc(&c->d_wn, c->N1));
    RSEM_HIP_TRY(hipMemcpyAsync(c->d_theta[0], theta, nb, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(c->d_ctrl, 0, sizeof(Ctrl), st));
    RSEM_HIP_TRY(clear_scratch(c));
    // counts: the main E-step kernel (same launch as every theta-only round), then + noise + N0 in bin 0 (EM.cpp:392) as the SOLO
    // loop finishes a round (the theta it writes beside them goes to the spare buffer); weights: their own file-order pass
    int rc = launch_estep(c, c->d_theta[0], c->d_counts, st, c->d_totals);
    if (rc != RSEM_OK) return rc;
    hipLaunchKernelGGL(k_solo_finish, dim3(rsem::ceil_div((uint64_t)c->M + 1, kBlock)), dim3(kBlock), 0, st, c->M, N0, (const double*)c->d_red,
                       c->d_theta[1], c->d_counts_last);
    RSEM_HIP_TRY(hipGetLastError());
    if ((w || w_noise) && c->N1) {
        rc = launch_weights(c, c->d_theta[0], st);
        if (rc != RSEM_OK) return rc;
    }
    if (counts) RSEM_HIP_TRY(hipMemcpyAsync(counts, c->d_counts_last, nb, hipMemcpyDeviceToHost, st));
    if (w && c->nnz) RSEM_HIP_TRY(hipMemcpyAsync(w, c->d_w, sizeof(double) * c->nnz, hipMemcpyDeviceToHost, st));
    if (w_noise && c->N1) RSEM_HIP_TRY(hipMemcpyAsync(w_noise, c->d_wn, sizeof(double) * c->N1, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(clear_scratch(c));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    return RSEM_OK;
}

}  // extern "C"


// ---- internal hooks for model.hip (em_internal.hpp) ------------------------------------------------
namespace rsem {

int em_device_view(rsem_em_ctx* c, EmDeviceView* v) {
    RSEM_REQUIRE(c && v, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    { int rc0 = ensure_csr(c); if (rc0 != RSEM_OK) return rc0; }
    // (the weight buffers -- 8 B per alignment -- are allocated by the first pass that fills them, em_step_with_weights /
    // rsem_em_expected_weights: the round kernel of model.hip never needs them)
    v->device = c->device;
    v->stream = c->stream;
    v->M = c->M;
    v->N1 = c->N1;
    v->nnz = c->nnz;
    v->d_row_ptr = c->d_row_ptr;
    v->d_sid = c->d_sid;
    v->d_cp = c->d_cp;
    v->d_ncp = c->d_ncp;
    v->d_w = c->d_w;
    v->d_wn = c->d_wn;
    return RSEM_OK;
}

__global__ void k_invert_order(uint64_t n, const uint32_t* __restrict__ order, uint32_t* rank) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) rank[order[p]] = (uint32_t)p;
}

void em_view_hold(rsem_em_ctx* c) {
    if (c) c->views_out += 1;
}
void em_view_release(rsem_em_ctx* c) {
    if (c && c->views_out > 0) c->views_out -= 1;
}

bool em_planes_writable(const rsem_em_ctx* c) {
    return c && c->layout_ok && !c->layout_has_q32 && c->value_bits != 32 && !c->L.n_x_rows;
}

int em_planes_view(rsem_em_ctx* c, EmPlanesView* v) {
    RSEM_REQUIRE(c && v, "NULL argument");
    if (!em_planes_writable(c)) {
        set_last_error("the layout holds Q32 planes or split rows");
        return RSEM_ERR_STATE;
    }
    RSEM_HIP_TRY(hipSetDevice(c->device));
    if (!c->d_rank && c->N1) {
        RSEM_HIP_TRY(dmalloc(&c->d_rank, (size_t)c->N1));
        hipLaunchKernelGGL(k_invert_order, dim3(ceil_div(c->N1, kBlock)), dim3(kBlock), 0, c->stream, c->N1, (const uint32_t*)c->L.d_order, c->d_rank);
        RSEM_HIP_TRY(hipGetLastError());
    }
    v->d_rank = c->d_rank;
    v->d_shapes = c->L.d_shapes;
    v->n_shapes = c->L.n_shapes;
    v->T = c->L.T;
    v->n_sell_rows = c->L.n_sell_rows;
    v->d_sval = c->d_sval;
    v->d_sncp = c->d_sncp;
    return RSEM_OK;
}

int em_values_written_in_place(rsem_em_ctx* c) {
    RSEM_REQUIRE(c, "NULL argument");
    if (!c->layout_ok || c->layout_has_q32) { set_last_error("the layout cannot have been written in place"); return RSEM_ERR_STATE; }
    c->have_values = true;
    return RSEM_OK;
}

int em_values_changed(rsem_em_ctx* c) {
    RSEM_REQUIRE(c, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->device));
    c->have_values = true;
    return fill_values(c);
}


}  // namespace rsem

// rsem_hip_preload (status.hip): the first launch of a translation unit makes the runtime load its code object
namespace { __global__ void k_preload_em() {} }
namespace rsem { void preload_em() { hipLaunchKernelGGL(k_preload_em, dim3(1), dim3(1), 0, nullptr); (void)hipGetLastError(); } }
