// round_close.hpp -- closing an EM round: the convergence statistics of EM.cpp:400-416, the stop rule and the ROUND line, once.
//
// A round is closed by n_closers workgroups, each over a slice of the transcripts: the closers in the prologue of
// k_estep_lane<true, true> and k_solo_close (SOLO loop) and k_mstep_fast (PLAIN and FUSED loops, rsem_em_step).
// Each of them walks its slice (SliceWalk), gathers the statistics per thread (CloseAcc), reduces them over the workgroup
// (close_reduce) and lets thread 0 arrive (close_arrive); the last one to arrive publishes the round.  What a caller keeps:
// how it forms a count and theta, which buffer it clears, where theta goes and who clears which totals.
//
// Included by em.hip INSIDE its anonymous namespace, after sell_layout.hpp (kBlock) and estep_block.hpp (wave_sum), and by
// tests/round_close_emu.cpp, which runs this very code on the CPU (tests/simt_emu.hpp): everything that differs between the
// two goes through simt_macros.hpp.  The calling kernel owns the LDS scratch (CloseScratch) and hands it in.
#pragma once
#include "simt_macros.hpp"

struct Ctrl {  // device-resident loop control, one per ctx
    int done;
    int final_round;
    unsigned long long bbits; // accumulating max |dtheta|/theta as ordered bits
    double last_sum;
    double last_bchange;
    int last_totNum;
    int last_round;
    unsigned long long tick2;  // (sum of totNum) << 32 | arrivals, one atomic per closer
    // The floating-point sum of the round's counts -- the SUM of the reference's ROUND line -- is put together from one partial sum
    // per closer, ADDED IN CLOSER ORDER by the last one to arrive: its last digits do not depend on who arrived when.
    double fslot[1024];
};
constexpr int kSumSlots = 1024;

// What the host reads while the loop runs, in pinned host memory the last closer writes directly (no stream sync, no
// copy): the statistics line of every finished round (EM.cpp:415) and the stop flag.  hist is a ring; the host keeps
// fewer than kHistCap rounds in flight.
constexpr int kHistCap = 1024;
struct RoundStat { double sum, bchange; int totNum, round; };
struct HostMirror {
    int last_round;  // rounds <= last_round have their RoundStat in hist[(round - 1) % kHistCap]
    int done;
    int final_round;
    int pad;
    RoundStat hist[kHistCap];
};

// One thread's share of a slice.  c and th are the caller's: the closers form them from different buffers.
struct CloseAcc {
    int tot = 0;
    double bmax = 0.0, csum = 0.0;
    RSEM_DEVFN void add(double c, double th, double old) {
        csum += c;
        if (old >= 1e-7) {
            const double change = fabs(th - old) / old;
            if (change >= 0.001) ++tot;
            bmax = fmax(bmax, change);
        }
    }
};

// The walk over a slice [lo, hi) of two arrays: thread t takes lo + t, lo + t + step, ...  A slice of up to kPre elements
// per thread is requested whole by load() -- which the caller places BEFORE it reduces its totals, so that the slice
// arrives meanwhile -- and handed out of registers by each(); a longer one is read by each() as it goes.
// step: the workgroup's size as the caller spells it (the constant in the lane kernel, blockDim.x in the M-step kernels:
// each keeps the code it had -- with the constant k_mstep_fast takes 16 registers more and loses a wave per SIMD).
struct SliceWalk {
    static constexpr int kPre = 8;
    int lo, hi, step;
    bool pre;
    double pa[kPre], pb[kPre];
    RSEM_DEVFN void load(int lo_, int hi_, int step_, const double* a, const double* b) {
        lo = lo_;
        hi = hi_;
        step = step_;
        pre = hi - lo <= kPre * step;
        if (pre) {
#pragma unroll
            for (int k = 0; k < kPre; k++) {
                const int i = lo + RSEM_TIDX + step * k;
                pa[k] = i < hi ? a[i] : 0.0;
                pb[k] = i < hi ? b[i] : 0.0;
            }
        }
    }
    template <typename F>
    RSEM_DEVFN void each(const double* a, const double* b, F&& one) {  // one(i, a[i], b[i])
        if (pre) {
#pragma unroll
            for (int k = 0; k < kPre; k++) {
                const int i = lo + RSEM_TIDX + step * k;
                if (i < hi) one(i, pa[k], pb[k]);
            }
        } else {
            for (int i = lo + RSEM_TIDX; i < hi; i += step) one(i, a[i], b[i]);
        }
    }
};

// The workgroup's statistics, in thread 0's acc: a butterfly over each wave, then the waves in index order.
struct CloseScratch {
    int tot[kBlock / 64];
    double bmax[kBlock / 64], csum[kBlock / 64];
};
RSEM_DEVFN void close_reduce(CloseAcc& acc, CloseScratch* s) {
    for (int d = 32; d >= 1; d >>= 1) {
        acc.tot += RSEM_SHFL_XOR(acc.tot, d);
        acc.bmax = fmax(acc.bmax, RSEM_SHFL_XOR(acc.bmax, d));
    }
    acc.csum = wave_sum(acc.csum);
    const int w = RSEM_TIDX >> 6;
    if ((RSEM_TIDX & 63) == 0) { s->tot[w] = acc.tot; s->bmax[w] = acc.bmax; s->csum[w] = acc.csum; }
    RSEM_SYNC();
    if (RSEM_TIDX == 0)
        for (int i = 1; i < kBlock / 64; i++) { acc.tot += s->tot[i]; acc.bmax = fmax(acc.bmax, s->bmax[i]); acc.csum += s->csum[i]; }
}

// 0, but only once x is there: what is added to the operand of an atomic that must not overtake the atomic x came back
// from.  No fence: an agent-scope fence in the middle of a kernel writes back and invalidates the XCD's L2 under everybody
// else's feet (the closers run beside an E step); the dependency costs one more trip for this thread only.
RSEM_DEVFN unsigned int zero_after(unsigned int x) {
    unsigned int z;
    RSEM_ZERO_DEP(z, x);
    return z;
}

// Thread 0 of closer `me` of n_closers arrives with its workgroup's statistics: one max (bChange), one exchange (its share
// of the floating-point sum of the counts, the reference's SUM, EM.cpp:394-398,415, into its slot) and one returning add
// that carries both its count and its arrival and follows the other two by a data dependency.  The last to arrive
// publishes the round -- Ctrl::last_*, the stop rule (EM.cpp:416), the host's line and THEN the counters that announce it
// -- and leaves bbits / tick2 clean for the next round.  Returns whether this closer was the last (the caller clears what is
// its own).
RSEM_DEVFN bool close_arrive(Ctrl* ctrl, HostMirror* mirror, int me, int n_closers, const CloseAcc& acc, int round, int min_round,
                             int max_round) {
    unsigned int zero = 0;
    if (acc.bmax > 0.0) zero = zero_after((unsigned int)RSEM_AGENT_FETCH_MAX(&ctrl->bbits, (unsigned long long)RSEM_DOUBLE_AS_LL(acc.bmax)));
    zero += zero_after((unsigned int)RSEM_DOUBLE_AS_LL(RSEM_AGENT_EXCHANGE(&ctrl->fslot[me], acc.csum)));
    const unsigned long long old = RSEM_AGENT_FETCH_ADD(&ctrl->tick2, (((unsigned long long)(unsigned)acc.tot << 32) | 1ull) + zero);
    if ((int)(old & 0xffffffffull) != n_closers - 1) return false;
    const int totNum = (int)(old >> 32) + acc.tot;
    const double bchange = RSEM_LL_AS_DOUBLE((long long)RSEM_AGENT_LOAD(&ctrl->bbits));
    double fsum = 0.0;
    for (int i = 0; i < n_closers; i++) fsum += RSEM_AGENT_LOAD(&ctrl->fslot[i]);
    ctrl->last_sum = fsum;
    ctrl->last_bchange = bchange;
    ctrl->last_totNum = totNum;
    ctrl->last_round = round;
    const bool stop = !(round < min_round || (totNum > 0 && round < max_round));
    if (stop) {
        ctrl->done = 1;
        ctrl->final_round = round;
    }
    if (mirror) {
        RoundStat* h = &mirror->hist[(round - 1) % kHistCap];
        h->sum = fsum;
        h->bchange = bchange;
        h->totNum = totNum;
        h->round = round;
        if (stop) mirror->final_round = round;
        RSEM_HOST_RELEASE_STORE(&mirror->last_round, round);
        if (stop) RSEM_HOST_RELEASE_STORE(&mirror->done, 1);
    }
    RSEM_AGENT_STORE(&ctrl->bbits, 0ull);
    RSEM_AGENT_STORE(&ctrl->tick2, 0ull);
    return true;
}
