// unit_groups.hpp -- which units of the sliced layout go to which launch of the lane kernel (em.hip: k_estep_lane).  Host code
// only, no HIP: em.hip asks it every round, tests/unit_groups_check.cpp enumerates it on the CPU.
//
// The unit table stands in up to three groups (em.hip: partition_units):
//   [0, n_compact)        compact units: every id inside the unit's LDS window, or too many outside for the far queue;
//   [n_compact, n_main)   units with a few ids outside their window: the far-queue instantiation (kFQ), adopted only where they
//                         are at least one main unit in 25;
//   [n_main, n)           units of the split rows' shapes (F64X), between their two side passes (k_far_rowsum / k_far_colsum).
// The three EM loops deal these groups to launches each in its own way -- plan_lane_launches is that table.
#pragma once
#include <cstdint>

namespace rsem {

// ---- the groups ---------------------------------------------------------------------------------------------------------------------
// The far-queue launch takes the units with FEW entries outside their window per slice -- reads of a gene that also hit a couple of
// transcripts elsewhere: the queue then empties every few slices; a unit of reads without a gene, half of whose entries are
// outside, would empty it before every slice and is better off with its atomics inline (configs[1]'s size without genes: 0.634
// against 0.650 ms, profiles/r06g_xrows_probe.log).  has_far / far_entries: Unit::pad[0] / pad[1] (sell_flag_far_units).
inline bool unit_queued(int32_t has_far, int32_t far_entries, uint32_t n_slices) {
    return has_far != 0 && (uint64_t)far_entries <= 48ull * n_slices;
}
// ... and only where such units are worth a launch of their own: one main unit in twenty-five, and at least one (configs[2] itself
// has 53 among 3 903 and paid 1 % for the second stream).  Not adopted: every unit keeps its place in the longest-first order.
inline bool far_group_adopted(bool far_queue, uint32_t n_queued, uint32_t n_main) {
    return far_queue && n_queued * 25ull >= n_main && n_queued;
}

// ---- the launches -------------------------------------------------------------------------------------------------------------------
// PLAIN: E-step launches, then an M-step kernel (also every entry point that runs one E step); FUSED: the statistics kernel of round
// r on a second stream beside the E step of round r+1; SOLO: one launch per round, the closers of round r-1 riding on it.
enum class Loop { PLAIN, FUSED, SOLO };

struct UnitGroups {
    uint32_t n = 0, n_main = 0, n_compact = 0;
    bool far_queue = false;   // option far_queue / RSEM_HIP_FAR_QUEUE
    bool x_overlap = false;   // option split_overlap: the split rows' chain on the second stream
    bool split_rows = false;  // the layout has split rows (PLAIN only: the other loops are not taken for such a layout)
    bool stream_x = false;    // the second stream exists
};

struct LaneLaunch {
    bool far_queue;  // the far-queue instantiation
    uint32_t u0, u1; // units [u0, u1), never empty
    bool second;     // on the second stream (stream_x) instead of the caller's
};

struct LanePlan {
    int n = 0;
    LaneLaunch at[3];       // in enqueue order
    bool fork_join = false; // the second stream waits for the caller's before the first launch, the caller's for it after the last
    bool x_second = false;  // PLAIN: the split rows' side passes go to the second stream with their launch
    void add(bool fq, uint32_t u0, uint32_t u1, bool second) {
        if (u1 > u0) at[n++] = LaneLaunch{fq, u0, u1, second};
    }
};

inline LanePlan plan_lane_launches(const UnitGroups& g, Loop loop) {
    LanePlan p;
    const uint32_t nc = g.n_compact, n_main = g.n_main, n = g.n;
    if (loop == Loop::PLAIN) {
        const bool far = g.far_queue && nc < n_main;
        const bool x_beside = g.x_overlap && g.split_rows && n_main > 0 && n_main < n;
        p.fork_join = g.stream_x && (x_beside || (far && nc > 0));
        p.x_second = x_beside && p.fork_join;
        // (every unit far-queued, nc == 0: that launch stays on the caller's stream unless the split rows opened the second one)
        p.add(true, far ? nc : n_main, n_main, p.fork_join);
        if (!far && !p.x_second) p.add(false, 0, n, false);
        else {
            p.add(false, 0, far ? nc : n_main, false);
            p.add(false, n_main, n, p.x_second);
        }
        return p;
    }
    // FUSED and SOLO (no split rows: n_main == n).  With no compact unit at all: one launch of all units, their far ids inline.
    const bool far = g.far_queue && nc < n && nc > 0 && g.stream_x;
    if (loop == Loop::FUSED) {  // both on the caller's stream: this loop keeps its second stream for the statistics kernel
        p.add(false, 0, far ? nc : n, false);
        if (far) p.add(true, nc, n, false);
    } else {  // the far units beside the compact ones, on stream_x; the closers ride on the compact launch
        p.fork_join = far;
        if (far) p.add(true, nc, n, true);
        p.add(false, 0, far ? nc : n, false);
    }
    return p;
}

}  // namespace rsem
