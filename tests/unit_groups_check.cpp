// unit_groups_check.cpp -- TEST INFRASTRUCTURE: rsem_amd/csrc/unit_groups.hpp (which units go to which launch of the lane kernel under
// each EM loop; which units are queued; when the far group is adopted) enumerated on the CPU.  The expected launches are written down
// here a second time, loop by loop, the way the three loops of em.hip issued them before they shared one plan: fork, the launches in
// enqueue order on the stream each went to, join.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rsem_amd/csrc/unit_groups.hpp"

using rsem::LanePlan;
using rsem::Loop;
using rsem::UnitGroups;

namespace {

struct L { bool fq; uint32_t u0, u1; bool second; };
struct Expect { std::vector<L> at; bool fork_join = false, x_second = false; };

// the kernel sequence (launch_estep): streams as small integers, 0 = the caller's, 1 = stream_x
Expect expect_plain(const UnitGroups& g) {
    Expect e;
    const int st = 0, stream_x = 1;
    const uint32_t nc = g.n_compact, n_main = g.n_main, n_all = g.n;
    const bool far_launch = g.far_queue && nc < n_main;
    const bool x_beside = g.x_overlap && g.split_rows && n_main > 0 && n_main < n_all;
    const bool second = g.stream_x && (x_beside || (far_launch && nc > 0));
    const int s2 = second ? stream_x : st;
    const int sx = x_beside ? s2 : st, sf = far_launch ? s2 : st;
    auto lane = [&](uint32_t u0, uint32_t u1, int s) { if (u1 > u0) e.at.push_back(L{false, u0, u1, s == stream_x}); };
    auto lane_fq = [&](uint32_t u0, uint32_t u1, int s) { if (u1 > u0) e.at.push_back(L{true, u0, u1, s == stream_x}); };
    if (far_launch) lane_fq(nc, n_main, sf);
    if (!far_launch && sx == st) lane(0, n_all, st);
    else {
        lane(0, far_launch ? nc : n_main, st);
        lane(n_main, n_all, sx);
    }
    e.fork_join = second;
    e.x_second = sx == stream_x;
    return e;
}
// statistics on a second stream: both launches on the caller's
Expect expect_fused(const UnitGroups& g) {
    Expect e;
    const uint32_t nc = g.n_compact;
    const bool far_launch = g.far_queue && nc < g.n && nc > 0 && g.stream_x;
    if ((far_launch ? nc : g.n) > 0) e.at.push_back(L{false, 0, far_launch ? nc : g.n, false});
    if (far_launch) e.at.push_back(L{true, nc, g.n, false});
    return e;
}
// one launch per round: the far units first, on stream_x between fork and join; the closers ride on the other launch
Expect expect_solo(const UnitGroups& g) {
    Expect e;
    const uint32_t nc = g.n_compact;
    const bool far_launch = g.far_queue && nc < g.n && nc > 0 && g.stream_x;
    if (far_launch) e.at.push_back(L{true, nc, g.n, true});
    if ((far_launch ? nc : g.n) > 0) e.at.push_back(L{false, 0, far_launch ? nc : g.n, false});
    e.fork_join = far_launch;
    return e;
}

int n_failed = 0;
void fail(const char* what, const UnitGroups& g, Loop loop) {
    ++n_failed;
    fprintf(stderr, "FAIL %s: loop=%d n=%u n_main=%u n_compact=%u far_queue=%d x_overlap=%d split_rows=%d stream_x=%d\n", what, (int)loop, g.n, g.n_main,
            g.n_compact, g.far_queue, g.x_overlap, g.split_rows, g.stream_x);
}

bool same(const LanePlan& p, const Expect& e) {
    if ((size_t)p.n != e.at.size() || p.fork_join != e.fork_join || p.x_second != e.x_second) return false;
    for (int i = 0; i < p.n; i++)
        if (p.at[i].far_queue != e.at[i].fq || p.at[i].u0 != e.at[i].u0 || p.at[i].u1 != e.at[i].u1 || p.at[i].second != e.at[i].second) return false;
    return true;
}

void check(const UnitGroups& g, Loop loop) {
    const LanePlan p = rsem::plan_lane_launches(g, loop);
    const Expect e = loop == Loop::PLAIN ? expect_plain(g) : loop == Loop::FUSED ? expect_fused(g) : expect_solo(g);
    if (!same(p, e)) fail("not the launches the loop issued", g, loop);
    if (p.n < 0 || p.n > 3) { fail("more than three launches", g, loop); return; }
    // disjoint, no launch empty, together [0, n)
    std::vector<int> hit(g.n, 0);
    for (int i = 0; i < p.n; i++) {
        if (p.at[i].u1 <= p.at[i].u0 || p.at[i].u1 > g.n) { fail("an empty launch or one past the table", g, loop); return; }
        for (uint32_t u = p.at[i].u0; u < p.at[i].u1; u++) hit[u]++;
        if (p.at[i].second && !g.stream_x) fail("a launch on a second stream that does not exist", g, loop);
        if (p.at[i].second && !p.fork_join) fail("a launch on the second stream without fork and join", g, loop);
    }
    for (uint32_t u = 0; u < g.n; u++)
        if (hit[u] != 1) { fail("units not covered exactly once", g, loop); break; }
    if (p.fork_join && !g.stream_x) fail("fork / join without a second stream", g, loop);
    if (loop == Loop::SOLO && g.n > 0) {  // the launch that carries the closers: the one without far queue, on the caller's stream
        int closers = 0;
        for (int i = 0; i < p.n; i++) closers += !p.at[i].far_queue && !p.at[i].second;
        if (closers != 1) fail("no launch (or more than one) to carry the closers", g, loop);
    }
}

UnitGroups groups(uint32_t n, uint32_t n_main, uint32_t nc, bool far_queue, bool x_overlap, bool split_rows, bool stream_x) {
    UnitGroups g;
    g.n = n; g.n_main = n_main; g.n_compact = nc;
    g.far_queue = far_queue; g.x_overlap = x_overlap; g.split_rows = split_rows; g.stream_x = stream_x;
    return g;
}

void named(const char* name, const UnitGroups& g, Loop loop, const Expect& e) {
    if (!same(rsem::plan_lane_launches(g, loop), e)) fail(name, g, loop);
}

}  // namespace

int main() {
    long n_cases = 0;
    for (uint32_t n = 0; n <= 6; n++)
        for (uint32_t n_main = 0; n_main <= n; n_main++)
            for (uint32_t nc = 0; nc <= n_main; nc++)
                for (int bits = 0; bits < 16; bits++) {
                    const bool far_queue = bits & 1, x_overlap = bits & 2, split_rows = bits & 4, stream_x = bits & 8;
                    if (n_main < n && !split_rows) continue;  // units behind the main ones ARE the split rows' units
                    const UnitGroups g = groups(n, n_main, nc, far_queue, x_overlap, split_rows, stream_x);
                    check(g, Loop::PLAIN);
                    ++n_cases;
                    if (split_rows) continue;  // the other loops are not taken for a layout with split rows (loop_wanted)
                    check(g, Loop::FUSED);
                    check(g, Loop::SOLO);
                    n_cases += 2;
                }
    // The named cases, launch by launch: {far queue, u0, u1, second stream}, fork / join, side passes on the second stream.
    {   // every unit far-queued (n_compact == 0): PLAIN gives them the far-queue launch on the caller's stream; the other two loops one
        // launch of everything without queue, their far ids inline
        const UnitGroups g = groups(4, 4, 0, true, false, false, true);
        named("every unit far-queued, PLAIN", g, Loop::PLAIN, Expect{{{true, 0, 4, false}}, false, false});
        named("every unit far-queued, FUSED", g, Loop::FUSED, Expect{{{false, 0, 4, false}}, false, false});
        named("every unit far-queued, SOLO", g, Loop::SOLO, Expect{{{false, 0, 4, false}}, false, false});
    }
    {   // far group below one in 25: not adopted, so n_compact == n_main and every loop makes one launch
        const UnitGroups g = groups(6, 6, 6, true, false, false, false);
        for (Loop loop : {Loop::PLAIN, Loop::FUSED, Loop::SOLO}) named("far group not adopted", g, loop, Expect{{{false, 0, 6, false}}, false, false});
    }
    {   // far group adopted beside compact units
        const UnitGroups g = groups(6, 6, 4, true, false, false, true);
        named("far group beside, PLAIN", g, Loop::PLAIN, Expect{{{true, 4, 6, true}, {false, 0, 4, false}}, true, false});
        named("far group beside, FUSED", g, Loop::FUSED, Expect{{{false, 0, 4, false}, {true, 4, 6, false}}, false, false});
        named("far group beside, SOLO", g, Loop::SOLO, Expect{{{true, 4, 6, true}, {false, 0, 4, false}}, true, false});
        // ... and with the far queue switched off: one launch
        const UnitGroups g0 = groups(6, 6, 6, false, false, false, true);
        for (Loop loop : {Loop::PLAIN, Loop::FUSED, Loop::SOLO}) named("far queue off", g0, loop, Expect{{{false, 0, 6, false}}, false, false});
    }
    {   // split rows (PLAIN only)
        named("split rows not beside: one launch of everything", groups(6, 4, 4, true, false, true, true), Loop::PLAIN, Expect{{{false, 0, 6, false}}, false, false});
        named("split rows beside", groups(6, 4, 4, true, true, true, true), Loop::PLAIN, Expect{{{false, 0, 4, false}, {false, 4, 6, true}}, true, true});
        named("split rows beside, no second stream", groups(6, 4, 4, true, true, true, false), Loop::PLAIN, Expect{{{false, 0, 6, false}}, false, false});
        named("split rows beside a far group", groups(6, 4, 2, true, true, true, true), Loop::PLAIN,
              Expect{{{true, 2, 4, true}, {false, 0, 2, false}, {false, 4, 6, true}}, true, true});
        named("split rows behind a far group", groups(6, 4, 2, true, false, true, true), Loop::PLAIN,
              Expect{{{true, 2, 4, true}, {false, 0, 2, false}, {false, 4, 6, false}}, true, false});
        named("split rows beside, every main unit far-queued", groups(6, 4, 0, true, true, true, true), Loop::PLAIN,
              Expect{{{true, 0, 4, true}, {false, 4, 6, true}}, true, true});
        named("split rows alone", groups(3, 0, 0, true, true, true, true), Loop::PLAIN, Expect{{{false, 0, 3, false}}, false, false});
    }
    // which units are queued: some id outside the window, and at most 48 such entries per slice
    if (rsem::unit_queued(0, 0, 8) || !rsem::unit_queued(1, 0, 8) || !rsem::unit_queued(1, 48 * 8, 8) || rsem::unit_queued(1, 48 * 8 + 1, 8) ||
        rsem::unit_queued(0, 5, 8) || rsem::unit_queued(1, -1, 8)) {
        ++n_failed;
        fprintf(stderr, "FAIL unit_queued\n");
    }
    // the adoption rule: one main unit in 25, and at least one
    if (!rsem::far_group_adopted(true, 1, 25) || rsem::far_group_adopted(true, 1, 26) || rsem::far_group_adopted(true, 0, 0) ||
        rsem::far_group_adopted(true, 0, 10) || rsem::far_group_adopted(false, 25, 25) || !rsem::far_group_adopted(true, 2, 50) ||
        rsem::far_group_adopted(true, 2, 51) || !rsem::far_group_adopted(true, 300, 300)) {
        ++n_failed;
        fprintf(stderr, "FAIL far_group_adopted\n");
    }
    printf("%ld cases, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}
