// round_close_emu.cpp -- TEST INFRASTRUCTURE: rsem_amd/csrc/round_close.hpp (the closer of an EM round: slice walk, statistics,
// workgroup reduction, arrival, the last arrival's publication) on the CPU, simt_emu.hpp's way: 256 OS threads are ONE workgroup.
// The closers of a round therefore run ONE AFTER ANOTHER, in a shuffled arrival order: this checks the protocol's logic -- who
// counts as last, what the last one publishes, what it leaves behind for the next round, that nothing depends on the order of
// arrival -- and NOT its concurrency (closers racing each other on bbits / tick2 only happen on the GPU).
//
//   round_close_emu slices N_CLOSERS N_ORDERS   n = M + 1 in {1, 5, 127, 128, 129, 2048 N_CLOSERS, 2048 N_CLOSERS + 1}
//   round_close_emu edges  N_CLOSERS N_ORDERS   n = 300 with elements ON the two thresholds of EM.cpp:406-411
//
// Per n: three consecutive rounds on one Ctrl (rounds 1023, 1024, 1025: the ring of the host's lines wraps) under N_ORDERS orders
// of arrival -- the first two are "closer n-1 last" and "closer 0 last" -- with min_round = 1024 and max_round = 1025; then, under
// two orders, a run whose theta does not move (totNum = 0: round 1023 goes on because it is below min_round, round 1024 stops).  Everything is compared with serial() below: the reference's lines
// (EM.cpp:400-416) written out, and the slot-order sum spelled as loops over arrays.
// Prints "ok" or lines starting with "BAD".  Build (tests/test_round_close_emu_cpu.py): hipcc -DRSEM_EMU tests/round_close_emu.cpp -lpthread
// A closer is some forty barriers and a case tens of thousands of closers: with the machine's default barrier (a sleep and a
// wake-up per lane and barrier) that is half an hour.
#define RSEM_EMU_SPIN_BARRIER
#include "simt_emu.hpp"

namespace {
using rsem::kEpsilon;
constexpr int kTotSlots = 64;
constexpr int kWindow = 2048;
#include "../rsem_amd/csrc/estep_block.hpp"
#include "../rsem_amd/csrc/round_close.hpp"
}  // namespace

static uint64_t g_rng = 1;
static double urand() {  // [0, 1)
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) * (1.0 / 9007199254740992.0);
}
static bool same_bits(double a, double b) { return !memcmp(&a, &b, 8); }

struct RoundData {
    std::vector<double> counts, old;
    double sum = 1.0;
    // serial(): what the round's line must say
    int tot = 0;
    double bmax = 0.0, slot_sum = 0.0;
    bool stop = false;
};

// EM.cpp:400-416 for one round, and the sum of the counts in the order the closers are specified to add it up: every thread its
// elements in index order, a butterfly over the 64 lanes of a wave, the 4 waves in order, the closers in order.
static void serial(RoundData& R, int n, int n_closers, int round, int min_round, int max_round) {
    R.tot = 0;
    R.bmax = 0.0;
    for (int i = 0; i < n; i++) {
        const double th = R.counts[i] / R.sum;
        if (R.old[i] >= 1e-7) {
            const double change = fabs(th - R.old[i]) / R.old[i];
            if (change >= 0.001) ++R.tot;
            if (R.bmax < change) R.bmax = change;
        }
    }
    R.stop = !(round < min_round || (R.tot > 0 && round < max_round));
    const int per = (n + n_closers - 1) / n_closers;
    R.slot_sum = 0.0;
    for (int me = 0; me < n_closers; me++) {
        double part[256] = {};
        for (int i = me * per; i < std::min(n, me * per + per); i++) part[(i - me * per) % 256] += R.counts[i];
        double closer = 0.0;
        for (int w = 0; w < 4; w++) {
            double v[64], t[64];
            memcpy(v, part + 64 * w, sizeof(v));
            for (int d = 32; d >= 1; d >>= 1) {
                for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ d];
                memcpy(v, t, sizeof(v));
            }
            closer = w == 0 ? v[0] : closer + v[0];
        }
        R.slot_sum += closer;
    }
}

struct Run {  // one n under one order of arrival
    int n = 0, n_closers = 0, round0 = 1022, min_round = 1024, max_round = 1025;
    RoundData* rounds = nullptr;  // [3]
    std::vector<int> order;
    int bad = 0;
    Ctrl ctrl;
    HostMirror mirror;
    CloseScratch scratch;
    int n_last = 0, last_me = -1;
    emu::Block blk;
};

#define CHECK(cond, what)                                                                                                      \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            printf("BAD n %d closers %d round %d last closer %d: %s\n", J->n, J->n_closers, round, J->order.back(), what);      \
            ++J->bad;                                                                                                          \
        }                                                                                                                      \
    } while (0)

static void check_round(Run* J, int round, const RoundData& R) {
    const Ctrl& c = J->ctrl;
    const double want_sum = R.slot_sum;
    CHECK(J->n_last == 1 && J->last_me == J->order.back(), "exactly the closer that arrived last must see itself as the last");
    CHECK(c.last_totNum == R.tot, "totNum");
    CHECK(same_bits(c.last_bchange, R.bmax), "bChange");
    CHECK(same_bits(c.last_sum, want_sum), "sum");
    CHECK(c.last_round == round, "last_round");
    const RoundStat& h = J->mirror.hist[(round - 1) % kHistCap];
    CHECK(h.round == round && h.totNum == R.tot && same_bits(h.bchange, R.bmax) && same_bits(h.sum, want_sum), "the host's line");
    CHECK(J->mirror.last_round == round, "the host's last_round");
    if (R.stop) CHECK(c.done == 1 && c.final_round == round && J->mirror.done == 1 && J->mirror.final_round == round, "stop: done / final_round");
    else CHECK(c.done == 0 && J->mirror.done == 0, "no stop: done must stay clear");
    CHECK(c.bbits == 0ull && c.tick2 == 0ull, "bbits / tick2 must be left clean");
}

static void thread_body(Run* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    const int per = (J->n + J->n_closers - 1) / J->n_closers;
    for (int q = 0; q < 3; q++) {
        const RoundData& R = J->rounds[q];
        const int round = J->round0 + 1 + q;
        for (int me : J->order) {  // a closer: what the kernels of em.hip do around the header's pieces
            const int lo = me * per, hi = std::min(J->n, lo + per);
            SliceWalk walk;
            walk.load(lo, hi, 256, R.counts.data(), R.old.data());
            CloseAcc acc;
            walk.each(R.counts.data(), R.old.data(), [&](int, double c, double old) { acc.add(c, c / R.sum, old); });
            close_reduce(acc, &J->scratch);
            if (tid == 0 && close_arrive(&J->ctrl, &J->mirror, me, J->n_closers, acc, round, J->min_round, J->max_round)) {
                ++J->n_last;
                J->last_me = me;
            }
            RSEM_SYNC();  // (the next closer takes the same scratch: on the GPU it is another workgroup's)
        }
        if (tid == 0) {
            check_round(J, round, R);
            J->n_last = 0;
            J->last_me = -1;
        }
        RSEM_SYNC();
        if (R.stop) break;  // (the kernels return at once behind a stop)
    }
}

static int run_one(Run* J) {
    memset(&J->ctrl, 0, sizeof(Ctrl));
    memset(&J->mirror, 0, sizeof(HostMirror));
    J->bad = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back(thread_body, J, t);
    for (auto& t : th) t.join();
    return J->bad;
}

// counts / previous theta of one round.  quiet: theta does not move (sum = 1, counts = previous theta).
static void fill(RoundData& R, int n, bool quiet) {
    R.counts.assign(n, 0.0);
    R.old.assign(n, 0.0);
    R.sum = quiet ? 1.0 : 1000.25;
    for (int i = 0; i < n; i++) {
        const double kind = urand();
        const double old = kind < 0.125 ? 0.0 : (kind < 0.25 ? 5e-8 * (1.0 + urand()) * 0.99 : (1.0 + urand()) / (n + 8.0));
        R.old[i] = old;
        if (quiet) R.counts[i] = old;
        else R.counts[i] = old == 0.0 ? urand() * 1e-3 : old * R.sum * (1.0 + (urand() - 0.5) * 0.006);
    }
}

// elements ON the thresholds (sum = 1: theta is the count itself).  Returns false when no pair with change == 0.001 was found.
static bool plant_edges(RoundData& R) {
    R.sum = 1.0;
    double e_old = 0.0, e_th = 0.0;
    for (int j = 0; j < 200000 && e_old == 0.0; j++) {
        const double old = 1e-3 * (1.0 + j * 1e-6);
        double th = old * 1.001;
        for (int k = 0; k < 4; k++) th = nextafter(th, 0.0);
        for (int k = 0; k < 9; k++, th = nextafter(th, 1.0))
            if (fabs(th - old) / old == 0.001) { e_old = old; e_th = th; break; }
    }
    if (e_old == 0.0) return false;
    double below = nextafter(e_th, 0.0);
    while (fabs(below - e_old) / e_old >= 0.001) below = nextafter(below, 0.0);
    const double under = nextafter(1e-7, 0.0);
    struct { int i; double old, c; } E[] = {
        {0, e_old, e_th}, {1, e_old, below},        // change exactly 0.001: counted; just below: not
        {127, 1e-7, 2e-7}, {128, under, 4.0 * under},  // old exactly 1e-7: its change of 1 enters; just below: its change of 3 must not
        {129, 0.0, 0.25}, {255, e_old, below}, {256, e_old, e_th}, {299, 1e-7, 1e-7 * 1.002},
    };
    for (const auto& e : E) { R.old[e.i] = e.old; R.counts[e.i] = e.c; }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const bool edges = !strcmp(argv[1], "edges");
    const int n_closers = atoi(argv[2]), n_orders = atoi(argv[3]);
    if (n_closers < 1 || n_closers > kSumSlots || n_orders < 2) return 2;
    std::vector<int> ns = {1, 5, 127, 128, 129, 2048 * n_closers, 2048 * n_closers + 1};
    if (edges) ns = {300};
    Run* J = new Run();
    emu::barrier_init(&J->blk.bar, 256);
    for (int w = 0; w < 4; w++) emu::barrier_init(&J->blk.w[w].bar, 64);
    int bad = 0;
    for (int n : ns) {
        g_rng = 1000003ull * n + n_closers;
        RoundData moving[3], quiet[3];
        for (int q = 0; q < 3; q++) {
            fill(moving[q], n, false);
            fill(quiet[q], n, true);
            if (edges && !plant_edges(moving[q])) { printf("BAD no theta with a change of exactly 0.001 found\n"); return 1; }
            serial(moving[q], n, n_closers, J->round0 + 1 + q, J->min_round, J->max_round);
            serial(quiet[q], n, n_closers, J->round0 + 1 + q, J->min_round, J->max_round);
        }
        if (edges) {  // the planted elements do what they were planted for (the rest of the slice moves by less than 0.3 %)
            RoundData only = moving[0];
            for (int i = 0; i < n; i++)
                if (i != 0 && i != 1 && i != 127 && i != 128 && i != 129 && i != 255 && i != 256 && i != 299) only.old[i] = 0.0;
            serial(only, n, n_closers, 1, 1, 1);
            if (only.tot != 4 || only.bmax != 1.0) { printf("BAD the planted elements give totNum %d bChange %.17g, not 4 and 1\n", only.tot, only.bmax); ++bad; }
        }
        if (quiet[0].tot != 0 || quiet[0].stop || !quiet[1].stop || !moving[2].stop) { printf("BAD n %d: the quiet run's own expectations\n", n); ++bad; }
        J->n = n;
        J->n_closers = n_closers;
        std::vector<int> id(n_closers);
        for (int i = 0; i < n_closers; i++) id[i] = i;
        double first_sum[3] = {};
        for (int o = 0; o < n_orders + 2; o++) {
            J->order = id;
            if (o % 2 == 1) std::reverse(J->order.begin(), J->order.end());  // closer 0 last (o even: closer n-1 last)
            if (o >= 2 && o < n_orders) {                                      // ... and shuffles
                for (int i = n_closers - 1; i > 0; i--) std::swap(J->order[i], J->order[(int)(urand() * (i + 1))]);
            }
            J->rounds = o >= n_orders ? quiet : moving;
            bad += run_one(J);
            // the sum is the same bits under every order (check_round compared it with serial()'s; this is the direct statement)
            if (J->rounds == moving) {
                if (o == 0) first_sum[0] = J->ctrl.last_sum;
                else if (!same_bits(first_sum[0], J->ctrl.last_sum)) { printf("BAD n %d: the sum depends on the order of arrival\n", n); ++bad; }
            }
        }
        printf("n %d closers %d: totNum %d %d %d bChange %.17g sum %.17g\n", n, n_closers, moving[0].tot, moving[1].tot, moving[2].tot, moving[2].bmax,
               moving[2].slot_sum);
        fflush(stdout);
    }
    delete J;
    printf(bad ? "BAD\n" : "ok\n");
    return bad ? 1 : 0;
}
