// simulate_emu.cpp -- TEST INFRASTRUCTURE: runs rsem_amd/csrc/simulate_block.hpp (the attempt of rsem-simulate-reads and the search
// for the attempts a stream of generator words holds: the file simulate.hip compiles for the GPU) on the CPU, over the tables
// rsem_amd/csrc/host/simulate_host.hpp builds from a program's input files.  No lane of those kernels talks to another one, so a lane
// is a loop iteration here; the kernels' order is kept: an attempt at every word of a chunk, the tiles' exits, the hop, the marks,
// the prefix sums, the reads.  Built with the sanitizers by tests/test_simulate_emu_cpu.py.  Never part of the product.
//
//   simulate_emu ref model results theta0 N seed reference|counter chunk_words tile out.txt
//
// out.txt: a line per read "rid dir sid pos insertL attempts seq1 qual1 seq2 qual2" ("-": none), "counts ..." and "resim n".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rsem_amd/csrc/host/ci_stream.hpp"
#include "../rsem_amd/csrc/host/simulate_host.hpp"
#include "../rsem_amd/csrc/simulate_block.hpp"

using namespace rsem_simk;

namespace {

struct Read {
    Attempt a;
    uint64_t attempts;
    std::string s1, q1, s2, q2;
};

Tables tables_of(const rsem_sim_model& m) {
    Tables T{};
    T.type = m.type; T.M = m.M; T.has_mld = m.has_mld; T.est_rspd = m.est_rspd; T.B = m.B; T.pro_len = m.pro_len;
    T.g_lb = m.g_lb; T.g_ub = m.g_ub; T.m_lb = m.m_lb; T.m_ub = m.m_ub; T.prob_f = m.prob_f;
    T.theta_cdf = m.theta_cdf; T.full_len = m.full_len; T.tot_len = m.tot_len; T.seq_off = m.seq_off; T.seq = m.seq;
    T.g_cdf = m.g_cdf; T.m_cdf = m.m_cdf; T.r_pdf = m.r_pdf; T.r_cdf = m.r_cdf; T.qc_init = m.qc_init; T.qc_trans = m.qc_trans; T.pc = m.pc; T.npc = m.npc;
    T.max_len = m.has_mld ? m.m_ub : m.g_ub;
    T.plain = tables_plain(m) ? 1 : 0;
    return T;
}

template <class Src>
Read emit(const Tables& T, Src& s) {
    Read r;
    std::vector<uint8_t> b((size_t)T.max_len * 4 + 4, 0);
    uint8_t *s1 = b.data(), *q1 = s1 + T.max_len, *s2 = q1 + T.max_len, *q2 = s2 + T.max_len;
    attempt<true>(T, s, r.a, s1, q1, s2, q2);
    if (r.a.ok) {
        r.s1.assign((const char*)s1, r.a.len1);
        if (T.has_q()) r.q1.assign((const char*)q1, r.a.len1);
        if (T.paired()) {
            r.s2.assign((const char*)s2, r.a.len2);
            if (T.has_q()) r.q2.assign((const char*)q2, r.a.len2);
        }
    }
    return r;
}

[[noreturn]] void stop(const char* what, int status) {
    fprintf(stderr, "simulate_emu: %s (status %d)\n", what, status);
    exit(3);
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc != 11) { fprintf(stderr, "usage: simulate_emu ref model results theta0 N seed reference|counter chunk_words tile out.txt\n"); return 2; }
    rsemh::SimInputs in;
    rsemh::load_sim_inputs(in, argv[1], argv[2], argv[3], argv[4], false);
    const Tables T = tables_of(in.sm);
    const long long N = atoll(argv[5]);
    const uint32_t seed = (uint32_t)strtoul(argv[6], nullptr, 10);
    const bool counter = !strcmp(argv[7], "counter");
    const uint64_t chunk = strtoull(argv[8], nullptr, 10);
    const uint32_t tile = (uint32_t)strtoul(argv[9], nullptr, 10);
    std::vector<Read> reads;
    std::vector<uint64_t> counts((size_t)T.M + 1, 0);
    uint64_t resim = 0;

    if (counter) {  // k_sim_counter
        for (long long j = 0; j < N; j++) {
            uint32_t failed = 0;
            for (;;) {
                CounterSource s(seed, (uint64_t)j, failed);
                Read r = emit(T, s);
                if (r.a.status != kOk) stop("an attempt ended with a status", r.a.status);
                if (r.a.ok) { r.attempts = failed; reads.push_back(r); break; }
                if (++failed >= kDefaultAttemptCap) stop("attempt cap", kAttemptCap);
            }
            resim += failed;
        }
    } else {  // rsem_sim_reference_batch with every read in one batch
        rsemh::RefMt19937 gen(seed);
        std::vector<uint32_t> pending;
        const uint32_t longest = longest_attempt(T);
        uint64_t carry = 0;
        long long got = 0;
        while (got < N) {
            const long long want = N - got;
            const uint32_t n_pos = (uint32_t)std::min<uint64_t>(chunk, (uint64_t)want * longest), n_words = n_pos + longest, n_tiles = (n_pos + tile - 1) / tile;
            while (pending.size() < n_words) pending.push_back(gen.next());
            std::vector<uint32_t> next_ok(n_pos), exit_of(n_pos), entry(n_tiles, 0xffffffffu), starts;
            std::vector<uint64_t> flags((size_t)n_pos + 1, 0), sums((size_t)n_pos + 1, 0);
            for (uint32_t p = 0; p < n_pos; p++) {  // k_sim_heads
                WordSource s(pending.data(), n_words, p);
                Attempt a;
                attempt<false>(T, s, a, nullptr, nullptr, nullptr, nullptr);
                next_ok[p] = (p + (a.draws ? a.draws : 1u)) | ((a.ok || (a.status != kOk && a.status != kPastWords)) ? kOkBit : 0u);
            }
            for (uint32_t t = 0; t < n_tiles; t++) {  // k_sim_tile_exits
                const uint32_t t0 = t * tile, t1 = std::min(t0 + tile, n_pos);
                std::vector<uint32_t> lds(next_ok.begin() + t0, next_ok.begin() + t1);
                tile_exits_in_place(lds.data(), t0, t1);
                std::copy(lds.begin(), lds.end(), exit_of.begin() + t0);
            }
            uint32_t p = 0;  // k_sim_hop
            while (p < n_pos) { entry[p / tile] = p; p = exit_of[p]; }
            const uint32_t exit_pos = p;
            for (uint32_t t = 0; t < n_tiles; t++) {  // k_sim_mark
                uint32_t q = entry[t];
                if (q == 0xffffffffu) continue;
                const uint32_t t1 = std::min(t * tile + tile, n_pos);
                while (q < t1) { flags[q] = (next_ok[q] & kOkBit) ? 1ull : 1ull << 32; q = next_ok[q] & ~kOkBit; }
            }
            for (uint32_t q = 0; q < n_pos; q++) sums[q + 1] = sums[q] + flags[q];  // the exclusive sum
            const uint64_t seen = sums[n_pos] & 0xffffffffull, fails = sums[n_pos] >> 32;
            const uint32_t n = (uint32_t)std::min<uint64_t>(seen, (uint64_t)want);
            starts.resize(n);
            for (uint32_t q = 0; q < n_pos; q++)  // k_sim_starts
                if ((flags[q] & 0xffffffffull) && (sums[q] & 0xffffffffull) < n) starts[sums[q] & 0xffffffffull] = q;
            uint64_t consumed = exit_pos, last_fails = 0;
            for (uint32_t j = 0; j < n; j++) {  // k_sim_body
                WordSource s(pending.data(), n_words, starts[j]);
                Read r = emit(T, s);
                if (r.a.status != kOk || !r.a.ok) stop("the attempt at a visited start gave no read", r.a.status);
                const uint64_t before = sums[starts[j]] >> 32;
                r.attempts = j ? before - (sums[starts[j - 1]] >> 32) : before + carry;
                if (j == n - 1) { last_fails = before; if (seen > n) consumed = starts[j] + r.a.draws; }
                reads.push_back(r);
            }
            if (n) {  // a failed attempt counts when a read claims it; those behind the last read taken are carried
                resim += carry + last_fails;
                carry = seen > n ? 0 : fails - last_fails;
            } else carry += fails;
            if (carry >= kDefaultAttemptCap) stop("attempt cap", kAttemptCap);
            if (exit_pos < n_pos || consumed == 0 || consumed > n_words) stop("the chunk's exit is out of range", -1);
            pending.erase(pending.begin(), pending.begin() + (size_t)consumed);
            got += n;
        }
    }

    FILE* fo = fopen(argv[10], "w");
    if (!fo) { perror(argv[10]); return 2; }
    for (size_t i = 0; i < reads.size(); i++) {
        const Read& r = reads[i];
        counts[(size_t)r.a.sid]++;
        auto txt = [](const std::string& s) { return s.empty() ? "-" : s.c_str(); };
        fprintf(fo, "%zu %d %d %d %d %llu %s %s %s %s\n", i, r.a.dir, r.a.sid, r.a.pos, r.a.insert_l, (unsigned long long)r.attempts, txt(r.s1), txt(r.q1), txt(r.s2), txt(r.q2));
    }
    fprintf(fo, "counts");
    for (uint64_t c : counts) fprintf(fo, " %llu", (unsigned long long)c);
    fprintf(fo, "\nresim %llu\n", (unsigned long long)resim);
    fclose(fo);
    return 0;
}
