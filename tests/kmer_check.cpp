// kmer_check.cpp -- the arithmetic of the shared-k-mer count (rsem_amd/csrc/kmer_block.hpp) and the FASTA reader of
// rsem-for-ebseq-calculate-clustering-info (rsem_amd/csrc/host/fasta_codes.hpp) on the host, built by tests/test_kmer_cpu.py with
// AddressSanitizer and UBSan.
//
//   kmer_check pipeline      walks the steps of rsem_amd/csrc/kmer.hip with the header's functions -- a lane's 8 starts with the
//                            separator search and the rolled keys (lane_starts, the body k_tile runs), one stable sort per
//                            chunk (last chunk first) over key_bits bits, head flags, group indices, shared flags from neighbours, per-wave runs -- over random
//                            two- and five-letter sequences at k = 1, 2, 25, 26, 27, 28, 54, 55, 60, whole and in batches, and
//                            compares every step with brute force; then the constructions of tests/kmer_limits.py: sequences of
//                            k + 40 bases that differ in one base of the first, the last, a middle chunk or in base 27, at k = 81,
//                            82, 108, 109 and 2049, and separators on the word, lane and tile seams of the separated layout with
//                            runs of empty transcripts, at k = 1, 8, 25, 28.  Prints "ok <cases>".
//   kmer_check limits        those constructions alone.
//   kmer_check fasta FILE    prints the reader's entries as name <TAB> bases (after its warnings).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../rsem_amd/csrc/host/fasta_codes.hpp"
#include "../rsem_amd/csrc/kmer_block.hpp"

using namespace rsem_kmer;

namespace {

[[noreturn]] void fail(const char* what, int k, long at) {
    fprintf(stderr, "kmer_check: %s (k = %d, at %ld)\n", what, k, at);
    exit(1);
}

struct Input {
    std::vector<uint64_t> seq_off{0};
    std::vector<uint8_t> codes;
    int M() const { return (int)seq_off.size() - 1; }
};

Input random_input(std::mt19937& rng, int letters, int M, int max_len) {
    Input in;
    std::vector<uint8_t> motif(70);
    for (auto& c : motif) c = (uint8_t)(rng() % letters);
    for (int t = 0; t < M; t++) {
        int len = (int)(rng() % (max_len + 1));
        if (t % 7 == 3) len = 0;  // the C ABI takes empty transcripts
        std::vector<uint8_t> s(len);
        for (auto& c : s) c = (uint8_t)(rng() % letters);
        if (t % 3 == 0 && len >= 70) std::copy(motif.begin(), motif.end(), s.begin() + (int)(rng() % (len - 69)));  // shared by several
        if (t % 4 == 1 && len >= 40) std::fill(s.end() - 40, s.end(), (uint8_t)0);                                 // a poly(A) tail
        if (t % 5 == 2 && len >= 64) std::copy(s.begin(), s.begin() + 32, s.begin() + 32);                         // a repeat inside
        in.codes.insert(in.codes.end(), s.begin(), s.end());
        in.seq_off.push_back(in.codes.size());
    }
    if (M >= 2) {  // two identical transcripts
        const std::vector<uint8_t> twin(in.codes.begin() + in.seq_off[0], in.codes.begin() + in.seq_off[1]);
        for (int r = 0; r < 2; r++) {
            in.codes.insert(in.codes.end(), twin.begin(), twin.end());
            in.seq_off.push_back(in.codes.size());
        }
    }
    return in;
}

void add_seq(Input& in, const std::vector<uint8_t>& s) {
    in.codes.insert(in.codes.end(), s.begin(), s.end());
    in.seq_off.push_back(in.codes.size());
}

// tests/kmer_limits.py: large_k_seqs
Input large_k_input(std::mt19937& rng, int k) {
    std::vector<uint8_t> a(k + 40);
    for (auto& c : a) c = (uint8_t)(rng() % 4);
    const int nc = n_chunks(k), mid = kChunkBases * (nc / 2);
    Input in;
    add_seq(in, a);
    for (int at : {0, k + 39, mid, kChunkBases, kChunkBases - 1, kChunkBases * (nc - 1), kChunkBases * (nc - 1) - 1}) {
        std::vector<uint8_t> s = a;
        s[at] = (uint8_t)((s[at] + 1) % 4);
        add_seq(in, s);
    }
    add_seq(in, a);
    add_seq(in, std::vector<uint8_t>(a.begin() + 20, a.begin() + 20 + k));
    add_seq(in, std::vector<uint8_t>(a.begin() + 3, a.begin() + 3 + k - 1));
    return in;
}

// tests/kmer_limits.py: seam_seqs -- the separators' places in the separated layout
Input seam_input(std::mt19937& rng, int extra) {
    std::vector<int> seps;
    for (int i = 0; i < 16; i++) seps.push_back(300 + 41 * i);
    for (int p : {1000, 1001, 2046, 2047, 2048, 2049, 4095, 4096}) seps.push_back(p);
    for (int p = 4097; p < 3 * 2048 + extra; p++) seps.push_back(p);
    std::vector<uint8_t> motif(97), flat(seps.back() + 1);
    for (auto& c : motif) c = (uint8_t)(rng() % 4);
    for (size_t i = 0; i < flat.size(); i++) flat[i] = i % 61 ? motif[i % 97] : (uint8_t)(rng() % 5);
    Input in;
    int prev = -1;
    for (int p : seps) {
        add_seq(in, std::vector<uint8_t>(flat.begin() + prev + 1, flat.begin() + p));
        prev = p;
    }
    if (in.seq_off.back() + (uint64_t)in.M() != (uint64_t)(3 * 2048 + extra)) fail("the seam input's size", 0, extra);
    return in;
}

// brute force: k-mer -> the transcripts that hold it
std::vector<uint32_t> brute(const Input& in, int k, uint64_t& n_groups) {
    std::map<std::string, std::set<int>> owners;
    for (int t = 0; t < in.M(); t++)
        for (uint64_t p = in.seq_off[t]; p + k <= in.seq_off[t + 1]; p++) owners[std::string(in.codes.begin() + p, in.codes.begin() + p + k)].insert(t);
    std::vector<uint32_t> S(in.M(), 0);
    for (int t = 0; t < in.M(); t++)
        for (uint64_t p = in.seq_off[t]; p + k <= in.seq_off[t + 1]; p++)
            if (owners[std::string(in.codes.begin() + p, in.codes.begin() + p + k)].size() > 1) S[t]++;
    n_groups = owners.size();
    return S;
}

struct Elem { uint64_t key, pos; };

// the steps of kmer.hip for the k-mers of buckets [b_lo, b_hi)
void device_steps(const std::vector<uint8_t>& sep, const std::vector<uint64_t>& soff, int M, uint64_t Ls, int k, uint32_t b_lo, uint32_t b_hi,
                  std::vector<uint32_t>& S, uint64_t& n_groups, std::map<uint32_t, uint64_t>* hist) {
    const int nC = n_chunks(k), pb = bucket_bases(k), last_off = (nC - 1) * kChunkBases, last_len = chunk_len(k, nC - 1);
    const uint8_t* s = sep.data();
    std::vector<Elem> cur;
    // k_tile: a lane's 8 consecutive starts (the index inside the tile is the index into the separated codes here)
    for (uint64_t q0 = 0; q0 < Ls; q0 += kLaneStarts) {
        const int p0 = (int)q0;
        lane_starts(s, p0, k, last_off, last_len, pb, [&](int j, bool valid, uint64_t key, uint32_t bucket) {
            const int l = p0 + j;
            bool clean = true;
            for (int i = 0; i < k; i++) clean = clean && s[l + i] != kSep;
            if (valid != clean) fail("the separator search disagrees with the window", k, l);
            if (valid) {
                if (key != encode(s + l + last_off, last_len)) fail("the rolled key differs from the encoded one", k, l);
                if (bucket != (uint32_t)encode(s + l, pb) || bucket >= pow5(pb)) fail("the rolled bucket differs from the encoded one", k, l);
                if (hist) (*hist)[bucket]++;
                if (bucket >= b_lo && bucket < b_hi) cur.push_back({key, (uint64_t)l});
            }
        });
    }
    // one stable sort per chunk over the bits its keys can have, last chunk first
    for (int c = nC - 1; c >= 0; c--) {
        const int len = chunk_len(k, c), bits = key_bits(len);
        if (c < nC - 1)
            for (Elem& e : cur) e.key = encode(s + e.pos + c * kChunkBases, len);
        const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
        for (const Elem& e : cur)
            if (e.key & ~mask) fail("a key has more bits than key_bits says", k, (long)e.pos);
        std::stable_sort(cur.begin(), cur.end(), [&](const Elem& a, const Elem& b) { return (a.key & mask) < (b.key & mask); });
    }
    const size_t n = cur.size();
    if (!n) return;
    // k_heads, the scan, k_flags
    std::vector<uint32_t> gid(n);
    std::vector<int32_t> tid(n);
    for (size_t i = 0; i < n; i++) {
        tid[i] = find_transcript(soff.data(), M, cur[i].pos);
        if (!(soff[tid[i]] <= cur[i].pos && cur[i].pos + k < soff[tid[i] + 1])) fail("find_transcript", k, (long)cur[i].pos);
        const bool head = i == 0 || is_head(s, k, cur[i].key, cur[i - 1].key, cur[i].pos, cur[i - 1].pos);
        const bool differs = i == 0 || !std::equal(s + cur[i].pos, s + cur[i].pos + k, s + cur[i - 1].pos);
        if (head != differs) fail("the head flag disagrees with the k-mers", k, (long)i);
        gid[i] = (i ? gid[i - 1] : 0) + (head ? 1 : 0);
    }
    std::vector<uint8_t> group(n, 0);
    for (size_t i = 1; i < n; i++)
        if (gid[i] == gid[i - 1] && tid[i] != tid[i - 1]) group[gid[i] - 1] = 1;
    n_groups += gid[n - 1];
    // k_count: waves of 64, one add per run of equal transcript
    for (size_t w0 = 0; w0 < n; w0 += 64) {
        int32_t t[64];
        for (int lane = 0; lane < 64; lane++) t[lane] = (w0 + lane < n && group[gid[w0 + lane] - 1]) ? tid[w0 + lane] : -1;
        uint64_t boundary = 0;
        for (int lane = 0; lane < 64; lane++)
            if (lane == 0 || t[lane - 1] != t[lane]) boundary |= 1ull << lane;
        for (int lane = 0; lane < 64; lane++)
            if (t[lane] >= 0 && (boundary >> lane & 1)) {
                const int len = run_length(boundary, lane, 64);
                for (int i = 0; i < len; i++)
                    if (t[lane + i] != t[lane]) fail("a run holds another transcript", k, (long)(w0 + lane));
                if (lane + len < 64 && t[lane + len] == t[lane]) fail("a run ends early", k, (long)(w0 + lane));
                S[t[lane]] += (uint32_t)len;
            }
    }
}

int check_input(const Input& in, int k) {
    const int M = in.M();
    const uint64_t L = in.seq_off[M], Ls = L + (uint64_t)M;
    std::vector<uint8_t> sep((size_t)Ls + k + 32, (uint8_t)kSep);
    std::vector<uint64_t> soff(M + 1);
    for (int t = 0; t < M; t++) {
        soff[t] = in.seq_off[t] + t;
        std::copy(in.codes.begin() + in.seq_off[t], in.codes.begin() + in.seq_off[t + 1], sep.begin() + soff[t]);
    }
    soff[M] = Ls;
    uint64_t want_groups = 0;
    const std::vector<uint32_t> want = brute(in, k, want_groups);
    const uint32_t nbuckets = (uint32_t)pow5(bucket_bases(k));

    std::map<uint32_t, uint64_t> hist;
    std::vector<uint32_t> S(M, 0);
    uint64_t groups = 0, total = 0;
    device_steps(sep, soff, M, Ls, k, 0, nbuckets, S, groups, &hist);
    if (S != want || groups != want_groups) fail("the counts of the whole input differ from brute force", k, -1);
    for (auto& h : hist) total += h.second;

    int cases = 1;
    std::vector<uint64_t> dense(nbuckets, 0);
    for (auto& h : hist) dense[h.first] = h.second;
    for (uint64_t budget : {total / 3 + 1, (uint64_t)1}) {
        if (budget == 1 && hist.size() > 400) continue;  // one batch per bucket: kept to the inputs with few buckets
        std::fill(S.begin(), S.end(), 0u);
        groups = 0;
        uint64_t seen = 0;
        int nb = 0;
        for (uint32_t lo = 0; lo < nbuckets;) {
            uint64_t items;
            const uint32_t hi = batch_end(dense, nbuckets, lo, budget, items);
            if (hi <= lo) fail("a batch without a bucket", k, lo);
            if (items > budget) {  // only a single bucket may exceed the budget
                int nonempty = 0;
                for (uint32_t b = lo; b < hi; b++) nonempty += dense[b] > 0;
                if (nonempty != 1) fail("a batch above the budget holds more than one bucket", k, lo);
            }
            if (items) {
                device_steps(sep, soff, M, Ls, k, lo, hi, S, groups, nullptr);
                nb++;
            }
            seen += items;
            lo = hi;
        }
        if (seen != total) fail("the batches do not hold every k-mer", k, -1);
        if (total && budget < total && budget > 1 && nb < 2) fail("one batch where several were expected", k, nb);
        if (S != want || groups != want_groups) fail("the counts of the batched input differ from brute force", k, (long)budget);
        cases++;
    }
    return cases;
}

// the constructions of tests/kmer_limits.py
int limit_cases(std::mt19937& rng) {
    int cases = 0;
    for (int k : {81, 82, 108, 109, 2049}) cases += check_input(large_k_input(rng, k), k);
    for (int extra : {0, 1}) {
        const Input in = seam_input(rng, extra);
        for (int k : {1, 8, 25, 28}) cases += check_input(in, k);
    }
    {  // exactly one k-mer, between transcripts that have none
        Input in;
        add_seq(in, {});
        add_seq(in, std::vector<uint8_t>(27, 1));
        add_seq(in, std::vector<uint8_t>(28, 2));
        add_seq(in, {});
        cases += check_input(in, 28);
    }
    return cases;
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc == 2 && std::string(argv[1]) == "limits") {  // the limit constructions alone
        std::mt19937 rng(12345);
        printf("ok %d\n", limit_cases(rng));
        return 0;
    }
    if (argc == 2 && std::string(argv[1]) == "pipeline") {
        if (pow5(27) >= (1ull << 63) || key_bits(27) != 63 || key_bits(1) != 3 || key_bits(2) != 5) fail("key_bits", 0, 0);
        if (n_chunks(27) != 1 || n_chunks(28) != 2 || n_chunks(54) != 2 || n_chunks(55) != 3 || chunk_len(60, 2) != 6 || chunk_len(28, 1) != 1)
            fail("chunks", 0, 0);
        std::mt19937 rng(12345);
        int cases = 0;
        for (int letters : {2, 5})
            for (int k : {1, 2, 25, 26, 27, 28, 54, 55, 60}) {
                const Input in = random_input(rng, letters, 24, 150);
                cases += check_input(in, k);
            }
        cases += limit_cases(rng);
        printf("ok %d\n", cases);
        return 0;
    }
    if (argc == 3 && std::string(argv[1]) == "fasta") {
        rsemh::FastaCodes fa;
        if (!rsemh::read_fasta_codes(argv[2], fa)) return 2;
        for (int i = 0; i < fa.M(); i++) {
            fwrite(fa.names[i].data(), 1, fa.names[i].size(), stdout);
            fputc('\t', stdout);
            for (uint64_t p = fa.seq_off[i]; p < fa.seq_off[i + 1]; p++) fputc("ACGTN"[fa.codes[p]], stdout);
            fputc('\n', stdout);
        }
        return 0;
    }
    fprintf(stderr, "usage: kmer_check pipeline | kmer_check limits | kmer_check fasta FILE\n");
    return 64;
}
