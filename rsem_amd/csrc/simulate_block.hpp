// simulate_block.hpp -- one attempt of rsem-simulate-reads: the draw program of the four read models'
// simulate members (SingleModel.h:413-452, SingleQModel.h:428-471, PairedEndModel.h:372-415, PairedEndQModel.h:386-433) and of their
// parts (simul.h:17-35, Orientation.h:36, LenDist.h:255-263, RSPD.h:195-198, QualDist.h:132-145, Profile.h:207-214, QProfile.h:195-202,
// NoiseProfile.h:146-153, NoiseQProfile.h:168-175), and the search for the attempts a stream of generator words holds.
// simulate.hip runs it on the device, a lane an attempt; tests/simulate_emu.cpp runs the same source on the host.
//
// An attempt is a pure function of the tables and of its uniforms: uniform k of an attempt is word k of its source times 2^-32.
// Two sources: a place in an array of MT19937 outputs (the reference's own stream) and a Philox4x32-10 counter (read, attempt, k / 4).
// No lane talks to another one here and nothing is accumulated in floating point: every double is the reference's, bit for bit
// (the file is compiled without contraction into fused multiply-adds).
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include "rng.hpp"
#define RSEM_SIM_FN __host__ __device__ inline
#else
#error "simulate_block.hpp is compiled by hipcc (device code in simulate.hip, host code in tests/simulate_emu.cpp)"
#endif

namespace rsem_simk {

constexpr int kQ = 100;       // QualDist.h:34, QProfile.h:35, NoiseQProfile.h:43
constexpr int kCodes = 5;     // A C G T N
constexpr uint32_t kDefaultAttemptCap = 1u << 20;  // failed attempts after which a read ends the run

// rsem_sim_batch.status (include/rsem_hip.h)
enum Status : int32_t { kOk = 0, kAttemptCap = 1, kShortInsert = 2, kPastProfile = 3, kQualityRange = 4, kPastWords = 5 };
constexpr int kMaxQuality = 93;  // QualDist.h:11: 33 to 126 encode 0 to 93; the tables have 100 rows

// the tables of a model after startSimulation, flat; index 0 of the per-transcript arrays is the noise "transcript"
struct Tables {
    int32_t type;      // 0 Single, 1 SingleQ, 2 PairedEnd, 3 PairedEndQ
    int32_t M;
    int32_t has_mld;   // single-end: a mate-length distribution was given; paired-end: always
    int32_t est_rspd, B;
    int32_t pro_len;   // positions of the no-quality profile
    int32_t g_lb, g_ub, m_lb, m_ub;
    int32_t plain;     // no table an attempt can reach has a total of 0: every sample() takes one uniform
    int32_t max_len;   // the longest read (the stride of the output bytes)
    double prob_f;
    const double* theta_cdf;   // [M + 1]
    const int32_t* full_len;   // [M + 1]
    const int32_t* tot_len;    // [M + 1]
    const uint64_t* seq_off;   // [M + 2]: transcript i's forward strand (poly(A) tail included) at seq + seq_off[i]
    const uint8_t* seq;
    const double* g_cdf;       // [g_ub - g_lb + 1], [0] = 0
    const double* m_cdf;
    const double* r_pdf;       // [B + 2]
    const double* r_cdf;
    const double* qc_init;     // [100]
    const double* qc_trans;    // [100][100]
    const double* pc;          // [100][5][5] with qualities, [pro_len][5][5] without: after the repair of all-zero rows
    const double* npc;         // [100][5] with qualities, [5] without
    RSEM_SIM_FN bool has_q() const { return type == 1 || type == 3; }
    RSEM_SIM_FN bool paired() const { return type >= 2; }
};

// ---- the two sources of uniforms ------------------------------------------------------------------------------------------------

// words[at + k]; a read past the array is not made: it counts as word 0 and is reported
struct WordSource {
    const uint32_t* words;
    uint64_t n_words, at;
    uint32_t k = 0;
    bool past = false;
    RSEM_SIM_FN WordSource(const uint32_t* w, uint64_t n, uint64_t start) : words(w), n_words(n), at(start) {}
    RSEM_SIM_FN double next() {
        const uint64_t i = at + k++;
        if (i >= n_words) { past = true; return 0.0; }
        return (double)words[i] * (1.0 / 4294967296.0);
    }
    RSEM_SIM_FN void skip(uint32_t n) { k += n; }
};

// Philox4x32-10 keyed by the seed, counter = (read id low, read id high, attempt, k / 4); uniform k is word k % 4
struct CounterSource {
    rsem::Philox ph;
    uint32_t c0, c1, c2;
    uint32_t k = 0, have = 0xffffffffu;
    uint32_t w[4];
    bool past = false;
    RSEM_SIM_FN CounterSource(uint64_t seed, uint64_t read, uint32_t attempt) : ph{(uint32_t)seed, (uint32_t)(seed >> 32)}, c0((uint32_t)read), c1((uint32_t)(read >> 32)), c2(attempt) {}
    RSEM_SIM_FN double next() {
        const uint32_t blk = k >> 2;
        if (blk != have) { ph.gen(c0, c1, c2, blk, w); have = blk; }
        return (double)w[k++ & 3u] * (1.0 / 4294967296.0);
    }
    RSEM_SIM_FN void skip(uint32_t n) { k += n; }
};

// ---- simul::sample (simul.h:17-35) -------------------------------------------------------------------------------------------------

// at(i): entry i of a running-sum table of len entries.  prb = u * total; the first entry above prb: an entry equal to prb is passed
// (zero-width entries are never picked, a tie goes right); a table whose total is 0 takes a second uniform: int(u * len)
template <class Src, class At>
RSEM_SIM_FN int sample(Src& s, At at, int len) {
    const double prb = s.next() * at(len - 1);
    int l = 0, r = len - 1;
    while (l <= r) {
        const int mid = (l + r) / 2;
        if (at(mid) <= prb) l = mid + 1;
        else r = mid - 1;
    }
    if (l >= len) l = (int)(s.next() * len);
    return l;
}

struct ArrayAt {
    const double* a;
    RSEM_SIM_FN double operator()(int i) const { return a[i]; }
};

// RSPD::evalCDF (RSPD.h:63-68); entry j of the table RSPD::startSimulation builds for a transcript (RSPD.h:191) is eval_cdf(j + 1)
RSEM_SIM_FN double eval_cdf(const Tables& T, int fpos, int full_len) {
    const int i = (int)(((long long)fpos) * T.B / full_len);
    const double val = fpos * 1.0 / full_len * T.B;
    return T.r_cdf[i] + (val - i) * T.r_pdf[i + 1];
}
struct RspdAt {
    const Tables* T;
    int full_len;
    RSEM_SIM_FN double operator()(int j) const { return eval_cdf(*T, j + 1, full_len); }
};

// LenDist::simulate (LenDist.h:255-263): -1, WITHOUT a draw, where no length fits
template <class Src>
RSEM_SIM_FN int draw_length(Src& s, int lb, int ub, const double* cdf, int ref_l) {
    if (ref_l == -1) ref_l = ub;
    if (ref_l <= lb) return -1;
    const int dlen = (ub < ref_l ? ub : ref_l) - lb;
    if (cdf[dlen] <= 0.0) return -1;
    return lb + 1 + sample(s, ArrayAt{cdf + 1}, dlen);
}

// RefSeq::get_id (RefSeq.h:84-87, utils.h:36-76): the code of the base at pos of strand dir
RSEM_SIM_FN int base_code(uint8_t c) {
    switch (c | 0x20) {
        case 'a': return 0;
        case 'c': return 1;
        case 'g': return 2;
        case 't': return 3;
        default: return 4;
    }
}
RSEM_SIM_FN int ref_code(const Tables& T, int sid, int pos, int dir) {
    const uint8_t* s = T.seq + T.seq_off[sid];
    if (dir == 0) return base_code(s[pos]);
    const int c = base_code(s[T.tot_len[sid] - pos - 1]);
    return c == 4 ? 4 : 3 - c;
}
RSEM_SIM_FN uint8_t code_letter(int c) { return (uint8_t)("ACGTN"[c]); }

// ---- one read (one mate): its qualities, then its bases ----------------------------------------------------------------------------

// kEmit: the bytes are written; otherwise only the uniforms are counted -- and where the tables are plain they are skipped, not drawn.
// sid 0: bases from the noise profile; otherwise from the profile row of the reference base.
template <bool kEmit, class Src>
RSEM_SIM_FN int32_t draw_mate(const Tables& T, Src& s, int sid, int len, int pos, int dir, uint8_t* seq, uint8_t* qual) {
    const bool q = T.has_q();
    if (!q && len > T.pro_len && (sid != 0)) return kPastProfile;  // Profile.h:211 would read past its table
    if (!kEmit && T.plain) { s.skip(q ? 2u * (uint32_t)len : (uint32_t)len); return kOk; }
    if (q) {
        // The reference draws all qualities (QualDist.h:132-145), then all bases.  Where the bytes are written the qualities are read back
        // from them.  Where the uniforms are only counted nothing is kept: a copy of the source draws the chain of qualities a second
        // time, one step ahead of the bases that need them.
        Src again = s;
        int qv = 0;
        for (int i = 0; i < len; i++) {
            qv = i == 0 ? sample(s, ArrayAt{T.qc_init}, kQ) : sample(s, ArrayAt{T.qc_trans + qv * kQ}, kQ);
            if (qv > kMaxQuality) return kQualityRange;  // (the reference ends at the assertion of c2q, QProfile.h:40)
            if (kEmit) qual[i] = (uint8_t)(qv + 33);
        }
        qv = 0;
        for (int i = 0; i < len; i++) {
            if (kEmit) qv = qual[i] - 33;
            else qv = i == 0 ? sample(again, ArrayAt{T.qc_init}, kQ) : sample(again, ArrayAt{T.qc_trans + qv * kQ}, kQ);
            const double* row = sid == 0 ? T.npc + qv * kCodes : T.pc + (qv * kCodes + ref_code(T, sid, i + pos, dir)) * kCodes;
            const int c = sample(s, ArrayAt{row}, kCodes);
            if (kEmit) seq[i] = code_letter(c);
        }
        return kOk;
    }
    for (int i = 0; i < len; i++) {
        const double* row = sid == 0 ? T.npc : T.pc + ((size_t)i * kCodes + ref_code(T, sid, i + pos, dir)) * kCodes;
        const int c = sample(s, ArrayAt{row}, kCodes);
        if (kEmit) seq[i] = code_letter(c);
    }
    return kOk;
}

// what an attempt leaves
struct Attempt {
    int32_t ok;       // the attempt gave a read
    int32_t status;   // kOk, or why the run cannot go on
    int32_t sid, dir, pos, insert_l, len1, len2;
    uint32_t draws;   // the uniforms it took, whether it gave a read or not
};

template <bool kEmit, class Src>
RSEM_SIM_FN void attempt(const Tables& T, Src& s, Attempt& a, uint8_t* seq1, uint8_t* qual1, uint8_t* seq2, uint8_t* qual2) {
    a.ok = 0; a.status = kOk; a.dir = 0; a.pos = 0; a.insert_l = 0; a.len1 = 0; a.len2 = 0;
    const bool paired = T.paired();
    a.sid = sample(s, ArrayAt{T.theta_cdf}, T.M + 1);
    if (a.sid == 0) {
        a.len1 = T.has_mld ? draw_length(s, T.m_lb, T.m_ub, T.m_cdf, -1) : draw_length(s, T.g_lb, T.g_ub, T.g_cdf, -1);
        a.status = draw_mate<kEmit>(T, s, 0, a.len1, 0, 0, seq1, qual1);
        if (paired) {
            a.len2 = draw_length(s, T.m_lb, T.m_ub, T.m_cdf, -1);
            if (a.status == kOk) a.status = draw_mate<kEmit>(T, s, 0, a.len2, 0, 0, seq2, qual2);
        }
        a.ok = a.status == kOk;
    } else {
        const int tot = T.tot_len[a.sid], full = T.full_len[a.sid];
        a.dir = s.next() < T.prob_f ? 0 : 1;
        const int frag = draw_length(s, T.g_lb, T.g_ub, T.g_cdf, tot);
        if (frag >= 0) {
            const int t = tot - frag + 1, eff = full < t ? full : t;
            int pos;
            if (T.est_rspd) pos = eval_cdf(T, eff, full) > 0.0 ? sample(s, RspdAt{&T, full}, eff) : -1;
            else pos = (int)(s.next() * eff);
            if (pos >= 0) {
                if (a.dir > 0) pos = tot - pos - frag;
                a.pos = pos;
                if (paired) {
                    a.insert_l = frag;
                    // (PairedEndQModel.h:415-417 goes on with a length of -1: undefined there, a status here)
                    a.len1 = draw_length(s, T.m_lb, T.m_ub, T.m_cdf, frag);
                    if (a.len1 < 0) a.status = kShortInsert;
                    else a.status = draw_mate<kEmit>(T, s, a.sid, a.len1, pos, a.dir, seq1, qual1);
                    if (a.status == kOk) {
                        a.len2 = draw_length(s, T.m_lb, T.m_ub, T.m_cdf, frag);
                        a.status = draw_mate<kEmit>(T, s, a.sid, a.len2, tot - pos - frag, !a.dir, seq2, qual2);
                    }
                    a.ok = a.status == kOk;
                } else {
                    a.len1 = T.has_mld ? draw_length(s, T.m_lb, T.m_ub, T.m_cdf, frag) : frag;
                    if (a.len1 >= 0) {
                        a.status = draw_mate<kEmit>(T, s, a.sid, a.len1, pos, a.dir, seq1, qual1);
                        a.ok = a.status == kOk;
                    }
                }
            }
        }
    }
    if (s.past) { a.status = kPastWords; a.ok = 0; }
    a.draws = s.k;
}

// the uniforms the longest attempt of a model can take: a header of 6, and per base a quality and a letter, each of one or two
RSEM_SIM_FN uint32_t longest_attempt(const Tables& T) { return 8u + 4u * 2u * (uint32_t)T.max_len; }

// ---- what the search of a stream may skip ------------------------------------------------------------------------------------------

// Is there a table with a total of 0 that an attempt can reach?  Then sample() takes a second uniform there (simul.h:29-32) and the
// length of an attempt depends on every draw of it.  Qualities: the values the chain can reach from qc_init; a reachable row without
// mass reaches every value.
template <class Model>
inline bool tables_plain(const Model& m) {
    if (!(m.theta_cdf[m.M] > 0.0)) return false;
    const bool q = m.type == 1 || m.type == 3;
    if (!q) {
        if (!(m.npc[kCodes - 1] > 0.0)) return false;
        for (size_t r = 0; r < (size_t)m.pro_len * kCodes; r++)
            if (!(m.pc[r * kCodes + kCodes - 1] > 0.0)) return false;
        return true;
    }
    if (!(m.qc_init[kQ - 1] > 0.0)) return false;
    std::vector<char> seen(kQ, 0);
    std::vector<int> todo;
    for (int v = 0; v < kQ; v++)
        if (m.qc_init[v] > (v ? m.qc_init[v - 1] : 0.0)) { seen[v] = 1; todo.push_back(v); }
    while (!todo.empty()) {
        const int v = todo.back();
        todo.pop_back();
        const double* row = m.qc_trans + (size_t)v * kQ;
        if (!(row[kQ - 1] > 0.0)) return false;
        for (int w = 0; w < kQ; w++)
            if (!seen[w] && row[w] > (w ? row[w - 1] : 0.0)) { seen[w] = 1; todo.push_back(w); }
    }
    for (int v = 0; v < kQ; v++) {
        if (!seen[v]) continue;
        if (!(m.npc[v * kCodes + kCodes - 1] > 0.0)) return false;
        for (int r = 0; r < kCodes; r++)
            if (!(m.pc[(v * kCodes + r) * kCodes + kCodes - 1] > 0.0)) return false;
    }
    return true;
}

// ---- the attempts a stream holds -----------------------------------------------------------------------------------------------------

// next_ok[p] of word position p: the position behind the attempt that begins at p, bit 31: that attempt gives a read
constexpr uint32_t kOkBit = 0x80000000u;

// A tile of positions [t0, t1), t[p - t0] = next_ok[p] on entry: on return t[p - t0] is the first position at or behind t1 that the
// chain p -> next[p] -> ... reaches.  The chain only goes forward, so one sweep from the tile's last position to its first does it in
// place: a position whose attempt ends outside the tile is its own answer, every other one copies the entry of a later position, which
// the sweep has already turned into an exit.  (LDS on the device, an array on the host.)
RSEM_SIM_FN void tile_exits_in_place(uint32_t* t, uint32_t t0, uint32_t t1) {
    for (uint32_t p = t1; p-- > t0;) {
        const uint32_t nx = t[p - t0] & ~kOkBit;
        t[p - t0] = nx >= t1 ? nx : t[nx - t0];
    }
}

}  // namespace rsem_simk
