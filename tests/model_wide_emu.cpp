// model_wide_emu.cpp -- TEST INFRASTRUCTURE: the wide-address instantiation of the model rounds' kernel body
// (model_group_rows<..., kWide = true> of rsem_amd/csrc/model_block.hpp: window addresses of 40 bits, for strand arrays of 4 GiB and
// more) against the narrow one, on the CPU (one OS thread per lane, tests/simt_emu.hpp).  A dozen transcripts and ~200 reads; the wide
// run sees the same strands behind a pad of nearly 2^32 bytes -- address space reserved with mmap(MAP_NORESERVE), never touched -- so
// that real addresses lie on both sides of 2^32.  Without the update the kernel has no atomics: conprb and the noise conprb of the
// two runs must be the same bits.  Never part of the product.
//
//   model_wide_emu <model_type 0..3> <seed>     narrow once, then wide with 2^32 (a) between two transcripts, (b) inside a forward
//                                               strand with windows starting in the 8 bytes below it, (c) between a transcript's
//                                               two strands; each placement is first proven from the alignments.  exit 0 = identical
//   model_wide_emu decide                       window_addr_bits: which path for which strand_bytes / pad, the refusal
// Build (tests/test_model_wide_emu_cpu.py): hipcc -DRSEM_EMU -O1 -std=c++17 tests/model_wide_emu.cpp -lpthread
#include <sys/mman.h>

#include <random>

#include "simt_emu.hpp"

namespace {
using rsem::kEpsilon;
#include "../rsem_amd/csrc/model_block.hpp"
}  // namespace

struct Job {
    DevData D;
    DevTables T;
    double *cp, *ncp;
    PlaneOut PO;
    int n_blocks, block;
    double s_prob[kQProbLds], s_nprob[kQNoiseProbLds], s_one[1];  // "LDS"
    emu::Block blk;
};

template <bool kQ, bool kPE, bool kWide>
static void lane_body(Job* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    // the wrapper of k_model_group (model.hip) without the update, block size 256 here
    if (kQ) for (int i = tid; i < kQProbLds; i += 256) J->s_prob[i] = i < 2500 ? J->T.prof[i] : 1.0;
    for (int i = tid; i < (kQ ? kQNoiseProbLds : 5); i += 256) J->s_nprob[i] = i < (kQ ? 500 : 5) ? J->T.noise[i] : 1.0;
    RSEM_SYNC();
    model_group_rows<kQ, kPE, false, kWide>(J->D, J->T, nullptr, J->cp, J->ncp, AccumPtrs{nullptr, nullptr, nullptr, nullptr, 0, 0}, kQ ? J->s_prob : J->T.prof,
                                            J->s_nprob, J->s_one, J->s_one, J->s_one, J->s_one, (uint64_t)(tid >> 6) * 4, 16, tid & 63, J->PO, 48, (uint64_t)J->block,
                                            (uint64_t)J->n_blocks);
}

static void run_kernel(const DevData& D, const DevTables& T, bool q, bool pe, bool wide, double* cp, double* ncp) {
    Job* J = new Job();
    pthread_barrier_init(&J->blk.bar, nullptr, 256);
    for (int w = 0; w < 4; w++) pthread_barrier_init(&J->blk.w[w].bar, nullptr, 64);
    J->D = D; J->T = T; J->cp = cp; J->ncp = ncp;
    J->PO = PlaneOut{nullptr, nullptr, 0, 0, 0, nullptr, nullptr};
    J->n_blocks = 3;
    void (*fn)(Job*, int) = nullptr;
#define PICK(QQ, PP, WW) if (q == QQ && pe == PP && wide == WW) fn = lane_body<QQ, PP, WW>;
    PICK(false, false, false) PICK(false, false, true) PICK(true, false, false) PICK(true, false, true)
    PICK(false, true, false) PICK(false, true, true) PICK(true, true, false) PICK(true, true, true)
#undef PICK
    for (J->block = 0; J->block < J->n_blocks; J->block++) {
        std::vector<std::thread> th;
        for (int t = 0; t < 256; t++) th.emplace_back(fn, J, t);
        for (auto& t : th) t.join();
    }
    delete J;
}

// ---- the host decision, no device and no kernel involved --------------------------------------------------------------------
static int decide() {
    struct Row { uint64_t strand_bytes, pad; int want; };
    const uint64_t G4 = 1ull << 32, T1 = 1ull << 40;
    const Row rows[] = {
        {0, 0, 32}, {1000, 0, 32}, {G4 - 24, 0, 32},           // strand_bytes + 16 < 2^32: the narrow path, as before the wide one existed
        {G4 - 16, 0, 40}, {G4, 0, 40}, {4600000000ull, 0, 40},  // what used to be refused
        {1000, G4 - 1024, 32}, {1000, G4 - 1016, 40},           // the pad counts: the last narrow one, the first wide one
        {1000, G4, 40}, {2000000, G4 - 800, 40},
        {T1 - 24, 0, 40}, {T1 - 16, 0, 0}, {T1, 0, 0}, {1000, T1 - 1016, 0}, {1000, T1 - 1024, 40}, {1000, T1, 0},  // the remaining limit
        {~0ull - 7, 8, 0}, {1ull << 63, 1ull << 63, 0}, {8, ~0ull - 7, 0},  // sums that would wrap
    };
    int bad = 0;
    for (const Row& r : rows) {
        const int got = window_addr_bits(r.strand_bytes, r.pad);
        printf("strand_bytes %llu pad %llu -> %d bits%s\n", (unsigned long long)r.strand_bytes, (unsigned long long)r.pad, got, got == r.want ? "" : "   <-- MISMATCH");
        if (got != r.want) ++bad;
    }
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "decide")) return decide();
    if (argc < 3) return 2;
    const int type = atoi(argv[1]);
    const unsigned seed = (unsigned)atoi(argv[2]);
    const bool q = type == 1 || type == 3, pe = type >= 2;
    std::mt19937_64 rng(seed);
    auto irand = [&](int a, int b) { return (int)(rng() % (uint64_t)(b - a + 1)) + a; };
    auto urand = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };

    // a dozen transcripts: two families of near-copies, so that a read's consecutive alignments mostly see equal windows
    const int M = 12;
    std::vector<int32_t> fullLen(M + 1, 0), totLen(M + 1, 0);
    std::vector<std::vector<uint8_t>> tseq(M + 1);
    for (int t = 1; t <= M; t++) {
        if ((t - 1) % 6 == 0) {
            tseq[t].resize((size_t)irand(400, 900));
            for (auto& b : tseq[t]) b = (uint8_t)(rng() % 100 == 0 ? 4 : rng() & 3);
        } else {
            tseq[t] = tseq[t - 1];
            for (int k = 0; k < 6; k++) tseq[t][(size_t)irand(0, (int)tseq[t].size() - 1)] = (uint8_t)(rng() & 3);
        }
        totLen[t] = (int32_t)tseq[t].size();
        fullLen[t] = totLen[t] - (t % 5 == 0 ? 30 : 0);
    }
    std::vector<uint64_t> soff(2 * (size_t)(M + 1), 0), mask_off(M + 2, 0);
    uint64_t tot = 0;
    for (int t = 1; t <= M; t++)
        for (int d = 0; d < 2; d++) { soff[2 * t + d] = tot; tot += ((uint64_t)totLen[t] + 7) / 8 * 8; }
    std::vector<uint8_t> strands(tot + 32, 0);
    for (int t = 1; t <= M; t++)
        for (int p = 0; p < totLen[t]; p++) {
            strands[soff[2 * t] + p] = tseq[t][p];
            const uint8_t b = tseq[t][totLen[t] - p - 1];
            strands[soff[2 * t + 1] + p] = b == 4 ? 4 : 3 - b;
        }
    std::vector<uint32_t> mask_words;
    for (int t = 1; t <= M; t++) {
        mask_off[t] = mask_words.size();
        for (int w = 0; w < (totLen[t] + 31) / 32; w++) mask_words.push_back(rng() % 10 == 0 ? (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng() : 0u);
    }
    mask_off[M + 1] = mask_words.size();

    // ~200 reads; every 17th has 17..40 alignments (several 16-alignment chunks: carry_a crosses a chunk)
    const uint64_t N1 = 203;
    const int minLen = 30, maxLen = 150;
    std::vector<uint64_t> row_ptr{0};
    std::vector<int32_t> sid_signed, pos, insertL;
    std::vector<uint8_t> lq(N1, 0);
    std::vector<std::vector<uint8_t>> rseq[2], rqual[2];
    for (int m = 0; m < 2; m++) { rseq[m].resize(N1); rqual[m].resize(N1); }
    for (uint64_t i = 0; i < N1; i++) {
        const int fam = irand(0, M / 6 - 1) * 6 + 1;
        const int len1 = irand(minLen, maxLen), len2 = irand(minLen, maxLen);
        const int insert = pe ? irand(std::max(len1, len2), std::min(std::max(len1, len2) + 150, 380)) : len1;
        const int dir = (int)(rng() & 1);
        const int p0 = irand(0, 400 - insert - 3);
        const int nal = (i % 17 == 0) ? irand(17, 40) : irand(1, 12);
        lq[i] = (i % 23 == 5) ? 1 : 0;
        for (int k = 0; k < nal; k++) {
            const int t = fam + (k % 6);
            sid_signed.push_back(dir ? -t : t);
            pos.push_back(p0 + ((k / 6) % 3));
            insertL.push_back(insert);
        }
        row_ptr.push_back(sid_signed.size());
        for (int m = 0; m < (pe ? 2 : 1); m++) {
            const int len = m ? len2 : len1, d = m ? !dir : dir, wp = m ? totLen[fam] - p0 - insert : p0;
            rseq[m][i].resize(len);
            rqual[m][i].resize(len);
            for (int k = 0; k < len; k++) {
                uint8_t b = strands[soff[2 * fam + d] + (uint64_t)std::min(std::max(wp + k, 0), totLen[fam] - 1)];
                if (rng() % 20 == 0) b = (uint8_t)(rng() % 5);
                rseq[m][i][k] = b;
                rqual[m][i][k] = (uint8_t)irand(2, 93);
            }
        }
    }
    const uint64_t nnz = sid_signed.size();
    std::vector<uint64_t> roff8[2], seqw[2], qualw[2];
    std::vector<int32_t> rlen[2];
    for (int m = 0; m < (pe ? 2 : 1); m++) {
        roff8[m].assign(N1 + 1, 0);
        rlen[m].resize(N1);
        for (uint64_t i = 0; i < N1; i++) { rlen[m][i] = (int32_t)rseq[m][i].size(); roff8[m][i + 1] = roff8[m][i] + (rseq[m][i].size() + 7) / 8; }
        seqw[m].assign(roff8[m][N1] + 2, 0);
        qualw[m].assign(roff8[m][N1] + 2, 0);
        for (uint64_t i = 0; i < N1; i++) {
            const size_t l = rseq[m][i].size();
            if (!q) {
                for (size_t k = 0; k < l; k++) seqw[m][roff8[m][i] + k / 8] |= (uint64_t)rseq[m][i][k] << (8 * (k % 8));
                continue;
            }
            for (size_t k = 0; k < (l + 7) / 8 * 8; k++) {
                const uint64_t c = k < l ? read_code8(rqual[m][i][k], rseq[m][i][k]) : kPadCode8;
                ((k % 8) < 4 ? seqw : qualw)[m][roff8[m][i] + k / 8] |= c << (16 * (k % 4));
            }
        }
    }
    // the window of mate m of alignment j: (strand 2 t + d, position in it) -> unpadded byte address
    auto win = [&](uint64_t j, int m) -> uint64_t {
        const int s = sid_signed[j], t = s < 0 ? -s : s, d = s < 0 ? 1 : 0;
        return m == 0 ? soff[2 * t + d] + (uint64_t)pos[j] : soff[2 * t + !d] + (uint64_t)(totLen[t] - pos[j] - insertL[j]);
    };
    std::vector<uint8_t> same_prev(nnz, 0);
    std::vector<uint32_t> row_of(nnz, 0);
    for (uint64_t i = 0; i < N1; i++)
        for (uint64_t j = row_ptr[i]; j < row_ptr[i + 1]; j++) {
            row_of[j] = (uint32_t)i;
            if (lq[i] || j == row_ptr[i]) continue;
            for (int m = 0; m < (pe ? 2 : 1); m++)
                if (!memcmp(&strands[win(j, m)], &strands[win(j - 1, m)], (size_t)rlen[m][i])) same_prev[j] |= (uint8_t)(1 << m);
        }
    int long_rows = 0, shared = 0, contd = 0;
    for (uint64_t i = 0; i < N1; i++) {
        if (row_ptr[i + 1] - row_ptr[i] > 16 && !lq[i]) ++long_rows;
        for (uint64_t j = row_ptr[i]; j < row_ptr[i + 1]; j++) {
            if (same_prev[j] & 3) ++shared;
            if ((same_prev[j] & 3) && (j - row_ptr[i]) % 16 == 0) ++contd;
        }
    }
    printf("transcripts %d reads %llu alignments %llu, reads with > 16 alignments %d, alignments sharing a window with their predecessor %d, of them first of a chunk %d\n",
           M, (unsigned long long)N1, (unsigned long long)nnz, long_rows, shared, contd);
    if (!long_rows || !shared || !contd) { printf("test data lacks a special case\n"); return 1; }

    // tables
    const int B = 20;
    std::vector<double> rspd_pdf(B + 2, 0.0), rspd_cdf(B + 2, 0.0);
    for (int i = 1; i <= B; i++) rspd_pdf[i] = 0.2 + urand();
    { double s = 0; for (int i = 1; i <= B; i++) s += rspd_pdf[i]; for (int i = 1; i <= B; i++) { rspd_pdf[i] /= s; rspd_cdf[i] = rspd_cdf[i - 1] + rspd_pdf[i]; } }
    auto make_ld = [&](int lb, int ub, std::vector<double>& pdf, std::vector<double>& cdf) {
        pdf.assign(ub - lb + 1, 0.0); cdf.assign(ub - lb + 1, 0.0);
        double s = 0;
        for (int i = 1; i <= ub - lb; i++) { pdf[i] = 0.1 + urand(); s += pdf[i]; }
        for (int i = 1; i <= ub - lb; i++) { pdf[i] /= s; cdf[i] = cdf[i - 1] + pdf[i]; }
    };
    std::vector<double> gld_pdf, gld_cdf, mld_pdf, mld_cdf;
    const int gld_lb = pe ? 20 : minLen - 1, gld_ub = pe ? 420 : maxLen;
    make_ld(gld_lb, gld_ub, gld_pdf, gld_cdf);
    make_ld(minLen - 1, maxLen, mld_pdf, mld_cdf);
    const int prof_rows = q ? 100 : maxLen;
    std::vector<double> prof((size_t)prof_rows * 25), noise(q ? 500 : 5), mw(M + 1, 1.0);
    for (auto& v : prof) v = 0.05 + urand();
    for (auto& v : noise) v = 0.05 + 0.5 * urand();
    for (int t = 0; t <= M; t++) mw[t] = t == 3 ? 0.0 : 0.5 + 0.5 * urand();
    mw[0] = 0.9;
    DevTables T{};
    T.probF = 0.3; T.seedLen = 25; T.estRSPD = 1; T.B = B; T.rspd_pdf = rspd_pdf.data(); T.rspd_cdf = rspd_cdf.data();
    T.gld_lb = gld_lb; T.gld_ub = gld_ub; T.gld_pdf = gld_pdf.data(); T.gld_cdf = gld_cdf.data();
    T.has_mld = pe ? 1 : 0; T.mld_lb = minLen - 1; T.mld_ub = maxLen; T.mld_pdf = mld_pdf.data(); T.mld_cdf = mld_cdf.data();
    T.prof_rows = prof_rows; T.prof = prof.data(); T.noise = noise.data(); T.mw = mw.data();
    DevData D0{};
    D0.model_type = type; D0.M = M; D0.N1 = N1; D0.nnz = nnz; D0.row_ptr = row_ptr.data(); D0.hit_row = row_of.data();
    D0.sid_signed = sid_signed.data(); D0.pos = pos.data(); D0.insertL = insertL.data();
    for (int m = 0; m < (pe ? 2 : 1); m++) { D0.roff8[m] = roff8[m].data(); D0.rlen[m] = rlen[m].data(); D0.rseq_w[m] = seqw[m].data(); D0.rqual_w[m] = qualw[m].data(); }
    D0.lq = lq.data(); D0.fullLen = fullLen.data(); D0.totLen = totLen.data(); D0.mask_off = mask_off.data(); D0.mask_words = mask_words.data();

    // One run: the per-alignment fields with the product's own function (k_alignment_fields of model.hip), then the kernel body.
    // `base`: the strand array as the run sees it; soff_run: its offsets (shifted by the pad in the wide runs).
    struct Out { std::vector<double> cp, ncp; int high = 0; };
    auto run = [&](bool wide, const uint64_t* base, const std::vector<uint64_t>& soff_run) {
        DevData D = D0;
        D.soff = soff_run.data();
        D.refw = base;
        std::vector<uint32_t> aw0(nnz, 0), aw1(nnz, 0), afull(nnz, 1), atot(nnz, 1);
        std::vector<uint8_t> aw0h(nnz, 0), aw1h(nnz, 0), flags(same_prev);
        Out O;
        for (uint64_t j = 0; j < nnz; j++) {
            if (lq[row_of[j]]) continue;
            const AlnFields F = wide ? (pe ? alignment_fields<true, true>(D, T.seedLen, j) : alignment_fields<false, true>(D, T.seedLen, j))
                                     : (pe ? alignment_fields<true>(D, T.seedLen, j) : alignment_fields<false>(D, T.seedLen, j));
            aw0[j] = F.a0; aw1[j] = F.a1; afull[j] = F.full; atot[j] = F.tot; aw0h[j] = F.h0; aw1h[j] = F.h1;
            if (F.masked) flags[j] |= 4;
            if (F.h0 || F.h1) ++O.high;
        }
        D.same_prev = flags.data();
        D.aw0 = aw0.data(); D.aw1 = aw1.data(); D.afull = afull.data(); D.atot = atot.data();
        if (wide) { D.aw0h = aw0h.data(); D.aw1h = aw1h.data(); }  // (the narrow instantiation never looks at them: nullptr there)
        O.cp.assign(nnz, -1.0);
        O.ncp.assign(N1, -1.0);
        run_kernel(D, T, q, pe, wide, O.cp.data(), O.ncp.data());
        return O;
    };
    const Out narrow = run(false, (const uint64_t*)strands.data(), soff);
    {
        int nz = 0;
        for (double v : narrow.cp) { if (v < 0) { printf("an alignment was never written\n"); return 1; } if (v > 0) ++nz; }
        printf("narrow: %d of %llu alignment probabilities are positive\n", nz, (unsigned long long)nnz);
        if (nz < (int)nnz / 4) { printf("the data does not exercise the products\n"); return 1; }
    }

    // ---- the three placements of 2^32: b = the unpadded byte offset that the pad moves there -----------------------------------
    const uint64_t G4 = 1ull << 32;
    auto live = [&](uint64_t j) { return !lq[row_of[j]]; };
    auto wlen = [&](uint64_t j, int m) { return (uint64_t)rlen[m][row_of[j]]; };
    const int mates = pe ? 2 : 1;
    int bad = 0;
    for (int placement = 0; placement < 3; placement++) {
        uint64_t b = 0, n_case = 0;
        char why[200] = "";
        if (placement == 0) {  // (a) between two transcripts: the end of 6's reverse strand | the start of 7's forward strand
            b = soff[2 * 7];
            uint64_t below = 0, above = 0;
            for (uint64_t j = 0; j < nnz; j++)
                for (int m = 0; m < mates && live(j); m++) {
                    const uint64_t a = win(j, m);
                    if (a >= soff[2 * 6 + 1] && a + wlen(j, m) <= b) ++below;       // in the strand right below
                    if (a >= b && a < soff[2 * 7 + 1]) ++above;                      // in the strand right above
                }
            n_case = std::min(below, above);
            snprintf(why, sizeof why, "windows in the strand below %llu, in the strand above %llu", (unsigned long long)below, (unsigned long long)above);
        } else if (placement == 1) {  // (b) inside a forward strand, a window starting in the 8 bytes below: funnel8 takes a word from each side
            for (uint64_t j = 0; j < nnz && !b; j++)
                for (int m = 0; m < mates && live(j); m++) {
                    const int fwd = (sid_signed[j] < 0) == (m == 1);  // mate 1 of a forward alignment, mate 2 of a reverse one
                    const uint64_t a = win(j, m);
                    if (fwd && (a & 7) && wlen(j, m) > 8) { b = (a | 7) + 1; break; }
                }
            for (uint64_t j = 0; j < nnz && b; j++)
                for (int m = 0; m < mates && live(j); m++) {
                    const int s = sid_signed[j], t = s < 0 ? -s : s;
                    const uint64_t a = win(j, m);
                    const bool fwd = a >= soff[2 * t] && a < soff[2 * t + 1];
                    if (fwd && a < b && a + 8 > b && (a & 7) && a + wlen(j, m) > b) ++n_case;
                }
            snprintf(why, sizeof why, "forward-strand windows starting unaligned in the 8 bytes below it");
        } else {  // (c) between a transcript's two strands
            if (pe) {
                for (uint64_t j = 0; j < nnz && !b; j++)
                    if (live(j) && sid_signed[j] > 0) b = soff[2 * sid_signed[j] + 1];
                for (uint64_t j = 0; j < nnz && b; j++)
                    if (live(j) && sid_signed[j] > 0 && soff[2 * sid_signed[j] + 1] == b && win(j, 0) + wlen(j, 0) <= b && win(j, 1) >= b) ++n_case;
                snprintf(why, sizeof why, "pairs with mate 1 below and mate 2 above");
            } else {
                uint64_t below = 0, above = 0;
                const int t = 2;
                b = soff[2 * t + 1];
                for (uint64_t j = 0; j < nnz; j++)
                    if (live(j) && std::abs(sid_signed[j]) == t) { if (sid_signed[j] > 0) ++below; else ++above; }
                n_case = std::min(below, above);
                snprintf(why, sizeof why, "windows in the forward strand below %llu, in the reverse strand above %llu", (unsigned long long)below, (unsigned long long)above);
            }
        }
        printf("placement (%c): 2^32 at strand offset %llu of %llu; %s: %llu\n", "abc"[placement], (unsigned long long)b, (unsigned long long)tot, why,
               (unsigned long long)n_case);
        if (!b || b % 8 || b >= tot || !n_case) { printf("   the data does not have this placement   <-- MISMATCH\n"); ++bad; continue; }  // before anything runs
        const uint64_t pad = G4 - b;
        if (window_addr_bits(tot, pad) != kWideAddrBits) { printf("   not on the wide path   <-- MISMATCH\n"); ++bad; continue; }
        // the padded strand array: address space for the pad, reserved and never touched; the strands behind it
        const size_t map_bytes = (size_t)(pad + tot + 32);
        void* map = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (map == MAP_FAILED) { perror("mmap"); return 3; }
        memcpy((uint8_t*)map + pad, strands.data(), (size_t)(tot + 32));
        std::vector<uint64_t> soff_w(soff);
        for (int t = 1; t <= M; t++) { soff_w[2 * t] += pad; soff_w[2 * t + 1] += pad; }
        const Out wide = run(true, (const uint64_t*)map, soff_w);
        munmap(map, map_bytes);
        const bool same = !memcmp(wide.cp.data(), narrow.cp.data(), nnz * 8) && !memcmp(wide.ncp.data(), narrow.ncp.data(), N1 * 8);
        printf("   alignments with an address above 2^32: %d; conprb and noise conprb against the narrow run: %s\n", wide.high,
               same ? "bit-identical" : "DIFFERENT   <-- MISMATCH");
        if (!same) {
            ++bad;
            for (uint64_t j = 0; j < nnz; j++)
                if (memcmp(&wide.cp[j], &narrow.cp[j], 8)) { printf("   first at alignment %llu (read %u): %.17g vs %.17g\n", (unsigned long long)j, row_of[j], wide.cp[j], narrow.cp[j]); break; }
        }
        if (!wide.high || wide.high == (int)nnz) { printf("   the addresses do not lie on both sides of 2^32   <-- MISMATCH\n"); ++bad; }
    }
    return bad ? 1 : 0;
}
