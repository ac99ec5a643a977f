// gmap_block.hpp -- the arithmetic of rsem-tbam2gbam: transcript coordinates -> genome coordinates with a
// CIGAR (sam_utils.h:137-208, tr2chr; BamConverter.h:150-191), and the collapse of a read's alignments that land on one genomic
// locus (bc_aux.h, CollapseMap: a std::map keyed by the converted alignment, float weights added in file order).  gmap.hip runs it
// on the device, tests/gmap_check.cpp runs the same source on the host -- the collapse body on tests/simt_emu.hpp.
//
// The reference walks a transcript's exons from the first one for every record; here the exons' cumulative lengths are searched by
// bisection.  Its std::map becomes a STABLE RANK SORT inside the read's group: the rank of alignment i is the number of j with
// key_j < key_i plus the number of j < i with key_j == key_i.  The first record of a run of equal keys (the one the map keeps)
// adds the weights of the run's later records to its own, in file order, in float: the additions of the reference, in its order.
#pragma once
#include <cstdint>

#include "simt_macros.hpp"

#ifdef __HIPCC__
#define RSEM_GMAP_FN __host__ __device__ inline
#else
#define RSEM_GMAP_FN inline
#endif

namespace rsem_gmapk {

constexpr int kWave = 64;                            // a group of up to 64 alignments: one wave
constexpr int kGroupThreads = 256;                   // anything longer: one workgroup, i in strides of 256, j in tiles of 256
constexpr uint64_t kDefaultBatchItems = 1ull << 22;  // alignments a batch
constexpr int32_t kMaxExons = 32766;                 // n_cigar <= 2 * exons + 2 stays within BAM's 16 bits
constexpr uint32_t kOpM = 0, kOpI = 1, kOpN = 3;     // BAM_CMATCH, BAM_CINS, BAM_CREF_SKIP

// the reference on the device: per transcript the strand, the length without poly-A tail (= the sum of its exons), the output tid and
// where its exons start in the flat arrays; per exon start and end (1-based, inclusive) and the transcript bases before it
struct Ref {
    const uint8_t* minus;     // 1: '-' strand
    const int32_t* length;
    const int32_t* out_tid;
    const uint64_t* exon_off;  // n_tr + 1
    const int32_t* start;
    const int32_t* end;
    const int32_t* cum;        // cum[e] = bases of the transcript's exons before exon e; one more entry per transcript is NOT kept: length closes it
};

// what a mate becomes
struct Mapped {
    int32_t tid, pos;  // output reference id, 0-based position
    uint32_t flag, n_cigar, bin, has_n;
    // for the fill: the (mirrored, clipped) range, the first and last exon (relative), what hangs off either end
    int32_t sp, ep, lead, tail, i0, j0, only_i;
};

// hts_reg2bin(beg, end, 14, 5) (htslib 1.3 hts.h); end < beg happens: bam_endpos of a CIGAR without a reference-consuming
// operation is pos itself (sam.c:336-342, bam_cigar2rlen = 0), and the shifts are arithmetic
RSEM_GMAP_FN uint32_t reg2bin(int64_t beg, int64_t end) {
    int l, s = 14, t = ((1 << 15) - 1) / 7;
    for (--end, l = 5; l > 0; --l, s += 3, t -= 1 << (l * 3))
        if ((beg >> s) == (end >> s)) return (uint32_t)(t + (int)(beg >> s));
    return 0u;
}

// the first exon e of [0, s) with cum[e] + len(e) >= x, for 1 <= x <= length: the exon that holds transcript base x
RSEM_GMAP_FN int32_t exon_of(const int32_t* cum, int32_t s, int32_t x) {
    int32_t lo = 0, hi = s - 1;  // the last e with cum[e] < x
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (cum[mid] < x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// convert + tr2chr for one mate, everything but the CIGAR words
RSEM_GMAP_FN Mapped map_mate(const Ref& R, int32_t tr, int32_t pos, int32_t l_qseq, uint32_t flag) {
    Mapped m;
    const uint64_t e0 = R.exon_off[tr];
    const int32_t s = (int32_t)(R.exon_off[tr + 1] - e0), L = R.length[tr];
    const int32_t *st = R.start + e0, *en = R.end + e0, *cum = R.cum + e0;
    const bool minus = R.minus[tr] != 0;
    int32_t sp = pos + 1, ep = pos + l_qseq;
    if (minus) {
        const int32_t t = sp;
        sp = L - ep + 1;
        ep = L - t + 1;
        flag ^= 0x10u;
        if (flag & 1u) flag ^= 0x20u;
    }
    m.tid = R.out_tid[tr];
    m.flag = flag;
    m.lead = m.tail = 0;
    m.i0 = m.j0 = 0;
    m.has_n = 0;
    int64_t gend;  // bam_endpos
    if (ep < 1 || sp > L) {  // wholly in the poly-A tail: one I at the transcript's end
        m.only_i = 1;
        m.pos = sp > L ? en[s - 1] : st[0] - 1;
        m.n_cigar = 1;
        gend = m.pos;
    } else {
        m.only_i = 0;
        if (sp < 1) { m.lead = 1 - sp; sp = 1; }
        const int32_t i = exon_of(cum, s, sp);
        m.pos = st[i] + (sp - cum[i] - 1) - 1;
        int32_t j;
        if (ep > L) { m.tail = ep - L; j = s - 1; gend = en[s - 1]; }
        else { j = exon_of(cum, s, ep); gend = (int64_t)st[j] - 1 + (ep - cum[j]); }
        m.i0 = i; m.j0 = j;
        m.n_cigar = (uint32_t)((m.lead ? 1 : 0) + 2 * (j - i) + 1 + (m.tail ? 1 : 0));
        m.has_n = j > i;
    }
    m.sp = sp; m.ep = ep;
    m.bin = reg2bin(m.pos, gend);
    return m;
}

// the CIGAR words of a mate, n_cigar of them, with the reference's operands
RSEM_GMAP_FN void fill_cigar(const Ref& R, int32_t tr, const Mapped& m, uint32_t* out) {
    if (m.only_i) { out[0] = (uint32_t)(m.ep - m.sp + 1) << 4 | kOpI; return; }
    const uint64_t e0 = R.exon_off[tr];
    const int32_t L = R.length[tr];
    const int32_t *st = R.start + e0, *en = R.end + e0, *cum = R.cum + e0;
    uint32_t k = 0;
    if (m.lead) out[k++] = (uint32_t)m.lead << 4 | kOpI;
    int32_t sp = m.sp;
    const int32_t ep = m.tail ? L : m.ep;
    for (int32_t e = m.i0; e <= m.j0; e++) {
        const int32_t cur_end = cum[e] + (en[e] - st[e] + 1);  // transcript base the exon ends at
        if (e < m.j0) {
            out[k++] = (uint32_t)(cur_end - sp + 1) << 4 | kOpM;
            out[k++] = (uint32_t)(st[e + 1] - en[e] - 1) << 4 | kOpN;  // two exons that touch: 0N, kept
            sp = cur_end + 1;
        } else out[k++] = (uint32_t)(ep - sp + 1) << 4 | kOpM;
    }
    if (m.tail) out[k++] = (uint32_t)m.tail << 4 | kOpI;
}

// ---- the collapse ------------------------------------------------------------------------------------------------------------

// the fixed part of an alignment's key (SingleEndT::compare of bc_aux.h, for mate 1 and mate 2): tid, pos, then the reverse bit
// above n_cigar in one word; where its CIGAR words are; its weight
struct Key {
    int32_t tid1, pos1;
    uint32_t rn1, c1;
    int32_t tid2, pos2;
    uint32_t rn2, c2;
    float w;
};

RSEM_GMAP_FN uint32_t rev_ncigar(uint32_t flag, uint32_t n_cigar) { return ((flag >> 4) & 1u) << 16 | n_cigar; }

// -1, 0, 1 as key a is below, equal to, above key b: mate 1 whole (its CIGAR words too) before mate 2, as PairedEndT::operator<
RSEM_GMAP_FN int compare_keys(const Key& a, const Key& b, const uint32_t* cigar, int mates) {
    if (a.tid1 != b.tid1) return a.tid1 < b.tid1 ? -1 : 1;
    if (a.pos1 != b.pos1) return a.pos1 < b.pos1 ? -1 : 1;
    if (a.rn1 != b.rn1) return a.rn1 < b.rn1 ? -1 : 1;
    const uint32_t n1 = a.rn1 & 0xffffu;
    for (uint32_t k = 0; k < n1; k++) {
        const uint32_t x = cigar[a.c1 + k], y = cigar[b.c1 + k];
        if (x != y) return x < y ? -1 : 1;
    }
    if (mates < 2) return 0;
    if (a.tid2 != b.tid2) return a.tid2 < b.tid2 ? -1 : 1;
    if (a.pos2 != b.pos2) return a.pos2 < b.pos2 ? -1 : 1;
    if (a.rn2 != b.rn2) return a.rn2 < b.rn2 ? -1 : 1;
    const uint32_t n2 = a.rn2 & 0xffffu;
    for (uint32_t k = 0; k < n2; k++) {
        const uint32_t x = cigar[a.c2 + k], y = cigar[b.c2 + k];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// the per-mate arrays of a batch as the count kernel left them
struct MateArrays {
    const int32_t* tid;
    const int32_t* pos;
    const uint32_t* flag;
    const uint32_t* n_cigar;
    const uint32_t* cigar_off;  // n_mates + 1, inside the batch
};

RSEM_GMAP_FN Key load_key(const MateArrays& A, const float* w, uint32_t a, int mates) {
    Key k;
    const uint32_t m1 = a * (uint32_t)mates;
    k.tid1 = A.tid[m1]; k.pos1 = A.pos[m1]; k.rn1 = rev_ncigar(A.flag[m1], A.n_cigar[m1]); k.c1 = A.cigar_off[m1];
    if (mates == 2) { k.tid2 = A.tid[m1 + 1]; k.pos2 = A.pos[m1 + 1]; k.rn2 = rev_ncigar(A.flag[m1 + 1], A.n_cigar[m1 + 1]); k.c2 = A.cigar_off[m1 + 1]; }
    else { k.tid2 = 0; k.pos2 = 0; k.rn2 = 0; k.c2 = 0; }
    k.w = w[a];
    return k;
}

// One group -- the alignments [g0, g0 + n) of the batch -- on WIDTH lanes that share `stage` (LDS, WIDTH keys): a wave (WIDTH 64,
// n <= 64, `lane` its lane) or a workgroup (WIDTH 256, any n).  Lane i's alignment meets every j of the group, a tile of WIDTH at
// a time, every lane reading the same staged key at the same time (a broadcast).  For the sorted slot p = g0 + rank it writes
//   order[p]  the alignment (index in the batch),
//   head[p]   1 where no earlier alignment has the key: the record the map keeps,
//   wsum[p]   its weight plus, in file order, the weights of the later alignments with the same key (float, one add at a time).
template <int WIDTH>
RSEM_DEVFN void collapse_group(uint32_t g0, uint32_t n, int lane, int mates, const MateArrays& A, const float* w, const uint32_t* cigar, Key* stage,
                               uint32_t* order, uint32_t* head, float* wsum) {
    for (uint32_t i0 = 0; i0 < n; i0 += WIDTH) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool live = i < n;
        Key mine = load_key(A, w, g0 + (live ? i : 0u), mates);
        uint32_t below = 0, same_before = 0;
        float acc = mine.w;
        for (uint32_t j0 = 0; j0 < n; j0 += WIDTH) {
            const uint32_t m = n - j0 < (uint32_t)WIDTH ? n - j0 : (uint32_t)WIDTH;
            if (WIDTH == kWave) RSEM_WAVE_SYNC(); else RSEM_SYNC();  // every lane is done with the tile before
            if ((uint32_t)lane < m) stage[lane] = load_key(A, w, g0 + j0 + (uint32_t)lane, mates);
            if (WIDTH == kWave) RSEM_WAVE_SYNC(); else RSEM_SYNC();
            if (live)
                for (uint32_t t = 0; t < m; t++) {
                    const uint32_t j = j0 + t;
                    if (j == i) continue;
                    const int c = compare_keys(stage[t], mine, cigar, mates);
                    if (c < 0) below++;
                    else if (c == 0) {
                        if (j < i) same_before++;
                        else acc += stage[t].w;  // j ascends: file order
                    }
                }
        }
        if (live) {
            const uint32_t p = g0 + below + same_before;
            order[p] = g0 + i;
            head[p] = same_before == 0 ? 1u : 0u;
            wsum[p] = acc;
        }
    }
}

// Batches: whole groups in their order while their alignments stay within `budget`; a group above the budget is a batch of its own.
RSEM_GMAP_FN uint64_t batch_end(const uint64_t* group_off, uint64_t n_groups, uint64_t lo, uint64_t budget) {
    uint64_t g = lo, items = 0;
    while (g < n_groups) {
        const uint64_t it = group_off[g + 1] - group_off[g];
        if (g > lo && items + it > budget) break;
        items += it;
        g++;
    }
    return g;
}

}  // namespace rsem_gmapk
