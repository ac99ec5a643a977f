// pairscan_block.hpp -- the reordering of rsem-scan-for-paired-end-reads: the loop of scanForPairedEndReads.cpp:78-126
// with add_to_appropriate_arr (:24-32), get_pattern_code (:34-37) and less_than (:39-51).  pairscan.hip runs it on the device,
// tests/pairscan_check.cpp runs the same source on the host -- the bodies that work across a wave or a workgroup on tests/simt_emu.hpp.
//
// The reference walks the file record by record on one thread, collects a read's records in four vectors, sorts one and pops the others
// from the back.  Here a lane takes a record.  Where a group starts is a prefix count (mark_record, opens_group); a record's rank in its
// class and its group's four totals are differences of prefix sums; the place of a partial or unknown record is arithmetic on those
// (partial_slot); the proper records of a group get their stable rank by meeting every other one of the group in LDS (rank_group).
// No floating point takes part, and every word but the verdict has one writer.
#pragma once
#include <cstdint>

#include "alncheck_block.hpp"

namespace rsem_pairk {

using rsem_alnk::canonical_len;
using rsem_alnk::kMaxName;
using rsem_alnk::kNoVerdict;
using rsem_alnk::same_bytes;
using rsem_alnk::wave_min_to;

constexpr uint64_t kDefaultBatchItems = 1ull << 22;  // records a batch
constexpr int kWave = 64, kGroupThreads = 256;

// the codes of rsem_pairscan_verdict (include/rsem_hip.h), in the order the reference checks (:85, :89, :90; NO_PARTNER is where it
// calls back() on an empty vector, :105,109)
enum Code : uint32_t { kOk = 0, kMixed = 1, kOddFull = 2, kOddPartial = 3, kNoPartner = 4 };

// what mark_record says of a record: it opens a run of equal canonical names (hard), or its canonical name is the record before's
// and its raw name is longer than that (soft: the only records at which a single-end group and a paired one part ways); bit 0 of the
// word: hard or soft, with bit 0x1 in its flag.  kHard is the bit that starts the scan's count again.
constexpr uint32_t kHard = 0x80000000u, kSoft = 0x40000000u;

// a batch's records: the arrays start at the batch's first record; the offsets are the call's own, `name_base` the offset of the
// batch's first byte
struct Recs {
    const uint64_t* name_off;
    const uint8_t* names;
    uint64_t name_base;
    const uint32_t* flag;
    const int32_t* tid;
    const int32_t* pos;
    const int32_t* mpos;
    int64_t n;
    RSEM_ALN_FN const uint8_t* name(int64_t r) const { return names + (name_off[r] - name_base); }
    RSEM_ALN_FN uint32_t name_len(int64_t r) const { return (uint32_t)(name_off[r + 1] - name_off[r]); }
};

// add_to_appropriate_arr (:24-32): 0 both (mapped and proper), 1 partial_1, 2 partial_2, 3 unknown
RSEM_ALN_FN uint32_t class_of(uint32_t flag) {
    if (!(flag & 4u) && (flag & 2u)) return 0;
    if (flag & 0x40u) return 1;
    if (flag & 0x80u) return 2;
    return 3;
}

// the two words the class sums run over: both | partial_1 << 32 and partial_2 | unknown << 32
RSEM_ALN_FN uint64_t class_word_a(uint32_t c) { return c == 0 ? 1ull : (c == 1 ? 1ull << 32 : 0ull); }
RSEM_ALN_FN uint64_t class_word_b(uint32_t c) { return c == 2 ? 1ull : (c == 3 ? 1ull << 32 : 0ull); }

// record i of the batch (a batch starts where a canonical name starts).  The word for the scan below: kHard | kSoft | paired count
RSEM_ALN_FN uint32_t mark_record(const Recs& R, int64_t i) {
    const uint32_t paired = R.flag[i] & 1u;
    if (i == 0) return kHard | paired;
    const uint8_t *a = R.name(i), *b = R.name(i - 1);
    const uint32_t la = R.name_len(i), ca = canonical_len(a, la);
    if (!same_bytes(a, ca, b, canonical_len(b, R.name_len(i - 1)))) return kHard | paired;
    return la > ca && a[ca] ? (kSoft | paired) : 0u;  // (a NUL ends the raw name too: the reference compares C strings, :119)
}

// the scan's operator: a count that starts again at every hard record (kSoft is dropped).  After the inclusive scan, word i &
// 0x3fffffff is the number of hard or soft records with bit 0x1 from the start of i's run up to i itself.
struct RunCount {
    RSEM_ALN_FN uint32_t operator()(uint32_t a, uint32_t b) const {
        if (b & kHard) return b & ~kSoft;
        return (a & kHard) | (((a & 0x3fffffffu) + (b & 0x3fffffffu)) & 0x3fffffffu);
    }
};

// does record i open a group (:84, :119)?  A hard record does.  A soft one does iff no hard or soft record before it in its run
// has bit 0x1: until then every group of the run is single-end and ends at the next raw name that differs from the canonical one; the
// first paired group runs to the run's end.
RSEM_ALN_FN uint32_t opens_group(uint32_t mark, uint32_t scanned) {
    if (mark & kHard) return 1u;
    if (!(mark & kSoft)) return 0u;
    return ((scanned & 0x3fffffffu) - (mark & 1u)) == 0u ? 1u : 0u;
}

// the place, behind the group's `both` records, of a record of class c (1, 2, 3) that is the r-th of its class in its group, the
// group having n1, n2, nu records of the three classes (:98-115 written as arithmetic).  b counts from the back, as pop_back does.
// While both partial vectors last, pair t is (partial_1[b = t], partial_2[b = t]) at 2t and 2t + 1; the L = |n1 - n2| left over of
// the longer one follow at 2b, each with unknown[b = t'] behind it at 2 min(n1, n2) + 2t' + 1; the other unknown records close.
RSEM_ALN_FN uint64_t partial_slot(uint32_t c, uint64_t r, uint64_t n1, uint64_t n2, uint64_t nu) {
    const uint64_t m = n1 < n2 ? n1 : n2, L = (n1 < n2 ? n2 : n1) - m;
    if (c == 1) return 2 * (n1 - 1 - r);
    if (c == 2) { const uint64_t b = n2 - 1 - r; return b < m ? 2 * b + 1 : 2 * b; }
    const uint64_t b = nu - 1 - r;
    return b < L ? 2 * m + 2 * b + 1 : 2 * m + L + b;
}

// the first check of :89-90 and of the loop of :98-111 that a group of these totals fails
RSEM_ALN_FN uint32_t totals_code(uint64_t nb, uint64_t n1, uint64_t n2, uint64_t nu) {
    if (nb & 1ull) return kOddFull;
    if ((n1 + n2 + nu) & 1ull) return kOddPartial;
    if ((n1 < n2 ? n2 - n1 : n1 - n2) > nu) return kNoPartner;
    return kOk;
}

// less_than's key (:39-51), every field as the reference compares it: signed 32 bits, then the pattern code
struct Key {
    int32_t tid, p1, p2;
    uint32_t pat;
};

RSEM_ALN_FN Key load_key(const Recs& R, uint32_t r) {
    const int32_t a = R.pos[r], b = R.mpos[r];
    const uint32_t f = R.flag[r], rev = (f >> 4) & 1u;
    return Key{R.tid[r], a < b ? a : b, a < b ? b : a, (f & 0x40u) ? rev : 1u - rev};
}

RSEM_ALN_FN int compare_keys(const Key& a, const Key& b) {
    if (a.tid != b.tid) return a.tid < b.tid ? -1 : 1;
    if (a.p1 != b.p1) return a.p1 < b.p1 ? -1 : 1;
    if (a.p2 != b.p2) return a.p2 < b.p2 ? -1 : 1;
    if (a.pat != b.pat) return a.pat < b.pat ? -1 : 1;
    return 0;
}

// what the scans leave per record of the batch (n + 1 words each: the last is the total)
struct Scans {
    const uint32_t* ord;   // inclusive: groups opened up to and with the record
    const uint64_t* ca;    // exclusive: both | partial_1 << 32 before the record
    const uint64_t* cb;    // exclusive: partial_2 | unknown << 32
};

// record i of the batch (every lane of the wave calls this; `live` lanes have a record): a single-end group's record stays where it
// is; a paired group's record of the three partial classes goes to its place, a `both` record behind the group's start in file order
// (both_src: what rank_group sorts).  The lane of a group's first record says what is wrong with the group and whether it needs
// the sort (sort_word: 1 for 2 to 64 `both` records, 1 << 32 for more).  A group that fails is left in file order.
RSEM_DEVFN void place_body(bool live, int64_t i, const Recs& R, const Scans& S, const uint32_t* goff, uint64_t group_base, uint32_t rec_base, uint32_t* perm,
                           uint32_t* both_src, uint64_t* sort_word, unsigned long long* verdict) {
    unsigned long long cand = kNoVerdict;
    if (live) {
        const uint32_t g = S.ord[i] - 1u, gs = goff[g], ge = goff[g + 1];
        uint64_t sw = 0;
        if (!(R.flag[gs] & 1u)) perm[i] = rec_base + (uint32_t)i;
        else {
            const uint64_t a0 = S.ca[gs], b0 = S.cb[gs], a1 = S.ca[ge], b1 = S.cb[ge];
            const uint64_t nb = (a1 - a0) & 0xffffffffull, n1 = (a1 >> 32) - (a0 >> 32), n2 = (b1 - b0) & 0xffffffffull, nu = (b1 >> 32) - (b0 >> 32);
            const uint32_t f = R.flag[i], code = totals_code(nb, n1, n2, nu);
            if (!(f & 1u)) cand = (group_base + g) << 8 | (uint64_t)kMixed;
            else if ((uint32_t)i == gs && code) cand = (group_base + g) << 8 | (uint64_t)code;
            if (code) perm[i] = rec_base + (uint32_t)i;
            else {
                const uint32_t c = class_of(f);
                if (c == 0) {
                    const uint64_t r = (S.ca[i] - a0) & 0xffffffffull;
                    both_src[gs + r] = (uint32_t)i;
                } else {
                    const uint64_t r = c == 1 ? (S.ca[i] >> 32) - (a0 >> 32) : (c == 2 ? (S.cb[i] - b0) & 0xffffffffull : (S.cb[i] >> 32) - (b0 >> 32));
                    perm[gs + nb + partial_slot(c, r, n1, n2, nu)] = rec_base + (uint32_t)i;
                }
                if ((uint32_t)i == gs && nb >= 2) sw = nb <= (uint64_t)kWave ? 1ull : 1ull << 32;
            }
        }
        sort_word[i] = sw;
    }
    wave_min_to(cand, verdict);
}

// The `both` records of one group, both_src[g0 .. g0 + n), into perm[g0 .. g0 + n) by less_than, records that tie in file order:
// rank = |{j : key_j < key_i}| + |{j < i : key_j == key_i}| (std::stable_sort's order; the reference's std::sort is an insertion sort,
// which is stable, up to 16 records).  By a wave (WIDTH 64, n <= 64, `lane` its lane) or a workgroup (WIDTH 256, any n): lane i's key
// meets every j of the group, a tile of WIDTH at a time, every lane reading the same staged key at the same time (a broadcast).
template <int WIDTH>
RSEM_DEVFN void rank_group(uint32_t g0, uint32_t n, int lane, const Recs& R, const uint32_t* both_src, Key* stage, uint32_t rec_base, uint32_t* perm) {
    for (uint32_t i0 = 0; i0 < n; i0 += WIDTH) {
        const uint32_t i = i0 + (uint32_t)lane;
        const bool live = i < n;
        const uint32_t src = both_src[g0 + (live ? i : 0u)];
        const Key mine = load_key(R, src);
        uint32_t below = 0, same_before = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += WIDTH) {
            const uint32_t m = n - j0 < (uint32_t)WIDTH ? n - j0 : (uint32_t)WIDTH;
            if (WIDTH == kWave) RSEM_WAVE_SYNC(); else RSEM_SYNC();  // every lane is done with the tile before
            if ((uint32_t)lane < m) stage[lane] = load_key(R, both_src[g0 + j0 + (uint32_t)lane]);
            if (WIDTH == kWave) RSEM_WAVE_SYNC(); else RSEM_SYNC();
            if (live)
                for (uint32_t t = 0; t < m; t++) {
                    const int c = compare_keys(stage[t], mine);
                    below += c < 0 ? 1u : 0u;
                    same_before += (c == 0 && j0 + t < i) ? 1u : 0u;
                }
        }
        if (live) perm[g0 + below + same_before] = rec_base + src;
    }
}

// does record b of the call open a run of equal canonical names?
RSEM_ALN_FN bool run_starts(const Recs& R, uint64_t b) {
    const uint8_t *x = R.name((int64_t)b), *y = R.name((int64_t)b - 1);
    return !same_bytes(x, canonical_len(x, R.name_len((int64_t)b)), y, canonical_len(y, R.name_len((int64_t)b - 1)));
}

// Batches end only where the canonical name changes: whole runs in their order while their records stay within `budget`; a run
// above the budget is a batch of its own.  R: the call's records on the host.
RSEM_ALN_FN uint64_t batch_end(const Recs& R, uint64_t lo, uint64_t budget) {
    const uint64_t n = (uint64_t)R.n;
    if (n - lo <= budget) return n;
    for (uint64_t b = lo + budget; b > lo; b--)
        if (run_starts(R, b)) return b;
    uint64_t b = lo + budget + 1;
    while (b < n && !run_starts(R, b)) b++;
    return b;
}

}  // namespace rsem_pairk
