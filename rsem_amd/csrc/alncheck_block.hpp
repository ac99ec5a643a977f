// alncheck_block.hpp -- the checks of rsem-sam-validator and rsem-get-unique: the loop of samValidator.cpp:82-183
// with check_read (:26-59), and output() of getUnique.cpp:25-30 with the grouping of :55-65.  alncheck.hip runs it on the device,
// tests/alncheck_check.cpp runs the same source on the host -- the bodies that reduce across a wave on tests/simt_emu.hpp.
//
// The reference walks the file record by record on one thread and keeps every read name it has seen in a std::set<std::string>.
// Here a lane takes a unit (a record, or the two records of a pair): its own checks, the cut of its name at the first white space,
// a 64-bit hash of that name, and whether it opens a group (its name differs from the unit before).  "Has an earlier group this
// name?" -- the set -- is a bisection by hash in the sorted runs the earlier batches left on the device, and an exact comparison of
// the name bytes for every entry with that hash.  The first record the reference would stop at is the failing unit of smallest index:
// an integer minimum over (unit << 8 | code).  No floating point takes part.
#pragma once
#include <cstdint>

#include "simt_macros.hpp"

#ifdef __HIPCC__
#define RSEM_ALN_FN __host__ __device__ inline
#else
#define RSEM_ALN_FN inline
#endif

#ifndef RSEM_ATOMIC_MIN_U64
#ifndef RSEM_EMU
#define RSEM_ATOMIC_MIN_U64(p, v) (void)atomicMin((unsigned long long*)(p), (unsigned long long)(v))
#else
#define RSEM_ATOMIC_MIN_U64(p, v)                                                                                              \
    do {                                                                                                                       \
        unsigned long long _o = __atomic_load_n((unsigned long long*)(p), __ATOMIC_RELAXED), _v = (unsigned long long)(v);      \
        while (_v < _o && !__atomic_compare_exchange_n((unsigned long long*)(p), &_o, _v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} \
    } while (0)
#endif
#endif

namespace rsem_alnk {

constexpr uint64_t kDefaultBatchItems = 1ull << 22;  // records a batch
constexpr uint32_t kMaxName = 254;                   // BAM's l_read_name is a byte and counts the NUL
constexpr unsigned long long kNoVerdict = ~0ull;

// the codes of rsem_alncheck_verdict (include/rsem_hip.h), in the order the reference checks
enum Code : uint32_t {
    kOk = 0, kMixed = 1, kOneMate = 2, kSameMateNumber = 3, kOneMateAligned = 4, kDiscordant = 5, kSameStrand = 6, kPairBoundary = 7,
    kCigarSkip = 8, kCigarIndel = 9, kCigarClip = 10, kBoundary = 11, kNotGrouped = 12, kDifferentLengths = 13
};

// a batch's records: the arrays start at the batch's first record; the offsets are the call's own, `name_base` / `cigar_base` the
// offsets of the batch's first byte / word
struct Recs {
    const uint64_t* name_off;
    const uint8_t* names;
    uint64_t name_base;
    const uint32_t* flag;
    const int32_t* tid;
    const int32_t* pos;
    const int32_t* isize;
    const int32_t* lq;
    const uint64_t* cigar_off;
    const uint32_t* cigar;
    uint64_t cigar_base;
    int64_t n;  // records of the batch
    RSEM_ALN_FN const uint8_t* name(int64_t r) const { return names + (name_off[r] - name_base); }
    RSEM_ALN_FN uint32_t name_len(int64_t r) const { return (uint32_t)(name_off[r + 1] - name_off[r]); }
};

// what the unit before the batch's first one left: its name (cut) and its two lengths
struct Carry {
    uint32_t has, clen;
    int32_t len1, len2;
    uint8_t name[256];
};

RSEM_ALN_FN bool is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

// bam_get_canonical_name (sam_utils.h:45,54-61): the bytes before the first white space
RSEM_ALN_FN uint32_t canonical_len(const uint8_t* s, uint32_t n) {
    uint32_t k = 0;
    while (k < n && s[k] && !is_space(s[k])) k++;
    return k;
}

RSEM_ALN_FN bool same_bytes(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    if (na != nb) return false;
    for (uint32_t k = 0; k < na; k++)
        if (a[k] != b[k]) return false;
    return true;
}

// FNV-1a over the bytes, then the finaliser of MurmurHash3; `bits` of it are kept (RSEM_ALNCHECK_HASH_BITS)
RSEM_ALN_FN uint64_t name_hash(const uint8_t* s, uint32_t n, int bits) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t k = 0; k < n; k++) { h ^= s[k]; h *= 0x100000001b3ull; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return bits >= 64 ? h : h & ((1ull << bits) - 1ull);
}

RSEM_ALN_FN uint32_t detail(uint32_t code, uint32_t mate, uint32_t op) { return code | mate << 8 | op << 16; }

// check_read (samValidator.cpp:26-59) of record r, the `mate`-th of its unit: the first offending operation in CIGAR order, then the
// boundary with bam_endpos of htslib 1.3 (sam.c:336-342) in 64 bits
RSEM_ALN_FN uint32_t check_read(const Recs& R, int64_t r, uint32_t mate, const uint32_t* target_len) {
    const uint32_t* c = R.cigar + (R.cigar_off[r] - R.cigar_base);
    const uint64_t nc = R.cigar_off[r + 1] - R.cigar_off[r];
    int64_t rlen = 0;
    for (uint64_t k = 0; k < nc; k++) {
        const uint32_t op = c[k] & 15u;
        if (op == 3) return detail(kCigarSkip, mate, 'N');
        if (op == 1 || op == 2) return detail(kCigarIndel, mate, op == 1 ? 'I' : 'D');
        if (op == 4 || op == 5 || op == 6) return detail(kCigarClip, mate, op == 4 ? 'S' : (op == 5 ? 'H' : 'P'));
        if (op == 0 || op == 7 || op == 8) rlen += (int64_t)(c[k] >> 4);  // M, =, X consume the reference (D and N never get here)
    }
    const int64_t pos = R.pos[r], end = (!(R.flag[r] & 4u) && nc > 0) ? pos + rlen : pos + 1;
    if (pos < 0 || end > (int64_t)target_len[R.tid[r]]) return detail(kBoundary, mate, 0);
    return kOk;
}

// a unit's own checks (samValidator.cpp:91-164); len1 / len2: readlen and readlen2 there (read 1 first in a pair)
RSEM_ALN_FN uint32_t check_unit(const Recs& R, int64_t r0, int paired, const uint32_t* target_len, int32_t& len1, int32_t& len2) {
    const uint32_t f0 = R.flag[r0];
    len1 = R.lq[r0];
    len2 = 0;
    if ((int)(f0 & 1u) != paired) return detail(kMixed, 0, 0);
    if (!paired) return (f0 & 4u) ? (uint32_t)kOk : check_read(R, r0, 0, target_len);
    if (r0 + 1 >= R.n) return detail(kOneMate, 0, 0);
    const int64_t r1 = r0 + 1;
    const uint32_t f1 = R.flag[r1];
    const uint8_t *n0 = R.name(r0), *n1 = R.name(r1);
    if (!same_bytes(n0, canonical_len(n0, R.name_len(r0)), n1, canonical_len(n1, R.name_len(r1))) || !(f1 & 1u)) return detail(kOneMate, 0, 0);
    if (!(((f0 & 0x40u) && (f1 & 0x80u)) || ((f1 & 0x40u) && (f0 & 0x80u)))) return detail(kSameMateNumber, 0, 0);
    const int value = (int)!(f0 & 4u) + (int)!(f1 & 4u);
    if (value == 1) return detail(kOneMateAligned, 0, 0);
    const uint32_t m1 = (f0 & 0x40u) ? 0u : 1u;  // which record is read 1: the one the later messages name
    const int64_t a = r0 + m1, b = r0 + (1 - m1);
    len1 = R.lq[a];
    len2 = R.lq[b];
    if (value == 2) {
        if (R.tid[a] != R.tid[b]) return detail(kDiscordant, m1, 0);
        const uint32_t strandedness = ((R.flag[a] >> 4) & 1u) << 1 | ((R.flag[b] >> 4) & 1u);
        if (strandedness != 1 && strandedness != 2) return detail(kSameStrand, m1, 0);
        const int64_t t = R.pos[a] < R.pos[b] ? a : b;
        const int64_t isz = R.isize[t], span = isz < 0 ? -isz : isz;
        if (!(R.pos[t] >= 0 && (int64_t)R.pos[t] + span <= (int64_t)target_len[R.tid[t]])) return detail(kPairBoundary, m1, 0);
        if (uint32_t d = check_read(R, a, m1, target_len)) return d;
        if (uint32_t d = check_read(R, b, 1 - m1, target_len)) return d;
    }
    return kOk;
}

// the lengths alone (of the unit before a batch-local one: no lane waits for another)
RSEM_ALN_FN void unit_lengths(const Recs& R, int64_t r0, int paired, int32_t& len1, int32_t& len2) {
    len1 = R.lq[r0];
    len2 = 0;
    if (paired && r0 + 1 < R.n) {
        const uint32_t m1 = (R.flag[r0] & 0x40u) ? 0u : 1u;
        len1 = R.lq[r0 + m1];
        len2 = R.lq[r0 + (1 - m1)];
    }
}

// ---- what needs a wave ---------------------------------------------------------------------------------------------------------

// the smallest candidate of the wave goes into *verdict: one atomic a wave, and only where a lane has one
RSEM_DEVFN void wave_min_to(unsigned long long cand, unsigned long long* verdict) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = RSEM_SHFL_XOR(cand, d);
        cand = o < cand ? o : cand;
    }
    if ((RSEM_TIDX & 63) == 0 && cand != kNoVerdict) RSEM_ATOMIC_MIN_U64(verdict, cand);
}

// what the unit kernel leaves per unit of the batch
struct UnitArrays {
    uint32_t* detail;   // code | mate << 8 | op << 16
    uint64_t* hash;     // of the cut name
    uint64_t* open;     // 1ull << 40 | clen where the unit opens a group, else 0: one scan gives ordinal and byte offset
};

// unit u of the batch (every lane of the wave calls this; `live` lanes have a unit).  unit_base: units of the push before the batch.
RSEM_DEVFN void unit_body(bool live, int64_t u, const Recs& R, int paired, const uint32_t* target_len, const Carry* before, Carry* after, int64_t n_units,
                          int hash_bits, uint64_t unit_base, const UnitArrays& A, unsigned long long* verdict) {
    unsigned long long cand = kNoVerdict;
    if (live) {
        const int mates = paired ? 2 : 1;
        const int64_t r0 = u * mates;
        int32_t l1, l2;
        uint32_t d = check_unit(R, r0, paired, target_len, l1, l2);
        const uint8_t* nm = R.name(r0);
        const uint32_t clen = canonical_len(nm, R.name_len(r0));
        const uint8_t* pn;
        uint32_t pclen;
        int32_t p1, p2;
        bool has_prev = true;
        if (u > 0) {
            pn = R.name(r0 - mates);
            pclen = canonical_len(pn, R.name_len(r0 - mates));
            unit_lengths(R, r0 - mates, paired, p1, p2);
        } else {
            has_prev = before->has != 0;
            pn = before->name; pclen = before->clen; p1 = before->len1; p2 = before->len2;
        }
        const bool opens = !has_prev || !same_bytes(nm, clen, pn, pclen);
        if (!d && !opens && (l1 != p1 || (paired && l2 != p2))) d = detail(kDifferentLengths, 0, 0);
        A.detail[u] = d;
        A.hash[u] = name_hash(nm, clen, hash_bits);
        A.open[u] = opens ? (1ull << 40 | clen) : 0ull;
        if (d) cand = (unit_base + (uint64_t)u) << 8 | (d & 0xffu);
        if (u == n_units - 1) {
            after->has = 1; after->clen = clen; after->len1 = l1; after->len2 = l2;
            for (uint32_t k = 0; k < clen; k++) after->name[k] = nm[k];
        }
    }
    wave_min_to(cand, verdict);
}

// a name of the resident store: its first byte and its length in one word
RSEM_ALN_FN uint64_t make_ref(uint64_t at, uint32_t len) { return at << 8 | len; }

// the opening units' names go behind the resident names; `scan` is the exclusive sum of A.open
RSEM_ALN_FN void gather_unit(int64_t u, const Recs& R, int mates, const uint64_t* open, const uint64_t* scan, const uint64_t* hash, uint64_t names_used,
                             uint8_t* res_names, uint64_t* g_hash, uint32_t* g_unit, uint64_t* u_ref) {
    if (!open[u]) return;
    const uint64_t g = scan[u] >> 40, at = names_used + (scan[u] & ((1ull << 40) - 1ull));
    const uint32_t clen = (uint32_t)(open[u] & 0xffu);
    const uint8_t* nm = R.name(u * mates);
    for (uint32_t k = 0; k < clen; k++) res_names[at + k] = nm[k];
    g_hash[g] = hash[u];
    g_unit[g] = (uint32_t)u;
    u_ref[u] = make_ref(at, clen);
}

// the resident groups: runs sorted by (hash, group index); run r is the entries run_off[r] .. run_off[r + 1] - 1
struct Resident {
    const uint64_t* hash;
    uint64_t* ref;
    const uint8_t* names;
    const uint64_t* run_off;
    uint32_t n_runs;  // runs before the batch's own, which starts at run_off[n_runs]
};

RSEM_ALN_FN bool same_ref(const uint8_t* names, uint64_t a, uint64_t b) {
    return same_bytes(names + (a >> 8), (uint32_t)(a & 0xffu), names + (b >> 8), (uint32_t)(b & 0xffu));
}

// the batch's own run, sorted position p (every lane of the wave calls this): has an earlier group the name of the group at p?
// Behind it in its own run lie the groups of equal hash and smaller index (the sort is stable); in every earlier run the entries of
// its hash are found by bisection.  Every candidate is settled by its bytes.
RSEM_DEVFN void lookup_body(bool live, uint64_t p, const Resident& S, const uint32_t* sorted_unit, const uint64_t* u_ref, uint32_t* unit_detail,
                            uint64_t unit_base, unsigned long long* verdict) {
    unsigned long long cand = kNoVerdict;
    if (live) {
        const uint64_t own = S.run_off[S.n_runs];
        const uint64_t h = S.hash[own + p];
        const uint32_t u = sorted_unit[p];
        const uint64_t me = u_ref[u];
        S.ref[own + p] = me;
        bool hit = false;
        for (uint64_t q = p; !hit && q > 0 && S.hash[own + q - 1] == h; q--) hit = same_ref(S.names, u_ref[sorted_unit[q - 1]], me);
        for (uint32_t r = 0; !hit && r < S.n_runs; r++) {
            uint64_t lo = S.run_off[r], hi = S.run_off[r + 1];
            const uint64_t end = hi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (S.hash[mid] < h) lo = mid + 1; else hi = mid;
            }
            for (; !hit && lo < end && S.hash[lo] == h; lo++) hit = same_ref(S.names, S.ref[lo], me);
        }
        if (hit && !unit_detail[u]) {
            unit_detail[u] = detail(kNotGrouped, 0, 0);
            cand = (unit_base + (uint64_t)u) << 8 | (uint64_t)kNotGrouped;
        }
    }
    wave_min_to(cand, verdict);
}

// ---- rsem-get-unique ---------------------------------------------------------------------------------------------------------------

// getUnique.cpp:56: a record whose RAW name differs from the record before starts a group
RSEM_ALN_FN uint32_t unique_start(const Recs& R, int64_t i) {
    if (i == 0) return 1u;
    return same_bytes(R.name(i), R.name_len(i), R.name(i - 1), R.name_len(i - 1)) ? 0u : 1u;
}

// output() of getUnique.cpp:25-30 for record i's group, found in the inclusive sum of the starts by bisection: kept iff no record of
// it is unmapped and it has 2 records where its first is flagged paired, else 1
RSEM_ALN_FN uint8_t unique_keep(const uint32_t* incl, const uint32_t* flag, int64_t n, int64_t i) {
    const uint32_t g = incl[i];
    int64_t lo = 0, hi = i;  // the first record with incl == g
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (incl[mid] < g) lo = mid + 1; else hi = mid;
    }
    const int64_t b = lo;
    lo = i; hi = n;          // the first record with incl > g
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (incl[mid] <= g) lo = mid + 1; else hi = mid;
    }
    const int64_t size = lo - b;
    if (size != ((flag[b] & 1u) ? 2 : 1)) return 0;
    for (int64_t k = b; k < lo; k++)
        if (flag[k] & 4u) return 0;
    return 1;
}

// how many records of [lo, n) a batch takes: whole units; for the unique pass the caller moves the end behind the group it cuts
RSEM_ALN_FN uint64_t batch_records(uint64_t left, uint64_t budget, int mates) {
    uint64_t take = budget < left ? budget : left;
    if (mates == 2 && (take & 1ull) && take < left) take++;
    return take;
}

}  // namespace rsem_alnk
