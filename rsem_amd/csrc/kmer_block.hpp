// kmer_block.hpp -- the arithmetic of the shared-k-mer count (rsem-for-ebseq-calculate-clustering-info), as
// RSEM_KMER_FN functions: kmer.hip runs them on the device, and tests/kmer_check.cpp runs the same source on the host.
//
// The sequences are one byte per base, codes 0 .. 4 (A C G T N: N is an ordinary fifth letter), laid one after the other with the
// separator code 5 behind every transcript: transcript t occupies [soff[t], soff[t+1] - 1) and its separator sits at soff[t+1] - 1.
// A window of k bytes that holds a separator is not a k-mer.  A k-mer is cut into chunks of 27 bases, the last one shorter; the
// key of a chunk is its bases as a number in base 5, first base most significant (5^27 < 2^63).  Everything here is integer.
#pragma once
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define RSEM_KMER_FN __host__ __device__ inline  // kmer.hip: its host side sizes the sorts and cuts the batches with the same functions
#else
#define RSEM_KMER_FN inline  // a host program that includes this header alone
#endif

namespace rsem_kmer {

constexpr int kChunkBases = 27;
constexpr int kSep = 5;
constexpr int kBucketBases = 8;  // batches are cut by the value of the first min(k, 8) bases: at most 5^8 = 390625 buckets

RSEM_KMER_FN uint64_t pow5(int n) {
    uint64_t r = 1;
    for (int i = 0; i < n; i++) r *= 5;
    return r;
}
RSEM_KMER_FN int n_chunks(int k) { return (k + kChunkBases - 1) / kChunkBases; }
RSEM_KMER_FN int chunk_len(int k, int c) {
    const int r = k - c * kChunkBases;
    return r < kChunkBases ? r : kChunkBases;
}
// bits of the largest key of a chunk of len bases (the radix sort looks at no more)
RSEM_KMER_FN int key_bits(int len) {
    uint64_t m = pow5(len) - 1;
    int b = 0;
    while (m) { b++; m >>= 1; }
    return b ? b : 1;
}
RSEM_KMER_FN int bucket_bases(int k) { return k < kBucketBases ? k : kBucketBases; }

// the len bases from c[0] on as a number in base 5
RSEM_KMER_FN uint64_t encode(const uint8_t* c, int len) {
    uint64_t key = 0;
    for (int j = 0; j < len; j++) key = key * 5 + c[j];
    return key;
}
// the key of the window one base further: `out` leaves at the top (top = 5^(len-1)), `in` enters at the bottom.  Unsigned
// arithmetic: a window that holds a separator (a digit 5) rolls on to the right key of the next clean window as well.
RSEM_KMER_FN uint64_t roll(uint64_t key, uint64_t top, uint32_t out, uint32_t in) { return (key - (uint64_t)out * top) * 5 + in; }

// index of the first separator in s[from, to), or `to`.  s is 4-byte aligned; whole words are looked at where the index is.
// Among the codes 0 .. 5 only the separator has bits 0 and 2 set.
RSEM_KMER_FN int first_sep(const uint8_t* s, int from, int to) {
    int i = from;
    while (i < to && (i & 3)) {
        if (s[i] == kSep) return i;
        i++;
    }
    while (i + 4 <= to) {
        uint32_t w;
        memcpy(&w, __builtin_assume_aligned(s + i, 4), 4);
        if ((w >> 2) & w & 0x01010101u) break;
        i += 4;
    }
    while (i < to) {
        if (s[i] == kSep) return i;
        i++;
    }
    return to;
}

// A lane of k_tile: the kLaneStarts consecutive starts p0, p0 + 1, .. of the staged codes s (readable up to p0 + kLaneStarts + k - 1).
// For every start j the lane learns whether the window of k codes is a k-mer (the next separator is looked for again only once a
// start has passed it), the key of the k-mer's last chunk [last_off, last_off + last_len) and the bucket of its first pb bases,
// both rolled along from start to start: f(j, valid, key, bucket).
constexpr int kLaneStarts = 8;
template <class F>
RSEM_KMER_FN void lane_starts(const uint8_t* s, int p0, int k, int last_off, int last_len, int pb, F&& f) {
    const int scan_end = p0 + kLaneStarts + k - 1;
    const uint64_t top_key = pow5(last_len - 1), top_b = pow5(pb - 1);
    uint64_t key = encode(s + p0 + last_off, last_len);
    uint32_t bucket = (uint32_t)encode(s + p0, pb);
    int ns = first_sep(s, p0, scan_end);
    for (int j = 0; j < kLaneStarts; j++) {
        const int l = p0 + j;
        if (ns < l) ns = first_sep(s, l, scan_end);
        f(j, ns >= l + k, key, bucket);
        if (j + 1 < kLaneStarts) {
            key = roll(key, top_key, s[l + last_off], s[l + last_off + last_len]);
            bucket = (uint32_t)roll(bucket, top_b, s[l], s[l + pb]);
        }
    }
}

// the bases [from, k) of the k-mers at a and b are the same
RSEM_KMER_FN bool tail_equal(const uint8_t* s, uint64_t a, uint64_t b, int from, int k) {
    if (a == b) return true;
    for (int j = from; j < k; j++)
        if (s[a + j] != s[b + j]) return false;
    return true;
}
// An element of the sorted list opens a group where its k-mer differs from its predecessor's: the key of the first chunk tells for
// k <= 27, the codes behind the first chunk decide otherwise.
RSEM_KMER_FN bool is_head(const uint8_t* s, int k, uint64_t key, uint64_t key_prev, uint64_t pos, uint64_t pos_prev) {
    if (key != key_prev) return true;
    return k > kChunkBases && !tail_equal(s, pos, pos_prev, kChunkBases, k);
}

// the transcript whose bases hold position p: the largest t < M with soff[t] <= p (soff is strictly increasing, M + 1 entries)
RSEM_KMER_FN int32_t find_transcript(const uint64_t* soff, int32_t M, uint64_t p) {
    int32_t lo = 0, hi = M;  // soff[lo] <= p < soff[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (soff[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Runs of equal transcript inside a wave: bit l of `boundary` is set where lane l starts a run (lane 0 always does).  The number
// of lanes of the run that starts at `lane`, of `width` lanes in all.
RSEM_KMER_FN int run_length(uint64_t boundary, int lane, int width) {
    const uint64_t above = lane + 1 < 64 ? boundary >> (lane + 1) : 0;
    const int next = above ? lane + 1 + __builtin_ctzll(above) : width;
    return (next < width ? next : width) - lane;
}

// Batches: whole buckets in ascending order, as many as stay within `budget` items; a bucket above the budget is a batch of its
// own.  Returns the end (exclusive) of the batch that starts at bucket lo and its number of items.
template <class Hist>
RSEM_KMER_FN uint32_t batch_end(const Hist& hist, uint32_t nbuckets, uint32_t lo, uint64_t budget, uint64_t& items) {
    items = 0;
    uint32_t b = lo;
    while (b < nbuckets) {
        const uint64_t h = hist[b];
        if (items > 0 && items + h > budget) break;
        items += h;
        b++;
    }
    return b;
}

}  // namespace rsem_kmer
