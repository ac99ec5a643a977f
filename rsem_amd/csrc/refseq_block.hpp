// refseq_block.hpp -- the byte work of rsem-prepare-reference's three programs: FASTA bodies -> contiguous
// bases (the getline / check / += loops of extractRef.cpp:336-349, synthesisRef.cpp:175-188 and Refs.h:96-102) and segments of
// bases -> sequences (Transcript::extractSeq, Transcript.h:90-117; RefSeqPolicy::convert, AlignerRefSeqPolicy::convert and the
// poly-A append of RefSeq.h:23-28).  refseq.hip runs the two bodies on the device, tests/refseq_check.cpp runs the same source on
// tests/simt_emu.hpp.
//
// Load: the raw bytes of a batch lie in tiles of kTile bytes, a wave a tile, a lane 16 bytes a step.  A byte is KEPT when it lies
// inside the body of a record that is kept and is not '\n'.  Pass 1 counts the kept bytes of every tile and, in checked mode, takes
// per record the minimum offset of a byte that is not a letter (whether the record is kept or not); an exclusive sum over the tile
// counts lies between the passes; pass 2 recomputes the masks, finds every kept byte's place with a popcount prefix over the lanes'
// masks, moves a lane's kept bytes together in registers, puts the wave's step together in LDS at the alignment of its destination
// (a lane stores aligned pieces of 1 to 16 bytes, never a byte at a time) and writes it with 16-byte stores, bytes at the
// two ragged ends.  No workgroup waits for another.
//
// Gather: a wave takes a fixed span of the segments' cumulative length, finds its first segment by bisection and walks.  Every
// output byte has one writer: whole aligned 16-byte words inside a wave's part of a segment, single bytes at its ragged ends.
#pragma once
#include <cstdint>

#include "simt_macros.hpp"

#ifdef __HIPCC__
#define RSEM_REFSEQ_FN __host__ __device__ inline
#else
#define RSEM_REFSEQ_FN inline
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

namespace rsem_refseqk {

constexpr int kWave = 64;
constexpr int kThreads = 256;                     // four waves, each on its own
constexpr uint32_t kChunk = 1024;                 // C: 64 lanes x 16 bytes, a step of a wave
constexpr uint32_t kSteps = 4;
constexpr uint32_t kTile = kChunk * kSteps;       // T: the raw bytes of a wave in the load kernels
constexpr uint32_t kSpan = 4096;                  // cumulative segment bytes of a wave in the gather kernel
constexpr uint32_t kGroupSpan = kSpan * 4;        // W: of a workgroup
constexpr uint32_t kStage = kChunk + 16;          // LDS bytes a wave: a step's kept bytes at the alignment of their destination
constexpr uint32_t kPad = 32;                     // bytes kept free in front of and behind the bases: the 16-byte loads of the gather may reach there
constexpr uint64_t kNone = ~0ull;                 // no bad byte
constexpr uint64_t kMaxBases = 0x7fffffffull;     // a record: the reference's coordinates are int

enum : uint32_t { kModeRaw = 0, kModeChecked = 1 };
enum : uint32_t { kFlagRC = 1, kFlagUpperN = 2, kFlagN2G = 4, kFlagFill = 8, kFlagAll = 15 };

struct alignas(16) V16 { uint64_t lo, hi; };

// what check() of extractRef.cpp:297-303 makes of a letter
RSEM_REFSEQ_FN uint8_t check_map(uint8_t c) {
    const uint8_t l = c | 0x20u;
    if (l == 'a' || l == 'c' || l == 'g' || l == 't') return c;
    return (c & 0x20u) ? 'n' : 'N';
}
RSEM_REFSEQ_FN bool is_letter(uint8_t c) { const uint8_t l = c | 0x20u; return l >= 'a' && l <= 'z'; }
// getOpp (utils.h:78-94) on what check() lets through; anything else stays (the reference would stop there)
RSEM_REFSEQ_FN uint8_t opp(uint8_t c) {
    const uint8_t l = c | 0x20u, cs = c & 0x20u;
    const uint8_t u = l == 'a' ? 'T' : l == 't' ? 'A' : l == 'c' ? 'G' : l == 'g' ? 'C' : 0;
    return u && (c & 0xc0u) == 0x40u ? (uint8_t)(u | cs) : c;
}
// RefSeqPolicy::convert: toupper, then anything but A, C, G, T becomes N
RSEM_REFSEQ_FN uint8_t upper_n(uint8_t c) {
    const uint8_t l = c | 0x20u;
    return (c & 0xc0u) == 0x40u && (l == 'a' || l == 'c' || l == 'g' || l == 't') ? (uint8_t)(c & ~0x20u) : (uint8_t)'N';
}
RSEM_REFSEQ_FN uint8_t apply_flags(uint8_t c, uint32_t flags) {
    if (flags & kFlagRC) c = opp(c);
    if (flags & kFlagUpperN) c = upper_n(c);
    if ((flags & kFlagN2G) && c == 'N') c = 'G';
    return c;
}
RSEM_REFSEQ_FN uint8_t byte_of(const V16& v, uint32_t k) { return (uint8_t)((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xffu); }
RSEM_REFSEQ_FN V16 map16(V16 v, uint32_t flags, bool reverse) {
    V16 r{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint64_t b = apply_flags(byte_of(v, reverse ? 15u - k : k), flags);
        if (k < 8) r.lo |= b << (8 * k); else r.hi |= b << (8 * (k - 8));
    }
    return r;
}
// 16 bytes from byte offset off of p (p is 16-byte aligned; off may be anything, 16 bytes around the range must be readable)
RSEM_REFSEQ_FN V16 load16(const uint8_t* p, int64_t off) {
    const int64_t a = off & ~(int64_t)15;
    const uint32_t sh = (uint32_t)(off & 15) * 8u;
    const V16 x = *(const V16*)(p + a);
    if (sh == 0) return x;
    const V16 y = *(const V16*)(p + a + 16);
    V16 r;
    if (sh < 64) { r.lo = x.lo >> sh | x.hi << (64 - sh); r.hi = x.hi >> sh | y.lo << (64 - sh); }
    else if (sh == 64) { r.lo = x.hi; r.hi = y.lo; }
    else { r.lo = x.hi >> (sh - 64) | y.lo << (128 - sh); r.hi = y.lo >> (sh - 64) | y.hi << (128 - sh); }
    return r;
}

// the 128-bit value as a row of 16 bytes, byte 0 lowest: shifted towards byte 0 / away from it by n bytes, its first n bytes (n in 0..16)
RSEM_REFSEQ_FN V16 shr_bytes(V16 v, uint32_t n) {
    if (n == 0) return v;
    if (n >= 16) return V16{0, 0};
    const uint32_t b = 8u * (n & 7u);
    if (n >= 8) return V16{b ? v.hi >> b : v.hi, 0};
    return V16{v.lo >> b | v.hi << (64 - b), v.hi >> b};
}
RSEM_REFSEQ_FN V16 shl_bytes(V16 v, uint32_t n) {
    if (n == 0) return v;
    if (n >= 16) return V16{0, 0};
    const uint32_t b = 8u * (n & 7u);
    if (n >= 8) return V16{0, b ? v.lo << b : v.lo};
    return V16{v.lo << b, v.hi << b | v.lo >> (64 - b)};
}
RSEM_REFSEQ_FN V16 low_bytes(V16 v, uint32_t n) {
    if (n >= 16) return v;
    if (n >= 8) return V16{v.lo, n == 8 ? 0ull : v.hi & ((1ull << (8u * (n - 8u))) - 1ull)};
    return V16{n ? v.lo & ((1ull << (8u * n)) - 1ull) : 0ull, 0};
}
RSEM_REFSEQ_FN V16 check16(V16 v) {  // check_map on every byte, in registers
    V16 r{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint64_t b = check_map(byte_of(v, k));
        if (k < 8) r.lo |= b << (8 * k); else r.hi |= b << (8 * (k - 8));
    }
    return r;
}
// The kept bytes of v (bit k of keep: byte k) moved together, in their order, into the low bytes of the result.  A step per RUN of kept
// bytes -- a chunk holds a line end or two, or a body's edge, so one to three runs -- not per byte.
RSEM_REFSEQ_FN V16 compact16(V16 v, uint32_t keep) {
    V16 acc{0, 0};
    uint32_t cnt = 0;
    while (keep) {
        const uint32_t s = (uint32_t)__builtin_ctz(keep), run = (uint32_t)__builtin_ctz(~(keep >> s));
        const V16 piece = shl_bytes(low_bytes(shr_bytes(v, s), run), cnt);
        acc.lo |= piece.lo;
        acc.hi |= piece.hi;
        cnt += run;
        keep &= ~(((1u << run) - 1u) << s);
    }
    return acc;
}
// cnt bytes (the low ones of v) to stage[p, p + cnt) in naturally aligned pieces of 16, 8, 4, 2 or 1 bytes -- five at most for 16 bytes at an
// odd place -- so that no store touches a byte of a neighbouring lane's range
RSEM_REFSEQ_FN void store_pieces(uint8_t* stage, uint32_t p, V16 v, uint32_t cnt) {
    while (cnt) {
        const uint32_t al = (p | 16u) & (0u - (p | 16u)), fit = 1u << (31 - __builtin_clz(cnt)), n = al < fit ? al : fit;
        if (n == 16) *(V16*)(stage + p) = v;
        else if (n == 8) { const uint64_t x = v.lo; __builtin_memcpy(__builtin_assume_aligned(stage + p, 8), &x, 8); }
        else if (n == 4) { const uint32_t x = (uint32_t)v.lo; __builtin_memcpy(__builtin_assume_aligned(stage + p, 4), &x, 4); }
        else if (n == 2) { const uint16_t x = (uint16_t)v.lo; __builtin_memcpy(__builtin_assume_aligned(stage + p, 2), &x, 2); }
        else stage[p] = (uint8_t)v.lo;
        v = shr_bytes(v, n);
        p += n;
        cnt -= n;
    }
}

// ---- load --------------------------------------------------------------------------------------------------------------------

// a batch on the device: raw[0, raw_len) is the file from byte `origin` (a multiple of 16) on; records [0, n) with their bodies
// [lo[r], hi[r]) as offsets into raw, ascending and apart
struct Batch {
    const uint8_t* raw;
    uint64_t raw_len;
    uint32_t n;
    const uint64_t* lo;
    const uint64_t* hi;
    const uint8_t* keep;  // per record
    uint32_t mode;
};

// the first record of [a, b) whose body ends behind x (b where there is none)
RSEM_REFSEQ_FN uint32_t record_at(const uint64_t* hi, uint32_t a, uint32_t b, uint64_t x) {
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (hi[m] > x) b = m; else a = m + 1;
    }
    return a;
}

// bit k set: byte k of v is c
RSEM_REFSEQ_FN uint32_t eq_mask(const V16& v, uint8_t c) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) m |= (uint32_t)(byte_of(v, k) == c) << k;
    return m;
}
RSEM_REFSEQ_FN uint32_t letter_mask(const V16& v) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) m |= (uint32_t)is_letter(byte_of(v, k)) << k;
    return m;
}
RSEM_REFSEQ_FN uint32_t bits_between(uint64_t a, uint64_t b, uint64_t x) {  // the bits of [a, b) in a chunk that starts at x (a, b clipped to it)
    const uint32_t s = a > x ? (uint32_t)(a - x) : 0u, e = b < x + 16 ? (uint32_t)(b - x) : 16u;
    return s < e ? ((1u << e) - 1u) & ~((1u << s) - 1u) : 0u;
}

// what a lane makes of its 16 bytes at x: the kept bytes' mask; in checked mode the records' first bad bytes go to bad[]; with
// `place` (pass 2) the bases' start and end of a record whose body begins / ends in the chunk: pos0 is the place of the chunk's first
// kept byte.  The second call (place) follows a wave prefix, so the mask comes first and the places second.
// The records a tile can meet: [a, b) holds, for every byte of the tile, the first record that ends behind it -- a lane bisects there
// and not over all records.  Record a's body is kept at hand: a step that lies strictly inside it (the common case: a chromosome is
// many tiles long) needs no search at all, and no record starts or ends in it.
struct TileRecords {
    uint32_t a, b;
    uint64_t a_lo, a_hi;
    uint32_t a_keep;
};
RSEM_REFSEQ_FN TileRecords tile_records(const Batch& B, uint64_t t0) {
    TileRecords R;
    R.a = record_at(B.hi, 0u, B.n, t0);
    const uint32_t e = record_at(B.hi, R.a, B.n, t0 + kTile - 1);
    R.b = e < B.n ? e + 1u : B.n;
    const bool any = R.a < B.n;
    R.a_lo = any ? B.lo[R.a] : ~0ull;
    R.a_hi = any ? B.hi[R.a] : 0ull;
    R.a_keep = any ? B.keep[R.a] : 0u;
    return R;
}
RSEM_REFSEQ_FN bool step_inside(const TileRecords& R, uint64_t xs) { return R.a_lo < xs && R.a_hi > xs + kChunk; }

// xs: where the wave's step starts, x: the lane's 16 bytes
RSEM_REFSEQ_FN uint32_t chunk_mask(const Batch& B, const TileRecords& R, uint64_t xs, uint64_t x, const V16& v, uint64_t* bad) {
    if (x >= B.raw_len) return 0u;
    const uint32_t nl = eq_mask(v, '\n');
    const uint32_t letters = B.mode == kModeChecked && bad ? letter_mask(v) : 0xffffu;
    if (step_inside(R, xs)) {
        const uint32_t body = 0xffffu & ~nl, b = body & ~letters;
        if (b) RSEM_ATOMIC_MIN_U64(bad + R.a, x + (uint64_t)__builtin_ctz(b));
        return R.a_keep ? body : 0u;
    }
    uint32_t keep = 0;
    for (uint32_t r = record_at(B.hi, R.a, R.b, x); r < B.n && B.lo[r] < x + 16; r++) {
        const uint32_t body = bits_between(B.lo[r], B.hi[r], x) & ~nl;
        if (B.keep[r]) keep |= body;
        const uint32_t b = body & ~letters;
        if (b) RSEM_ATOMIC_MIN_U64(bad + r, x + (uint64_t)__builtin_ctz(b));
    }
    return keep;
}
RSEM_REFSEQ_FN void chunk_places(const Batch& B, const TileRecords& R, uint64_t xs, uint64_t x, uint32_t keep, uint64_t pos0, uint64_t* base, uint64_t* end) {
    if (x >= B.raw_len || step_inside(R, xs)) return;
    for (uint32_t r = record_at(B.hi, R.a, R.b, x); r < B.n && B.lo[r] < x + 16; r++) {
        if (!B.keep[r]) continue;
        if (B.lo[r] >= x) base[r] = pos0 + (uint64_t)__builtin_popcount(keep & ((1u << (uint32_t)(B.lo[r] - x)) - 1u));
        if (B.hi[r] <= x + 16) end[r] = pos0 + (uint64_t)__builtin_popcount(keep & ((1u << (uint32_t)(B.hi[r] - x)) - 1u));
    }
}

template <class T>
RSEM_DEVFN T wave_inclusive(T v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = RSEM_SHFL_UP(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// pass 1, a wave on tile t: count[t] = its kept bytes
RSEM_DEVFN void load_count(const Batch& B, uint64_t t, int lane, uint64_t* count, uint64_t* bad) {
    uint32_t c = 0;
    const TileRecords R = tile_records(B, t * kTile);
    for (uint32_t s = 0; s < kSteps; s++) {
        const uint64_t xs = t * kTile + s * kChunk, x = xs + (uint64_t)lane * 16u;
        V16 v{0, 0};
        if (x < B.raw_len) v = *(const V16*)(B.raw + x);
        c += (uint32_t)__builtin_popcount(chunk_mask(B, R, xs, x, v, bad));
    }
    const uint32_t tot = wave_inclusive(c, lane);
    if (lane == kWave - 1) count[t] = tot;
}

// pass 2, a wave on tile t: its kept bytes to out[start[t] ...], checked mode through check_map; stage: kStage bytes of LDS, 16-byte aligned
RSEM_DEVFN void load_write(const Batch& B, uint64_t t, int lane, const uint64_t* start, uint8_t* out, uint8_t* stage, uint64_t* base, uint64_t* end) {
    uint64_t g = start[t];  // where the step's first kept byte goes
    const TileRecords R = tile_records(B, t * kTile);
    for (uint32_t s = 0; s < kSteps; s++) {
        const uint64_t xs = t * kTile + s * kChunk, x = xs + (uint64_t)lane * 16u;
        V16 v{0, 0};
        if (x < B.raw_len) v = *(const V16*)(B.raw + x);
        const uint32_t keep = chunk_mask(B, R, xs, x, v, nullptr);
        const uint32_t mine = (uint32_t)__builtin_popcount(keep);
        const uint32_t incl = wave_inclusive(mine, lane);
        const uint32_t total = RSEM_SHFL(incl, kWave - 1);
        const uint32_t mis = (uint32_t)(g & 15u);
        chunk_places(B, R, xs, x, keep, g + (incl - mine), base, end);
        // the lane's kept bytes, moved together in registers, go to their place in the stage in aligned pieces: no loop over bytes
        store_pieces(stage, mis + incl - mine, compact16(B.mode == kModeChecked ? check16(v) : v, keep), mine);
        RSEM_WAVE_SYNC();
        // [mis, mis + total) of the stage -> out[g, g + total): bytes up to the first aligned word, words, bytes behind the last
        const uint32_t e = mis + total;
        const uint32_t w0 = mis ? 16u : 0u, w1 = e & ~15u;
        const uint64_t o0 = g - mis;  // the aligned address stage[0] stands for
        if (w0 < w1) {
            for (uint32_t w = w0 + (uint32_t)lane * 16u; w < w1; w += kWave * 16u) *(V16*)(out + o0 + w) = *(const V16*)(stage + w);
            if (mis && (uint32_t)lane < 16u - mis) out[g + lane] = stage[mis + lane];
            if ((uint32_t)lane >= 16u && (uint32_t)lane - 16u < e - w1) out[o0 + w1 + (lane - 16)] = stage[w1 + (lane - 16)];
        } else {
            for (uint32_t k = (uint32_t)lane; k < total; k += kWave) out[g + k] = stage[mis + k];  // (at most 31 bytes)
        }
        RSEM_WAVE_SYNC();
        g += total;
    }
}

// ---- gather ------------------------------------------------------------------------------------------------------------------

struct Segments {
    uint64_t n;
    const uint64_t* cum;    // n + 1: the lengths before segment i
    const uint64_t* src;    // where the segment's first base lies in the bases (unused with kFlagFill)
    const uint64_t* dst;    // where it goes in the store
    const uint32_t* flags;
};

// the segment that holds cumulative byte c (c < cum[n]): the last i with cum[i] <= c
RSEM_REFSEQ_FN uint64_t segment_of(const uint64_t* cum, uint64_t n, uint64_t c) {
    uint64_t a = 0, b = n - 1;
    while (a < b) {
        const uint64_t m = a + ((b - a + 1) >> 1);
        if (cum[m] <= c) a = m; else b = m - 1;
    }
    return a;
}

// 16 output bytes of a segment from its position p on (what lies behind the segment's end is not meant to be stored)
RSEM_REFSEQ_FN V16 fetch16(const uint8_t* bases, uint64_t src, uint64_t len, uint64_t p, uint32_t flags) {
    if (flags & kFlagFill) return V16{0x4141414141414141ull, 0x4141414141414141ull};
    if (flags & kFlagRC) return map16(load16(bases, (int64_t)(src + len - p) - 16), flags, true);
    return map16(load16(bases, (int64_t)(src + p)), flags, false);
}
RSEM_REFSEQ_FN uint8_t fetch1(const uint8_t* bases, uint64_t src, uint64_t len, uint64_t p, uint32_t flags) {
    if (flags & kFlagFill) return 'A';
    return apply_flags(bases[(flags & kFlagRC) ? src + len - 1 - p : src + p], flags);
}

// a wave on the cumulative bytes [c0, c1)
RSEM_DEVFN void gather_span(const Segments& S, uint64_t c0, uint64_t c1, int lane, const uint8_t* bases, uint8_t* store) {
    const uint64_t total = S.cum[S.n];
    if (c1 > total) c1 = total;
    if (c0 >= c1) return;
    for (uint64_t i = segment_of(S.cum, S.n, c0); i < S.n && S.cum[i] < c1; i++) {
        const uint64_t len = S.cum[i + 1] - S.cum[i];
        if (!len) continue;
        const uint64_t p0 = c0 > S.cum[i] ? c0 - S.cum[i] : 0, p1 = c1 - S.cum[i] < len ? c1 - S.cum[i] : len;
        const uint64_t d = S.dst[i], src = S.src[i];
        const uint32_t flags = S.flags[i];
        const uint64_t d0 = d + p0, d1 = d + p1;
        uint64_t a0 = (d0 + 15u) & ~15ull, a1 = d1 & ~15ull;
        if (a0 > d1) a0 = d1;
        if (a1 < a0) a1 = a0;
        const uint32_t head = (uint32_t)(a0 - d0), tail = (uint32_t)(d1 - a1);
        const uint64_t words = (a1 - a0) >> 4, units = head + words + tail;
        for (uint64_t u = (uint64_t)lane; u < units; u += kWave) {
            if (u < head) store[d0 + u] = fetch1(bases, src, len, p0 + u, flags);
            else if (u < head + words) {
                const uint64_t a = a0 + ((u - head) << 4);
                *(V16*)(store + a) = fetch16(bases, src, len, a - d, flags);
            } else {
                const uint64_t a = a1 + (u - head - words);
                store[a] = fetch1(bases, src, len, a - d, flags);
            }
        }
    }
}

// Batches: records in their order while the raw bytes from the first body's start to the last body's end stay within `budget`; a
// record above the budget is a batch of its own.
RSEM_REFSEQ_FN uint64_t batch_end(const uint64_t* lo, const uint64_t* hi, uint64_t n, uint64_t first, uint64_t budget) {
    uint64_t r = first;
    while (r < n && (r == first || hi[r] - lo[first] <= budget)) r++;
    return r;
}

}  // namespace rsem_refseqk
