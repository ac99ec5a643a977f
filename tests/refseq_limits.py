"""TEST INFRASTRUCTURE: the inputs of tests/test_refseq_limits_gpu.py -- rsem_refseq_load / rsem_refseq_gather where the value domain and
the records degenerate: every byte value, bodies of no byte, bodies that touch, eight records in a 16-byte chunk, more segments than a
wave's span has bytes, segments at the two ends of the bases and of the store.  Plain data: (raw, body_lo, body_hi[, keep]) and segment
lists (record, first base, length, destination, flags) for tests/refseq_ref.py.  tests/refseq_check.cpp restates the same shapes in C++
(`limits`) for the lane emulator."""
import random

import refseq_ref as rr

CHUNK, STEP, TILE, SPAN, GROUP_SPAN = 16, 1024, 4096, 4096, 16384  # a lane's bytes, kChunk, kTile, kSpan, kGroupSpan of refseq_block.hpp
LETTERS = bytes(range(65, 91)) + bytes(range(97, 123))
VALUES = bytes(v for v in range(256) if v != 10)  # every byte a body can hold


def letters(rng, n, width=0):
    """n bytes of A-Z and a-z, with a line end after every `width` of them where width > 0"""
    out = bytearray()
    col = 0
    while len(out) < n:
        if width and col == width:
            out.append(10)
            col = 0
        else:
            out.append(rng.choice(LETTERS))
            col += 1
    return bytes(out)


# ---- load ------------------------------------------------------------------------------------------------------------------------------

def every_byte_raw():
    """one record: the 255 values but the line end, three times over -- 255 = 15 mod 16, so a value meets three lane positions"""
    body = VALUES * 3
    raw = b">raw\n" + body + b"\n"
    return raw, [5], [5 + len(body)]


def every_byte_checked():
    """255 records AC?GT, seven bytes apart: the value under test meets every position of a chunk"""
    raw, lo, hi = bytearray(), [], []
    for v in VALUES:
        raw += b">\n"
        lo.append(len(raw))
        raw += b"AC" + bytes([v]) + b"GT"
        hi.append(len(raw))
    return bytes(raw), lo, hi


def empty_and_adjacent():
    """(raw, lo, hi, what): bodies of no byte at a chunk, step and tile start, mid-chunk, at offset 0 and at the end of the raw bytes,
    two at one offset, next to bodies on either side; bodies without a byte between them whose shared edge is a chunk, step and tile
    start; a body of line ends alone that spans a step; a byte that is no letter in a record of even and in one of odd index"""
    rng = random.Random(17)
    size = 2 * TILE + 819
    raw = bytearray(letters(rng, size, 61))
    raw[3060:3090] = b"\n" * 30
    recs = [(0, 0, "empty at offset 0, touches the next"), (0, 16, "ends on a chunk start"), (16, 16, "empty at a chunk start between two bodies"),
            (16, 40, "touches an empty one on both sides"), (40, 40, "empty mid-chunk, touches the one before"), (48, 48, "empty at a chunk start, alone"),
            (48, 48, "a second one at the same offset"), (50, STEP, "ends on a step start"), (STEP, STEP, "empty at a step start between two bodies"),
            (STEP, 1030, "starts on a step start"), (1030, 2 * STEP, "no gap: a step start"), (2 * STEP, 2100, ""), (2100, 2112, "no gap: a chunk start"),
            (2112, 2200, ""), (2200, 3060, ""), (3060, 3090, "line ends alone, over a step start"), (3090, TILE, "ends on a tile start"),
            (TILE, TILE, "empty at a tile start between two bodies"), (TILE, 4200, ""), (4200, 2 * TILE, "no gap: a tile start"), (2 * TILE, 8250, ""),
            (8253, 8253, "empty mid-chunk, alone"), (8260, 8300, ""), (8300, 9000, ""), (9000, size, "ends with the raw bytes"), (size, size, "empty at the end")]
    lo, hi, what = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    assert size % 16
    raw[2105], raw[2150] = ord("*"), ord("-")  # in a record of even index and in one of odd index: kept and not kept where keep alternates
    assert [[r for r in range(len(lo)) if lo[r] <= p < hi[r]] for p in (2105, 2150)] == [[12], [13]]
    return bytes(raw), lo, hi, what


def lone_empty(offset):
    """a call whose only record is empty: with offset a multiple of 16 nothing is uploaded (raw_len == 0, no tile)"""
    raw = letters(random.Random(offset), 64)
    return raw, [offset], [offset]


def dense(variant):
    """256 bodies of one byte, a byte apart, in one tile: eight to a lane.  variant 0: line ends between them; 1: every fourth separator
    is no letter (outside every body: none is reported); 2: every seventh body is a byte that is no letter"""
    rng = random.Random(5 + variant)
    raw = bytearray(b">dense....\n" + b"\n" * 53)  # 64 bytes: the first body starts a chunk
    lo, hi = [], []
    for k in range(256):
        lo.append(len(raw))
        raw.append(b"*-[`{@~"[k // 7 % 7] if variant == 2 and k % 7 == 3 else rng.choice(LETTERS))
        hi.append(len(raw))
        raw.append(b"*\x00\x80\xff"[k // 4 % 4] if variant == 1 and k % 4 == 0 else 10)
    assert lo[0] % 16 == 0 and hi[-1] < TILE
    return bytes(raw), lo, hi


def smallest_budget(lo, hi):
    """the smallest body that has a byte (RSEM_REFSEQ_BATCH_BYTES is a whole number from 1 on)"""
    return min(b - a for a, b in zip(lo, hi) if b > a)


def batches_of(lo, hi, budget):
    n, first = 0, 0
    while first < len(lo):
        r = first
        while r < len(lo) and (r == first or hi[r] - lo[first] <= budget):
            r += 1
        first = r
        n += 1
    return n


def expected_load(raw, lo, hi, keep, mode):
    """per record (bases or b"" where it is not kept, bad): an unkept record is still checked in mode 1"""
    want = rr.load_ref(raw, lo, hi, mode == 1)
    return [(s if keep is None or keep[r] else b"", bad) for r, (s, bad) in enumerate(want)]


# ---- gather ----------------------------------------------------------------------------------------------------------------------------

def chromosomes():
    """(raw, lo, hi, bases): two records of letters of every kind, the first of GROUP_SPAN + 20 bases, in lines of 70"""
    rng = random.Random(29)
    seqs = [letters(rng, GROUP_SPAN + 20), letters(rng, 333)]
    raw, lo, hi = bytearray(), [], []
    for k, s in enumerate(seqs):
        raw += b">c%d\n" % k
        lo.append(len(raw))
        raw += b"\n".join(s[i:i + 70] for i in range(0, len(s), 70))
        hi.append(len(raw))
        raw += b"\n"
    return bytes(raw), lo, hi, seqs


def many_segments(n=5000):
    """n segments of one base, flags cycling 0..7, destinations three apart: every cumulative byte starts a segment"""
    return [(0, (7 * i) % 16000, 1, 2 + 3 * i, i % 8) for i in range(n)], 3 * n + 8


def whole_span_segments(length):
    """three segments of exactly `length` bytes (a wave's span, a workgroup's), destinations of three misalignments"""
    segs, d = [], 5
    for k, flags in enumerate((0, rr.RC, rr.RC | rr.UPPER_N | rr.N2G)):
        segs.append((0, k, length, d, flags))
        d += length + 9
    return segs, d + 16


def end_segments(n_bases_last):
    """forward and reverse segments from base 0 of the first record and up to the last base of the last one, at every destination
    misalignment: the 16-byte loads reach in front of and behind the bases"""
    segs, d = [], 0
    for flags in (0, rr.RC, rr.RC | rr.UPPER_N):
        for dm in range(16):
            for n in (1, 15, 16, 17, 40):
                d = ((d + 15) & ~15) + dm
                segs.append((0, 0, n, d, flags))
                d += n
                d = ((d + 15) & ~15) + dm
                segs.append((1, n_bases_last - n, n, d, flags))
                d += n
    return segs, d + 20


def store_edge_segments(size):
    """a segment whose first byte is the store's byte 0 and one whose last byte is its last"""
    out = []
    for n in (1, 17, 40):
        for flags in (0, rr.RC):
            out.append([(1, 3, n, 0, flags), (1, 50, n, size - n, flags)])
    return out
