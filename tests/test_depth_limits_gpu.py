"""Per-base read depth at the widths of the tile id (rsem_amd/csrc/depth.hip: tile_bits(n_tiles) is the radix sort's end_bit): numbers
of tiles at 2^b and 2^b + 1, where a tile id needs one bit more, past one radix digit (2^8) and past two (2^16).  Every touched tile
holds more entries than an LDS chunk, order-sensitive ones, and the blocks of the tiles are interleaved in the input: a sort that
looked at too few bits would merge two tiles' entries, one that was not stable would fold in another order.  Doubles are compared by
their bits against tests/depth_ref.py."""
import numpy as np
import pytest

import depth_ref as dr
from depth_ref import order_sensitive_blocks

pytestmark = pytest.mark.gpu

T, CHUNK = dr.TILE, dr.CHUNK
N_PER_TILE = 300  # more than a chunk: the order inside a tile shows


def capi():
    from rsem_amd import capi as c
    return c


def limit_blocks(n_tiles):
    """n_bases and the blocks: 300 order-sensitive blocks on each of tile 0, the last tile and tile n_tiles / 2, interleaved block by
    block; a block from tile n_tiles - 2 into the last; above 2^16 tiles a block over every radix digit's seam"""
    n_bases = n_tiles * T - 3
    where = [0, n_tiles - 1, n_tiles // 2]
    parts = [order_sensitive_blocks(N_PER_TILE, seed=s + 1, span=T - 3) for s in range(3)]  # the last tile has T - 3 bases
    for st, ln, w in parts:  # the precondition of the order claim, per tile
        assert N_PER_TILE > CHUNK and np.any(dr.bits(dr.fold(T, st, ln, w)) != dr.bits(dr.fold(T, st[::-1], ln[::-1], w[::-1])))
    start = np.stack([p[0] + np.uint64(t * T) for p, t in zip(parts, where)], axis=1).reshape(-1)
    length = np.stack([p[1] for p in parts], axis=1).reshape(-1)
    w = np.stack([p[2] for p in parts], axis=1).reshape(-1)
    extra = [((n_tiles - 1) * T - 5, 10, 0.7)]
    if n_tiles >= 65536:  # over the seam of the first digit; from tile 65534 through 65535 to the end, or into tile 65536
        extra += [(256 * T - 4, 9, np.float32(0.1)), (65535 * T - 2, T + 4 if n_tiles > 65536 else T - 1, 0.7)]
    # the extra blocks go into the middle of the input: entries of their tiles come before AND after them
    half = len(start) // 2
    es, el, ew = (np.array(x) for x in zip(*extra))
    start = np.concatenate([start[:half], es.astype(np.uint64), start[half:]])
    length = np.concatenate([length[:half], el.astype(np.uint32), length[half:]])
    w = np.concatenate([w[:half], ew.astype(np.float64), w[half:]])
    assert int((start + length).max()) <= n_bases
    return n_bases, start.astype(np.uint64), length.astype(np.uint32), w.astype(np.float64)


def fold_touched(n_bases, start, length, w):
    """dr.fold, tile by touched tile (the fold of a base sees only the blocks over it, in their order): the depth, the touched tiles"""
    want = np.zeros(n_bases)
    s, e = start.astype(np.int64), start.astype(np.int64) + length.astype(np.int64)
    touched = sorted({t for a, b in zip(s, e) for t in range(a // T, (b - 1) // T + 1)})
    for t in touched:
        lo, hi = t * T, min((t + 1) * T, n_bases)
        on = (s < hi) & (e > lo)
        cs, ce = np.maximum(s[on], lo), np.minimum(e[on], hi)
        want[lo:hi] = dr.fold(hi - lo, cs - lo, ce - cs, w[on])
    return want, touched


_cache = {}


def limit_case(n_tiles):
    """computed once per size, shared, never changed"""
    if n_tiles not in _cache:
        blocks = limit_blocks(n_tiles)
        want, touched = fold_touched(*blocks)
        if n_tiles <= 257:  # the tile-wise fold is the fold
            assert np.array_equal(dr.bits(want), dr.bits(dr.fold(*blocks)))
        _cache[n_tiles] = (blocks, want, touched)
    return _cache[n_tiles]


def run_case(n_tiles):
    (n_bases, start, length, w), want, touched = limit_case(n_tiles)
    got, info = capi().depth_accumulate(n_bases, start, length, w)
    return got, info, want, touched, sum(dr.tiles_of(int(s), int(l)) for s, l in zip(start, length))


@pytest.mark.parametrize("n_tiles", [5, 8, 9, 255, 256, 257, 65536, 65537])
def test_tile_ids_at_a_power_of_two_and_one_past(monkeypatch, n_tiles):
    monkeypatch.delenv("RSEM_DEPTH_BATCH_ITEMS", raising=False)
    got, info, want, touched, entries = run_case(n_tiles)
    # the path first: one batch, the tiles the test placed blocks on, the highest id among them
    assert info["n_batches"] == 1 and info["n_tiles_touched"] == len(touched) and info["n_entries"] == entries
    assert touched[0] == 0 and touched[-1] == n_tiles - 1 and n_tiles // 2 in touched and n_tiles - 2 in touched
    if n_tiles >= 65536:
        assert {255, 256, 65535} <= set(touched)
    assert len(got) == n_tiles * T - 3
    # the untouched tiles are +0.0 in `want`: one comparison of all the bits says they stayed so
    assert np.count_nonzero(dr.bits(got) != dr.bits(want)) == 0


def test_tile_ids_past_one_digit_in_batches(monkeypatch):
    """257 tiles in batches of 7 items: every batch sorts ids of nine bits, a tile's entries come in many batches"""
    monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", "7")
    (n_bases, start, length, w), want, touched = limit_case(257)
    got, info = capi().depth_accumulate(n_bases, start, length, w)
    batches = dr.expected_batches(start, length, 7)
    assert info["n_batches"] == len(batches) > 100 and info["n_entries"] == sum(e for _, e in batches)
    per_batch, b0 = 0, 0
    for nb, _ in batches:  # a tile counts once per batch that has an entry of it
        per_batch += len({t for s, l in zip(start[b0:b0 + nb], length[b0:b0 + nb]) for t in range(int(s) // T, (int(s) + int(l) - 1) // T + 1)})
        b0 += nb
    assert info["n_tiles_touched"] == per_batch > 3 * 100
    assert np.array_equal(dr.bits(got), dr.bits(want))
