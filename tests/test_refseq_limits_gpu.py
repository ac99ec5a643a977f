"""rsem_refseq_load / rsem_refseq_gather on the GPU where the value domain and the records degenerate (inputs: tests/refseq_limits.py),
against the plain restatement (tests/refseq_ref.py).  Equality of bytes throughout; the whole store is compared, pre-filled by one
FILL segment, so a byte written outside every segment shows.

  every byte value    check_map, is_letter, opp, upper_n and the N -> G step are bit tricks on c | 0x20, c & 0xc0 and c & 0x20: they part
                      from isalpha / toupper / switch at @ [ \\ ] ^ _ ` { | } ~ DEL, below 0x20 and from 0x80 on
  degenerate records  bodies of no byte at every kind of edge, bodies that touch, eight records in one lane's 16 bytes
  segment counts      more segments than a wave's span has bytes; spans and workgroups that are one segment
  the two ends        segments from base 0 and up to the last base (the 16-byte loads reach into the pad), at byte 0 and the last
                      byte of the store"""
import numpy as np
import pytest

import refseq_limits as rl
import refseq_ref as rr

pytestmark = pytest.mark.gpu

BUDGETS = [None, "smallest", 1]


@pytest.fixture(scope="module")
def capi():
    from rsem_amd import capi as c
    if c.device_count() < 1:
        pytest.skip("needs a GPU")
    return c


def set_knobs(monkeypatch, budget, pad=None):
    for k, v in (("RSEM_REFSEQ_BATCH_BYTES", budget), ("RSEM_REFSEQ_STORE_PAD", pad)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def check_load(capi, monkeypatch, raw, lo, hi, keep, mode, budget):
    """every record loaded, batch after batch, and every one that has bases (and, in mode 1, no bad byte: what becomes of such a record's
    bases is not part of the contract) copied to a place of its own at an odd offset; n_bases, bad, the whole store and the number of
    batches against the restatement.  Returns the handle's info."""
    b = rl.smallest_budget(lo, hi) if budget == "smallest" else budget
    set_knobs(monkeypatch, b)
    want = rl.expected_load(raw, lo, hi, keep, mode)
    n = len(lo)
    place = np.concatenate([[0], np.cumsum([((len(s) + 15) & ~15) + 16 for s, _ in want])]) + 1
    size = int(place[-1]) + 16
    h = capi.Refseq(size)
    h.gather([0], [0], [size], [0], [rr.FILL])
    expect = bytearray(b"A" * size)
    first, n_bases, bad = 0, np.zeros(n, np.uint64), np.zeros(n, np.int64)
    while first < n:
        taken, nb, bd = h.load(mode, raw, lo, hi, keep, first)
        assert taken >= 1
        sl = slice(first, first + taken)
        n_bases[sl], bad[sl] = nb[sl], bd[sl]
        idx = [r for r in range(first, first + taken) if nb[r] > 0 and bd[r] < 0]
        h.gather(idx, [0] * len(idx), [int(nb[r]) for r in idx], [int(place[r]) for r in idx], [0] * len(idx))
        first += taken
    store, info = h.download(), h.info()
    h.close()
    assert n_bases.tolist() == [len(s) for s, _ in want]
    assert bad.tolist() == [x if mode == 1 else -1 for _, x in want]
    for r, (s, x) in enumerate(want):
        if mode == 0 or x < 0:
            expect[int(place[r]):int(place[r]) + len(s)] = s
    assert store == bytes(expect)
    assert info["n_batches"] == (1 if b is None else rl.batches_of(lo, hi, b))
    return info


def check_gather(capi, monkeypatch, chrom, segs, size, budget, pad=None, mode=0):
    """the store filled with 'A' from end to end, then the segments over it; the whole store and gathered_bytes against the restatement"""
    raw, lo, hi, bases = chrom
    set_knobs(monkeypatch, budget, pad)
    want = bytes(rr.gather_ref(bytearray(b"A" * size), bases, segs))
    h = capi.Refseq(size)
    h.gather([0], [0], [size], [0], [rr.FILL])
    n_bases, _ = h.run(mode, raw, lo, hi, segs)
    got, info = h.download(), h.info()
    h.close()
    assert n_bases.tolist() == [len(s) for s in bases]
    assert got == want
    assert info["gathered_bytes"] == size + sum(s[2] for s in segs) and info["store_pad"] == (pad or 0)
    return info


# ---- every byte value --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget", BUDGETS)
def test_every_byte_value_in_raw_mode(capi, budget, monkeypatch):
    raw, lo, hi = rl.every_byte_raw()
    (bases, _), = rr.load_ref(raw, lo, hi, False)
    assert len(bases) == 3 * 255 and set(bases) == set(rl.VALUES)
    first, n = 1, len(bases) - 2  # an odd source offset; every value is still there twice
    outs = [rr.segment_ref(bases, first, n, f) for f in range(8)]
    src = bases[first:first + n]
    differ = {c for i, c in enumerate(src) if outs[0][i] != outs[rr.UPPER_N][i]}
    assert any(c >= 0x80 for c in differ) and any(c in b"@[`{" for c in differ)  # the flag sets part ways at the bytes the bit tricks could mistake
    assert all(outs[rr.UPPER_N][i] == 78 for i, c in enumerate(src) if c >= 0x80 or c in b"@[\\]^_`{|}~\x7f" or c < 0x20) and outs[rr.RC] == src[::-1].translate(rr.OPP)
    assert len(set(outs)) == 8
    info = check_load(capi, monkeypatch, raw, lo, hi, None, 0, budget)
    assert info["n_bases"] == 3 * 255
    segs, d = [], 3
    for f in range(8):
        segs.append((0, first, n, d, f))
        d += n + (n & 1) + 6  # every destination is odd
    assert all(s[3] & 1 and s[1] & 1 for s in segs)
    check_gather(capi, monkeypatch, (raw, lo, hi, [bases]), segs, d + 11, rl.smallest_budget(lo, hi) if budget == "smallest" else budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_every_byte_value_in_checked_mode(capi, budget, monkeypatch):
    raw, lo, hi = rl.every_byte_checked()
    want = rr.load_ref(raw, lo, hi, True)
    assert len(lo) == 255
    for v, a, (s, bad) in zip(rl.VALUES, lo, want):
        letter = 65 <= v <= 90 or 97 <= v <= 122
        assert bad == (-1 if letter else a + 2) and len(s) == 5
        if letter:
            assert s == b"AC" + (bytes([v]) if v in b"ACGTacgt" else (b"N" if v < 97 else b"n")) + b"GT"
    assert sum(bad >= 0 for _, bad in want) == 255 - 52
    info = check_load(capi, monkeypatch, raw, lo, hi, None, 1, budget)
    assert info["n_batches"] == (1 if budget is None else 255)


# ---- degenerate records --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("keep", ["all", "alternating"])
@pytest.mark.parametrize("mode", [1, 0])
def test_empty_and_adjacent_bodies(capi, mode, keep, budget, monkeypatch):
    raw, lo, hi, what = rl.empty_and_adjacent()
    kp = None if keep == "all" else [1 - r % 2 for r in range(len(lo))]
    want = rl.expected_load(raw, lo, hi, kp, mode)
    empty = [r for r in range(len(lo)) if lo[r] == hi[r]]
    # the input reaches the limits: an empty body at a chunk, step and tile start, mid-chunk, at 0 and at the end; touching pairs
    assert {lo[r] for r in empty} >= {0, 16, 40, 48, rl.STEP, rl.TILE, len(raw)} and sum(lo[r] == 48 for r in empty) == 2 and len(raw) <= 3 * rl.TILE
    shared = {lo[r] for r in range(1, len(lo)) if lo[r] == hi[r - 1] and lo[r] < hi[r] and lo[r - 1] < hi[r - 1]}
    assert shared >= {2 * rl.STEP, 2112, 2 * rl.TILE} and 2112 % 16 == 0 and 2112 % rl.STEP
    assert all(want[r] == (b"", -1) for r in empty)
    nl = [r for r in range(len(lo)) if hi[r] > lo[r] and set(raw[lo[r]:hi[r]]) == {10}]
    assert len(nl) == 1 and lo[nl[0]] < 3 * rl.STEP < hi[nl[0]] and want[nl[0]] == (b"", -1)
    if mode == 1:
        assert [(r, x) for r, (_, x) in enumerate(want) if x >= 0] == [(12, 2105), (13, 2150)]  # record 13 is not kept where keep alternates
    check_load(capi, monkeypatch, raw, lo, hi, kp, mode, budget)


@pytest.mark.parametrize("budget", [None, 1])
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("offset", [32, 21])
def test_a_call_whose_only_record_is_empty(capi, offset, mode, budget, monkeypatch):
    """at a multiple of 16 nothing is uploaded and no tile runs; at 21 the batch is five bytes before the body"""
    raw, lo, hi = rl.lone_empty(offset)
    for keep in (None, [0]):
        info = check_load(capi, monkeypatch, raw, lo, hi, keep, mode, budget)
        assert info["raw_bytes"] == offset % 16 and info["n_bases"] == 0 and info["n_launches"] == (3 if offset % 16 else 0) + 1


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_eight_records_in_a_chunk(capi, variant, mode, budget, monkeypatch):
    raw, lo, hi = rl.dense(variant)
    assert len(lo) == 256 and all(sum(16 * c <= a < 16 * c + 16 for a in lo) == 8 for c in range(4, 36))
    want = rr.load_ref(raw, lo, hi, True)
    n_bad = sum(x >= 0 for _, x in want)
    assert n_bad == (0 if variant < 2 else len(range(3, 256, 7)))  # a separator that is no letter lies outside every body
    for keep in ([r % 2 for r in range(256)], None):
        check_load(capi, monkeypatch, raw, lo, hi, keep, mode, budget)


# ---- segment counts ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chrom():
    return rl.chromosomes()


GATHER_BUDGETS = [None, 1]


@pytest.mark.parametrize("budget", GATHER_BUDGETS)
def test_more_segments_than_a_span_has_bytes(capi, chrom, budget, monkeypatch):
    segs, size = rl.many_segments()
    cum = np.concatenate([[0], np.cumsum([s[2] for s in segs])])
    assert len(segs) == 5000 > rl.SPAN and {rl.SPAN * k for k in range(1, len(segs) // rl.SPAN + 1)} <= set(cum[:-1].tolist())  # a wave's span starts where a segment starts
    assert [s[4] for s in segs[:9]] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and all(b[3] - a[3] == 3 for a, b in zip(segs, segs[1:]))
    info = check_gather(capi, monkeypatch, chrom, segs, size, budget)
    assert info["n_batches"] == (1 if budget is None else 2)


@pytest.mark.parametrize("budget", GATHER_BUDGETS)
@pytest.mark.parametrize("length", [rl.SPAN, rl.GROUP_SPAN])
def test_spans_that_are_one_segment(capi, chrom, length, budget, monkeypatch):
    segs, size = rl.whole_span_segments(length)
    assert [s[2] for s in segs] == [length] * 3 and len({s[3] % 16 for s in segs}) == 3
    check_gather(capi, monkeypatch, chrom, segs, size, budget)


@pytest.mark.parametrize("budget", GATHER_BUDGETS)
def test_segments_at_the_two_ends_of_the_bases(capi, chrom, budget, monkeypatch):
    bases = chrom[3]
    segs, size = rl.end_segments(len(bases[1]))
    assert {s[3] % 16 for s in segs if s[0] == 0 and s[1] == 0} == set(range(16)) == {s[3] % 16 for s in segs if s[0] == 1 and s[1] + s[2] == len(bases[1])}
    assert {s[4] for s in segs} == {0, rr.RC, rr.RC | rr.UPPER_N}
    check_gather(capi, monkeypatch, chrom, segs, size, budget)


@pytest.mark.parametrize("pad", [None, 16])
def test_segments_at_the_two_ends_of_the_store(capi, chrom, pad, monkeypatch):
    size = 203
    for segs in rl.store_edge_segments(size):
        assert segs[0][3] == 0 and segs[-1][3] + segs[-1][2] == size
        check_gather(capi, monkeypatch, chrom, segs, size, None, pad)
