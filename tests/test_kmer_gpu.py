"""Shared k-mers on the GPU (rsem_amd/csrc/kmer.hip through capi.kmer_shared_counts and rsem-for-ebseq-calculate-clustering-info)
against the files the unmodified reference program wrote (tests/golden/clustering/) and the Python restatement (tests/kmer_ref.py).
The arithmetic is integer: every comparison is equality.

k = 1, 2, 25, 26, 27 take one chunk of 27 bases, 28 and 54 two, 55 and 60 three; most entries of the random inputs are shorter than
54 bases; at k = 1 every group is huge.  The inputs span some 20 tiles of 2048 positions.
"""
import os
import subprocess

import numpy as np
import pytest

import kmer_ref as kr
from kmer_ref import PROG, recorded, recorded_id

pytestmark = pytest.mark.gpu

KS = [1, 2, 25, 26, 27, 28, 54, 55, 60]
INVALID = -1  # RSEM_ERR_INVALID


def capi():
    from rsem_amd import capi as c
    return c


def random_seqs(letters, seed=11, entries=300):
    """<= 300 entries of <= 400 bases: six in ten shorter than 50; the long ones carry shared segments, most a poly(A) tail of 40,
    some a run of 70 times the last letter; two identical entries; an entry repeated inside itself"""
    rng = np.random.default_rng(seed + letters)
    pool = [rng.integers(0, letters, 120).astype(np.uint8) for _ in range(5)]
    seqs = []
    for t in range(entries - 2):
        if rng.random() < 0.6:
            s = rng.integers(0, letters, rng.integers(1, 50)).astype(np.uint8)
        else:
            s = rng.integers(0, letters, rng.integers(170, 400)).astype(np.uint8)
            if rng.random() < 0.5:
                seg = pool[rng.integers(0, 5)]
                at = rng.integers(0, len(s) - 160)
                s[at:at + 120] = seg
            if rng.random() < 0.3:
                s[60:130] = letters - 1
            if rng.random() < 0.1:
                s[100:150] = s[40:90]
            if rng.random() < 0.7:
                s[-40:] = 0
        seqs.append(s)
    seqs += [seqs[-1].copy(), seqs[-3].copy()]
    return seqs


_cache = {}


def case(letters, k):
    """(seqs, offsets, codes, S, number of distinct k-mers): computed once, shared, never changed"""
    if ("in", letters) not in _cache:
        seqs = random_seqs(letters)
        _cache[("in", letters)] = (seqs,) + kr.codes_and_offsets(seqs)
    if (letters, k) not in _cache:
        seqs = _cache[("in", letters)][0]
        S, groups = kr.shared_counts(seqs, k)
        _cache[(letters, k)] = (np.array(S, np.uint32), groups)
    return _cache[("in", letters)] + _cache[(letters, k)]


@pytest.fixture(scope="module")
def program():
    assert os.path.exists(PROG), "rsem-for-ebseq-calculate-clustering-info was not built"
    return PROG


@pytest.mark.parametrize("rec", recorded(), ids=recorded_id)
def test_program_writes_the_recorded_file(program, tmp_path, rec):
    fa, k, u = rec
    out = os.path.join(str(tmp_path), "out.ump")
    r = subprocess.run([program, str(k), fa, out, "-q"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(u, "rb").read()
    names, _, dropped = kr.read_fasta(open(fa, "rb").read())
    assert r.stdout == kr.warnings_text(dropped)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("letters", [2, 5])
def test_random_inputs_equal_restatement(letters, k):
    seqs, off, codes, S, groups = case(letters, k)
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert np.array_equal(got, S)
    assert info["n_kmers"] == sum(max(len(s) - k + 1, 0) for s in seqs)
    assert info["n_groups"] == groups
    assert info["n_batches"] == 1 and info["n_chunks"] == (k + 26) // 27
    assert info["upload_ms"] > 0 and info["kernel_ms"] > 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("letters", [2, 5])
def test_batches_change_nothing(monkeypatch, letters, k):
    """A quarter of the k-mers per batch: at least 3 batches wherever the k-mers have 3 different values of their first min(k, 8)
    bases (two letters at k = 1 have two: there each value is a batch of its own, above the budget)."""
    seqs, off, codes, S, groups = case(letters, k)
    total = sum(max(len(s) - k + 1, 0) for s in seqs)
    budget = total // 4
    sizes = kr.expected_batches(seqs, k, budget)
    assert len(sizes) >= min(3, len(kr.bucket_histogram(seqs, k)))
    monkeypatch.setenv("RSEM_KMER_BATCH_ITEMS", str(budget))
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert np.array_equal(got, S)
    assert info["n_batches"] == len(sizes) and info["max_batch_items"] == max(sizes) and info["batch_items"] == budget
    assert info["n_groups"] == groups and info["n_kmers"] == total


@pytest.mark.parametrize("letters,k", [(2, 2), (5, 25), (5, 55)])
def test_a_bucket_above_the_budget_is_a_batch_of_its_own(monkeypatch, letters, k):
    seqs, off, codes, S, groups = case(letters, k)
    hist = kr.bucket_histogram(seqs, k)
    budget = max(c for _, c in hist) - 1  # the poly(A) bucket (the largest of four at k = 2)
    assert budget >= 200
    sizes = kr.expected_batches(seqs, k, budget)
    assert max(sizes) == budget + 1 and 3 <= len(sizes) <= 400
    monkeypatch.setenv("RSEM_KMER_BATCH_ITEMS", str(budget))
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert np.array_equal(got, S)
    assert info["n_batches"] == len(sizes) and info["max_batch_items"] == budget + 1 and info["n_groups"] == groups


@pytest.mark.parametrize("k", [25, 28])
def test_wide_sort_values(monkeypatch, k):
    """the 64-bit positions that references of 2^32 bases and more sort by, asked for on a small input"""
    seqs, off, codes, S, groups = case(5, k)
    monkeypatch.setenv("RSEM_KMER_WIDE_VALUES", "1")
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert np.array_equal(got, S) and info["n_groups"] == groups


def test_common_tail_makes_one_huge_group():
    """2000 entries that all end in the same 200 bases: groups of 2000 members, every one of them shared"""
    rng = np.random.default_rng(3)
    tail = rng.integers(0, 4, 200).astype(np.uint8)
    tail[-60:] = 0
    seqs = [np.concatenate([rng.integers(0, 4, rng.integers(20, 120)).astype(np.uint8), tail]) for _ in range(2000)]
    off, codes = kr.codes_and_offsets(seqs)
    S, groups = kr.shared_counts(seqs, 25)
    got, info = capi().kmer_shared_counts(off, codes, 25)
    assert np.array_equal(got, np.array(S, np.uint32)) and info["n_groups"] == groups
    assert min(S) >= 176
    # the budget counts 24 bytes per k-mer (keys and 32-bit positions, twice): the batch buffers must not hold a third copy of
    # keys and positions (12 bytes per k-mer) hidden in the library's temporary storage
    n = info["max_batch_items"]
    assert n == info["n_kmers"] > 400000 and 24 * n <= info["batch_bytes"] < 36 * n


def test_one_entry_500_times():
    """long runs of one transcript in the sorted list stay apart from their copies': every k-mer is shared, self-repeats included"""
    rng = np.random.default_rng(4)
    one = rng.integers(0, 4, 300).astype(np.uint8)
    one[200:250] = one[100:150]
    one[-45:] = 0
    other = rng.integers(0, 4, 260).astype(np.uint8)
    other[50:100] = other[150:200]  # repeated inside this entry only
    seqs = [one.copy() for _ in range(500)] + [other]
    off, codes = kr.codes_and_offsets(seqs)
    for k in (25, 28):
        S, groups = kr.shared_counts(seqs, k)
        assert S[:500] == [300 - k + 1] * 500 and S[500] == 0
        got, info = capi().kmer_shared_counts(off, codes, k)
        assert np.array_equal(got, np.array(S, np.uint32)) and info["n_groups"] == groups


def test_two_runs_give_identical_bytes(program, tmp_path):
    seqs = case(5, 25)[0]
    fa = os.path.join(str(tmp_path), "in.fa")
    with open(fa, "wb") as f:
        for t, s in enumerate(seqs):
            f.write(b">e%d\n" % t + bytes(b"ACGTN"[c] for c in s) + b"\n")
    outs = []
    for r in range(2):
        out = os.path.join(str(tmp_path), "out%d.ump" % r)
        subprocess.run([program, "25", fa, out, "-q", "--device", "0"], check=True)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == kr.ump(open(fa, "rb").read(), 25)


def test_invalid_arguments_are_refused(monkeypatch):
    c = capi()
    off = np.array([0, 4, 6], np.uint64)
    codes = np.array([0, 1, 2, 3, 4, 0], np.uint8)
    for bad_off, bad_codes, k in [(off, codes, 0), (off, codes, -25), (np.array([0, 5, 3], np.uint64), codes, 2),
                                  (np.array([1, 4, 6], np.uint64), codes, 2), (off, np.array([0, 1, 2, 3, 5, 0], np.uint8), 2)]:
        with pytest.raises(c.RsemHipError) as e:
            c.kmer_shared_counts(bad_off, bad_codes, k)
        assert e.value.status == INVALID
    for bad in ("0", "-5", "many", "12x", ""):
        monkeypatch.setenv("RSEM_KMER_BATCH_ITEMS", bad)
        with pytest.raises(c.RsemHipError) as e:
            c.kmer_shared_counts(off, codes, 2)
        assert e.value.status == INVALID and "RSEM_KMER_BATCH_ITEMS" in str(e.value)
    monkeypatch.delenv("RSEM_KMER_BATCH_ITEMS")
    long_off = np.array([0, 40000], np.uint64)
    with pytest.raises(c.RsemHipError) as e:  # a tile's halo of k - 1 codes has to fit the LDS
        c.kmer_shared_counts(long_off, np.zeros(40000, np.uint8), 32769)
    assert e.value.status == INVALID
    got, info = c.kmer_shared_counts(off, codes, 2)
    assert got.tolist() == [0, 0] and info["n_kmers"] == 4 and info["n_groups"] == 4
