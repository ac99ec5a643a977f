"""Shared k-mers on the GPU at the limits the kernels name (inputs: tests/kmer_limits.py) against the Python restatement
(tests/kmer_ref.py): equality of every count, of the number of distinct k-mers and of the number of chunks.

  chunk counts      k = 81 | 82 and 108 | 109 on the random inputs of tests/test_kmer_gpu.py: three to four and four to five sorts
  large k           2047, 2048, 2049, 4100 and kMaxK = 32768 (1214 chunks, the last of 17 bases; a halo of 32767 codes in LDS): the halo
                    spans one tile and more, k-mers that differ in the first chunk, the last chunk, base 27 or a middle chunk alone
  seams             separators on the tile, lane and word seams of the separated layout; tiles of separators only; one k-mer"""
import numpy as np
import pytest

import kmer_limits as kl
import kmer_ref as kr
from test_kmer_gpu import case

pytestmark = pytest.mark.gpu

_cache = {}


def capi():
    from rsem_amd import capi as c
    return c


def expected(name, seqs, k):
    """(offsets, codes, S, groups) of an input: computed once, shared, never changed"""
    if (name, k) not in _cache:
        S, groups = kr.shared_counts(seqs, k)
        _cache[(name, k)] = kr.codes_and_offsets(seqs) + (np.array(S, np.uint32), groups)
    return _cache[(name, k)]


def check(name, seqs, k, batches=1):
    off, codes, S, groups = expected(name, seqs, k)
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert info["n_chunks"] == (k + 26) // 27 and info["n_kmers"] == sum(max(len(s) - k + 1, 0) for s in seqs)  # the path first
    assert info["n_batches"] == batches if batches else info["n_batches"] > 1
    assert np.array_equal(got, S) and info["n_groups"] == groups
    return S, info


@pytest.mark.parametrize("k", [81, 82, 108, 109])
def test_one_chunk_more(k):
    seqs, off, codes, S, groups = case(5, k)
    got, info = capi().kmer_shared_counts(off, codes, k)
    assert info["n_chunks"] == (k + 26) // 27 == {81: 3, 82: 4, 108: 4, 109: 5}[k] and info["n_batches"] == 1
    assert np.array_equal(got, S) and info["n_groups"] == groups and S.max() > 0


@pytest.mark.parametrize("k", [2047, 2048, 2049, 4100, 32768])
def test_k_of_a_tile_and_more(monkeypatch, k):
    monkeypatch.delenv("RSEM_KMER_BATCH_ITEMS", raising=False)
    monkeypatch.delenv("RSEM_KMER_WIDE_VALUES", raising=False)
    seqs = kl.large_k_seqs(k)
    S, info = check("large", seqs, k)
    # A, its copy and the one changed behind the first k-mers share everything or nearly; k bases of A are one shared k-mer; k - 1 none
    assert S[0] == S[4] == 41 and S[1] == S[2] == 40 and S[5] == 1 and S[6] == 0 and S[3] == 0 and S[7] < 41
    if k == 32768:
        assert info["n_chunks"] == 1214 and k - 27 * 1213 == 17


def test_k_of_a_tile_and_more_in_batches_and_with_wide_values(monkeypatch):
    k = 2049
    seqs = kl.large_k_seqs(k)
    total = sum(max(len(s) - k + 1, 0) for s in seqs)
    monkeypatch.setenv("RSEM_KMER_BATCH_ITEMS", str(total // 4))
    sizes = kr.expected_batches(seqs, k, total // 4)
    assert len(sizes) >= 3
    _, info = check("large", seqs, k, batches=len(sizes))
    assert info["max_batch_items"] == max(sizes)
    monkeypatch.delenv("RSEM_KMER_BATCH_ITEMS")
    monkeypatch.setenv("RSEM_KMER_WIDE_VALUES", "1")
    check("large", seqs, k)


@pytest.mark.parametrize("extra", [0, 1], ids=["tiles_full", "one_past"])
@pytest.mark.parametrize("k", [1, 8, 25, 28])
def test_separators_on_every_seam(monkeypatch, k, extra):
    monkeypatch.delenv("RSEM_KMER_BATCH_ITEMS", raising=False)
    seqs = kl.seam_seqs(extra)
    at = kl.separated_positions(seqs)
    assert set(kl.SEAM_SEPARATORS) <= set(at) and at[-1] + 1 == 3 * kl.TILE + extra and at[-kl.TILE:] == list(range(2 * kl.TILE + extra, 3 * kl.TILE + extra))
    assert {p % 8 for p in at[:16]} == set(range(8)) and [len(s) for s in seqs[16:24]] == [1000 - 916, 0, 1044, 0, 0, 0, 2045, 0]
    S, _ = check("seams%d" % extra, seqs, k)
    assert S.max() > 0
    monkeypatch.setenv("RSEM_KMER_BATCH_ITEMS", "1")  # every bucket of first bases a batch of its own
    check("seams%d" % extra, seqs, k, batches=len(kr.expected_batches(seqs, k, 1)))


@pytest.mark.parametrize("k", [1, 8, 25, 28])
def test_exactly_one_kmer(k):
    seqs = [np.zeros(0, np.uint8), np.arange(k - 1, dtype=np.uint8) % 4, np.arange(k, dtype=np.uint8) % 5, np.zeros(0, np.uint8)]
    S, info = check("one", seqs, k)
    assert info["n_kmers"] == 1 and info["n_groups"] == 1 and S.tolist() == [0, 0, 0, 0]
