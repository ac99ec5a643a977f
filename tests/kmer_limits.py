"""Inputs at the limits rsem_amd/csrc/kmer.hip and kmer_block.hpp name, for tests/test_kmer_limits_gpu.py: k up to kMaxK = 32768 (a tile
stages 2048 + k - 1 codes, a k-mer is (k + 26) // 27 chunks and as many sorts, is_head compares k - 27 codes), and separators placed
on the tile (2048 starts), lane (8 starts) and word (4 codes) seams of the SEPARATED layout, where transcript t starts at
seq_off[t] + t and its separator sits one behind its last base.  tests/kmer_check.cpp builds the same two constructions."""
import numpy as np

TILE = 2048  # starts a workgroup: kTile of kmer.hip
CHUNK = 27   # kChunkBases


def large_k_seqs(k, seed=7):
    """sequences of k + 40 bases that differ from the first one, A, in one base: the first (chunk 0 of the k-mer at 0), the last (the
    last chunk of the k-mer at 40), base 27 (the first one is_head looks at), one in a middle chunk; an exact copy; k bases of A, a
    k-mer of their own; k - 1 bases, none"""
    rng = np.random.default_rng(seed + k)
    a = rng.integers(0, 4, k + 40).astype(np.uint8)
    nc = (k + CHUNK - 1) // CHUNK
    mid = CHUNK * 600 if k + 40 > CHUNK * 601 else CHUNK * (nc // 2)

    def changed(at):
        s = a.copy()
        s[at] = (s[at] + 1) % 4
        return s

    return [a, changed(0), changed(len(a) - 1), changed(mid), a.copy(), a[20:20 + k].copy(), a[3:3 + k - 1].copy(), changed(CHUNK)]


SEAM_SEPARATORS = ([300 + 41 * i for i in range(16)]      # every residue mod 4 and mod 8, twice; transcripts of 40 bases between them
                   + [1000, 1001]                         # a transcript of no bases, alone
                   + [2046, 2047, 2048, 2049]             # three of them in a row over the tile seam
                   + [4095, 4096])                        # the last start of a tile, the first of the next: one more of no bases


def seam_seqs(extra, seed=5):
    """the transcripts whose separators sit on SEAM_SEPARATORS and then on every position up to L + M = 3 * 2048 + extra: the last tile
    (two tiles for extra = 1) holds separators only.  The bases repeat a motif of 97 with a change every 61: most k-mers are shared."""
    rng = np.random.default_rng(seed)
    seps = sorted(SEAM_SEPARATORS) + list(range(4097, 3 * TILE + extra))
    motif = rng.integers(0, 4, 97).astype(np.uint8)
    flat = np.tile(motif, seps[-1] // 97 + 1)[:seps[-1] + 1].copy()
    flat[::61] = rng.integers(0, 5, len(flat[::61]))  # an N now and then: the fifth letter
    seqs, prev = [], -1
    for p in seps:
        seqs.append(flat[prev + 1:p].copy())
        prev = p
    assert sum(len(s) for s in seqs) + len(seqs) == 3 * TILE + extra
    return seqs


def separated_positions(seqs):
    """where the separators sit in the separated layout"""
    return (np.cumsum([len(s) for s in seqs]) + np.arange(len(seqs))).tolist()
