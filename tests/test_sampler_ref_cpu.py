"""tests/sampler_ref.py -- the CPU restatement the GPU replay tests (test_gibbs_replay_gpu.py, test_ci_replay_gpu.py) hold the
device samplers to -- is itself checked here: its Philox against the Random123 known-answer vectors, its two gamma samplers
against the Gamma distribution, its z pass on an input small enough to follow by hand.  No GPU involved."""
import math

import numpy as np
import pytest
import torch

import sampler_ref as sr


def test_philox_known_answers():
    """The vectors of Random123's kat_vectors that tests/rng_kat_check.cpp runs through rng.hpp."""
    k4 = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
          ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, o in k4:
        assert tuple(int(w[0]) for w in sr.philox4x32_10(k[0], k[1], *c)) == o
    k2 = [((0, 0), 0, (0xff1dae59, 0x6cd10df2)), ((0xffffffff, 0xffffffff), 0xffffffff, (0x2c3f628b, 0xab4fd7ad)),
          ((0x243f6a88, 0x85a308d3), 0x13198a2e, (0xdd7ce038, 0xf62a4c12))]
    for c, k, o in k2:
        assert tuple(int(w[0]) for w in sr.philox2x32_10(k, *c)) == o
    # vectorised = element by element
    c0 = np.array([0, 0xffffffff, 0x243f6a88])
    got = sr.philox2x32_10(0x13198a2e, c0, 0x85a308d3)
    assert (int(got[0][2]), int(got[1][2])) == k2[2][2]
    # u53: the top 27 bits of the first word over the top 26 of the second
    assert sr.u53(np.array([0xffffffff], np.uint64), np.array([0xffffffff], np.uint64))[0] == 1.0 - 2.0 ** -53
    assert sr.u53(np.array([1 << 5], np.uint64), np.array([0], np.uint64))[0] == 2.0 ** -27
    assert sr.u53(np.array([0], np.uint64), np.array([1 << 6], np.uint64))[0] == 2.0 ** -53


N_KS = 100_000
# Kolmogorov's limit P(D_n > x) = 2 sum_k (-1)^(k-1) exp(-2 k^2 n x^2); at p = 1e-6 the first term is all of it:
# x = sqrt(ln(2 / p) / (2 n)) = 0.008517 for n = 1e5.
KS_CRIT = math.sqrt(math.log(2.0 / 1e-6) / (2.0 * N_KS))


@pytest.mark.parametrize("kind", ["gamma_draw", "gamma_draw_bulk"])
@pytest.mark.parametrize("a", [0.05, 0.3, 1.0, 1.5, 40.0, 1e5])
def test_reference_gamma_is_gamma(kind, a):
    """1e5 draws of the reference, fixed seed, against the regularized incomplete gamma function."""
    assert abs(KS_CRIT - 0.008517) < 1e-6
    idx = np.arange(N_KS)
    if kind == "gamma_draw":
        x, margin = sr.gamma_draw(20251, sr.KEY_GIBBS, idx, 7, np.full(N_KS, a))
    else:
        x, margin = sr.gamma_draw_bulk(20251, sr.KEY_CI, idx % 977, idx // 977, sr.CI_TAG, np.full(N_KS, a))
    assert np.all(x >= 0) and np.all(np.isfinite(x)) and np.all(margin > 0)
    x = np.sort(x)
    F = torch.special.gammainc(torch.full((N_KS,), a, dtype=torch.float64), torch.from_numpy(x)).numpy()
    i = np.arange(1, N_KS + 1)
    D = max((i / N_KS - F).max(), (F - (i - 1) / N_KS).max())
    print("a = %g %s: KS D = %.5f (critical %.5f), smallest decision margin %.3g" % (a, kind, D, KS_CRIT, margin.min()))
    assert D < KS_CRIT


def test_gamma_counter_conventions():
    """Draws that differ only in a counter word are different draws, and a < 1 is Gamma(a + 1)'s draw of the NEXT counter
    value times the boost: the running counter of gamma_draw, the separate boost block of gamma_draw_bulk."""
    one = np.array([5])
    g, _ = sr.gamma_draw(1, 2, one, 3, [0.25])
    r = sr.philox4x32_10(1, 2, 5, 3, sr.GAMMA_TAG, 0)
    u = sr.u53(r[0], r[1])[0]
    # Gamma(1.25) drawn with the counter starting at 1 = the draw of (idx, sweep) whose first block is skipped
    skipped = {"n": 0}

    def block(kind, sel):
        skipped["n"] += 1
        rr = sr.philox4x32_10(1, 2, 5, 3, sr.GAMMA_TAG, skipped["n"])
        return (sr.u53(rr[0], rr[1]), sr.u53(rr[2], rr[3]), None) if kind == "attempt" else sr.u53(rr[0], rr[1])
    g1, _ = sr._gamma(block, [1.25])
    assert g[0] == g1[0] * np.exp(np.log(u) / 0.25)
    gb, _ = sr.gamma_draw_bulk(1, 2, one, one, 9, [0.25])
    gb1, _ = sr.gamma_draw_bulk(1, 2, one, one, 9, [1.25])
    r = sr.philox4x32_10(1, 2, 5, 5, 9, 0x80000000)
    assert gb[0] == gb1[0] * np.exp(np.log(sr.u53(r[0], r[1])[0]) / 0.25)


def test_z_pass_by_hand():
    """Three reads, g = 1 everywhere, weights in units of a quarter: the picks follow from the printed uniforms."""
    #          read 0: noise 1, sid 1: 1, sid 2: 2      read 1 (two lanes): sids 3, 4, 5, no noise     read 2: noise only
    rp = np.array([0, 3, 6, 7])
    sid = np.array([0, 1, 2, 3, 4, 5, 0])
    cp = np.array([1.0, 1.0, 2.0, 1.0, 2.0, 1.0, 0.5])
    order, lg = np.array([2, 0, 1]), np.array([0, 0, 1])     # sorted position -> read
    reads = sr.Reads(rp, sid, cp, order, lg)
    assert list(reads.ncp) == [0.5, 1.0, 0.0]
    assert [list(s) for s in reads.sid] == [[], [1, 2], [3, 5, 4]]  # lane-major: lane 0 holds items 0 and 2, lane 1 item 1
    assert list(sr.lane_major(7, 2)) == [0, 4, 1, 5, 2, 6, 3]
    seed, sweep = 11, 4
    u = reads.uniforms(seed, sweep)
    key = seed ^ (((sr.KEY_GIBBS << 13) | (sr.KEY_GIBBS >> 19)) & 0xffffffff) ^ 0x5a5a5a5a
    for p in range(3):  # a sliced read's uniform: Philox2x32-10 keyed by the folded key, counter (position, sweep)
        w = sr.philox2x32_10(key, p, sweep)
        assert u[p] == sr.u53(w[0], w[1])[0]
    print("uniforms of positions 0..2:", u)
    exp = np.zeros(6, np.int64)
    exp[0] += 1                                                   # position 0 = read 2: only the noise item
    exp[0 if u[1] < 0.25 else 1 if u[1] < 0.5 else 2] += 1        # position 1 = read 0: 1/4 noise, 1/4 sid 1, 1/2 sid 2
    exp[3 if u[2] < 0.25 else 5 if u[2] < 0.5 else 4] += 1        # position 2 = read 1: sid 3, then 5, then 4 (weight 2)
    counts = np.zeros(6, np.int64)
    worst = reads.z_pass(np.ones(6), seed, sweep, counts)
    assert np.array_equal(counts, exp)
    assert 0 < worst <= 0.5
    # a read that stays in the CSR: plain item order, Philox4x32-10 (position, sweep, tag, 0), words 0 and 1
    long_reads = sr.Reads(rp, sid, cp, order, np.array([0, 0, sr.LONG]))
    assert list(long_reads.sid[2]) == [3, 4, 5]
    w = sr.philox4x32_10(seed, sr.KEY_GIBBS, 2, sweep, 0x5a5a5a5a, 0)
    assert long_reads.uniforms(seed, sweep)[2] == sr.u53(w[0], w[1])[0]
    # g = 0 for a transcript takes it out; a read whose every weight is zero is assigned nowhere; the clamp at u -> 1
    assert sr.pick([0.0, 1.0, 0.0, 1.0, 0.0], 0.75)[0] == 3
    assert sr.pick([0.0, 0.0], 0.3)[0] == -1
    assert sr.pick([1.0, 1.0, 0.0], 1.0 - 2.0 ** -53)[0] == 1
    k, m = sr.pick([1.0, 1.0, 2.0], 0.5 + 1e-12)
    assert k == 2 and abs(m - 1e-12) < 1e-15


def test_chain_follows_the_host_loop():
    """burnin / gap / thin bookkeeping: the kept vectors of (burnin 1, gap 2) are rounds 2 and 4 of the (0, 1) chain, every
    vector holds every read once on top of N0, and an omitted transcript nobody points to stays at -1."""
    rng = np.random.default_rng(3)
    M, n = 12, 40
    lens = rng.integers(1, 6, n)
    rp = np.concatenate([[0], np.cumsum(lens)])
    sid = np.concatenate([np.sort(rng.choice(np.arange(0, 11), L, replace=False)) for L in lens])
    cp = rng.uniform(0.1, 1.0, len(sid))
    init = np.zeros(M + 1, np.int32)
    init[12] = -1
    reads = sr.Reads(rp, sid, cp, rng.permutation(n), np.zeros(n, np.uint8))
    every, mp, mg = sr.parallel_chain(reads, M, init, None, 0.7, 9, 5, 0, 4, 1)
    some, _, _ = sr.parallel_chain(reads, M, init, None, 0.7, 9, 5, 1, 2, 2)
    assert np.array_equal(some, every[[1, 3]])
    assert np.all(every[:, 12] == -1) and np.all(every[:, :12].sum(1) == 9 + n) and np.all(every[:, 0] >= 9)
    assert mp > 0 and mg > 0
    thin2, _, _ = sr.parallel_chain(reads, M, init, None, 0.7, 9, 5, 0, 2, 1, thin=2)
    assert np.array_equal(thin2, every[[1, 3]])   # two pairs per round = every second round of the thin = 1 chain
