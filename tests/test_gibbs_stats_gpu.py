"""The per-sample statistics behind rsem-run-gibbs's result files -- k_gibbs_stats_a, k_gibbs_stats_b, k_gibbs_group_stats,
k_sum_chains and k_reset_chains of rsem_amd/csrc/gibbs.hip -- against tests/stats_ref.py at the seams of their partition: the
statistics are taken by nblk = min(64, ceil(n / 2048)) workgroups per chain over n = M + 1 entries, `per` = ceil(n / nblk) each.

  n = 2048     one block
  n = 2049     two blocks of 1025 and 1024
  n = 5001     three blocks of 1667
  n = 131073   ceil(n / 2048) = 65 is capped to kStatMaxBlocks = 64: per = 2049, the last block holds 1986

What is compared is what the call itself returns: from the count vectors of the run, stats_ref forms the six accumulators, so the
comparison does not depend on which chain the sampler ran (in EXACT mode chain 0's vectors are checked against the oracle's
sequential chain as well, so the inputs of the comparison are anchored).  Three chains keep 4, 1 and 2 samples (burnin 1, gap 2):
in EXACT mode all chains share the statistics launches and chains 1 and 2 leave them early through `kept >= nsamples[chain]`.

Integer accumulators (pme_c, pve_c, pve_c_genes, pve_c_trans): sums of integers below 2^53 -- equal, whatever the order.

pme_tpm / pme_fpkm, bound from the number formats and the kernel's operation counts (u = 2^-53; every sum is over non-negative
terms, so relative errors only add up; first order, the second-order terms are 1e-13 of the bound and the count is rounded up):
  t_i = ((c_i + alpha_i) / totc) / mw_i                                   3 roundings
  S1, S2 = sums of t_i: at most D additions on the way of any term, D = ceil(per / 256) in the thread's strided sum + 6 shuffle
           levels + 4 for the waves' sums (the 6 + 2 level tree, its last two levels done one after the other) + nblk partials
           in pass B                                                       D + 3
  S3 = the same over t_i / eel_i                                           D + 4
  denom = S2 / S1                                                          2 D + 7
  fpkm_i = t_i / S1 / denom * 1e9 / eel_i        3 + (D + 3) + 1 + (2 D + 7) + 1 + 1 + 1 = 3 D + 17
  denom2 = S3 / S1 / denom * 1e9                 (D + 4) + (D + 3) + 1 + (2 D + 7) + 1 + 1 = 4 D + 17
  tpm_i = fpkm_i / denom2 * 1e6                  (3 D + 17) + (4 D + 17) + 2 = 7 D + 36
  += for each of a chain's kept samples (at most 4), k_sum_chains over 3 chains                    + 7
The reference's own error: stats_ref does WriteResults.h's sequential sums in longdouble (unit roundoff v, 2^-64 where
longdouble is the x87 format): by the same count with n additions per sum, (7 n + 37 + 7) v (see test_stats_ref_cpu.py).
  |device - reference| <= ((3 D + 24) u + (7 n + 44) v) |reference|   for pme_fpkm
  |device - reference| <= ((7 D + 43) u + (7 n + 44) v) |reference|   for pme_tpm
and zeros are zeros on both sides.  D = 19, 72 and 83 for the shapes above: 8.9e-15 (n = 2048) to 1.2e-13 (n = 131073) for tpm.

Largest |difference| / bound seen on an MI355X (every case prints its own):
  pme_fpkm at most 0.045 (n = 5001, PARALLEL, alpha), pme_tpm at most 0.025 (n = 2049, EXACT, alpha); at n = 131073, where the
  bound has its largest terms, 0.011 and 0.008; exactly 0 for both in the cases without any effective length; the four integer
  accumulators equal in all 24 cases.  (The bound is a worst case over every rounding, the errors seen behave like a random
  walk; a relative error of 1e-12 in one factor is 8 to 100 times the bound and fails every case.)
"""
import numpy as np
import pytest

import stats_ref
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

N1, N0 = 3000, 41
SEEDS, NSAMPLES, BURNIN, GAP = [11, 4000000011, 777], [4, 1, 2], 1, 2
SIZES = [2048, 2049, 5001, 131073]
CASES = ["pseudoC", "alpha", "no effective length"]
U = 2.0 ** -53
V = float(np.finfo(np.longdouble).eps) / 2


def capi():
    from rsem_amd import capi as c
    return c


def partition(n):
    nblk = max(1, min(64, -(-n // 2048)))
    return nblk, -(-n // nblk)


def _starts(M, rng, pool, forced):
    """group starts over 1..M: sizes drawn from pool, except that forced[start] = size groups sit where they are told"""
    out, pos, marks = [], 1, sorted(forced)
    while pos <= M:
        out.append(pos)
        if pos in forced:
            size = forced[pos]
        else:
            size = int(rng.choice(pool))
            nxt = [s for s in marks if s > pos]
            if nxt:
                size = min(size, nxt[0] - pos)
        pos = min(pos + size, M + 1)
    out.append(M + 1)
    return np.array(out, np.int32)


_INPUTS = {}


def inputs(n):
    """a few thousand short reads over n - 1 transcripts, many of them at the seams of the statistics' partition"""
    if n in _INPUTS:
        return _INPUTS[n]
    M = n - 1
    rng = np.random.default_rng(n)
    nblk, per = partition(n)
    rp, sid, cp = [0], [], []
    for i in range(N1):
        L = int(rng.integers(1, 5))
        kind = rng.random()
        if i < 4:           # (for certain: entries per - 2 .. per + 1 of the first boundary, and the last four)
            L, a = 4, (per - 2 if i < 2 else M - 3)
        elif kind < 0.4:      # around a boundary between two blocks (or the end of the only one)
            a = int(rng.integers(1, nblk + 1)) * per - 6 + int(rng.integers(0, 10))
        elif kind < 0.5:    # the last entries
            a = M - int(rng.integers(0, 8))
        else:
            a = int(rng.integers(1, M + 1))
        a = max(1, min(a, M - L + 1))
        scale = 10.0 ** rng.uniform(-8, -3)
        sid += [0] + list(range(a, a + L))
        cp += [scale * 2.0 ** rng.uniform(-14, -6)] + list(scale * 2.0 ** rng.uniform(-6, 0, L))
        rp.append(len(sid))
    sid = np.array(sid, np.int32)
    hit = np.bincount(sid, minlength=n) > 0
    free = np.flatnonzero(~hit[1:]) + 1
    omitted = rng.choice(free, max(4, len(free) // 50), replace=False)          # init = -1: transcripts no read points to
    init = np.zeros(n, np.int32)
    init[omitted] = -1
    eel = rng.uniform(200.0, 3000.0, n)
    eel[0] = 0.0
    eel[omitted[::2]] = 0.0
    eel[1:][rng.random(M) < 0.05] = 0.0
    mw = np.where(rng.random(n) < 0.1, 0.9, 1.0)
    mw[1:][rng.random(M) < 0.03] = 0.0
    big = min(3000, M // 3)
    forced = {per - 2: 5, per + 3: big} if nblk > 1 else {5: big}
    grp = _starts(M, rng, [1, 1, 1, 2, 3, 5], forced)
    ta = _starts(M, rng, [1, 1, 2, 3], {})
    sizes = np.diff(grp)
    assert grp[0] == 1 and grp[-1] == n and (sizes > 0).all() and (sizes == 1).sum() > 100 and sizes.max() == big
    if nblk > 1:            # a gene with members in two blocks: entries per - 1 and per
        g = np.searchsorted(grp, per - 1, side="right") - 1
        assert grp[g] <= per - 1 and grp[g + 1] > per
    assert ta[0] == 1 and ta[-1] == n and set(np.diff(ta)) == {1, 2, 3}
    assert hit[per - 1] and hit[min(per, M)] and hit[M] and (hit[1:] & (eel[1:] == 0)).any() and (hit[1:] & (mw[1:] == 0)).any()
    assert (eel[omitted] > 0).any()
    d = dict(M=M, rp=np.array(rp, np.uint64), sid=sid, cp=np.array(cp), init=init, eel=eel, mw=mw, grp=grp, ta=ta,
             alpha=rng.choice([0.05, 0.4, 1.0, 2.5], n))
    _INPUTS[n] = d
    return d


def _case(n, case):
    d = inputs(n)
    alpha = d["alpha"] if case == "alpha" else None
    eel = np.zeros(n) if case == "no effective length" else d["eel"]
    pseudoC = 1.0
    totc = float(N0 + N1 + (alpha.sum() if alpha is not None else n * pseudoC))
    return d, alpha, eel, pseudoC, totc


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", ["EXACT", "PARALLEL"])
@pytest.mark.parametrize("n", SIZES)
def test_six_accumulators_against_stats_ref(n, mode, case):
    c = capi()
    d, alpha, eel, pseudoC, totc = _case(n, case)
    M = d["M"]
    ctx = c.GibbsContext(M, d["rp"], d["sid"], d["cp"], d["init"], alpha, pseudoC, totc, N0, eel, d["mw"], d["grp"])
    ctx.set_allele_groups(d["ta"])
    cvs, acc, trans, prof = ctx.run_chains(c.GIBBS_EXACT if mode == "EXACT" else c.GIBBS_PARALLEL, SEEDS, BURNIN, NSAMPLES, GAP)
    again = ctx.get_pve_c_trans()
    ctx.close()
    assert prof.chains == 3 and [len(a) for a in cvs] == NSAMPLES
    for cv in cvs:          # every read once, omitted transcripts stay omitted
        assert np.all(cv.astype(np.int64).sum(1) == N0 + N1 + int(d["init"].sum())) and np.all(cv[:, d["init"] < 0] == -1)
    if mode == "EXACT":
        ocv, _ = orc.gibbs_chain(M, d["rp"], d["sid"], d["cp"], d["init"], alpha, pseudoC, totc, N0, eel, d["mw"], d["grp"], SEEDS[0],
                                 BURNIN, NSAMPLES[0], GAP)
        assert np.array_equal(cvs[0], ocv)
    ref = stats_ref.gibbs_stats(cvs, alpha, pseudoC, totc, eel, d["mw"], d["grp"], d["ta"])
    pme_c, pve_c, pme_tpm, pme_fpkm, pve_c_genes = acc
    for name, dev in (("pme_c", pme_c), ("pve_c", pve_c), ("pve_c_genes", pve_c_genes), ("pve_c_trans", trans)):
        want = ref[name].astype(np.float64)
        bad = np.flatnonzero(dev != want)
        assert len(bad) == 0, "%s[%d]: device %r, reference %r (%d entries differ)" % (name, bad[0], dev[bad[0]], want[bad[0]], len(bad))
    assert np.array_equal(again, trans)
    assert ref["pve_c"].max() > 0 and ref["pve_c_genes"].max() > 0 and ref["pve_c_trans"].max() > 0
    nblk, per = partition(n)
    D = -(-per // 256) + 6 + 4 + nblk
    ratios = []
    for name, dev, k in (("pme_fpkm", pme_fpkm, 3 * D + 24), ("pme_tpm", pme_tpm, 7 * D + 43)):
        r = ref[name]
        bound = (k * U + (7 * n + 44) * V) * r
        err = np.abs(dev.astype(np.longdouble) - r)
        ratios.append(float((err[r > 0] / bound[r > 0]).max()) if (r > 0).any() else 0.0)
        assert np.array_equal(dev == 0, r == 0), "%s: zeros must be zeros on both sides" % name
        bad = np.flatnonzero(err > bound)
        assert len(bad) == 0, "%s[%d]: device %r, reference %r, bound %.3g relative (%d entries beyond it)" % (
            name, bad[0], dev[bad[0]], float(r[bad[0]]), float(k * U + (7 * n + 44) * V), len(bad))
    print("n = %d, %s, %s: largest |difference| / bound: pme_fpkm %.3f, pme_tpm %.3f" % (n, mode, case, ratios[0], ratios[1]))
    if case == "no effective length":
        assert not pme_tpm.any() and not pme_fpkm.any()
    else:
        live = (d["eel"] > 0) & (d["mw"] > 0) & (d["init"] == 0)
        live[0] = False
        assert np.all(pme_tpm[live] > 0) and not pme_tpm[~live].any()
        assert abs(pme_tpm.sum() - 1e6 * sum(NSAMPLES)) < 1e-3


def test_pve_c_trans_accessor_needs_a_run():
    """rsem_gibbs_get_pve_c_trans: RSEM_ERR_STATE before allele groups are set, and after that until a chain has run; then
    the array the run returned."""
    c = capi()
    d, alpha, eel, pseudoC, totc = _case(2048, "pseudoC")
    ctx = c.GibbsContext(d["M"], d["rp"], d["sid"], d["cp"], d["init"], None, pseudoC, totc, N0, eel, d["mw"], d["grp"])
    try:
        for step in range(2):
            with pytest.raises(c.RsemHipError) as e:
                ctx.get_pve_c_trans()
            assert e.value.status == -5
            if step == 0:
                ctx.set_allele_groups(d["ta"])
        _, _, trans, _ = ctx.run_chains(c.GIBBS_PARALLEL, [5], 0, [1], 1)
        got = ctx.get_pve_c_trans()
        assert len(got) == len(d["ta"]) - 1 and np.array_equal(got, trans) and trans.any()
    finally:
        ctx.close()


def test_group_arrays_are_validated_on_the_host():
    """grp (rsem_gibbs_create) and ta (rsem_gibbs_set_allele_groups) index the count vector in k_gibbs_group_stats: an array
    that does not start at 1, end at M + 1 or that decreases is refused with RSEM_ERR_INVALID before anything is launched."""
    c = capi()
    d, alpha, eel, pseudoC, totc = _case(2048, "pseudoC")
    M = d["M"]
    bad = {"starts at 0": [0, 5, M + 1], "starts at 2": [2, 5, M + 1], "ends at M": [1, 5, M], "ends past M + 1": [1, 5, M + 2],
           "decreases": [1, 9, 5, M + 1], "runs out of range in between": [1, M + 7, M + 1]}
    for what, starts in bad.items():
        with pytest.raises(c.RsemHipError, match="first transcripts") as e:
            c.GibbsContext(M, d["rp"], d["sid"], d["cp"], d["init"], None, pseudoC, totc, N0, eel, d["mw"], np.array(starts, np.int32))
        assert e.value.status == -1, what
    ctx = c.GibbsContext(M, d["rp"], d["sid"], d["cp"], d["init"], None, pseudoC, totc, N0, eel, d["mw"], d["grp"])
    try:
        for what, starts in bad.items():
            with pytest.raises(c.RsemHipError, match="first alleles") as e:
                ctx.set_allele_groups(np.array(starts, np.int32))
            assert e.value.status == -1, what
    finally:
        ctx.close()
