"""The per-sample statistics of rsem-run-gibbs (Gibbs.cpp:313-346 with polishTheta / calcExpressionValues, WriteResults.h:55-104)
restated for the tests from kept count vectors alone -- what k_gibbs_stats_a / k_gibbs_stats_b / k_gibbs_group_stats / k_sum_chains
of rsem_amd/csrc/gibbs.hip accumulate on the device.  No GPU, no product code.

* pme_c, pve_c, pve_c_genes, pve_c_trans are sums of integers: computed in int64 (guarded: every result below 2^53, so a double
  holds it exactly whatever the order of summation);
* pme_tpm, pme_fpkm in np.longdouble, in the reference's own order of operations as orc_polish_theta / orc_calc_expression
  restate it: theta_i = (c_i + alpha_i) / totc, theta_i /= mw_i (0 where the transcript has no weight), every theta divided by
  their left-to-right sum; frac = theta over the transcripts with an effective length, divided by its sum (1 when below
  EPSILON); fpkm = frac * 1e9 / eel; tpm = fpkm / sum fpkm (1 when below EPSILON) * 1e6.  NOT the kernel's fused form.
"""
import numpy as np

L = np.longdouble
EPSILON = 1e-300


def _seq_sum(x):
    """left to right, as the reference's loops"""
    return np.cumsum(x, dtype=L)[-1] if len(x) else L(0)


def expression(counts, alpha, pseudoC, totc, eel, mw):
    """(tpm, fpkm) of one count vector, np.longdouble[M + 1]"""
    c = np.asarray(counts)
    n = len(c)
    eel, mw = np.asarray(eel, np.float64), np.asarray(mw, np.float64)
    a = (np.asarray(alpha, np.float64) if alpha is not None else np.full(n, float(pseudoC))).astype(L)
    theta = np.where(c < 0, L(0), (c.astype(L) + a) / L(totc))               # Gibbs.cpp:316-319
    idx = np.arange(n)
    dead = (idx > 0) & ((mw < EPSILON) | (eel < EPSILON))                       # polishTheta
    theta = np.where(dead, L(0), theta / np.where(dead, 1.0, mw).astype(L))
    s = _seq_sum(theta)
    if s >= EPSILON:
        theta = theta / s
    live = (idx >= 1) & (eel >= EPSILON)                                        # calcExpressionValues
    frac = np.where(live, theta, L(0))
    denom = _seq_sum(frac[1:])
    if denom < EPSILON:
        denom = L(1)
    frac = frac / denom
    fpkm = np.where(live, frac * L(1e9) / np.where(live, eel, 1.0).astype(L), L(0))
    denom2 = _seq_sum(fpkm[1:])
    if denom2 < EPSILON:
        denom2 = L(1)
    tpm = fpkm / denom2 * L(1e6)
    tpm[0] = 0
    return tpm, fpkm


def _group_sums(c, starts):
    """sum of c over [starts[g], starts[g + 1]) for every group, empty groups included"""
    cs = np.concatenate([[0], np.cumsum(c, dtype=np.int64)])
    s = np.asarray(starts, np.int64)
    g = cs[s[1:]] - cs[s[:-1]]
    assert np.abs(g).max(initial=0) < 2 ** 26     # (squares and their sums over the samples stay far inside int64)
    return g


def gibbs_stats(cvs, alpha, pseudoC, totc, eel, mw, grp, ta=None):
    """cvs: one (nsamples_k, M + 1) int32 array per chain.  Returns a dict: pme_c, pve_c, pve_c_genes, pve_c_trans (None without
    ta) as int64 arrays, pme_tpm, pme_fpkm as np.longdouble arrays: the sums over every kept sample of every chain."""
    if isinstance(cvs, np.ndarray):
        cvs = [cvs]
    n = cvs[0].shape[1]
    out = dict(pme_c=np.zeros(n, np.int64), pve_c=np.zeros(n, np.int64), pve_c_genes=np.zeros(len(grp) - 1, np.int64),
               pve_c_trans=None if ta is None else np.zeros(len(ta) - 1, np.int64), pme_tpm=np.zeros(n, L), pme_fpkm=np.zeros(n, L))
    for cv in cvs:                                            # release(): chain totals, added in chain order
        t_sum, f_sum = np.zeros(n, L), np.zeros(n, L)
        for counts in cv:
            c = counts.astype(np.int64)
            assert np.abs(c).max() < 2 ** 26
            out["pme_c"] += c
            out["pve_c"] += c * c
            out["pve_c_genes"] += _group_sums(c, grp) ** 2
            if ta is not None:
                out["pve_c_trans"] += _group_sums(c, ta) ** 2
            tpm, fpkm = expression(counts, alpha, pseudoC, totc, eel, mw)
            t_sum += tpm
            f_sum += fpkm
        out["pme_tpm"] += t_sum
        out["pme_fpkm"] += f_sum
    for k in ("pme_c", "pve_c", "pve_c_genes", "pve_c_trans"):
        assert out[k] is None or np.abs(out[k]).max(initial=0) < 2 ** 53, k
    return out
