"""tests/stats_ref.py (the reference the GPU test of the Gibbs statistics kernels compares with) pinned without a device: on
golden fixtures its accumulators agree with the oracle's restatement of Gibbs.cpp:313-346 (orc.gibbs_chain), whose own output is
pinned on the reference's result files (test_oracle_golden.py).

Bounds: the four integer accumulators are sums of integers below 2^53 -- equal.  pme_tpm / pme_fpkm: the oracle works in double
(u = 2^-53), left to right, every term non-negative, so relative errors only add up: theta_i / mw_i carries 3 roundings, their sum
over n = M + 1 terms n more, theta / sum: n + 7; the sum of those 2 n + 7, frac: 3 n + 15, fpkm: 3 n + 17; the sum of the fpkm
4 n + 17, tpm: 7 n + 36; and one rounding per kept sample and chain added.  stats_ref does the same in longdouble (2^-11 of that,
covered by rounding the count up): |a - b| <= (7 n + 37 + samples) u |b| for either, and zeros are zeros on both sides.
"""
import os

import numpy as np
import pytest

import rsem_files as rf
import stats_ref
from oracle import pyoracle as orc


def load(name):
    fx = rf.fixture(name)
    M, N0, rp, sid, val = rf.read_ofg(os.path.join(fx, "temp", "s.ofg"))
    model = rf.read_model(os.path.join(fx, "stat", "s.model"))
    full, tot = rf.read_seq_lens(os.path.join(fx, "ref.seq"))
    grp = rf.read_grp(os.path.join(fx, "ref.grp"))
    ta = rf.read_grp(os.path.join(fx, "ref.ta")) if os.path.exists(os.path.join(fx, "ref.ta")) else None
    eel = orc.calc_eel(M, full, tot, model["gld"])
    N1 = len(rp) - 1
    init, pseudoC, totc = rf.gibbs_setup(fx, M, N0, N1)
    return dict(fx=fx, M=M, N0=N0, N1=N1, rp=rp, sid=sid, val=val, eel=eel, mw=model["mw"], grp=grp, ta=ta,
                meta=rf.read_meta(fx), totc=totc, init=init, pseudoC=pseudoC)


@pytest.mark.parametrize("name,prior", [("se_q_allele", False), ("se_noq_rev_rspd_omit", False), ("se_q_allele", True)])
def test_stats_ref_agrees_with_the_oracle_chain(name, prior):
    d = load(name)
    M = d["M"]
    burnin, nsamples, gap = d["meta"]["gibbs"]
    alpha = np.random.default_rng(3).choice([0.05, 0.4, 1.0, 2.5], M + 1) if prior else None
    ns = [min(nsamples, 7), 3]
    seeds = orc.chain_seeds(d["meta"]["gibbs_seed"], 2)
    cvs, want = [], None
    for k in range(2):
        cv, acc = orc.gibbs_chain(M, d["rp"], d["sid"], d["val"], d["init"], alpha, d["pseudoC"], d["totc"], d["N0"], d["eel"],
                                  d["mw"], d["grp"], seeds[k], burnin, ns[k], gap)
        cvs.append(cv)
        want = acc if want is None else [x + y for x, y in zip(want, acc)]
    got = stats_ref.gibbs_stats(cvs, alpha, d["pseudoC"], d["totc"], d["eel"], d["mw"], d["grp"], d["ta"])
    for key, b in zip(("pme_c", "pve_c"), want[:2]):
        assert np.array_equal(got[key].astype(np.float64), b), key
    assert np.array_equal(got["pve_c_genes"].astype(np.float64), want[4])
    rtol = (7 * (M + 1) + 37 + sum(ns)) * 2.0 ** -53
    for key, b in zip(("pme_tpm", "pme_fpkm"), want[2:4]):
        a = got[key]
        assert np.array_equal(a == 0, b == 0), key
        err = np.abs(a - b.astype(np.longdouble))
        print("%s %s: largest |difference| / bound %.3f" % (name, key, float((err[b != 0] / (rtol * b[b != 0])).max())))
        assert np.all(err <= rtol * b), key
    assert abs(float(got["pme_tpm"].sum()) - 1e6 * sum(ns)) < 1e-3
    if d["ta"] is not None:                                   # the oracle has no allele groups: a plain loop over them
        ta = d["ta"]
        plain = [sum(int(cv[s, ta[t]:ta[t + 1]].sum()) ** 2 for cv in cvs for s in range(len(cv))) for t in range(len(ta) - 1)]
        assert got["pve_c_trans"].tolist() == plain
        assert any(ta[t + 1] - ta[t] > 1 for t in range(len(ta) - 1))
    else:
        assert got["pve_c_trans"] is None
