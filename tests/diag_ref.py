"""The definition of the Gibbs convergence diagnostics restated in numpy: plain float64 over the unshifted
values, no tricks.  diag_ref(cvs) -> dict(mean, sd, rhat, ess, lag, tie, n_used, sequences)."""
import numpy as np


def split_sequences(cvs):
    """list of (nsamples[k], M+1) integer arrays -> (m, n, M+1) float64: the last n' rows of every chain, cut in two."""
    nmin = min(int(a.shape[0]) for a in cvs)
    n = nmin // 2
    seqs = []
    for a in cvs:
        a = np.asarray(a)
        last = a[a.shape[0] - 2 * n:].astype(np.float64)
        seqs += [last[:n], last[n:]]
    return np.stack(seqs), n


def diag_ref(cvs):
    """tie: the smallest distance of any decision of Geyer's rule from a tie: |P_k| where it looks whether to stop, |P_k - P'_(k-1)|
    where it takes the minimum (inf if there was no decision)."""
    x, n = split_sequences(cvs)
    if n < 2:
        raise ValueError("n < 2")
    m, _, M1 = x.shape
    xbar = x.mean(axis=1)                      # (m, M1)
    s2 = x.var(axis=1, ddof=1)
    W = s2.mean(axis=0)
    B = n * xbar.var(axis=0, ddof=1)
    varp = (n - 1) / n * W + B / n
    mean = xbar.mean(axis=0)
    sd = np.sqrt(varp)
    rhat = np.full(M1, np.nan)
    ess = np.full(M1, np.nan)
    lag = np.zeros(M1, np.int32)
    pos = W > 0
    rhat[pos] = np.sqrt(varp[pos] / W[pos])
    rhat[(~pos) & (B > 0)] = np.inf
    d = x - xbar[:, None, :]
    S = m * n
    tie = np.inf
    idx = np.nonzero(pos)[0]
    # rho[t] for the defined columns
    rho = np.ones((n, idx.size))
    for t in range(1, n):
        gamma = (d[:, :n - t, idx] * d[:, t:, idx]).sum(axis=1) / (n - 1)   # (m, cols)
        rho[t] = 1.0 - (W[idx] - gamma.mean(axis=0)) / varp[idx]
    for c, i in enumerate(idx):
        total, prev, last = 0.0, None, 0
        k = 0
        while 2 * k + 1 <= n - 1:
            P = rho[2 * k, c] + rho[2 * k + 1, c]
            tie = min(tie, abs(P))
            if P <= 0:
                break
            if prev is not None:
                tie = min(tie, abs(P - prev))
                P = min(P, prev)
            total += P
            prev = P
            last = 2 * k + 1
            k += 1
        tau = max(-1.0 + 2.0 * total, 1.0 / np.log10(S))
        ess[i] = S / tau
        lag[i] = last
    return dict(mean=mean, sd=sd, rhat=rhat, ess=ess, lag=lag, tie=tie, n_used=2 * n, sequences=m)


def summary_ref(r, L0):
    """The summary's fields from the arrays (ids 1 .. M, ties to the smallest id)."""
    rhat, ess, lag = r["rhat"][1:], r["ess"][1:], r["lag"][1:]
    fin = np.isfinite(rhat)
    ok = ~np.isnan(ess)
    out = dict(n_used=r["n_used"], sequences=r["sequences"], n_defined=int(fin.sum()),
               n_rhat_gt_1p01=int((rhat > 1.01).sum()), n_rhat_gt_1p1=int((rhat > 1.1).sum()), n_long=int((lag > L0).sum()))
    if fin.any():
        v = np.where(fin, rhat, -np.inf)
        out["max_rhat_id"] = int(np.argmax(v)) + 1
        out["max_rhat"] = float(v.max())
    else:
        out["max_rhat_id"], out["max_rhat"] = 0, float("nan")
    if ok.any():
        v = np.where(ok, ess, np.inf)
        out["min_ess_id"] = int(np.argmin(v)) + 1
        out["min_ess"] = float(v.min())
    else:
        out["min_ess_id"], out["min_ess"] = 0, float("nan")
    return out


def ar1_counts(rng, phi, nsamples, ncols, centre=1000.0, sd=100.0):
    """(nsamples, ncols) int32 of a stationary AR(1) series per column, rounded to integers."""
    e = rng.standard_normal((nsamples, ncols))
    z = np.empty_like(e)
    z[0] = e[0]
    a = np.sqrt(1.0 - phi * phi)
    for s in range(1, nsamples):
        z[s] = phi * z[s - 1] + a * e[s]
    return np.rint(centre + sd * z).astype(np.int32)


def synthetic(seed=11, ncols=513, nsamples=(21, 20, 23), centre=1000.0, sd=100.0):
    """The smallest input at which each path can go wrong: 513 columns (full workgroup tiles and one column more; no multiple of 4, so the row pitch matters),
    chains of unequal length with an odd one, columns mixed from phi in {0, 0.5, 0.9, 0.98}, one column constant everywhere (NaN),
    one constant per chain (inf), one mostly zeros."""
    rng = np.random.default_rng(seed)
    phis = np.array([0.0, 0.5, 0.9, 0.98])[np.arange(ncols) % 4]
    cvs = []
    for k, ns in enumerate(nsamples):
        a = np.empty((ns, ncols), np.int32)
        for p in np.unique(phis):
            sel = np.nonzero(phis == p)[0]
            a[:, sel] = ar1_counts(rng, p, ns, sel.size, centre, sd)
        a[:, 5] = int(centre)                 # constant everywhere
        a[:, 6] = int(centre) + 3 * k         # constant per chain, different between chains
        a[:, 7] = 0
        a[rng.integers(0, ns, 2), 7] = rng.integers(1, 4, 2)   # mostly zeros
        cvs.append(a)
    return cvs


def compare(got, ref, what=""):
    """All five arrays, every transcript: lag exactly, NaN and inf in the same places, finite values to 1e-9 relative (slack for
    another order of a handful of double operations on exactly representable sums, not for accumulated error)."""
    assert np.array_equal(got["lag"], ref["lag"]), (what, np.nonzero(got["lag"] != ref["lag"])[0][:10])
    for key in ("mean", "sd", "rhat", "ess"):
        g, r = np.asarray(got[key], np.float64), ref[key]
        assert g.shape == r.shape, (what, key)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, key)
        assert np.array_equal(np.isposinf(g), np.isposinf(r)), (what, key)
        assert not np.isneginf(g).any(), (what, key)
        fin = np.isfinite(r)
        err = np.abs(g[fin] - r[fin]) / np.maximum(np.abs(r[fin]), 1e-300)
        assert err.size == 0 or err.max() <= 1e-9, (what, key, float(err.max()), int(np.nonzero(fin)[0][np.argmax(err)]))
