"""A plain CPU restatement of the two samplers that draw their random numbers on the device: the PARALLEL Gibbs chain
(k_sample_theta, k_sample_z_lane, k_sample_z_long of rsem_amd/csrc/gibbs.hip) and the credibility-interval draws (k_ci_draw,
k_ci_scales of ci.hip).  Both are pure functions of (seed, counter), so this file predicts every integer / float they write.

Written from the algorithm: reads one after the other, transcripts as numpy vectors; no lanes, slices, LDS or shuffles.
Running sums of a read's weights are formed in extended precision (np.longdouble), and every comparison whose outcome
decides a draw also reports its MARGIN -- the relative distance between its two sides.  A replay is meaningful where no
margin is small: a different summation order or a libm that differs in the last bits moves a boundary by ~1e-16, never by
the 1e-9 the tests ask for.
"""
import numpy as np

U64 = np.uint64
_M32 = U64(0xFFFFFFFF)
_TWO53 = 1.0 / 9007199254740992.0
_TWO32 = 1.0 / 4294967296.0
GAMMA_TAG = 0x47414D4D   # rng.hpp gamma_draw: counter word 2
Z_TAG = 0x5A5A5A5A       # the z pass's uniforms
KEY_GIBBS = 0x52534547   # 'RSEG'
KEY_CI = 0x52534349      # 'RSCI'
CI_TAG = 0x43495331      # 'CIS1'
LONG = 255               # lg marker of the reads that stay in the CSR (RSEM_GIBBS_ORDER_LONG)


def _u64(x):
    return np.atleast_1d(np.asarray(x)).astype(U64) & _M32


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 (Salmon et al., SC'11); scalars or arrays that broadcast -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    a, b = U64(k0 & 0xFFFFFFFF), U64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ a, p1 & _M32, (p0 >> U64(32)) ^ c3 ^ b, p0 & _M32
        a, b = (a + U64(0x9E3779B9)) & _M32, (b + U64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def philox2x32_10(key, c0, c1):
    c0, c1 = np.broadcast_arrays(_u64(c0), _u64(c1))
    k = U64(key & 0xFFFFFFFF)
    for _ in range(10):
        p = U64(0xD256D193) * c0
        c0, c1 = (p >> U64(32)) ^ k ^ c1, p & _M32
        k = (k + U64(0x9E3779B9)) & _M32
    return c0, c1


def u53(hi, lo):
    """53-bit uniform in [0, 1) from two 32-bit words."""
    return (((hi >> U64(5)) << U64(26)) | (lo >> U64(6))).astype(np.float64) * _TWO53


def _rel(a, b):
    """relative distance between the two sides of a comparison"""
    den = np.maximum(np.abs(a), np.abs(b))
    return np.where(den > 0, np.abs(a - b) / np.where(den > 0, den, 1.0), 0.0)


def _gamma(block, a):
    """Marsaglia & Tsang (2000) for shapes a > 0 (a < 1: Gamma(a + 1) * U^(1/a)).  block(kind, sel) -> the uniforms of one
    step ("boost", "attempt", "accept") for the elements `sel`; the caller's closure keeps the counters.  Returns (draws, margins)."""
    a = np.array(a, np.float64)
    n = a.size
    boost = np.ones(n)
    lt = np.flatnonzero(a < 1.0)
    if lt.size:
        u = block("boost", lt)
        u[u <= 0.0] = _TWO53
        boost[lt] = np.exp(np.log(u) / a[lt])
        a[lt] += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out, margin = np.zeros(n), np.full(n, np.inf)
    act = np.arange(n)
    while act.size:
        u1, u2, u = block("attempt", act)    # (u: None where the acceptance uniform is a block of its own)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)  # Box-Muller
        v = 1.0 + c[act] * x
        margin[act] = np.minimum(margin[act], _rel(np.ones(act.size), -c[act] * x))   # v <= 0 ?
        pos = v > 0.0
        again = act[~pos]
        act, x, v = act[pos], x[pos], v[pos]
        u = block("accept", act) if u is None else u[pos]
        u[u <= 0.0] = _TWO53
        v = v * v * v
        x2 = x * x
        sq = 1.0 - 0.0331 * x2 * x2
        margin[act] = np.minimum(margin[act], _rel(u, sq))                          # the squeeze
        ok = u < sq
        lhs, rhs = np.log(u), 0.5 * x2 + d[act] * (1.0 - v + np.log(v))
        margin[act] = np.minimum(margin[act], np.where(ok, np.inf, _rel(lhs, rhs)))  # the log test (where it is reached)
        ok = ok | (lhs < rhs)
        out[act[ok]] = d[act[ok]] * v[ok] * boost[act[ok]]
        act = np.concatenate([again, act[~ok]])
    return out, margin


def gamma_draw(k0, k1, idx, sweep, a):
    """rng.hpp gamma_draw: counters (idx, sweep, 'GAMM', ctr) with ONE running ctr per draw -- the boost uniform (a < 1), then
    per attempt a block for the normal (two 53-bit uniforms) and, unless v <= 0, a block for the acceptance uniform."""
    idx = np.asarray(idx, np.int64)
    used = np.zeros(idx.size, np.int64)

    def block(kind, sel):
        r = philox4x32_10(k0, k1, idx[sel], sweep, GAMMA_TAG, used[sel])
        used[sel] += 1
        if kind == "attempt":
            u1 = u53(r[0], r[1])
            u1[u1 <= 0.0] = _TWO53
            return u1, u53(r[2], r[3]), None
        return u53(r[0], r[1])
    return _gamma(block, a)


def gamma_draw_bulk(k0, k1, c0, c1, c2, a):
    """rng.hpp gamma_draw_bulk: one block (c0, c1, c2, attempt) per attempt -- 32-bit uniforms for the normal, words 2 and 3
    for the 53-bit acceptance uniform; the boost uniform of a < 1 comes from counter 0x80000000."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, np.int64), np.asarray(c1, np.int64))
    c0, c1 = c0.ravel(), c1.ravel()
    tries = np.zeros(c0.size, np.int64)

    def block(kind, sel):
        if kind == "boost":
            r = philox4x32_10(k0, k1, c0[sel], c1[sel], c2, 0x80000000)
            return u53(r[0], r[1])
        r = philox4x32_10(k0, k1, c0[sel], c1[sel], c2, tries[sel])
        tries[sel] += 1
        return (r[0].astype(np.float64) + 0.5) * _TWO32, r[1].astype(np.float64) * _TWO32, u53(r[2], r[3])
    return _gamma(block, a)


# ---- the z pass --------------------------------------------------------------------------------------------------------------

def pick(weights, u):
    """One read: weights in their order (noise first), u in [0, 1).  The first item whose running sum exceeds u * total;
    -1 where the total is zero.  Returns (index, margin = |u * total - nearest boundary| / total)."""
    cum = np.cumsum(np.asarray(weights, np.longdouble))
    total = cum[-1]
    if not total > 0:
        return -1, np.inf
    target = np.longdouble(u) * total
    if target >= total:
        target = total * np.longdouble(1.0 - 1.1102230246251565e-16)
    k = int(np.searchsorted(cum, target, side="right"))
    if k >= len(cum):                                 # (rounding: the last item of positive weight)
        k = int(np.flatnonzero(np.asarray(weights) > 0)[-1])
    m = cum[k] - target
    if k > 0:
        m = min(m, target - cum[k - 1])
    return k, float(abs(m) / total)


def lane_major(n, lg):
    """Weight order of a read of n items that takes G = 2^lg lanes of the sliced layout: item c sits in lane c mod G, plane
    c div G, and the kernel sums lane by lane (sell_layout.hpp sell_fill_row, gibbs_block.hpp)."""
    G = 1 << lg
    c = np.arange(n)
    return c[np.lexsort((c // G, c % G))]


class Reads:
    """The reads in the layout's sorted order, each with its noise weight and its other items in weight order."""

    def __init__(self, row_ptr, sid, conprb, order, lg):
        rp = np.asarray(row_ptr, np.int64)
        self.n = len(order)
        self.lg = np.asarray(lg)
        self.ncp = np.zeros(self.n)
        self.sid, self.cp = [], []
        for p, i in enumerate(np.asarray(order, np.int64)):
            s, v = np.asarray(sid[rp[i]:rp[i + 1]]), np.asarray(conprb[rp[i]:rp[i + 1]], np.float64)
            noise = s == 0
            self.ncp[p] = v[noise].sum()
            s, v = s[~noise], v[~noise]
            if self.lg[p] != LONG:
                o = lane_major(len(s), int(self.lg[p]))
                s, v = s[o], v[o]
            self.sid.append(s.astype(np.int64))
            self.cp.append(v)

    def uniforms(self, seed, sweep):
        k0, k1 = int(seed), KEY_GIBBS
        pos = np.arange(self.n)
        key = k0 ^ (((k1 << 13) | (k1 >> 19)) & 0xFFFFFFFF) ^ Z_TAG
        u = u53(*philox2x32_10(key, pos, sweep))
        r = philox4x32_10(k0, k1, pos, sweep, Z_TAG, 0)
        return np.where(self.lg == LONG, u53(r[0], r[1]), u)

    def z_pass(self, g, seed, sweep, counts):
        """counts[pick] += 1 for every read; returns the smallest margin of the pass"""
        u = self.uniforms(seed, sweep)
        worst = np.inf
        for p in range(self.n):
            w = np.concatenate([[g[0] * self.ncp[p]], g[self.sid[p]] * self.cp[p]])
            k, m = pick(w, u[p])
            if k >= 0:
                counts[0 if k == 0 else self.sid[p][k - 1]] += 1
                worst = min(worst, m)
        return worst


def parallel_chain(reads, M, init_counts, alpha, pseudoC, N0, seed, burnin, nsamples, gap, thin=1):
    """One chain of the PARALLEL sampler as rsem_gibbs_run_chains runs it: sweep 0 is a z pass with every g = 1; every round
    is `thin` pairs (g_i = Gamma(c_i + alpha_i), 0 where c_i < 0; counts re-armed; z pass).  Returns (kept count vectors
    [nsamples, M + 1], smallest pick margin, smallest gamma margin).

    Omitted transcripts (init_counts = -1): g is 0 only while the count is negative.  Sweep 0 draws with every g = 1, the
    omitted ones included, so an omitted transcript that reads point to with a non-zero weight starts at -1 + its picks and
    is live from then on.  That is the device's host loop (and the reference program's own start: Gibbs.cpp draws the first
    z from conprb alone), restated here as it is; rsem-run-gibbs never meets it, since a transcript is omitted for having
    no effective length and then every alignment to it has weight 0."""
    init = np.asarray(init_counts, np.int64).copy()
    init[0] += int(N0)
    a_vec = np.full(M + 1, float(pseudoC)) if alpha is None else np.asarray(alpha, np.float64)
    counts = init.copy()
    sweep = 0
    m_pick = reads.z_pass(np.ones(M + 1), seed, sweep, counts)
    sweep += 1
    m_gamma = np.inf
    kept = []
    last_round = burnin + 1 + (nsamples - 1) * gap
    for rnd in range(1, last_round + 1):
        for _ in range(max(1, thin)):
            live = np.flatnonzero(counts >= 0)
            g = np.zeros(M + 1)
            g[live], mg = gamma_draw(int(seed), KEY_GIBBS, live, sweep, counts[live] + a_vec[live])
            m_gamma = min(m_gamma, mg.min())
            counts = init.copy()
            m_pick = min(m_pick, reads.z_pass(g, seed, sweep, counts))
            sweep += 1
        if rnd > burnin and (rnd - burnin - 1) % gap == 0:
            kept.append(counts.copy())
    return np.array(kept, np.int32), m_pick, m_gamma


# ---- credibility-interval draws ---------------------------------------------------------------------------------------------

def ci_sample(cvecs, nSpC, eel, mw, pseudoC, seed, eps=1e-300):
    """rsem_ci_sample: (tpm float32 [M, nS], lbar float32 [nS], gamma margins [M, nS] -- inf where nothing is drawn)."""
    cvecs = np.asarray(cvecs, np.int64)
    nCV, M = cvecs.shape[0], cvecs.shape[1] - 1
    nS = nCV * nSpC
    eel, mw = np.asarray(eel, np.float64), np.asarray(mw, np.float64)
    w = np.zeros(M + 1)
    ok = (eel >= eps) & (mw >= eps)
    ok[0] = False
    w[ok] = 1.0 / (mw[ok] * eel[ok])
    s = np.arange(nS)
    c = cvecs[s // nSpC, 1:].T                               # [M, nS]
    j = np.broadcast_to(np.arange(1, M + 1)[:, None], c.shape)
    draw = (w[1:, None] > 0.0) & (c >= 0)
    y = np.zeros(c.shape, np.float32)
    margin = np.full(c.shape, np.inf)
    k0, k1 = int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) & 0xFFFFFFFF) ^ KEY_CI
    gam, mg = gamma_draw_bulk(k0, k1, np.broadcast_to(s[None, :], c.shape)[draw], j[draw], CI_TAG, c[draw] + float(pseudoC))
    y[draw] = (gam * np.broadcast_to(w[1:, None], c.shape)[draw]).astype(np.float32)
    margin[draw] = mg
    yd = y.astype(np.float64)
    T = yd.sum(0)
    L = (yd * eel[1:, None]).sum(0)
    tpm = (yd * (1e6 / T)[None, :]).astype(np.float32)
    return tpm, (L / T).astype(np.float32), margin
