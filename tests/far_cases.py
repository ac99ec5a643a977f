"""Split reads on the seams of the two passes that handle their far entries (rsem_amd/csrc/em.hip: k_far_rowsum, k_far_colsum) and of
the builders of those entries (sell_layout.hpp: sell_build_far), for tests/test_em_far_seams_gpu.py and tests/test_far_cases_cpu.py.

A split read keeps the ids inside [anchor, anchor + 2048) as a row of the sliced layout; the others are its far entries.  Every read
here is built around a GROUP of L_in consecutive ids that holds its anchor, with f far ids more than 2048 away from the group, about
half of them below it and half above.  The anchor rule of row_key_of, restated in anchor_of(): the anchor is the smallest id within
1024 below the read's median id; up to 64 alignments the median is exact (the id of rank L/2), above that it is the id at file
position L/2.  So (f + 1) // 2 far ids lie below the group -- rank L/2 then falls into the group for every f and L_in >= 1 --, and
a read of more than 64 alignments carries a group id at file position L/2.  With 2 * L_in <= L a read splits under split_policy 1,
so the layout's "one read in twenty" condition holds by itself.  One population cannot have that: a row of its own per slice needs
L_in > 128, and no read of up to 256 alignments is then mostly outside its window -- the reads of f56 split under split_policy 2
only, which splits every read with an id outside, and stay whole (sorted apart, their unit on the far path) under policy 1.

What the kernels see (sell_layout.hpp): reads of one in-window length share a shape; its rows are sorted by anchor and dealt to
blocks of T = 8 slices, lane-major: of a block's n rows, slice t holds rows t, t + Tb, t + 2 Tb, ... (Tb = ceil(n / rows per slice)).
A wave of k_far_rowsum takes 64 consecutive row slots, which for L_in <= 4 is one slice.  seams() therefore gives every population
anchors of its own, ascending, and whole blocks (512 reads for L_in <= 4) of one far count f: each wave of such a block holds 64 f
far entries, and the one read of f + 1 or f - 1 in it moves exactly one wave by one.  Anchors step by 2, so a block spans 1026 ids
and every unit's window holds all ids of its rows: nothing is refined away, the wave totals are exact.  refine() is the input where
the refinement does happen.

Values are drawn as tests/test_em_units_gpu.py draws them, but for theta0, which is random here: under a uniform theta a far entry
that gathered another id's theta would go unnoticed."""
import numpy as np

WINDOW = 2048          # kLayoutWindow
REACH = 1024           # kAnchorReach
CAP = 2 ** 23 - 1      # kKeyMinSidCap
MEDIAN_EXACT_MAX = 64  # kMedianExactMax
ROWSUM_CAP = 512       # kRowsumCap (em.hip): far entries of a wave staged in LDS
COLSUM_WG = 1024       # far entries per workgroup of k_far_colsum: 4 waves x 4 x 64

LOW0, GROUP0, HIGH0, TOP = 1, 24000, 40000, 60000   # far ids below the groups | the groups | far ids above them
COLSUM_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 7 * 1024 + 1, 8 * 1024, 8 * 1024 + 1, 15 * 1024 + 5, 16 * 1024 + 1]
COLSUM_GRIDS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 8, 8, 9, 16, 17]
COLSUM_POOLS = ("shared", "distinct", "runs")


def anchor_of(ids):
    """the anchor row_key_of gives a read with these ids, in file order"""
    ids = np.asarray(ids, np.int64)
    L = len(ids)
    if L == 1:
        return int(ids[0])
    med = int(np.sort(ids)[L // 2]) if L <= MEDIAN_EXACT_MAX else int(ids[L // 2])
    return int(ids[(ids >= max(med - REACH, 0)) & (ids <= med)].min())


def expected_layout(d, policy=1):
    """the rule of row_key_of, read by read -> dict(anchor[N1], split[N1] (bool), outside[nnz] (bool: the id lies outside its read's
    [anchor, anchor + 2048)), read_of[nnz])"""
    rp = d["row_ptr"].astype(np.int64)
    sid = d["sid"].astype(np.int64)
    N1 = len(rp) - 1
    anchor = np.array([anchor_of(sid[rp[i]:rp[i + 1]]) for i in range(N1)], np.int64)
    lens = np.diff(rp)
    read_of = np.repeat(np.arange(N1), lens)
    outside = (sid < anchor[read_of]) | (sid >= anchor[read_of] + WINDOW)
    n_out = np.bincount(read_of, outside, N1).astype(np.int64)
    inside = lens - n_out
    split = (lens >= 2) & (lens <= 256) & (n_out > 0) & (anchor <= CAP)
    if policy == 1:
        split &= 2 * inside <= lens
    return dict(anchor=anchor, split=split, outside=outside, read_of=read_of)


def predicted_wave_totals(d, policy=1, T=8):
    """the far entries of every wave of k_far_rowsum (64 consecutive row slots of the split shapes), from the layout rules of
    sell_layout.hpp / sell_shape.hpp restated: shapes by (lanes per read, planes), rows by anchor (which must differ within a shape:
    the tuple hash that breaks ties is not restated), row_to_slot.  For inputs that no window refinement touches."""
    E = expected_layout(d, policy)
    N1 = len(E["anchor"])
    n_far = np.bincount(E["read_of"], E["outside"], N1).astype(np.int64)
    L_in = np.diff(d["row_ptr"].astype(np.int64)) - n_far
    lg = np.where(L_in <= 4, 0, np.ceil(np.log2(np.maximum(L_in, 5) / 4.0)).astype(np.int64))
    K = (L_in + (1 << lg) - 1) >> lg
    per_slot = []
    for shape in sorted(set(zip(lg.tolist(), K.tolist()))):
        rows = np.flatnonzero((lg == shape[0]) & (K == shape[1]) & E["split"])
        if not len(rows):
            continue
        rows = rows[np.argsort(E["anchor"][rows], kind="stable")]
        assert len(np.unique(E["anchor"][rows])) == len(rows)
        R, n = 64 >> shape[0], len(rows)
        slots = np.zeros(-(-n // R) * R, np.int64)
        for q, i in enumerate(rows):
            b, qb = divmod(q, R * T)
            Tb = -(-min(n - b * R * T, R * T) // R)
            slots[(b * T + qb % Tb) * R + qb // Tb] = n_far[i]
        per_slot.append(slots)
    per_slot = np.concatenate(per_slot)
    return np.add.reduceat(per_slot, np.arange(0, len(per_slot), 64))


class _Pools:
    """far ids: `single` one id per side; `distinct` a fresh id per entry; `random` k different ids out of a thousand per side"""

    def __init__(self, rng):
        self.rng = rng
        self.next = {0: LOW0 + 2000, 1: HIGH0 + 2000}
        self.base = {0: LOW0, 1: HIGH0}

    def single(self, side, k):
        return np.full(k, self.base[side], np.int64)

    def run_id(self, j):  # the ids of the runs of 63, 64 and 65 entries (low side)
        return LOW0 + 1 + j

    def random(self, side, k):
        return self.base[side] + 10 + self.rng.choice(1000, k, replace=False)

    def distinct(self, side, k):
        out = np.arange(self.next[side], self.next[side] + k)
        self.next[side] += k
        return out


def _read(rng, group, lo, hi):
    """one read's ids in file order: shuffled; above 64 alignments a group id sits at file position L / 2"""
    ids = np.concatenate([lo, group, hi]).astype(np.int64)
    ids = ids[rng.permutation(len(ids))]
    L = len(ids)
    if L > MEDIAN_EXACT_MAX:
        j = int(np.flatnonzero(ids == group[len(group) // 2])[0])
        ids[[j, L // 2]] = ids[[L // 2, j]]
    return ids


def _finish(rows, rng, shuffle=True):
    """rows: [(population, anchor, ids)] -> the input dict; the reads shuffled, so that the layout and not the input brings a
    population's reads together"""
    if shuffle:
        rows = [rows[i] for i in rng.permutation(len(rows))]
    lens = np.array([len(r[2]) for r in rows], np.int64)
    sid = np.concatenate([r[2] for r in rows])
    assert sid.min() >= 1 and sid.max() < TOP
    M = TOP
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    cp = rng.uniform(0.05, 0.2, len(sid))
    cp[rp[:-1].astype(np.int64) + rng.integers(0, 1 << 30, len(lens)) % lens] = rng.uniform(0.5, 1.0, len(lens))
    ncp = rng.uniform(0.01, 1.0, len(lens)) * 1e-5
    theta0 = rng.uniform(0.5, 1.5, M + 1)
    theta0[0] = 0.0
    theta0 *= 0.95 / theta0.sum()
    theta0[0] = 0.05
    return dict(M=M, N0=100, row_ptr=rp, sid=sid.astype(np.int32), conprb=cp, ncp=ncp, theta0=theta0,
                anchor=np.array([r[1] for r in rows], np.int64), pop=[r[0] for r in rows])


# (population, reads, far ids per read, L_in, pool below, pool above, {read in anchor order: its own far count})
POPULATIONS = [
    ("f1", 100, 1, 1, "single", None, {}),                        # L_in = 1: a shape of its own, two waves of 50 far entries
    ("f4", 512, 4, 4, "distinct", "distinct", {100: 5}),          # a block of 8 waves of 256, one of them 257
    ("f8", 512, 8, 4, "distinct", "random", {100: 9, 357: 7}),    # 8 waves of 512, one of them 513, one 511 (100 % 8 != 357 % 8)
    ("f252", 70, 252, 4, "random", "random", {}),                 # L = 256: the median by file position; waves of 35 x 252
    ("f16", 128, 16, 16, "random", "single", {}),                 # 16 rows per slice; the one id above, 8 times in every read
    ("f56", 16, 56, 200, "distinct", "random", {}),               # one row per slice, L = 256; split by split_policy 2 only
]
RUNS = (63, 64, 65)   # in population f4: the first far id below of that many consecutive reads is one id


def seams(seed=31):
    """the main input: every population of POPULATIONS, the far-id pools mixed among them"""
    rng = np.random.default_rng(seed)
    pools = _Pools(rng)
    rows, cursor = [], GROUP0
    for name, n, f, L_in, plo, phi, own in POPULATIONS:
        for i in range(n):
            fi = own.get(i, f)
            n_lo = (fi + 1) // 2
            a = cursor + 2 * i
            lo = getattr(pools, plo)(0, n_lo)
            hi = getattr(pools, phi)(1, fi - n_lo) if fi > n_lo else np.zeros(0, np.int64)
            if name == "f4":
                edges = np.cumsum((0,) + RUNS)
                j = int(np.searchsorted(edges, i, "right")) - 1
                if j < len(RUNS):
                    lo[0] = pools.run_id(j)
            rows.append((name, a, _read(rng, a + np.arange(L_in), lo, hi)))
        cursor += 2 * n + L_in + 64
    assert cursor + WINDOW < HIGH0 and pools.next[0] + WINDOW < GROUP0 and pools.next[1] < TOP
    return _finish(rows, rng)


def colsum_family(n_far, pool, seed=37):
    """split reads only, one far id (below) and one id inside each: n_far far entries in all.  pool: `shared` one far id for all,
    `distinct` one each, `runs` ids in runs of 63, 64, 65, 63, ... entries.  Three reads in a row share their in-window id."""
    rng = np.random.default_rng(seed + n_far)
    i = np.arange(n_far)
    if pool == "shared":
        far = np.full(n_far, LOW0 + 5, np.int64)
    elif pool == "distinct":
        far = LOW0 + i
    else:
        edges = np.cumsum(np.tile(RUNS, n_far // sum(RUNS) + 1))
        far = LOW0 + np.searchsorted(edges, i, "right")
    rows = []
    for k in range(n_far):
        g = GROUP0 + k // 3
        rows.append(("colsum", g, np.array([far[k], g] if k % 2 else [g, far[k]], np.int64)))
    return _finish(rows, rng)


def refine(seed=41, n=300):
    """split reads that also carry an id 2000 above their anchor: inside the read's own [anchor, anchor + 2048), but a block of
    these reads has anchors 510 apart, so its unit's window (2048 ids from the smallest anchor) ends before the stray id of every
    read whose anchor lies 48 or more above the unit's first -- sell_refine_split_windows hands those ids to the far entries."""
    rng = np.random.default_rng(seed)
    pools = _Pools(rng)
    rows = []
    for i in range(n):
        a = GROUP0 + 2 * i
        group = np.concatenate([a + np.arange(4), [a + 2000]])
        rows.append(("stray", a, _read(rng, group, pools.distinct(0, 4), pools.random(1, 4))))
    return _finish(rows, rng)


def clamp_cases():
    """four split reads ([two far ids below, g, g + 1]: the anchor is g) around the 1e-300 clamp of EM.cpp:212-223; id 3 has
    theta = 1e-310, a conprb of 1e-300 times any theta is below the clamp:
      A  one far term under the clamp (its id's theta), everything else counts;
      B  both in-window terms clamp, the far terms do not;
      C  both far terms clamp, the in-window terms do not;
      D  every term clamps and the noise term is 0: a read without a normaliser; its two far terms are 6e-301 each, so unclamped they
         would add up to a normaliser above 1e-300."""
    M = 9000
    g = [5000, 5010, 5020, 5030]
    sid = np.array([3, 2, g[0], g[0] + 1, 1, 2, g[1], g[1] + 1, 1, 4, g[2], g[2] + 1, 2, 4, g[3], g[3] + 1], np.int32)
    t = 1e-300
    cp = np.array([0.3, 0.2, 0.5, 0.1, 0.3, 0.2, t, t, t, t, 0.4, 0.6, 6e-297, 3e-297, t, t])
    ncp = np.array([1e-6, 2e-6, 3e-6, 0.0])
    rp = np.arange(0, 17, 4).astype(np.uint64)
    theta = np.full(M + 1, 0.9 / M)
    theta[0], theta[3] = 0.1, 1e-310
    theta[[1, 2, 4]] = [3e-4, 1e-4, 2e-4]
    return dict(M=M, N0=2, row_ptr=rp, sid=sid, conprb=cp, ncp=ncp, theta0=theta, anchor=np.array(g, np.int64), pop=list("ABCD"))
