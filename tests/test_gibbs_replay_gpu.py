"""The PARALLEL Gibbs sampler (k_sample_theta, k_sample_z_lane / gibbs_block.hpp, k_sample_z_long of gibbs.hip) replayed draw
for draw on the CPU: the sampler is a pure function of (seed, counter), so tests/sampler_ref.py -- reads one after the other,
running sums in extended precision -- predicts every integer of every kept count vector.  The read order that keys the
uniforms comes from rsem_gibbs_debug_order.

Condition, not tolerance: the comparison is exact, and it means something only where no pick and no accept / reject decision
of a gamma draw sits within 1e-9 (relative) of its boundary -- six orders of magnitude above what another summation order
or a libm that differs in the last bits can move one.  Expected near-ties: reads x sweeps x 2e-9 < 1e-3 here.  Every case
asserts that the reference met none; if one ever does, the input or seed is unusable and must be changed (nothing is
skipped or exempted).

Smallest margins the reference reported with the committed input and seeds, on the read order of an MI355X, layout "default"
(pick / gamma decision): pseudoC=1 2.4e-07 / 2.6e-05, pseudoC=0.1 1.8e-06 / 5.5e-05, alpha 2.7e-06 / 4.4e-05, thin=3
2.8e-07 / 1.6e-05, three chains 1.1e-07 / 1.6e-05 -- two orders of magnitude clear of 1e-9 at the least.  Layout "T7-half"
sorts the reads otherwise, so its picks are keyed otherwise and its pick margins are its own (the gamma draws are keyed by
transcript, not by read order, but follow other counts): they are not recorded here, every test prints its own and asserts
the 1e-9 for its own layout.
"""
import numpy as np
import pytest

import sampler_ref as sr
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-9
M = 5000
N0 = 37
ROUNDS = 5


def capi():
    from rsem_amd import capi as c
    return c


def _items():
    """A few thousand reads that together reach every path of the sweep (see _check_shapes for what is asserted)."""
    rng = np.random.default_rng(20251)
    lens = np.concatenate([np.arange(1, 257),                   # every row length once: every K and lg of the layout
                           rng.integers(1, 5, 1500),            # lg 0: three blocks of 512 reads at the smallest block length
                           rng.integers(5, 9, 600), rng.integers(9, 17, 300), rng.integers(17, 33, 150), rng.integers(33, 65, 40),
                           [257, 300, 700],                     # stay in the CSR: one chunk + 1, no multiple of 64, several chunks
                           np.zeros(5, np.int64)])              # only the noise item
    rng.shuffle(lens)
    n = len(lens)
    # anchors: most reads in three gene-dense regions (units inside one 2048-id window), the rest anywhere
    region = rng.integers(0, 4, n)
    start = np.where(region < 3, 200 + 1500 * region + rng.integers(0, 40, n) * 8, rng.integers(1, M - 800, n))
    rp, sid, cp = [0], [], []
    two_noise = zero_tail = far = 0
    for i in range(n):
        L = int(lens[i])
        s = list(start[i] + np.arange(L))
        scale = 10.0 ** rng.uniform(-12, -3)
        v = list(scale * 2.0 ** rng.uniform(-6, 0, L))
        if L >= 2 and rng.random() < 0.08:                      # an id far outside the read's window (the global path)
            s[rng.integers(0, L)] = int((start[i] + 2500 + rng.integers(0, 300)) % M) + 1
            far += 1
        if L >= 2 and rng.random() < 0.1:                       # zero-weight alignments at the read's end
            for k in range(1, 1 + min(L - 1, int(rng.integers(1, 4)))):
                v[-k] = 0.0
            zero_tail += 1
        nz = scale * 2.0 ** rng.uniform(-14, -6)      # (small: the noise bin must not swallow the chain)
        if L >= 2 and rng.random() < 0.05:                      # two noise items, neither in first place
            a, b = sorted(rng.choice(np.arange(1, L + 1), 2, replace=False))
            s.insert(a, 0); v.insert(a, 0.25 * nz)
            s.insert(b + 1, 0); v.insert(b + 1, 0.75 * nz)
            two_noise += 1
        else:
            s.insert(0, 0); v.insert(0, nz)
        sid += s; cp += v
        rp.append(len(sid))
    assert two_noise > 20 and zero_tail > 50 and far > 50
    sid = np.array(sid, np.int32)
    assert sid.min() == 0 and sid.max() <= M
    init = np.zeros(M + 1, np.int32)
    hit = np.bincount(sid, minlength=M + 1)
    omitted = np.concatenate([np.flatnonzero(hit[1:] == 0)[:20] + 1, np.argsort(hit[1:], kind="stable")[-3:] + 1])  # ... and the three that most reads point to
    # (What the sampler does with an omitted transcript that reads DO point to -- sweep 0 draws with every g = 1, so it starts at
    # -1 + its picks >= 0 and is a live transcript from then on -- is what the host loop says and the replay follows; the
    # programs never give such a transcript a non-zero weight.  See sampler_ref.parallel_chain.)
    init[omitted] = -1
    assert (hit[omitted] > 0).sum() == 3
    eel = rng.uniform(200.0, 3000.0, M + 1)
    eel[omitted] = 0.0
    mw = np.where(rng.random(M + 1) < 0.1, 0.9, 1.0)
    grp = np.append(np.arange(1, M + 1, 7), M + 1).astype(np.int32)
    return dict(rp=np.array(rp, np.uint64), sid=sid, cp=np.array(cp), lens=lens, init=init, eel=eel, mw=mw, grp=grp,
                N1=n, totc=float(M + 1 + N0 + n))


def _ctx(d, alpha, pseudoC):
    return capi().GibbsContext(M, d["rp"], d["sid"], d["cp"], d["init"], alpha, pseudoC, d["totc"], N0, d["eel"], d["mw"], d["grp"])


def _check_shapes(d, order, lg, n_sell):
    """From the order accessor's output: the layout really holds what the input was built to put there.  (Presence only: which
    length takes how many lanes is the layout's business.)"""
    N1 = d["N1"]
    assert np.array_equal(np.sort(order), np.arange(N1))               # a permutation of the reads
    L = d["lens"][order]
    assert n_sell == N1 - 3 and np.all(lg[n_sell:] == capi().GIBBS_ORDER_LONG) and sorted(L[n_sell:]) == [257, 300, 700]
    assert sorted(set(lg[:n_sell])) == [0, 1, 2, 3, 4, 5, 6]
    assert set(L[:n_sell]) == set(range(257))                          # every row length 0 .. 256 sits in the sliced layout


def _check_units(T, units, want_crossing):
    """From the unit accessor's output: which paths of the sweep kernel this layout really takes.  A wave of a unit walks the
    slices [first + w * per_wave, + per_wave) of its shape, cut at the unit's end; block b of a shape = slices [b T, b T + T)."""
    odd = even = crossing = 0
    for first, n, per_wave, far, lg, K in units.astype(np.int64):
        for w in range(4):
            s0, s1 = first + w * per_wave, min(first + n, first + (w + 1) * per_wave)
            if s0 >= s1:
                continue
            odd += (s1 - s0) % 2 == 1
            even += (s1 - s0) % 2 == 0
            crossing += s0 // T != (s1 - 1) // T
    seen = {(int(u[4]), int(u[5])) for u in units}
    print("T = %d, %d units (%d far): wave ranges %d odd, %d even, %d cross a block boundary" % (T, len(units), int(units[:, 3].sum()), odd, even, crossing))
    assert {g for g, k in seen} == set(range(7)) and {k for g, k in seen} == {1, 2, 3, 4}, seen   # every lane-group size, every K
    assert set(units[:, 3]) == {0, 1}                                  # both instantiations: units inside their window, and far ones
    assert odd > 0 and even > 0, (odd, even)                           # both ends of the sweep loop: the peeled single slice, the pair
    if want_crossing:
        assert crossing > 0
    return crossing


# Two layouts of the same reads.  (Their sorted orders differ: which reads sort behind the others as reaching outside their unit's
# window depends on the units, hence on T -- so each layout has its own replay.)
#   default   what the product builds for an input of this size: T = 8, and every wave's range lies inside one block;
#   T7-half   T = 7 (RSEM_GIBBS_LAYOUT_T) and units of two blocks (RSEM_HIP_TAPER=0,1: 4 slices per wave), so that the second wave
#             of such a unit starts in one block and ends in the next -- the second branch of pos_of in gibbs_block.hpp, which an
#             input of a few thousand reads never reaches by itself (a wave crosses only where T is odd, and T = 8 up to ~120 k slices).
LAYOUTS = {"default": {}, "T7-half": {"RSEM_GIBBS_LAYOUT_T": "7", "RSEM_HIP_TAPER": "0,1"}}


@pytest.fixture(scope="module")
def data():
    d = _items()
    mp = pytest.MonkeyPatch()
    try:
        for name, env in LAYOUTS.items():
            for k, v in env.items():
                mp.setenv(k, v)
            ctx = _ctx(d, None, 1.0)
            order, lg, n_sell = ctx.debug_order()
            T, units = ctx.debug_units()
            ctx.close()
            _check_shapes(d, order, lg, n_sell)
            assert T == (8 if name == "default" else 7)
            _check_units(T, units, want_crossing=name != "default")
            d[name] = dict(order=order, lg=lg, reads=sr.Reads(d["rp"], d["sid"], d["cp"], order, lg))
    finally:
        mp.undo()
    return d


def _same(cv, ref, what):
    if not np.array_equal(cv, ref):
        r, t = np.argwhere(cv != ref)[0]
        pytest.fail("%s: first difference in kept round %d at transcript %d: device %d, replay %d (%d entries differ)"
                    % (what, r + 1, t, cv[r, t], ref[r, t], int((cv != ref).sum())))


def _usable(what, m_pick, m_gamma):
    print("%s: smallest pick margin %.3g, smallest gamma decision margin %.3g" % (what, m_pick, m_gamma))
    assert m_pick >= NEAR_TIE and m_gamma >= NEAR_TIE, \
        "%s: the reference met a near-tie (pick %.3g, gamma %.3g < 1e-9): this input / seed is unusable for an exact replay, choose another" % (what, m_pick, m_gamma)


CASES = {"pseudoC=1": dict(pseudoC=1.0, seed=101),
         "pseudoC=0.1": dict(pseudoC=0.1, seed=102),           # almost every gamma draw takes the a < 1 branch
         "alpha": dict(pseudoC=1.0, alpha=True, seed=103),     # per-transcript pseudo counts on both sides of 1
         "thin=3": dict(pseudoC=1.0, thin=3, seed=104)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(CASES))
def test_one_chain_replayed_draw_for_draw(data, case, layout, monkeypatch):
    """burnin 0, gap 1: every round is observed; five rounds of one chain, every kept count vector integer for integer."""
    d, c = data, CASES[case]
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    alpha = None
    if c.get("alpha"):
        alpha = np.random.default_rng(4).choice([0.05, 0.4, 1.0, 2.5], M + 1)
    thin = c.get("thin", 1)
    ctx = _ctx(d, alpha, c["pseudoC"])
    order, lg, n_sell = ctx.debug_order()
    assert np.array_equal(order, d[layout]["order"]) and np.array_equal(lg, d[layout]["lg"])   # the layout depends on the items alone
    ctx_T = ctx.debug_units()[0]
    cv, acc, _ = ctx.run(capi().GIBBS_PARALLEL, c["seed"], 0, ROUNDS, 1, thin)
    ctx.close()
    assert ctx_T == (8 if layout == "default" else 7)
    ref, m_pick, m_gamma = sr.parallel_chain(d[layout]["reads"], M, d["init"], alpha, c["pseudoC"], N0, c["seed"], 0, ROUNDS, 1, thin)
    _usable("%s, layout %s" % (case, layout), m_pick, m_gamma)
    assert np.all(ref[:, d["init"] == 0].sum(1) + (ref[:, d["init"] < 0] + 1).sum(1) == N0 + d["N1"])  # every read once
    _same(cv, ref, "%s, layout %s" % (case, layout))
    if case != "pseudoC=1":
        return
    # the accumulators: the oracle's per-sample statistics (Gibbs.cpp:313-346) applied to the replay's count vectors
    want = [np.zeros(M + 1) for _ in range(4)] + [np.zeros(len(d["grp"]) - 1)]
    for counts in ref:
        theta = np.where(counts < 0, 0.0, (counts + c["pseudoC"]) / d["totc"])
        tpm, fpkm = orc.calc_expression(M, orc.polish_theta(M, theta, d["eel"], d["mw"]), d["eel"])
        cd = counts.astype(np.float64)
        want[0] += cd; want[1] += cd * cd; want[2] += tpm; want[3] += fpkm
        want[4] += np.add.reduceat(cd, d["grp"][:-1]) ** 2
    for name, a, b in zip(("pme_c", "pve_c", "pme_tpm", "pme_fpkm", "pve_c_genes"), acc, want):
        assert np.allclose(a, b, rtol=1e-10, atol=1e-9), name


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_chains_replayed_separately(data, layout, monkeypatch):
    """rsem_gibbs_run_chains, unequal lengths: chain k is Philox keyed by seeds[k] and nothing else."""
    d = data
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    seeds, ns = [7, 4000000007, 12345], [5, 3, 4]
    ctx = _ctx(d, None, 1.0)
    cvs, _, _, prof = ctx.run_chains(capi().GIBBS_PARALLEL, seeds, 0, ns, 1)
    ctx.close()
    assert prof.chains == 3
    for k in range(3):
        ref, m_pick, m_gamma = sr.parallel_chain(d[layout]["reads"], M, d["init"], None, 1.0, N0, seeds[k], 0, ns[k], 1)
        _usable("chain %d, layout %s" % (k, layout), m_pick, m_gamma)
        _same(cvs[k], ref, "chain %d (seed %d), layout %s" % (k, seeds[k], layout))


def _aligner_like_items(d):
    """The same reads with repeated ids and ids in any order (tests/aligner_like.py; entry 0 of every read stays)."""
    import aligner_like as al
    sid = al.aligner_like(d["rp"], d["sid"], 9, first_fixed=True)
    rp = d["rp"].astype(np.int64)
    al.assert_on_path(al.describe(rp, sid, first_fixed=True), repeat=0.05, all_same=0.05, not_ascending=0.05, same_plane=0.05, same_lane=0.05)
    long_repeats = [i for i in np.flatnonzero(np.diff(rp) > 257) if len(np.unique(sid[rp[i] + 1:rp[i + 1]])) < rp[i + 1] - rp[i] - 1]
    print("reads of more than 256 items with a repeated id:", [int(rp[i + 1] - rp[i]) for i in long_repeats])
    assert long_repeats
    return dict(d, sid=sid)


def test_aligner_like_items_replayed_draw_for_draw(data):
    """A read's items of ONE transcript are picks of their own with weights of their own (Gibbs.cpp:297-311): in the lane kernel two
    lanes of a read, or one lane in two planes, add to one count; in k_sample_z_long (the reads of 300 and 700 items have repeats)
    the chunk scans meet the id again.  One chain, every kept count vector integer for integer, as above."""
    d = _aligner_like_items(data)
    ctx = _ctx(d, None, 1.0)
    order, lg, n_sell = ctx.debug_order()
    cv, _, _ = ctx.run(capi().GIBBS_PARALLEL, 105, 0, ROUNDS, 1, 1)
    ctx.close()
    _check_shapes(d, order, lg, n_sell)                                  # every lane-group size, the three long reads in the CSR
    reads = sr.Reads(d["rp"], d["sid"], d["cp"], order, lg)
    ref, m_pick, m_gamma = sr.parallel_chain(reads, M, d["init"], None, 1.0, N0, 105, 0, ROUNDS, 1, 1)
    _usable("aligner-like items", m_pick, m_gamma)
    assert np.all(ref[:, d["init"] == 0].sum(1) + (ref[:, d["init"] < 0] + 1).sum(1) == N0 + d["N1"])  # every read once
    _same(cv, ref, "aligner-like items")


@pytest.mark.parametrize("value", ["3", "257", "0", "7x", ""])
def test_layout_knob_rejects_what_is_not_tested(data, value, monkeypatch):
    """RSEM_GIBBS_LAYOUT_T outside 4..256, or not a number, fails the layout's construction instead of meaning the default."""
    monkeypatch.setenv("RSEM_GIBBS_LAYOUT_T", value)
    ctx = _ctx(data, None, 1.0)
    try:
        with pytest.raises(capi().RsemHipError, match="RSEM_GIBBS_LAYOUT_T"):
            ctx.debug_order()
    finally:
        ctx.close()
