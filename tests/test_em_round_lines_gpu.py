"""Every ROUND line of the three EM loops against the oracle stepped round by round, on the smallest shapes at which the
round closers (rsem_amd/csrc/round_close.hpp and its callers in em.hip) take another path: fewer units than closers, strided
closers, closers with an empty slice, and slices at and one past the prefetch limit of k_mstep_fast (64 workgroups) and of the
SOLO closers (128).  totNum is compared for equality, which only holds where no element sits on a threshold: each case asserts,
from the oracle alone, that no change lies within 1e-6 relative of 0.001 and no previous theta within 1e-6 relative of 1e-7."""
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

ROUNDS = 8


def _workload(n_ids, n_reads, seed):
    """Reads of 1..3 alignments to neighbouring transcripts among the first 1000 (every unit's ids fit its window)."""
    rng = np.random.default_rng(seed)
    M = n_ids - 1
    lens = rng.integers(1, min(3, M) + 1, n_reads)
    rp = np.zeros(n_reads + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    rows = np.repeat(np.arange(n_reads), lens)
    within = np.arange(int(rp[-1])) - rp[:-1].astype(np.int64)[rows]
    width = min(1000, M) - 2 if M > 4 else 1
    start = 1 + rng.integers(0, max(width, 1), n_reads)
    sid = np.minimum(start[rows] + within, M).astype(np.int32)
    if M <= 4:
        sid = (1 + (start[rows] + within) % M).astype(np.int32)
    cp = np.power(10.0, rng.uniform(-8, -3, len(sid)))
    ncp = np.power(10.0, rng.uniform(-12, -9, n_reads))
    N0 = 100.0
    theta0 = np.full(M + 1, (1.0 - 0.05) / M)
    theta0[0] = 0.05
    return dict(M=M, rp=rp, sid=sid, cp=cp, ncp=ncp, N0=N0, theta0=theta0)


def _oracle_rounds(wl, rounds):
    """[(counts, theta, sum, bChange, totNum)] per round, with the margin of every element from the two thresholds asserted."""
    th, out = wl["theta0"], []
    for r in range(rounds):
        c = orc.em_estep(wl["M"], wl["rp"], wl["sid"], wl["cp"], wl["ncp"], th)
        c, new, s, b, t = orc.em_mstep(wl["M"], wl["N0"], c, th)
        big = th >= 1e-7
        change = np.abs(new[big] - th[big]) / th[big]
        assert not np.any(np.abs(change - 0.001) <= 1e-6 * 0.001), "round %d: a change on the 0.001 threshold (choose another seed)" % (r + 1)
        assert not np.any(np.abs(th - 1e-7) <= 1e-6 * 1e-7), "round %d: a theta on the 1e-7 threshold (choose another seed)" % (r + 1)
        out.append((c, new, s, b, t))
        th = new
    return out


# name: (transcripts + noise, reads, seed, what the number of units must be for the shape to do its job)
# Reads of 1..3 alignments fill 64 to a slice in three shapes, and a unit is at most 4 x 8 slices: some 2000 reads per unit.
# The SOLO closers are min(units, 128) workgroups, every (units / 128)-th one: 128 of them, and with them a slice of
# (M + 1) / 128, take 128 units -- 300 000 reads, not the 50 000 that do for k_mstep_fast's 64 workgroups --, a stride of 2 takes 256.
CASES = {
    "few_units": (600, 2000, 1, lambda u: u < 128),
    "strided": (3000, 600000, 2, lambda u: u >= 256 and u % 128 != 0),
    "empty_slices": (5, 300000, 3, lambda u: u >= 128),
    "fast_2048": (131072, 50000, 4, None),   # (k_mstep_fast's grid does not depend on the units: SLICE below)
    "fast_2049": (131073, 50000, 5, None),
    "solo_2048": (262144, 300000, 6, lambda u: u >= 128),
    "solo_2049": (262145, 300000, 7, lambda u: u >= 128),
}
# the slice a closer must get for the case to sit on the prefetch limit (8 pairs x 256 threads) or one past it: k_mstep_fast runs
# min(64, ceil((M + 1) / 512)) workgroups (mstep_fast_grid of em.hip), the SOLO loop min(units, 128) closers
SLICE = {"fast_2048": 2048, "fast_2049": 2049, "solo_2048": 2048, "solo_2049": 2049}


@pytest.mark.parametrize("name", list(CASES))
def test_every_round_line_of_every_loop(name, monkeypatch):
    from rsem_amd import capi
    n_ids, n_reads, seed, prop = CASES[name]
    wl = _workload(n_ids, n_reads, seed)
    M, N0 = wl["M"], wl["N0"]
    want = _oracle_rounds(wl, ROUNDS)
    ctx = capi.EmContext(M, wl["rp"], wl["sid"], wl["cp"], wl["ncp"])
    units = ctx.info("units")
    print(name, "units", units, "far", ctx.info("far_units"), "M + 1", M + 1)
    if prop is not None:
        assert prop(units) and ctx.info("units_compact") == units, units
    if name in SLICE:
        closers = min(64, -(-(M + 1) // 512)) if name.startswith("fast") else min(units, 128)
        assert -(-(M + 1) // closers) == SLICE[name], (closers, M + 1)
    thetas = {}
    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        lines = []
        ctx.set_progress(lambda r, s, b, t: lines.append((r, s, b, t)))
        out = ctx.run(wl["theta0"], N0, min_round=ROUNDS, max_round=ROUNDS)
        ctx.set_progress(None)
        assert out["rounds"] == ROUNDS
        assert [l[0] for l in lines] == list(range(1, ROUNDS + 1)), (loop, [l[0] for l in lines])
        for (r, s, b, t), (_, _, os_, ob, ot) in zip(lines, want):
            print(name, "loop", loop, "round", r, "SUM %.17g / %.17g bChange %.17g / %.17g totNum %d / %d" % (s, os_, b, ob, t, ot))
            assert t == ot, (loop, r)
            assert abs(s - os_) <= 1e-9 * os_ and abs(s - (N0 + n_reads)) < 1e-6, (loop, r)
            assert abs(b - ob) <= 1e-6 * abs(ob), (loop, r)
        assert np.allclose(out["theta"], want[-1][1], rtol=1e-6, atol=1e-12), loop
        assert out["totNum"] == want[-1][4]
        thetas[loop] = out["theta"]
    for loop in ("1", "2"):
        assert np.allclose(thetas[loop], thetas["0"], rtol=1e-10, atol=1e-18), loop
    # the step: round 1 against the oracle ...
    counts, theta_new, s, b, t = ctx.step(wl["theta0"], N0)
    oc, oth, os_, ob, ot = want[0]
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-12)
    assert np.allclose(theta_new, oth, rtol=1e-9, atol=1e-15)
    assert abs(s - os_) < 1e-9 * os_
    assert t == ot and abs(b - ob) <= 1e-9 * max(ob, 1e-12) + 1e-12
    # ... and against a one-round run of the PLAIN loop, which it is (not bit for bit: the atomics' order differs between launches)
    monkeypatch.setenv("RSEM_EM_FUSED", "0")
    lines = []
    ctx.set_progress(lambda r, s, b, t: lines.append((r, s, b, t)))
    one = ctx.run(wl["theta0"], N0, min_round=1, max_round=1)
    ctx.set_progress(None)
    assert one["rounds"] == 1 and [l[0] for l in lines] == [1]
    print(name, "step SUM %.17g bChange %.17g totNum %d / one PLAIN round %.17g %.17g %d" % ((s, b, t) + lines[0][1:]))
    assert t == one["totNum"] == lines[0][3]
    assert abs(s - lines[0][1]) <= 1e-9 * abs(lines[0][1])
    assert abs(b - one["bChange"]) <= 1e-9 * abs(one["bChange"]) and one["bChange"] == lines[0][2]
    assert np.allclose(theta_new, one["theta"], rtol=1e-10, atol=0)
    assert np.allclose(counts, one["counts"], rtol=1e-10, atol=0)
    ctx.close()
