"""The inputs of tests/far_cases.py keep the rules they were built by (no GPU): every read splits under the rule of row_key_of as
restated there, its anchor is the first id of its group, its far ids lie more than a window from the group, and the layout rules
restated in predicted_wave_totals() put the far entries of the waves of k_far_rowsum on the seams tests/test_em_far_seams_gpu.py
asserts on the device."""
import numpy as np
import pytest

import far_cases as fc


def _check_reads(d, far_per_pop=None, whole=()):
    """whole: the populations that split_policy 1 keeps whole"""
    E = fc.expected_layout(d)
    keeps = np.array([p in whole for p in d["pop"]])
    assert np.array_equal(E["anchor"], d["anchor"]) and np.array_equal(E["split"], ~keeps) and fc.expected_layout(d, 2)["split"].all()
    rp, sid = d["row_ptr"].astype(np.int64), d["sid"].astype(np.int64)
    n_far = np.bincount(E["read_of"], E["outside"], len(rp) - 1).astype(np.int64)
    assert np.all((2 * (np.diff(rp) - n_far) <= np.diff(rp)) == ~keeps) and np.all(n_far >= 1)
    dist = np.abs(sid - d["anchor"][E["read_of"]])
    assert np.all(dist[E["outside"]] > fc.WINDOW) and np.all(dist[~E["outside"]] <= 2000)
    if far_per_pop:
        for i, p in enumerate(d["pop"]):
            assert n_far[i] in far_per_pop[p], (p, n_far[i])
    return E, n_far


def test_anchor_rule():
    assert fc.anchor_of([7]) == 7
    assert fc.anchor_of([5000, 1, 5001, 2]) == 5000                      # rank 2 of 4 is 5000
    assert fc.anchor_of([9000, 5000, 1, 5001, 2, 5900, 9001]) == 5000    # median 5001; 5000 lies within 1024 below it
    assert fc.anchor_of([9000, 3000, 1, 5001, 2, 5900, 9001]) == 5001    # ... 3000 does not
    ids = np.concatenate([np.arange(1, 41), [7000], np.arange(9000, 9040)])
    assert len(ids) > fc.MEDIAN_EXACT_MAX and fc.anchor_of(ids) == 7000  # above 64 alignments: the id at file position L / 2
    assert fc.anchor_of(ids[::-1]) == 7000 and fc.anchor_of(np.roll(ids, 1)) == 1    # (position L / 2 now holds 40)


def test_seams_input():
    d = fc.seams()
    far = {"f1": (1,), "f4": (4, 5), "f8": (7, 8, 9), "f252": (252,), "f16": (16,), "f56": (56,)}
    E, n_far = _check_reads(d, far, whole=("f56",))
    assert len(d["sid"]) < 100000 and 20 * E["split"].sum() >= len(n_far)
    assert sorted(n_far[np.array(d["pop"]) == "f8"].tolist())[::511] == [7, 9] and (n_far == 5).sum() == 1
    nw = fc.predicted_wave_totals(d)
    print("predicted far entries per wave:", nw.tolist())
    have = set(nw.tolist())
    assert {256, 257, 511, 512, 513} <= have and min(have) <= 64 and max(have) > 4096
    assert (nw == 256).sum() >= 4 and (nw == 512).sum() >= 6
    groups = [nw[g:g + 4] for g in range(0, len(nw) - 3, 4)]
    assert any((g <= fc.ROWSUM_CAP).any() and (g > fc.ROWSUM_CAP).any() for g in groups)
    nw2 = fc.predicted_wave_totals(d, policy=2)   # f56 joins: 16 more row slots, one per slice, behind all the others
    assert np.array_equal(nw2[:-1], nw) and nw2[-1] == 16 * 56
    # the far-id pools: one id per side, runs of 63 / 64 / 65, ids that no other entry has
    _, cnt = np.unique(d["sid"][E["outside"]], return_counts=True)
    assert {63, 64, 65} <= set(cnt.tolist()) and cnt.max() == 1024 and (cnt == 1).sum() > 3000


@pytest.mark.parametrize("pool", fc.COLSUM_POOLS)
def test_colsum_family_input(pool):
    assert [max(1, -(-n // fc.COLSUM_WG)) for n in fc.COLSUM_SIZES] == fc.COLSUM_GRIDS
    assert {g & 7 for g in fc.COLSUM_GRIDS} >= {0, 1, 2} and min(fc.COLSUM_GRIDS) < 8 < max(fc.COLSUM_GRIDS)
    for n in (1, 65, 1025, 8 * 1024 + 1):
        d = fc.colsum_family(n, pool)
        _, n_far = _check_reads(d)
        assert n_far.sum() == n == len(d["row_ptr"]) - 1


def test_refine_and_clamp_inputs():
    d = fc.refine()
    E, n_far = _check_reads(d)
    assert np.all(n_far == 8) and np.all(np.diff(d["row_ptr"].astype(np.int64)) == 13)
    assert (d["sid"].astype(np.int64) - d["anchor"][E["read_of"]] == 2000).sum() == len(d["anchor"])
    assert d["anchor"].max() - d["anchor"].min() + 2000 >= fc.WINDOW   # a unit's window cannot hold every stray id
    c = fc.clamp_cases()
    E, n_far = _check_reads(c)
    assert np.all(n_far == 2)
    f = c["theta0"][c["sid"]] * c["conprb"]
    under = (f < 1e-300).reshape(4, 4)
    far = E["outside"].reshape(4, 4)
    assert [int((under[i] & far[i]).sum()) for i in range(4)] == [1, 0, 2, 2]
    assert [int((under[i] & ~far[i]).sum()) for i in range(4)] == [0, 2, 0, 2]
    assert f[12:14].sum() >= 1e-300   # read D: unclamped, its far terms alone would be a normaliser
    assert c["ncp"][3] == 0 and np.all(c["ncp"][:3] * c["theta0"][0] >= 1e-300)
