"""Gibbs on the reads of tests/em_id_cap.py as items: ids at and above the anchor cap of the sliced layout (sell_layout.hpp:
kKeyMinSidCap = 2^23 - 1), M = cap + 12000.  The exact mode's count vectors are the oracle's sequential chain's bit for bit, for every
team size tests/test_gibbs_gpu.py sweeps; the parallel sampler, which walks the sliced layout, puts every read on one of its own ids.
Burn-in 2 and 2 samples a chain: the oracle draws 8.4 M gammas a round."""
import numpy as np
import pytest

import em_id_cap as cap
from oracle import pyoracle as orc
from tools.synth_data import to_gibbs_items

pytestmark = pytest.mark.gpu

BURNIN, SAMPLES, GAP, N0 = 2, 2, 1, 100
_cache = {}


def capi():
    from rsem_amd import capi as c
    return c


def items():
    """the context's arguments and the oracle's two chains: computed once, shared, never changed"""
    if not _cache:
        d = cap.reads()
        M, N1 = d["M"], len(d["row_ptr"]) - 1
        irp, isid, icp = to_gibbs_items(d)
        args = (M, irp, isid, icp, np.zeros(M + 1, np.int32), None, 1.0, float((M + 1) + N0 + N1), N0, np.full(M + 1, 500.0), np.ones(M + 1),
                np.array([1, M + 1], np.int32))
        seeds = capi().gibbs_chain_seeds(4242, 2)
        _cache["args"], _cache["seeds"], _cache["N1"], _cache["d"] = args, seeds, N1, d
        _cache["want"] = [orc.gibbs_chain(*args, seeds[k], BURNIN, SAMPLES, GAP)[0] for k in range(2)]
    return _cache["args"], _cache["seeds"], _cache["want"]


def assert_units_at_the_cap(ctx):
    """the path: the units of the parallel layout whose reads all have their anchor above the cap have their window AT the cap, and
    those without an id that far down run the far path with a window of one id"""
    _, units = ctx.debug_units()
    win = ctx.debug_unit_windows()
    assert len(win) == len(units) > 0
    at_cap = win[:, 0] == cap.CAP
    print("units", len(units), "with base == cap", int(at_cap.sum()), "of them one id wide", int((at_cap & (win[:, 1] == 1)).sum()))
    assert at_cap.any() and win[:, 0].max() == cap.CAP and (win[:, 0] < cap.CAP - 2 * cap.WINDOW).any()
    assert (at_cap & (win[:, 1] == 1) & (units[:, 3] == 1)).any()
    assert np.all((win[:, 1] >= 1) & (win[:, 1] <= cap.WINDOW))


def test_exact_chains_for_every_team_size(monkeypatch):
    args, seeds, want = items()
    assert [w.sum(1).tolist() for w in want] == [[N0 + _cache["N1"]] * SAMPLES] * 2 and int(args[2].max()) > cap.CAP + 2 * cap.WINDOW
    ctx = capi().GibbsContext(*args)
    assert_units_at_the_cap(ctx)
    for W in (1, 2, 7, 16, 17, 0):
        if W:
            monkeypatch.setenv("RSEM_GX_TEAM", str(W))
        else:
            monkeypatch.delenv("RSEM_GX_TEAM")  # the product's choice
        cvs, _, _, p = ctx.run_chains(capi().GIBBS_EXACT, seeds, BURNIN, [SAMPLES] * 2, GAP)
        for k in range(2):
            assert np.array_equal(cvs[k], want[k]), (W, k)
    ctx.close()


def test_parallel_sampler_keeps_every_read_on_its_own_ids():
    args, seeds, _ = items()
    d = _cache["d"]
    ctx = capi().GibbsContext(*args)
    assert_units_at_the_cap(ctx)
    cv1, _, _ = ctx.run(capi().GIBBS_PARALLEL, 7, 2, 2, 1)
    cv2, _, _ = ctx.run(capi().GIBBS_PARALLEL, 7, 2, 2, 1)
    ctx.close()
    assert np.array_equal(cv1, cv2) and cv1.min() >= 0 and np.all(cv1.sum(1) == N0 + _cache["N1"])
    touched = np.unique(np.concatenate([[0], d["sid"]]))
    assert np.count_nonzero(cv1) == np.count_nonzero(cv1[:, touched])  # no count on an id that no read has
    # a read counts on one of its own ids: no more counts above the cap than reads with an id there, and the same below
    rp = d["row_ptr"].astype(np.int64)
    above = np.array([(d["sid"][rp[i]:rp[i + 1]] > cap.CAP).any() for i in range(len(rp) - 1)])
    below = np.array([(d["sid"][rp[i]:rp[i + 1]] <= cap.CAP).any() for i in range(len(rp) - 1)])
    assert 0 < above.sum() < len(above) and 0 < below.sum() < len(below)
    assert np.all(cv1[:, cap.CAP + 1:].sum(1) <= above.sum()) and np.all(cv1[:, 1:cap.CAP + 1].sum(1) <= below.sum())
    assert cv1[:, cap.CAP + 1:].any() and cv1[:, 1:cap.CAP + 1].any()
