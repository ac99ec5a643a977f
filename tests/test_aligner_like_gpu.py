"""The E step and the EM loops on reads as an aligner reports them: a transcript hit twice or more by one read, ids in any order
(tests/aligner_like.py).  The reference keeps every such alignment as a hit of its own and adds each hit's share to its
transcript's count; every other input of the suite gives a read distinct, ascending ids.

Inputs: the hand-built groupings G0, G2, G3, G4, G5, G7 of test_em_units_gpu.py passed through aligner_like() -- each read's
smallest id and its ids 2000 or more above it are kept, so that every input stays in the grouping it was built for, which is
asserted with that file's own assertions --, one input of every read length 1..256 (test_estep_emu_cpu._data), and two
hand-made far-entry cases on G4 and G7.  Every input is checked against the oracle on the same arrays: step, expected weights,
whole runs of the three loops, Q32 planes, the values read back after release_csr, a change of split policy.  describe()'s
counts are asserted (and printed) first: a test that no longer has the repeats it names fails there."""
import numpy as np
import pytest

import aligner_like as al
from oracle import pyoracle as orc
from tests.test_em_units_gpu import INPUTS, MAX_ROUND, _assert_grouping, _build, _check_runs, _info
from tests.test_estep_emu_cpu import _data
from tools.q32_ref import quantize_q32

pytestmark = pytest.mark.gpu

GROUPS = ["G0", "G2", "G3", "G4", "G5", "G7"]
FAR_CASES = ["G4-far-twice-in-a-row", "G7-far-twice-in-a-row", "G4-far-in-many-rows", "G7-far-in-many-rows"]
ALL = GROUPS + ["L1-256"] + FAR_CASES
_DATA, _ORACLE = {}, {}


def capi():
    from rsem_amd import capi as c
    return c


def _keep(rp, sid):
    """Entries aligner_like() must not overwrite: each read's smallest id and its ids 2000 or more above it (the 2000- and
    3000-offset entries of the stray, apart and outside reads).  A read of which these are half or more is kept whole: it is a
    split row BECAUSE half of it lies outside its window, and what its one free entry becomes would decide whether it still is
    (the far-entry cases below write those reads by hand)."""
    keep = []
    rp = rp.astype(np.int64)
    for i in range(len(rp) - 1):
        ids = sid[rp[i]:rp[i + 1]].astype(np.int64)
        k = np.flatnonzero((ids == ids.min()) | (ids >= ids.min() + 2000))
        keep.append(rp[i] + (np.arange(len(ids)) if 2 * len(k) >= len(ids) else k))
    return np.concatenate(keep)


def _input(name):
    """-> (input, grouping it must land in or None, describe() counts)"""
    if name in _DATA:
        return _DATA[name]
    g = name[:2] if name[:2] in INPUTS else None
    if name == "L1-256":
        M, rp, sid, cp, ncp, theta = _data(5, M=500, n=1200, aligner_like=True)
        theta0 = np.full(M + 1, 0.95 / M)
        theta0[0] = 0.05
        d = dict(M=M, N0=100, row_ptr=rp, sid=sid, conprb=cp, ncp=ncp, theta0=theta0, theta_step=theta)
    else:
        d = _build(INPUTS[g], seed=sorted(INPUTS).index(g) + 1)   # (a fresh copy: that file's own inputs stay as they are)
        rp, sid = d["row_ptr"], d["sid"]
        if name in GROUPS:
            d["sid"] = al.aligner_like(rp, sid, 40 + GROUPS.index(g), keep=_keep(rp, sid))
        else:
            # the outside reads (4 alignments: a, a + 1, a + 3000, a + 3001; the window starts at a + 3000, so a and a + 1 are the
            # far entries of a split row)
            fr = rp[:-1].astype(np.int64)[np.diff(rp.astype(np.int64)) == 4]
            sid = sid.copy()
            if "twice" in name:
                sid[fr + 1] = sid[fr]          # the same far id twice in one split row
            else:
                sid[fr] = sid[fr[0]]           # one far id in every split row (k_far_colsum: a column of many entries)
            d["sid"] = sid
        d["theta_step"] = d["theta0"]
    assert len(d["row_ptr"]) - 1 < 6000
    _DATA[name] = (d, g, al.describe(d["row_ptr"], d["sid"]))
    return _DATA[name]


def _on_path(name):
    d, g, counts = _input(name)
    if name in FAR_CASES:
        n4 = int(np.sum(np.diff(d["row_ptr"].astype(np.int64)) == 4))
        if "twice" in name:
            al.assert_on_path(counts, repeat=0.05, far_repeat=0.05)
            assert counts["far_repeat"] == n4
        else:
            al.assert_on_path(counts)
            ids, n = np.unique(d["sid"], return_counts=True)
            print("rows with far id %d: %d" % (ids[np.argmax(n)], n.max()))
            assert n.max() == n4 >= 200
    elif name in ("G0", "L1-256"):
        al.assert_on_path(counts, repeat=0.05, all_same=0.05, not_ascending=0.05, same_plane=0.05, same_lane=0.05)
    elif name == "G7":   # (kept whole: see _keep; only the order of its reads' ids moves)
        al.assert_on_path(counts, not_ascending=0.05)
    else:   # (G3: every read has an id outside its window, and in one in twenty it is a repeated one)
        al.assert_on_path(counts, repeat=0.05, not_ascending=0.05, same_plane=0.05, same_lane=0.05, **(dict(far_repeat=0.05) if g == "G3" else {}))
    return d, g


def _oracle(name, bits=64):
    """E-step counts (N0 added), theta and totNum of that step, weights, and the whole run; Q32: on the values the planes hold."""
    key = (name, bits)
    if key not in _ORACLE:
        d = _input(name)[0]
        M, rp, sid, ncp = d["M"], d["row_ptr"], d["sid"], d["ncp"]
        cp = d["conprb"] if bits == 64 else quantize_q32(rp, d["conprb"], 8)[0]
        raw, w, wn = orc.em_estep(M, rp, sid, cp, ncp, d["theta_step"], want_weights=True)
        oc, theta_new, _, _, tot = orc.em_mstep(M, d["N0"], raw, d["theta_step"])
        oth, orounds, _, ot = orc.em_run(M, rp, sid, cp, ncp, d["N0"], d["theta0"], max_round=MAX_ROUND)
        _ORACLE[key] = dict(counts=oc, theta_new=theta_new, totNum=tot, w=w, wn=wn, run=(oc, oth, orounds, ot))
    return _ORACLE[key]


def _ctx(d, bits=64):
    ctx = capi().EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])
    if bits == 32:
        ctx.set_option("value_bits", 32)
    return ctx


def _grouped(ctx, g, tag, bits=64):
    if g is not None:
        _assert_grouping(g, _info(ctx, tag), 1, bits)


def _check_step(ctx, d, o, tag):
    counts, theta_new, s, _, tot = ctx.step(d["theta_step"], d["N0"])
    assert np.allclose(counts, o["counts"], rtol=1e-9, atol=1e-12), tag
    assert np.allclose(theta_new, o["theta_new"], rtol=1e-9, atol=1e-12), tag
    assert tot == o["totNum"], (tag, tot, o["totNum"])


@pytest.mark.parametrize("name", ALL)
def test_step_and_weights(name):
    d, g = _on_path(name)
    o = _oracle(name)
    ctx = _ctx(d)
    _grouped(ctx, g, name)
    _check_step(ctx, d, o, name)
    counts, w, wn = ctx.expected_weights(d["theta_step"], d["N0"])
    assert np.allclose(counts, o["counts"], rtol=1e-9, atol=1e-12), name
    assert np.allclose(w, o["w"], rtol=1e-12, atol=0) and np.allclose(wn, o["wn"], rtol=1e-12, atol=0), name
    # every read hands out one unit of mass, over however many entries of one transcript, or none at all
    rp = d["row_ptr"].astype(np.int64)
    mass = np.add.reduceat(w, rp[:-1]) + wn
    assert np.all((np.abs(mass - 1.0) <= 1e-12) | (mass == 0.0)), name
    assert np.count_nonzero(mass) > 0.9 * len(mass)
    ctx.close()


@pytest.mark.parametrize("name", ALL)
def test_every_loop(name, monkeypatch):
    """RSEM_EM_FUSED 0, 1, 2: the oracle's ROUND count, theta at 1e-6, the three loops within 1e-10 of each other."""
    d, g = _on_path(name)
    ctx = _ctx(d)
    _grouped(ctx, g, name)
    _check_runs(ctx, d, _oracle(name)["run"], name, monkeypatch)
    _grouped(ctx, g, name + " after the runs")
    ctx.close()


@pytest.mark.parametrize("name", ALL)
def test_q32_planes(name):
    """value_bits 32: one exponent per read, whichever of its entries share an id; against the oracle on the rounded values."""
    d, g = _on_path(name)
    ctx = _ctx(d, 32)
    _grouped(ctx, g, name + " value_bits=32", 32)
    print("reads_q32", ctx.info("reads_q32"))
    assert ctx.info("reads_q32") > 0
    _check_step(ctx, d, _oracle(name, 32), name)
    ctx.close()


@pytest.mark.parametrize("name", ALL)
def test_values_read_back_after_release_csr(name):
    """release_csr frees the caller-order ids and values; get_values() reads them back from the planes, by POSITION within the
    read: a read-back keyed by id would give a repeated id one value twice.  The ids come back too: the weights pass walks them.
    Refused (nothing changes) where the planes do not hold everything: split rows, reads of more than 256 alignments."""
    d, g = _on_path(name)
    o = _oracle(name)
    ctx = _ctx(d)
    _grouped(ctx, g, name)
    if ctx.info("split_rows") > 0 or ctx.info("reads_long") > 0:
        assert g in ("G4", "G5", "G7")
        with pytest.raises(capi().RsemHipError):
            ctx.set_option("release_csr", 1)
        assert ctx.info("csr_released") == 0
    else:
        ctx.set_option("release_csr", 1)
        assert ctx.info("csr_released") == 1
        _check_step(ctx, d, o, name + " released")
        cp, ncp = ctx.get_values()
        assert ctx.info("csr_released") == 0
        assert np.array_equal(cp.view(np.uint64), d["conprb"].view(np.uint64)), name
        assert np.array_equal(ncp.view(np.uint64), d["ncp"].view(np.uint64)), name
    _, w, wn = ctx.expected_weights(d["theta_step"], d["N0"])
    assert np.allclose(w, o["w"], rtol=1e-12, atol=0) and np.allclose(wn, o["wn"], rtol=1e-12, atol=0), name
    ctx.close()


def test_split_policy_2_and_back():
    """G2 under split_policy 2: its apart reads split (the grouping of G4), their repeated far ids become far entries; and back."""
    d, _ = _on_path("G2")
    o = _oracle("G2")
    ctx = _ctx(d)
    _grouped(ctx, "G2", "G2")
    _check_step(ctx, d, o, "G2")
    ctx.set_option("split_policy", 2)
    i = _info(ctx, "G2 input, split_policy 2")
    _assert_grouping("G4", i)
    assert i["split_rows"] == 256
    _check_step(ctx, d, o, "split_policy 2")
    ctx.set_option("split_policy", 1)
    _grouped(ctx, "G2", "split_policy 1 again")
    _check_step(ctx, d, o, "split_policy 1 again")
    ctx.close()
