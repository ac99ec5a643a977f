"""The split rows' two side passes (rsem_amd/csrc/em.hip: k_far_rowsum before the lane kernel, k_far_colsum after it) and the
builders of their far-entry arrays (sell_layout.hpp: sell_build_far, sell_refine_split_windows) on their seams; the inputs and why
they land there: tests/far_cases.py.

Every test asserts its path first, from EmContext.debug_far() (rsem_em_debug_far): the invariants of the far-entry layout, then the
far entries of each wave of k_far_rowsum (64 row slots; up to kRowsumCap = 512 they are staged in LDS, 256 per trip of the batched
loop; above that every lane walks global memory) or the grid of k_far_colsum (1024 entries per workgroup, renumbered over 8 XCDs).
An input that a layout change moves elsewhere fails there instead of quietly testing something else.  The numbers are the oracle's
(oracle/pyoracle.py) within the bars of tests/test_em_units_gpu.py.  RSEM_HIP_ROWSUM_BATCHED and RSEM_HIP_COLSUM_XCD are read once
per process: their other halves run in one child process (tests/far_static_knobs_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import far_cases as fc
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

MAX_ROUND = 30
HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}
_STOP = []    # why nothing more may be started on the GPU


def capi():
    from rsem_amd import capi as c
    return c


def data(name, *args):
    key = (name,) + args
    if key not in _cache:
        _cache[key] = getattr(fc, name)(*args)
    return _cache[key]


def oracle(name, *args):
    """(step counts incl. N0, weights, noise weights) of the oracle: computed once per input, shared, never changed"""
    key = ("oracle", name) + args
    if key not in _cache:
        d = data(name, *args)
        oc, ow, own = orc.em_estep(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"], d["theta0"], want_weights=True)
        oc = oc.copy()
        oc[0] += d["N0"]
        _cache[key] = (oc, ow, own)
    return _cache[key]


def context(d):
    return capi().EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])


def check_layout(d, ctx, tag, block_lg=16, refined=False, policy=1):
    """the invariants of the far-entry layout -> (debug_far(), expected_layout(), far entries inside their read's own window)"""
    F = ctx.debug_far()
    E = fc.expected_layout(d, policy)
    rp, sid = d["row_ptr"].astype(np.int64), d["sid"].astype(np.int64)
    nf, nxs, base = F["n_far"], F["n_x_slots"], F["x_slot_base"]
    info = {k: ctx.info(k) for k in ("split_rows", "far_entries", "slots", "unit_tables_agree")}
    assert np.array_equal(E["anchor"], d["anchor"]), tag  # (the input's own statement of its anchors)
    assert info["split_rows"] == int(E["split"].sum()) and 20 * info["split_rows"] >= len(rp) - 1, (tag, info)
    assert info["far_entries"] == nf == len(F["far_sid"]) and info["unit_tables_agree"] == 1, (tag, info, nf)
    assert base + nxs <= info["slots"] and len(F["far_ptr"]) == nxs + 1, (tag, info, base, nxs)
    fp, src = F["far_ptr"].astype(np.int64), F["far_src"].astype(np.int64)
    assert fp[0] == 0 and fp[-1] == nf and np.all(np.diff(fp) >= 0), tag
    assert np.count_nonzero(np.diff(fp)) == info["split_rows"], tag  # (every split read here has a far entry; a slot holds one read)
    assert src.min() >= 0 and src.max() < len(sid) and len(np.unique(src)) == nf, tag
    assert np.array_equal(F["far_sid"], sid[src]), tag
    xs_of = np.searchsorted(fp, np.arange(nf), "right") - 1            # row slot - x_slot_base of far entry e
    same_slot = xs_of[1:] == xs_of[:-1]
    assert np.all(np.diff(src)[same_slot] > 0), tag                      # file order within a slot ...
    read_of_far = E["read_of"][src]
    assert np.all(read_of_far[1:][same_slot] == read_of_far[:-1][same_slot]), tag   # ... inside one read ...
    assert len(np.unique(read_of_far)) == len(np.unique(xs_of)), tag              # ... and a read in one slot
    is_far = np.zeros(len(sid), bool)
    is_far[src] = True
    split_entry = E["split"][E["read_of"]]
    assert not is_far[~split_entry].any(), tag
    assert is_far[split_entry & E["outside"]].all(), tag
    # ids inside the read's [anchor, anchor + 2048): the kept ones all lie below the far ones (the refined reach)
    kept_max = np.full(len(rp) - 1, -1, np.int64)
    far_min = np.full(len(rp) - 1, 1 << 40, np.int64)
    ins = split_entry & ~E["outside"]
    np.maximum.at(kept_max, E["read_of"][ins & ~is_far], sid[ins & ~is_far])
    np.minimum.at(far_min, E["read_of"][ins & is_far], sid[ins & is_far])
    assert np.all(kept_max < far_min), tag
    n_inside = int((ins & is_far).sum())
    assert nf == int((split_entry & E["outside"]).sum()) + n_inside and (n_inside > 0) == refined, (tag, nf, n_inside)
    # column order: a permutation of the far entries, sorted by (block of row slots, id), stable
    csrc = F["csc_src"].astype(np.int64)
    if nf:
        far_index = np.full(len(sid), -1, np.int64)
        far_index[src] = np.arange(nf)
        e = far_index[csrc]
        assert np.array_equal(np.sort(e), np.arange(nf)), tag
        assert np.array_equal(F["csc_sid"], F["far_sid"][e]) and np.array_equal(F["csc_slot"].astype(np.int64), base + xs_of[e]), tag
        keys = ((xs_of[e] >> block_lg) << 32) | F["csc_sid"].astype(np.int64)
        assert np.all(np.diff(keys) >= 0) and np.all(np.diff(e)[np.diff(keys) == 0] > 0), tag
        F["keys"] = keys
    print(tag, "split_rows=%d far_entries=%d n_x_slots=%d x_slot_base=%d far_inside_window=%d" % (info["split_rows"], nf, nxs, base, n_inside))
    return F, E, n_inside


def wave_totals(F):
    fp, nxs = F["far_ptr"].astype(np.int64), F["n_x_slots"]
    w = np.arange((nxs + 63) // 64)
    return fp[np.minimum(64 * (w + 1), nxs)] - fp[64 * w]


def assert_seam_path(F, tag):
    """the waves of k_far_rowsum this input must reach"""
    nw = wave_totals(F)
    print(tag, "far entries per wave of 64 row slots:", nw.tolist())
    have = set(nw.tolist())
    assert any(0 < v <= 64 for v in have), tag
    for v in (256, 257, 511, 512, 513):   # two full trips of the batched loop, a third, the last staged sizes, the first unstaged one
        assert v in have, (tag, v)
    assert max(have) > 4096, tag
    groups = [nw[g:g + 4] for g in range(0, len(nw) - 3, 4)]   # a workgroup = 4 consecutive waves
    assert any((g <= fc.ROWSUM_CAP).any() and (g > fc.ROWSUM_CAP).any() and (g > 0).all() for g in groups), tag
    runs = np.diff(np.flatnonzero(np.diff(F["csc_sid"], prepend=-1, append=-1)))   # runs of one id in column order
    print(tag, "longest runs of one id in column order:", sorted(set(runs.tolist()))[-8:])
    for v in (63, 64, 65):
        assert v in runs, (tag, v)
    assert runs.max() > 256, tag   # one id over more than a wave's step of 4 x 64 entries


def check_step(ctx, d, oc, tag):
    counts, theta_new, s, _, _ = ctx.step(d["theta0"], d["N0"])
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-9), tag
    assert np.allclose(theta_new, oc / oc.sum(), rtol=1e-9, atol=1e-12), tag
    assert np.count_nonzero(counts[1:]) == np.count_nonzero(oc[1:]), tag   # no count on an id that no read has
    return counts


def test_debug_far_without_split_rows():
    """whole reads only: every size is 0"""
    rp = np.arange(0, 33, 4).astype(np.uint64)
    sid = (1 + np.arange(32) % 7).astype(np.int32)
    ctx = capi().EmContext(10, rp, sid, np.full(32, 0.5), np.full(8, 1e-6))
    F = ctx.debug_far()
    assert ctx.info("split_rows") == 0
    assert (F["x_slot_base"], F["n_x_slots"], F["n_far"]) == (0, 0, 0) and F["far_ptr"].tolist() == [0]
    assert all(len(F[k]) == 0 for k in ("far_sid", "far_src", "csc_sid", "csc_slot", "csc_src"))
    ctx.close()


@pytest.mark.parametrize("policy,overlap", [(1, 0), (1, 1), (2, 1), (2, 0)])
def test_seams_step_and_weights(policy, overlap):
    """split_policy 2 (every read with an id outside splits) brings in the reads of population f56, a row per slice: no read of up to
    256 alignments with more than 128 inside its window is mostly outside it (tests/far_cases.py)"""
    d = data("seams")
    oc, ow, own = oracle("seams")
    ctx = context(d)
    ctx.set_option("split_policy", policy)
    ctx.set_option("split_overlap", overlap)
    tag = "seams split_policy=%d split_overlap=%d" % (policy, overlap)
    F, E, _ = check_layout(d, ctx, tag, policy=policy)
    assert_seam_path(F, tag)
    n_whole = int((~E["split"]).sum())
    assert n_whole == (16 if policy == 1 else 0) and (ctx.info("far_units") > 0) == (policy == 1), (tag, n_whole)
    assert np.array_equal(wave_totals(F), fc.predicted_wave_totals(d, policy)), tag   # far_ptr by row slot, empty slots included
    check_step(ctx, d, oc, tag)
    c2, w, wn = ctx.expected_weights(d["theta0"], d["N0"])
    assert np.allclose(c2, oc, rtol=1e-9, atol=1e-9), tag
    assert np.allclose(w, ow, rtol=1e-12, atol=0) and np.allclose(wn, own, rtol=1e-12, atol=0), tag
    G = ctx.debug_far()   # the accessor and the entry points leave the layout as it was
    assert all(np.array_equal(F[k], G[k]) for k in G), tag
    check_step(ctx, d, oc, tag + " again")
    ctx.close()


def test_seams_run():
    d = data("seams")
    ctx = context(d)
    F, _, _ = check_layout(d, ctx, "seams run")
    assert_seam_path(F, "seams run")
    oth, orounds, _, ot = orc.em_run(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"], d["N0"], d["theta0"], max_round=MAX_ROUND)
    out = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
    print("seams run: rounds", out["rounds"], "oracle", orounds)
    assert out["rounds"] == orounds and out["totNum"] == ot, (out["rounds"], orounds, out["totNum"], ot)
    assert np.allclose(out["theta"], oth, rtol=1e-6, atol=1e-12)
    ctx.close()


def test_seams_column_blocks_of_256_slots(monkeypatch):
    """RSEM_HIP_CSC_BLOCK_LG=8 (read per build): the column order is cut into blocks of 256 row slots -- more than one here --, the
    counts are the same"""
    d = data("seams")
    oc, _, _ = oracle("seams")
    ref_ctx = context(d)
    ref = check_step(ref_ctx, d, oc, "seams block_lg=16")
    ref_ctx.close()
    monkeypatch.setenv("RSEM_HIP_CSC_BLOCK_LG", "8")
    ctx = context(d)
    F, _, _ = check_layout(d, ctx, "seams block_lg=8", block_lg=8)
    blocks = np.unique(F["keys"] >> 32)
    print("seams block_lg=8: slot blocks in the keys:", blocks.tolist())
    assert len(blocks) > 1 and len(blocks) == (F["n_x_slots"] + 255) // 256
    counts = check_step(ctx, d, oc, "seams block_lg=8")
    assert np.allclose(counts, ref, rtol=1e-9, atol=1e-9)
    ctx.close()


@pytest.mark.parametrize("n_far,grid", list(zip(fc.COLSUM_SIZES, fc.COLSUM_GRIDS)))
def test_colsum_grid_sizes(n_far, grid):
    for pool in fc.COLSUM_POOLS:
        d = data("colsum_family", n_far, pool)
        oc, _, _ = oracle("colsum_family", n_far, pool)
        ctx = context(d)
        tag = "colsum n_far=%d %s" % (n_far, pool)
        F, _, _ = check_layout(d, ctx, tag)
        g = max(1, -(-F["n_far"] // fc.COLSUM_WG))
        print(tag, "grid=%d q=%d r=%d" % (g, g >> 3, g & 7))
        assert F["n_far"] == n_far and g == grid, (tag, F["n_far"], g)
        runs = np.diff(np.flatnonzero(np.diff(F["csc_sid"], prepend=-1, append=-1)))
        if pool == "shared":
            assert runs.tolist() == [n_far], tag
        elif pool == "distinct":
            assert runs.max() == 1, tag
        elif n_far >= sum(fc.RUNS):
            assert runs[:3].tolist() == list(fc.RUNS), tag
        check_step(ctx, d, oc, tag)
        ctx.close()


def test_clamp_on_split_rows():
    d = data("clamp_cases")
    oc, ow, own = oracle("clamp_cases")
    ctx = context(d)
    F, E, _ = check_layout(d, ctx, "clamp")
    assert E["split"].all() and F["n_far"] == 8
    counts, theta_new, s, _, _ = ctx.step(d["theta0"], d["N0"])
    # the oracle's reads with a normaliser: A, B, C (their weights sum to 1), not D
    per_read = np.add.reduceat(ow, d["row_ptr"][:-1].astype(np.int64)) + own
    n_norm = int((per_read > 0.5).sum())
    assert n_norm == 3 and np.all(ow[[0, 6, 7, 8, 9]] == 0) and np.all(ow[12:] == 0) and own[3] == 0
    got_norm = counts.sum() / theta_new.sum() - d["N0"]   # theta_new = counts / (N0 + reads with a normaliser)
    print("clamp: sum of counts %.17g (oracle %.17g), reads with a normaliser %.17g (oracle %d)" % (s, oc.sum(), got_norm, n_norm))
    assert abs(s - oc.sum()) < 1e-12 and abs(got_norm - n_norm) < 1e-9
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-9)
    assert counts[3] == 0 and np.count_nonzero(counts[1:]) == np.count_nonzero(oc[1:])
    ctx.close()


def test_refined_windows_move_ids_to_the_far_entries(monkeypatch):
    d = data("refine")
    oc, _, _ = oracle("refine")
    ctx = context(d)
    F, E, n_inside = check_layout(d, ctx, "refine", refined=True)
    assert n_inside >= 1 and ctx.info("far_units") == 0   # (what the refinement is for: no unit of split rows is left with an id outside)
    check_step(ctx, d, oc, "refine")
    ctx.close()
    monkeypatch.setenv("RSEM_HIP_X_REFINE", "0")   # (read per build)
    ctx = context(d)
    G, _, none_inside = check_layout(d, ctx, "refine RSEM_HIP_X_REFINE=0")
    assert none_inside == 0 and G["n_far"] == F["n_far"] - n_inside and ctx.info("far_units") >= 1
    check_step(ctx, d, oc, "refine RSEM_HIP_X_REFINE=0")
    ctx.close()


def test_static_knobs_in_a_child_process():
    """RSEM_HIP_ROWSUM_BATCHED=0 and RSEM_HIP_COLSUM_XCD=0: the other instantiation of either pass, in one fresh process"""
    assert not _STOP, "not started: " + _STOP[0]
    cmd = [sys.executable, os.path.join(HERE, "far_static_knobs_child.py")]
    env = dict(os.environ, RSEM_HIP_ROWSUM_BATCHED="0", RSEM_HIP_COLSUM_XCD="0")
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env, cwd=os.path.dirname(HERE))
    except subprocess.TimeoutExpired:
        _STOP.append("%s ran into its time limit" % " ".join(cmd))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STOP.append("%s ended with status %d" % (" ".join(cmd), r.returncode))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    print("child:", verdict)
    assert verdict["knobs"] == {"RSEM_HIP_ROWSUM_BATCHED": "0", "RSEM_HIP_COLSUM_XCD": "0"}
    assert sorted(verdict["cases"]) == sorted(["seams"] + ["colsum %d" % n for n in (1, 8 * 1024 + 1, 16 * 1024 + 1)])
    assert all(c["ok"] for c in verdict["cases"].values()), verdict
    assert verdict["cases"]["seams"]["waves_over_cap"] > 0 and verdict["cases"]["colsum 8193"]["grid"] == 9
