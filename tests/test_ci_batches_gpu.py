"""The interval stage of the credibility intervals (ci_after_sampling, RowSorter, rsem_ci_intervals of rsem_amd/csrc/ci.hip) in
BATCHES.  A batch holds at most 2^30 keys, so with the program's 50 000 samples a transcriptome of 200 k transcripts goes
through ten batches per pass -- yet 2^30 keys are more than any test can afford.  RSEM_CI_BATCH_KEYS replaces the 2^30 for one
call, so that a few hundred rows reach what only batches after the first do: the row offsets r0 > 0 (row0 of k_ci_keys_rows,
out + r0, rows + r0 * nSamples), a short last batch behind full ones, and the i0 loop over the multi-member groups.

Everything here is exact: the interval arithmetic is the reference's (orc.calc_ci, pinned on the reference's own sample matrices
by test_ci_cpu.py) applied to rows formed in float32 exactly as calcCI.cpp:336-345 forms them -- FPKM = float32(1e3 / l_bar *
tpm), a group's row = the float32 sums of its members' rows in order, single-member groups copy their member.
"""
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from rsem_amd import capi
from tests import rsem_files as rf
from tests.test_ci_cpu import CI_FIXTURES, load_pin

pytestmark = pytest.mark.gpu

KNOB = "RSEM_CI_BATCH_KEYS"


def _tie_heavy_rows(nrows, n):
    """the rows of test_ci_gpu.test_intervals_bit_exact_random_rows"""
    rng = np.random.default_rng(n)
    rows = rng.gamma(0.7, 3.0, size=(nrows, n)).astype(np.float32)
    rows[3] = 0.0                                   # all ties
    rows[4, : n // 2] = 0.0                          # half zeros
    rows[5] = np.round(rows[5])                      # many ties
    rows[6] = rows[6, 0]
    return rows


def test_intervals_in_batches(monkeypatch):
    """37 rows of 130 samples in batches of 1, of 5 (eight batches, the last one of 2) and of 37 rows."""
    rows = _tie_heavy_rows(37, 130)
    want = [orc.calc_ci(r, 0.95) for r in rows]
    monkeypatch.delenv(KNOB, raising=False)
    whole = capi.ci_intervals(rows, 0.95)
    for per_batch, keys in ((1, 130), (1, 259), (5, 5 * 130), (5, 6 * 130 - 1), (37, 37 * 130), (37, 1 << 30)):
        monkeypatch.setenv(KNOB, str(keys))
        lb, ub, cqv = capi.ci_intervals(rows, 0.95)
        for r in range(len(rows)):
            assert (lb[r], ub[r], cqv[r]) == want[r], (per_batch, r)
        assert all(np.array_equal(a, b) for a, b in zip((lb, ub, cqv), whole)), per_batch


def _sums(rows, b, e):
    acc = np.zeros(rows.shape[1], np.float32)
    for j in range(b, e):
        acc = (acc + rows[j - 1]).astype(np.float32)
    return acc


def _expected(tpm, lbar, conf, gene_starts, trans_starts):
    """the six outputs from sample rows alone: orc.calc_ci over rows built as calcCI.cpp:336-357 builds them"""
    M = tpm.shape[0]
    fpkm = (1e3 / lbar.astype(np.float64) * tpm).astype(np.float32)
    out = {"tpm": np.array([orc.calc_ci(tpm[j], conf) for j in range(M)], np.float32).T,
           "fpkm": np.array([orc.calc_ci(fpkm[j], conf) for j in range(M)], np.float32).T}
    for key, starts in (("gene", gene_starts), ("iso", trans_starts)):
        if starts is None:
            continue
        for kind, rows in (("tpm", tpm), ("fpkm", fpkm)):
            res = np.zeros((3, len(starts) - 1), np.float32)
            for g in range(len(starts) - 1):
                b, e = starts[g], starts[g + 1]
                res[:, g] = out[kind][:, b - 1] if e - b == 1 else orc.calc_ci(_sums(rows, b, e), conf)
            out["%s_%s" % (key, kind)] = res
    return out


def _same(got, want, what):
    for key, w in want.items():
        bad = np.argwhere(got[key] != w)
        assert len(bad) == 0, "%s: %s[%d, %d]: device %r, expected %r (%d entries differ)" % (
            what, key, bad[0][0], bad[0][1], got[key][tuple(bad[0])], w[tuple(bad[0])], len(bad))


def _cycle_starts(M, sizes):
    out, pos, i = [1], 1, 0
    while pos <= M:
        pos = min(pos + sizes[i % len(sizes)], M + 1)
        out.append(pos)
        i += 1
    return np.array(out, np.int32)


def test_calculate_in_batches(monkeypatch):
    """M = 203 transcripts, 3 count vectors x 43 samples (nS = 129: one past two waves) under 1, 7, 64 and M rows per batch:
    68 multi-member genes (more than any of the three small batches holds), allele groups of 1 to 3, transcripts without weight
    whose rows are all zeros.  All six outputs: the same under every batch size, and equal to orc.calc_ci on ci_sample's rows."""
    M, nCV, nSpC, conf, seed = 203, 3, 43, 0.9, 77
    rng = np.random.default_rng(203)
    cv = rng.choice([0, 0, 1, 2, 17, 1000, 99991], (nCV, M + 1)).astype(np.int32)
    omitted = rng.random(M + 1) < 0.08
    omitted[[0, 1]] = False
    cv[:, omitted] = -1
    eel = rng.uniform(100.0, 4000.0, M + 1)
    mw = np.where(rng.random(M + 1) < 0.2, 0.85, 1.0)
    live = np.flatnonzero(~omitted)[2:]
    eel[live[::9]] = 0.0
    mw[live[4::13]] = 0.0
    eel[0] = 0.0
    gene_starts = _cycle_starts(M, [2, 1, 2, 3, 2, 2, 4, 2, 5, 2, 6, 2])
    trans_starts = _cycle_starts(M, [1, 2, 3, 2])
    gsz, tsz = np.diff(gene_starts), np.diff(trans_starts)
    assert set(gsz) == {1, 2, 3, 4, 5, 6} and (gsz > 1).sum() == 68 and set(tsz) == {1, 2, 3} and (tsz > 1).sum() > 64
    # transcripts without weight: their rows are all zeros; one gene mixes such rows with others, one has none
    dead = np.concatenate([[True], (cv[0, 1:] < 0) | (eel[1:] == 0) | (mw[1:] == 0), [False]])
    kinds = {(bool(dead[b:e].all()), bool(dead[b:e].any())) for b, e in zip(gene_starts[:-1], gene_starts[1:]) if e - b > 1}
    assert dead[1:M + 1].sum() > 20 and (False, True) in kinds and (False, False) in kinds
    monkeypatch.delenv(KNOB, raising=False)
    tpm, lbar = capi.ci_sample(cv, nSpC, eel, mw, 1.0, seed=seed)
    assert tpm.shape == (M, 129) and np.array_equal(~tpm.any(axis=1), dead[1:M + 1])
    want = _expected(tpm, lbar, conf, gene_starts, trans_starts)
    for R in (None, 1, 7, 64, M):
        if R is not None:
            monkeypatch.setenv(KNOB, str(R * 129))
        out = capi.ci_calculate(cv, nSpC, eel, mw, gene_starts, conf, 1.0, seed=seed, trans_starts=trans_starts)
        _same(out, want, "rows per batch: %s" % R)
        assert out["profile"].n_keys_sorted == 129 * (2 * M + 2 * int((gsz > 1).sum()) + 2 * int((tsz > 1).sum()))
    # without allele groups the isoform rows are not asked for
    monkeypatch.setenv(KNOB, str(7 * 129))
    out = capi.ci_calculate(cv, nSpC, eel, mw, gene_starts, conf, 1.0, seed=seed)
    _same(out, {k: v for k, v in want.items() if not k.startswith("iso")}, "no allele groups")
    # the same rows through the entry point that takes the caller's samples
    out = capi.ci_calculate_samples(tpm, lbar, gene_starts, conf, trans_starts=trans_starts)
    _same(out, want, "ci_calculate_samples, 7 rows per batch")


@pytest.mark.parametrize("name", CI_FIXTURES)
def test_calculate_samples_prints_the_reference_rows(name, monkeypatch):
    """rsem_ci_calculate_samples (--ci-stream reference) on the reference's own sample matrix: the TPM rows per target and per
    gene print to the reference's strings, whole and in batches of 5 rows.  (l_bar is not in the matrix: recomputed as
    test_ci_cpu.py does, so the FPKM rows are held to orc.calc_ci on rows built from the same l_bar, not to the strings.)  The
    isoform rows of the allele-specific fixture are compared with sums built afresh: the reference's carry its accumulator
    quirk (test_ci_cpu.py)."""
    fx, M, S, rows = load_pin(name)
    full, tot = rf.read_seq_lens(os.path.join(fx, "ref.seq"))
    model = rf.read_model(os.path.join(fx, "stat", "s.model"))
    eel = orc.calc_eel(M, full, tot, model["gld"])
    lbar = (S.astype(np.float64) / 1e6 * eel[1:, None]).sum(axis=0).astype(np.float32)
    grp = rf.read_grp(os.path.join(fx, "ref.grp"))
    ta = rf.read_grp(os.path.join(fx, "ref.ta")) if "allele_res" in rows else None
    per_target = rows["allele_res"] if ta is not None else rows["iso_res"]
    want = _expected(S, lbar, 0.95, grp, ta)
    nS = S.shape[1]
    for keys in (None, 5 * nS):
        if keys is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, str(keys))
        out = capi.ci_calculate_samples(S, lbar, grp, 0.95, trans_starts=ta)
        for r in range(3):
            assert ["%.6g" % v for v in out["tpm"][r]] == per_target[r], (keys, r)
            assert ["%.6g" % v for v in out["gene_tpm"][r]] == rows["gene_res"][r], (keys, r)
        _same(out, want, "%s, %s keys per batch" % (name, keys))
        assert out["profile"].n_draws == 0 and out["profile"].n_keys_sorted > 0
    if ta is not None:
        assert (np.diff(ta) > 1).any()          # (multi-allele transcripts: rows that are sums)


@pytest.mark.parametrize("value", ["0", "12x", "", "129", "-5", " 500", "1073741825", "99999999999999999999"])
def test_batch_knob_rejects_what_it_cannot_mean(value, monkeypatch):
    """RSEM_CI_BATCH_KEYS is a whole number from nSamples (here 130) to 2^30: anything else fails the call and names the knob."""
    rows = _tie_heavy_rows(8, 130)
    monkeypatch.setenv(KNOB, value)
    with pytest.raises(capi.RsemHipError, match=KNOB) as e:
        capi.ci_intervals(rows, 0.95)
    assert e.value.status == -1
    with pytest.raises(capi.RsemHipError, match=KNOB):
        capi.ci_calculate_samples(rows, np.full(130, 1500.0, np.float32), np.array([1, 4, 9], np.int32), 0.95)
