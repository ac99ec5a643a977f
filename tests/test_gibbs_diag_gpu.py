"""Gibbs convergence diagnostics on the GPU (rsem_amd/csrc/gibbs_diag.hip through capi.gibbs_diagnose, and rsem-run-gibbs
--diagnostics) against the numpy restatement of the definition, tests/diag_ref.py.

Condition, not tolerance: every comparison covers every transcript, and means something only where no decision of Geyer's rule (stop
at a non-positive pair, take the minimum with the pair before) sits within 1e-7 of a tie; every case asserts that for its own input
first.  Smallest distances of the committed inputs: synthetic 4.0e-5, one chain of 4 samples 2.8e-5, counts around 5e7 2.6e-5.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import diag_ref as dr
import rsem_files as rf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rsem_amd", "bin")
DEFAULT_L0 = 15  # kDefaultL0 of gibbs_diag.hip
TIE = 1e-7


def capi():
    from rsem_amd import capi as c
    return c


def _long_series():
    """Past the sizes of the programs' runs, where the kernels take their other paths: sequences longer than the 128 samples a
    workgroup of the first kernel holds at a time (chunks that overlap by the lags), lags beyond one group of 64, ..."""
    rng = np.random.default_rng(5)
    return [dr.ar1_counts(rng, 0.95, ns, 130, 1000.0, 100.0) for ns in (300, 301)]


def _very_long_series():
    """... and a transcript's series past what the one-wave kernel keeps in LDS (32 KiB = 8192 values): read from global memory."""
    rng = np.random.default_rng(6)
    return [dr.ar1_counts(rng, 0.9, 8210, 5, 1000.0, 100.0)]


INPUTS = {"synthetic": dr.synthetic, "one_chain_of_4": lambda: dr.synthetic(nsamples=(4,)),
          "counts_5e7": lambda: dr.synthetic(centre=5e7, sd=300.0), "chunks": _long_series, "series_in_global": _very_long_series}
_cache = {}


def _input(name):
    if name not in _cache:
        cvs = INPUTS[name]()
        _cache[name] = (cvs, dr.diag_ref(cvs))
    return _cache[name]


def _as_dict(out):
    mean, sd, rhat, ess, lag, sm = out
    return dict(mean=mean, sd=sd, rhat=rhat, ess=ess, lag=lag), sm


def _check_summary(sm, got, ref, L0):
    want = dr.summary_ref(dict(got, n_used=ref["n_used"], sequences=ref["sequences"]), L0)
    for k, v in want.items():
        if isinstance(v, float):
            assert (np.isnan(v) and np.isnan(sm[k])) or sm[k] == v, (k, sm[k], v)
        else:
            assert sm[k] == v, (k, sm[k], v)
    assert sm["upload_ms"] > 0 and sm["kernel_ms"] > 0


@pytest.mark.parametrize("L0", [None, 1, 3, 63])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_diagnose_against_ref(name, L0, monkeypatch):
    cvs, ref = _input(name)
    print("%s: tie distance %.3g, largest lag %d" % (name, ref["tie"], ref["lag"].max()))
    assert ref["tie"] >= TIE
    if L0 is None:
        monkeypatch.delenv("RSEM_GIBBS_DIAG_L0", raising=False)
    else:
        monkeypatch.setenv("RSEM_GIBBS_DIAG_L0", str(L0))
    got, sm = _as_dict(capi().gibbs_diagnose(cvs))
    dr.compare(got, ref, (name, L0))
    eff = DEFAULT_L0 if L0 is None else L0
    _check_summary(sm, got, ref, eff)
    assert sm["n_long"] == int((ref["lag"][1:] > eff).sum())
    if name == "synthetic" and L0 in (1, 3):
        assert sm["n_long"] > 0
    if name in ("chunks", "series_in_global") and L0 != 63:
        assert sm["n_long"] > 0  # these inputs are there for the long path
    if name == "synthetic":
        assert np.isnan(got["rhat"][5]) and np.isposinf(got["rhat"][6])


def test_two_calls_are_bit_identical(monkeypatch):
    monkeypatch.setenv("RSEM_GIBBS_DIAG_L0", "3")
    cvs, _ = _input("synthetic")
    a, sa = _as_dict(capi().gibbs_diagnose(cvs))
    b, sb = _as_dict(capi().gibbs_diagnose(cvs))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in sa:
        if not k.endswith("_ms"):
            assert (sa[k] == sb[k]) or (np.isnan(sa[k]) and np.isnan(sb[k])), k


@pytest.mark.parametrize("value", ["0", "2", "65", "-3", "x", "7x", ""])
def test_bad_knob_values(value, monkeypatch):
    c = capi()
    monkeypatch.setenv("RSEM_GIBBS_DIAG_L0", value)
    with pytest.raises(c.RsemHipError) as e:
        c.gibbs_diagnose(_input("synthetic")[0])
    assert e.value.status == -1


def test_invalid_arguments(monkeypatch):
    import ctypes as C
    c = capi()
    monkeypatch.delenv("RSEM_GIBBS_DIAG_L0", raising=False)
    with pytest.raises(c.RsemHipError) as e:  # n < 2
        c.gibbs_diagnose(dr.synthetic(nsamples=(3, 9)))
    assert e.value.status == -1 and "at least 2" in str(e.value)
    cvs = _input("synthetic")[0]
    ns = np.array([a.shape[0] for a in cvs], np.int32)
    ptrs = (C.c_void_p * 3)(cvs[0].ctypes.data, None, cvs[2].ctypes.data)  # a NULL block
    L = c.lib()
    assert L.rsem_gibbs_diagnose(0, 512, 3, ns.ctypes.data, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == -1
    ptrs[1] = cvs[1].ctypes.data
    assert L.rsem_gibbs_diagnose(0, 512, 3, None, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == -1
    assert L.rsem_gibbs_diagnose(0, 512, 3, ns.ctypes.data, None, None, None, None, None, None, None) == -1
    assert L.rsem_gibbs_diagnose(0, -1, 3, ns.ctypes.data, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == -1
    assert L.rsem_gibbs_diagnose(0, 512, -1, ns.ctypes.data, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == -1
    assert L.rsem_gibbs_diagnose(-1, 512, 3, ns.ctypes.data, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == -1
    # every output may be NULL
    assert L.rsem_gibbs_diagnose(0, 512, 3, ns.ctypes.data, C.cast(ptrs, C.c_void_p), None, None, None, None, None, None) == 0


# ---- end to end: chains of the samplers themselves -------------------------------------------------------------------------

M_E2E = 300
PAIR = (M_E2E - 1, M_E2E)


def _items():
    """A few thousand reads over a few hundred transcripts, so that counts move, built the way tests/test_gibbs_replay_gpu.py builds
    its input; plus a pair of transcripts that share all their reads with equal probabilities: how those reads split between the
    two is a random walk."""
    rng = np.random.default_rng(20261)
    M = M_E2E
    n = 4000
    lens = rng.integers(1, 7, n)
    start = rng.integers(1, M - 8, n)
    rp, sid, cp = [0], [], []
    for i in range(n):
        L = int(lens[i])
        scale = 10.0 ** rng.uniform(-12, -3)
        sid += [0] + list(start[i] + np.arange(L))
        cp += [scale * 2.0 ** rng.uniform(-14, -6)] + list(scale * 2.0 ** rng.uniform(-3, 0, L))
        rp.append(len(sid))
    for i in range(400):
        sid += [0, PAIR[0], PAIR[1]]
        cp += [1e-12, 1e-5, 1e-5]
        rp.append(len(sid))
    n += 400
    N0 = 37
    return dict(M=M, rp=np.array(rp, np.uint64), sid=np.array(sid, np.int32), cp=np.array(cp), init=np.zeros(M + 1, np.int32),
                eel=rng.uniform(200.0, 3000.0, M + 1), mw=np.ones(M + 1), grp=np.append(np.arange(1, M + 1, 7), M + 1).astype(np.int32),
                N0=N0, totc=float(M + 1 + N0 + n))


def test_chains_of_both_samplers(monkeypatch):
    """3 chains of 100 kept samples in either mode.  The pair's counts random-walk: a sweep moves the split of its 400 reads by about
    ten reads where the posterior is flat over all 401 splits, so its autocorrelations stay positive far beyond the default L0."""
    monkeypatch.delenv("RSEM_GIBBS_DIAG_L0", raising=False)
    c = capi()
    d = _items()
    g = c.GibbsContext(d["M"], d["rp"], d["sid"], d["cp"], d["init"], None, 1.0, d["totc"], d["N0"], d["eel"], d["mw"], d["grp"])
    pair_lag = []
    try:
        for mode in (c.GIBBS_EXACT, c.GIBBS_PARALLEL):
            cvs, _, _, _ = g.run_chains(mode, [11, 12, 13], 20, [100, 100, 100], 1, thin=1, want_vectors=True)
            ref = dr.diag_ref(cvs)
            print("mode %d: tie distance %.3g, lags of the pair %s, largest rhat %.3f" % (mode, ref["tie"], ref["lag"][list(PAIR)],
                                                                                        np.nanmax(ref["rhat"][np.isfinite(ref["rhat"])])))
            assert ref["tie"] >= TIE
            got, sm = _as_dict(c.gibbs_diagnose(cvs))
            dr.compare(got, ref, mode)
            _check_summary(sm, got, ref, DEFAULT_L0)
            pair_lag.append(int(got["lag"][list(PAIR)].max()))
    finally:
        g.close()
    assert max(pair_lag) > DEFAULT_L0, pair_lag


# ---- the program ------------------------------------------------------------------------------------------------------------

def _run_gibbs(tmp_path, sub, mode, extra):
    fx = rf.fixture("pe_q")
    dst = os.path.join(str(tmp_path), sub)
    shutil.copytree(fx, dst)
    meta = rf.read_meta(fx)
    b, n, g = meta["gibbs"]
    imd = os.path.join(dst, "temp", "s")
    shutil.copy(imd + ".iso_res.em", imd + ".iso_res")
    shutil.copy(imd + ".gene_res.em", imd + ".gene_res")
    for k in range(meta["gibbs_threads"]):
        os.remove(imd + ".countvectors%d" % k)
    r = subprocess.run([os.path.join(BIN, "rsem-run-gibbs"), os.path.join(dst, "ref"), imd, os.path.join(dst, "stat", "s"), str(b), str(n), str(g),
                        "-p", str(meta["gibbs_threads"]), "--seed", str(meta["gibbs_seed"]), "--gibbs-mode", mode] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dst, imd, meta, r.stdout


@pytest.mark.parametrize("mode", ["exact", "parallel"])
def test_program_writes_the_diagnostics(mode, tmp_path):
    dst, imd, meta, out = _run_gibbs(tmp_path, "with", mode, ["--diagnostics"])
    dst0, imd0, _, out0 = _run_gibbs(tmp_path, "without", mode, [])
    nthreads = meta["gibbs_threads"]
    # nothing else changes
    for f in ["iso_res", "gene_res"] + ["countvectors%d" % k for k in range(nthreads)]:
        with open(imd + "." + f, "rb") as a, open(imd0 + "." + f, "rb") as b:
            assert a.read() == b.read(), f
    assert not os.path.exists(os.path.join(dst0, "stat", "s.gibbs_diag"))
    line = [l for l in out.split("\n") if l.startswith("Gibbs diagnostics:")]
    assert len(line) == 1 and "max_rhat" in line[0] and "min_ess" in line[0]
    assert out.replace(line[0] + "\n", "") == out0
    # the file against the definition over the count vectors the same run wrote
    cvs = [rf.read_countvectors(imd + ".countvectors%d" % k) for k in range(nthreads)]
    ref = dr.diag_ref(cvs)
    print("%s: tie distance %.3g" % (mode, ref["tie"]))
    assert ref["tie"] >= TIE
    lines = open(os.path.join(dst, "stat", "s.gibbs_diag")).read().rstrip("\n").split("\n")
    head = dict(l[2:].split(" ", 1) for l in lines if l.startswith("# "))
    rows = [l.split("\t") for l in lines if not l.startswith("# ")]
    assert rows[0] == ["transcript_id", "mean_count", "sd_count", "rhat", "ess", "lag"]
    rows = rows[1:]
    M = meta["M"]
    assert len(rows) == M
    ids = [l.split("\t")[0] for l in open(os.path.join(dst, "ref.ti")).read().split("\n")[1::6][:M]]
    assert [r[0] for r in rows] == ids
    for i, r in enumerate(rows, start=1):
        for col, key in enumerate(("mean", "sd", "rhat", "ess"), start=1):
            want = ref[key][i]
            if np.isnan(want):
                assert r[col] == "NA", (i, key, r[col])
            elif np.isinf(want):
                assert r[col] == "inf", (i, key, r[col])
            else:  # %.6g: half a unit of the sixth digit
                assert abs(float(r[col]) - want) <= 5.1e-6 * abs(want), (i, key, r[col], want)
        assert int(r[5]) == ref["lag"][i], (i, r[5])
    want = dr.summary_ref(ref, DEFAULT_L0)
    assert head["sampler"] == mode
    for k in ("n_used", "sequences", "n_defined", "n_rhat_gt_1p01", "n_rhat_gt_1p1", "n_long"):
        assert int(head[k]) == want[k], (k, head[k], want[k])
    # the ids: the device's own doubles decide among transcripts whose values agree to the last bits (the cap S log10 S is common)
    for k, key in (("max_rhat_id", "rhat"), ("min_ess_id", "ess")):
        assert 1 <= int(head[k]) <= M and abs(ref[key][int(head[k])] - ref[key][want[k]]) <= 1e-9 * abs(ref[key][want[k]]), (k, head[k], want[k])
    for k in ("max_rhat", "min_ess"):
        assert abs(float(head[k]) - want[k]) <= 5.1e-6 * abs(want[k]), (k, head[k], want[k])
    assert float(head["upload_ms"]) > 0 and float(head["kernel_ms"]) > 0


def test_dry_run_accepts_the_option(tmp_path):
    dst, imd, meta, out = _run_gibbs(tmp_path, "dry", "exact", ["--diagnostics", "--dry-run"])
    assert "dry run" in out and not os.path.exists(os.path.join(dst, "stat", "s.gibbs_diag"))
    assert not os.path.exists(imd + ".countvectors0")
