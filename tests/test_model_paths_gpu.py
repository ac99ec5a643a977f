"""The model-round kernel (k_model_group: rsem_amd/csrc/model.hip, model_block.hpp) on the device, on the paths that only the
CPU emulator of tests/test_model_emu_cpu.py reached: reads of several 16-alignment chunks, reads longer than 128 positions,
profile / fragment-length counts beyond their LDS tables, plane output for every shape of 8..64 lanes and reads that stay in
the CSR, mixed read lengths, N bases, low-quality reads, one-strand protocols, RSPD estimation, a mate-length distribution and
omitted transcripts -- and the combinations.  The inputs are generated (tools/gen_temp.cpp, table in model_path_cases.py);
the REFERENCE BINARY (oracle/_ref/rsem-run-em) and the drop-in run on the same files with the same argv, and every output is
compared at the bars of test_rsem_run_em_matches_reference: ROUND lines, .theta, every table of .model (a wrong count update
shows here), .ofg (every alignment's probability and every read's noise probability under the final model: a wrong lane mask
or a wrong plane slot shows here) and the TPM row of iso_res.

Each case first asserts, from s.dat and the read files, that it is on the path it is named after.  The same rows (17..300
alignments) go through the theta-only E step of the later rounds: k_estep_lane shapes of 8..64 lanes, k_estep_long.

Every subprocess has a time limit of its own; after one that a signal, an abort or its time limit ended nothing more of this
file touches the GPU (the remaining tests fail at once).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_path_cases as mc
import rsem_files as rf

pytestmark = pytest.mark.gpu

BIN = os.path.join(mc.ROOT, "rsem_amd", "bin")
OUTPUTS = ("stat/s.theta", "stat/s.model", "temp/s.ofg", "temp/s.iso_res")
VARIANTS = {
    "default": ([], {}),
    "lean": (["--lean-device"], {}),                       # .ofg comes from the planes
    "2shards": (["--ngpus", "2", "--devices", "0,0"], {}),
    "planes0": ([], {"RSEM_MODEL_PLANES": "0"}),           # the scatter pass instead of the kernel's plane output
}
_STOP = []    # why nothing more may be started on the GPU
_REF = {}     # case -> directory + parsed reference outputs


def _read_ofg_fast(path):
    """rf.read_ofg for files of millions of entries: one split of the whole text."""
    with open(path) as f:
        M, N0 = [int(x) for x in f.readline().split()]
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    n_tok = np.array([len(l.split()) for l in lines], np.int64)
    assert (n_tok % 2 == 0).all()
    tok = np.array(" ".join(lines).split(), np.float64)
    rp = np.zeros(len(lines) + 1, np.uint64)
    rp[1:] = np.cumsum(n_tok // 2)
    return M, N0, rp, tok[0::2].astype(np.int32), tok[1::2]


def _round_lines(log):
    return [l for l in log.split("\n") if l.startswith("ROUND")]


def _reference(name, tmp_path_factory):
    if name not in _REF:
        case = mc.CASES[name]
        d = str(tmp_path_factory.mktemp(name))
        mc.generate(case, d)
        P = mc.parse_inputs(case, d)
        mc.assert_path(name, P)                  # before anything runs
        log = mc.run_reference(case, d)
        os.makedirs(os.path.join(d, "refout"))
        for f in OUTPUTS:
            os.rename(os.path.join(d, f), os.path.join(d, "refout", os.path.basename(f)))
        r = os.path.join(d, "refout")
        mc.assert_path_ofg(name, _read_ofg_fast(os.path.join(r, "s.ofg")))
        _REF[name] = dict(d=d, P=P, rounds=_round_lines(log), theta=rf.read_theta(os.path.join(r, "s.theta")),
                          model=rf.read_model(os.path.join(r, "s.model")), ofg=_read_ofg_fast(os.path.join(r, "s.ofg")),
                          res=rf.read_res(os.path.join(r, "s.iso_res")))
    return _REF[name]


def _run_dropin(case, d, variant):
    extra, env = VARIANTS[variant]
    cmd = [os.path.join(BIN, "rsem-run-em")] + mc.em_args(case, d) + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        _STOP.append("%s ran into its time limit" % " ".join(cmd))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STOP.append("%s ended with status %d" % (" ".join(cmd), r.returncode))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _max_rel(a, b, floor=0.0):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    m = np.abs(b) > floor
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def _compare_rounds(my_log, ref_log):
    """As test_rsem_run_em_matches_reference: one ROUND line per round, the same number of them; rounds 1-11 the same totNum
    and SUM to 1e-6, later rounds the same totNum, bChange to the printed precision and SUM to 1e-9."""
    ref_rounds = int(ref_log[-1].split(",")[0].split("=")[1])
    my_rounds = int(my_log[-1].split(",")[0].split("=")[1])
    assert my_rounds == ref_rounds
    assert [int(l.split(",")[0].split("=")[1]) for l in my_log] == list(range(1, ref_rounds + 1))
    for a, b in zip(my_log[:11], ref_log[:11]):
        fa, fb = a.replace(",", "").split(), b.replace(",", "").split()
        assert fa[2] == fb[2] and abs(float(fa[5]) - float(fb[5])) < 1e-6 * float(fb[5]) and fa[-1] == fb[-1], (a, b)
    for a, b in zip(my_log[11:], ref_log[11:]):
        fa, fb = a.replace(",", "").split(), b.replace(",", "").split()
        assert fa[-1] == fb[-1] and abs(float(fa[8]) - float(fb[8])) <= 2e-5 * max(float(fb[8]), 1e-3), (a, b)
        assert abs(float(fa[5]) - float(fb[5])) <= 1e-9 * float(fb[5]), (a, b)
    return ref_rounds


def _compare_model(a, b):
    dev = 0.0
    assert a["type"] == b["type"] and a["gld"][:3] == b["gld"][:3]
    for key in ("qd_init", "qd_tran", "qpro", "nqpro", "pro", "npro", "rspd", "mw"):
        if key in b and b[key] is not None:
            assert a[key] is not None and a[key].shape == b[key].shape, key
            dev = max(dev, _max_rel(a[key], b[key], 1e-3))
            assert np.allclose(a[key], b[key], rtol=1e-6, atol=1e-9), (key, _max_rel(a[key], b[key], 1e-3))
    dev = max(dev, _max_rel(a["gld"][3], b["gld"][3], 1e-3))
    assert np.allclose(a["gld"][3], b["gld"][3], rtol=1e-6, atol=1e-9), ("gld", _max_rel(a["gld"][3], b["gld"][3], 1e-3))
    assert (a["mld"] is None) == (b["mld"] is None)
    if b["mld"] is not None:
        dev = max(dev, _max_rel(a["mld"][3], b["mld"][3], 1e-3))
        assert a["mld"][:3] == b["mld"][:3] and np.allclose(a["mld"][3], b["mld"][3], rtol=1e-6, atol=1e-12), "mld"
    return dev   # over the entries above 1e-3 (the bar itself is rtol 1e-6 + atol 1e-9 on every entry)


def _compare_ofg(mine, ref, P):
    M, N0, rp, sid, val = mine
    gM, gN0, grp, gsid, gval = ref
    assert (M, N0) == (gM, gN0) and np.array_equal(rp, grp) and np.array_equal(sid, gsid)
    bad = ~np.isclose(val, gval, rtol=1e-6, atol=0)
    if bad.any():  # name the path: the alignment counts and lengths of the offending reads, and where in the read the entries are
        rows = np.searchsorted(rp.astype(np.int64), np.flatnonzero(bad), side="right") - 1
        keep = np.flatnonzero(P["minlen"] >= mc.SEED_LEN)   # low-quality reads have no row in .ofg
        assert len(rp) - 1 == len(keep), ".ofg: %d values differ (rows %d, reads that are not low quality %d)" % (int(bad.sum()), len(rp) - 1, len(keep))
        urows = keep[np.unique(rows)]
        rp = np.concatenate([[0], np.cumsum(np.bincount(keep, np.diff(rp.astype(np.int64)), P["N1"]).astype(np.int64))])
        bad_of = lambda r: np.flatnonzero(bad[int(rp[r]):int(rp[r + 1])])
        first = [(int(r), int(P["nal"][r]), P["lens"][:, r].tolist(), (bad_of(r) - 1).tolist()[:8])
                 for r in urows[:12]]
        pytest.fail(".ofg: %d values of %d reads differ; alignments per offending read: min %d max %d, lengths: min %d max %d; "
                    "first (read, alignments, lengths, entries [-1 = noise]): %s"
                    % (int(bad.sum()), len(urows), P["nal"][urows].min(), P["nal"][urows].max(), P["lens"][:, urows].min(),
                       P["lens"][:, urows].max(), first))
    return _max_rel(val, gval)


# (RSEM_MODEL_PLANES=0 is run on the cases with reads of more than 16 alignments: path 4).  A case's variants follow each other:
# the reference runs once per case, before the first of them.
RUNS = [(n, v) for n, c in mc.CASES.items() for v in VARIANTS if v != "planes0" or c["planes0"]]


@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % nv for nv in RUNS])
def test_model_paths_vs_reference_binary(name, variant, tmp_path_factory):
    case = mc.CASES[name]
    if not (mc.have_tools() and os.path.exists(os.path.join(BIN, "rsem-run-em"))):
        pytest.skip("generator or reference binaries not built")
    assert not _STOP, "not started: " + _STOP[0]
    R = _reference(name, tmp_path_factory)
    d = R["d"]
    for f in OUTPUTS:
        if os.path.exists(os.path.join(d, f)):
            os.remove(os.path.join(d, f))
    out = _run_dropin(case, d, variant)
    if variant == "2shards":
        assert sum(l.startswith("GPU ") for l in out.split("\n")) == 2
    rounds = _compare_rounds(_round_lines(out), R["rounds"])
    raw, pol = rf.read_theta(os.path.join(d, "stat", "s.theta"))
    graw, gpol = R["theta"]
    dev_theta = max(_max_rel(raw, graw, 1e-7), _max_rel(pol, gpol, 1e-7))
    dev_model = _compare_model(rf.read_model(os.path.join(d, "stat", "s.model")), R["model"])
    res = rf.read_res(os.path.join(d, "temp", "s.iso_res"))
    tpm, gtpm = np.array(res[5], float), np.array(R["res"][5], float)
    dev_tpm = float(np.max(np.abs(tpm - gtpm)))
    # (figures first, then the bars)
    print("DEVIATION %s %s: rounds %d theta %.3g model %.3g tpm(abs) %.3g" % (name, variant, rounds, dev_theta, dev_model, dev_tpm))
    assert dev_theta < 1e-6 and np.allclose(raw, graw, rtol=1e-6, atol=1e-10) and np.allclose(pol, gpol, rtol=1e-6, atol=1e-10)
    assert np.allclose(tpm, gtpm, atol=0.011, rtol=1e-6)
    dev_ofg = _compare_ofg(_read_ofg_fast(os.path.join(d, "temp", "s.ofg")), R["ofg"], R["P"])
    print("DEVIATION %s %s: ofg %.3g" % (name, variant, dev_ofg))
    if (name, variant) == [nv for nv in RUNS if nv[0] == name][-1]:  # the case's last run: its files and parsed outputs are not needed again
        shutil.rmtree(d, ignore_errors=True)
        _REF[name] = None


# ---- every row length 1..300 through the theta-only E step ---------------------------------------------------------------------
SWEEP_MAX, SWEEP_READS, SWEEP_SPREAD = 300, 200, 8
MAX_ROUND = 1000
_SWEEP = {}


def _sweep_input():
    """SWEEP_READS reads of every length 1..300; length L owns the transcripts [a0(L), a0(L) + L + SWEEP_SPREAD): its reads hold L
    consecutive ids from one of SWEEP_SPREAD anchors -- compact inside one window.  Values as _build of test_em_units_gpu.py: one
    likely alignment per read, the others 5-20 times less likely (within 2^8 of it: every read of up to 256 alignments takes Q32 planes)."""
    if "d" not in _SWEEP:
        lens = np.repeat(np.arange(1, SWEEP_MAX + 1, dtype=np.int64), SWEEP_READS)
        width = np.arange(1, SWEEP_MAX + 1, dtype=np.int64) + SWEEP_SPREAD
        a0 = 1 + np.concatenate([[0], np.cumsum(width)[:-1]])          # first id of length L's group: a0[L - 1]
        M = int(a0[-1] + width[-1]) - 1
        anchor = np.repeat(a0, SWEEP_READS) + np.tile(np.arange(SWEEP_READS) % SWEEP_SPREAD, SWEEP_MAX)
        rp = np.zeros(len(lens) + 1, np.uint64)
        rp[1:] = np.cumsum(lens)
        within = np.arange(int(rp[-1]), dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lens)
        sid = np.repeat(anchor, lens) + within
        assert sid.min() == 1 and sid.max() <= M
        rng = np.random.default_rng(20)
        # the reads in random order: every slice of the layout is then filled by the layout's own sort, not by the caller's
        perm = rng.permutation(len(lens))
        start = rp[:-1].astype(np.int64)[perm]
        lens_p = lens[perm]
        rp_p = np.zeros(len(lens) + 1, np.uint64)
        rp_p[1:] = np.cumsum(lens_p)
        idx = np.repeat(start, lens_p) + (np.arange(int(rp[-1]), dtype=np.int64) - np.repeat(rp_p[:-1].astype(np.int64), lens_p))
        sid = sid[idx]
        cp = rng.uniform(0.05, 0.2, len(sid))
        # the likely alignment: the one to the group's transcript a0 + SPREAD - 1 + (L - 1) / 2 (the nearest the read holds) -- at 8
        # different places in the reads of one length, and few expressed transcripts per group: EM stops by its own rule
        hot = (np.repeat(a0, SWEEP_READS) + SWEEP_SPREAD - 1 + (lens - 1) // 2)[perm]
        first = sid[rp_p[:-1].astype(np.int64)]
        cp[rp_p[:-1].astype(np.int64) + np.clip(hot - first, 0, lens_p - 1)] = rng.uniform(0.5, 1.0, len(lens_p))
        ncp = rng.uniform(0.01, 1.0, len(lens_p)) * 1e-5
        theta0 = np.full(M + 1, 0.95 / M)
        theta0[0] = 0.05
        group = np.zeros(M + 1, np.int64)                               # transcript -> the row length that owns it (0: noise)
        group[1:] = np.repeat(np.arange(1, SWEEP_MAX + 1), width)
        _SWEEP["d"] = dict(M=M, N0=100, row_ptr=rp_p, sid=sid.astype(np.int32), conprb=cp, ncp=ncp, theta0=theta0, lens=lens_p, group=group)
    return _SWEEP["d"]


def _by_length(d, got, want, rtol, atol):
    """Row lengths whose transcripts hold a count (theta) that differs: a failure names its shape."""
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol)
    return sorted(set(d["group"][bad].tolist()))


@pytest.mark.parametrize("bits", [64, 32])
def test_every_row_length_step_and_every_loop(bits, monkeypatch):
    from oracle import pyoracle as orc
    from rsem_amd import capi
    from tools.q32_ref import quantize_q32
    d = _sweep_input()
    M, rp, sid, ncp, th0, N0 = d["M"], d["row_ptr"], d["sid"], d["ncp"], d["theta0"], d["N0"]
    n_long = int(np.count_nonzero(d["lens"] > 256))
    assert n_long == SWEEP_READS * (SWEEP_MAX - 256) and set(d["lens"].tolist()) == set(range(1, SWEEP_MAX + 1))
    cp = d["conprb"]
    if bits == 32:
        cp, took = quantize_q32(rp, d["conprb"], 8)
        assert np.array_equal(took, d["lens"] <= 256)
    ctx = capi.EmContext(M, rp, sid, d["conprb"], ncp)
    if bits == 32:
        ctx.set_option("value_bits", 32)
    # the layout holds what the input was built for: every read of up to 256 alignments sliced (Q32: in Q32 planes), the others in the
    # CSR, nothing split (every read compact inside its window)
    assert ctx.info("reads_long") == n_long and ctx.info("reads_sliced") == len(d["lens"]) - n_long
    assert ctx.info("split_rows") == 0 and ctx.info("reads_q32") == (len(d["lens"]) - n_long if bits == 32 else 0)
    oc = orc.em_estep(M, rp, sid, cp, ncp, th0)
    oc[0] += N0
    counts, *_ = ctx.step(th0, N0)
    assert _by_length(d, counts, oc, 1e-9, 1e-9) == [], "step, value_bits %d" % bits
    # the weights pass (always from the doubles)
    c2, w, wn = ctx.expected_weights(th0, N0)
    oc2, ow, own = orc.em_estep(M, rp, sid, d["conprb"], ncp, th0, want_weights=True)
    oc2[0] += N0
    badw = ~np.isclose(w, ow, rtol=1e-12, atol=0)
    assert sorted(set(np.repeat(d["lens"], d["lens"])[badw].tolist())) == [] and np.allclose(wn, own, rtol=1e-12, atol=0)
    assert _by_length(d, c2, oc2, 1e-9, 1e-9) == []
    oth, orounds, _, ot = orc.em_run(M, rp, sid, cp, ncp, N0, th0, max_round=MAX_ROUND)
    runs = {}
    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        out = ctx.run(th0, N0, max_round=MAX_ROUND)
        assert out["rounds"] == orounds and out["totNum"] == ot, (loop, out["rounds"], orounds)
        assert _by_length(d, out["theta"], oth, 1e-6, 1e-12) == [], "loop %s, value_bits %d" % (loop, bits)
        runs[loop] = out
    for loop in ("1", "2"):
        assert _by_length(d, runs[loop]["theta"], runs["0"]["theta"], 1e-10, 1e-18) == [], loop
    print("SWEEP value_bits %d: rounds %d, step max rel %.3g, theta max rel %.3g" %
          (bits, orounds, _max_rel(counts, oc, 1e-12), max(_max_rel(runs[l]["theta"], oth, 1e-12) for l in runs)))
    ctx.close()
