"""The wide window addresses of the model-round kernel (k_model_group<..., kWide = true>: rsem_amd/csrc/model.hip, model_block.hpp)
on the device, through the program: references whose two strands take 4 GiB and more have window addresses of 40 bits.  The
inputs are four generated cases of tests/model_path_cases.py (the four read types, reads longer than 128 positions, reads of
several 16-alignment chunks, a reverse-strand-only protocol) at kilobytes of reference; RSEM_MODEL_STRAND_PAD puts that many
unused device bytes in front of the strand array, chosen per case so that 2^32 falls on the multiple-of-8 strand offset that the
most alignment windows of s.dat straddle (computed here from ref.seq and s.dat, asserted to be at least one window).

The REFERENCE BINARY (oracle/_ref/rsem-run-em) runs once per case; the drop-in runs with the pad as one shard and as two, and
every output is held to the reference's at exactly the bars of test_model_paths_vs_reference_binary (its helpers are copied
here): ROUND lines, .theta, every table of .model, .ofg, the TPM column.  The program says "model: window addresses of N bits"
once per shard on the wide path and nothing without the pad.  The deviation of the padded run from the unpadded one is printed
without a bar: the update's LDS atomics make run-to-run noise.

Every subprocess has a time limit of its own; after one that a signal, an abort or its time limit ended nothing more of this
file touches the GPU (the remaining tests fail at once).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import model_path_cases as mc
import rsem_files as rf

pytestmark = pytest.mark.gpu

BIN = os.path.join(mc.ROOT, "rsem_amd", "bin")
OUTPUTS = ("stat/s.theta", "stat/s.model", "temp/s.ofg", "temp/s.iso_res")
CASES = ("chunks_two_pass_se_q", "chunks_pe_q", "chunks_two_pass_pe_noq", "stranded_rev_rspd_omit")
# variant -> (arguments, shards, with the pad)
VARIANTS = {
    "default": ([], 1, True),
    "2shards": (["--ngpus", "2", "--devices", "0,0"], 2, True),
    "nopad": ([], 1, False),
}
LINE = re.compile(r"^model: window addresses of (\d+) bits \(strands (\d+) bytes\)$")
_STOP = []    # why nothing more may be started on the GPU
_REF = {}     # case -> directory + parsed reference outputs + the pad
_PADDED = {}  # case -> (theta, ofg values) of the padded one-shard run, for the record against the unpadded one


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


def strand_layout(tot):
    """Byte offset of strand dir of transcript sid, soff[2 * sid + dir], and the bytes of all strands: sid ascending, forward then
    reverse, each strand rounded up to 8 bytes (rsem_model_create)."""
    size = (tot.astype(np.int64) + 7) // 8 * 8
    size[0] = 0
    start = 2 * (np.cumsum(size) - size)
    soff = np.zeros(2 * len(tot), np.int64)
    soff[0::2] = start
    soff[1::2] = start + size
    return soff, int(2 * size.sum())


def busiest_boundary(case, d, P):
    """-> (b, n, strand_bytes): the multiple-of-8 strand offset b that the most alignment windows of s.dat straddle (start < b <
    end; the windows the kernel walks: reads that are not low quality), and how many do."""
    pe = case["rt"] >= 2
    w = 3 if pe else 2
    _, tot = rf.read_seq_lens(os.path.join(d, "ref.seq"))
    soff, strand_bytes = strand_layout(tot)
    with open(os.path.join(d, "temp", "s.dat")) as f:
        f.readline()
        tok = np.array(f.read().split(), np.int64)
    nal = P["nal"]
    assert len(tok) == len(nal) + w * int(nal.sum())
    body = np.ones(len(tok), bool)
    body[np.concatenate([[0], np.cumsum(1 + w * nal)[:-1]])] = False   # the count in front of every read's alignments
    hits = tok[body].reshape(-1, w)
    sid, pos = hits[:, 0], hits[:, 1]
    row = np.repeat(np.arange(len(nal)), nal)
    live = P["minlen"][row] >= mc.SEED_LEN
    rev = (sid < 0).astype(np.int64)
    t = np.abs(sid)
    wins = [(soff[2 * t + rev] + pos, P["lens"][0][row])]
    if pe:
        wins.append((soff[2 * t + (1 - rev)] + tot[t] - pos - hits[:, 2], P["lens"][1][row]))
    diff = np.zeros(strand_bytes // 8 + 2, np.int64)
    for a, ln in wins:
        a, ln = a[live], ln[live]
        assert (a >= 0).all() and (a + ln <= strand_bytes).all()
        lo, hi = a // 8 + 1, (a + ln - 1) // 8           # the multiples of 8 inside (a, a + ln)
        ok = hi >= lo
        np.add.at(diff, lo[ok], 1)
        np.add.at(diff, hi[ok] + 1, -1)
    count = np.cumsum(diff)
    k = int(np.argmax(count))
    return 8 * k, int(count[k]), strand_bytes


def _reference(name, tmp_path_factory):
    if name not in _REF:
        case = mc.CASES[name]
        d = str(tmp_path_factory.mktemp(name))
        mc.generate(case, d)
        P = mc.parse_inputs(case, d)
        mc.assert_path(name, P)                  # before anything runs
        b, n, strand_bytes = busiest_boundary(case, d, P)
        print("BOUNDARY %s: 2^32 at strand offset %d of %d, inside %d alignment windows" % (name, b, strand_bytes, n))
        assert n >= 1 and b % 8 == 0 and 0 < b < strand_bytes
        log = mc.run_reference(case, d)
        os.makedirs(os.path.join(d, "refout"))
        for f in OUTPUTS:
            os.rename(os.path.join(d, f), os.path.join(d, "refout", os.path.basename(f)))
        r = os.path.join(d, "refout")
        _REF[name] = dict(d=d, P=P, pad=(1 << 32) - b, strand_bytes=strand_bytes, rounds=_round_lines(log), theta=rf.read_theta(os.path.join(r, "s.theta")),
                          model=rf.read_model(os.path.join(r, "s.model")), ofg=_read_ofg_fast(os.path.join(r, "s.ofg")),
                          res=rf.read_res(os.path.join(r, "s.iso_res")))
    return _REF[name]


def _run_dropin(case, d, extra, env, timeout=300, ok_to_fail=False):
    cmd = [os.path.join(BIN, "rsem-run-em")] + mc.em_args(case, d) + extra
    full = dict(os.environ, **env)
    if "RSEM_MODEL_STRAND_PAD" not in env:
        full.pop("RSEM_MODEL_STRAND_PAD", None)
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=full)
    except subprocess.TimeoutExpired:
        _STOP.append("%s ran into its time limit" % " ".join(cmd))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STOP.append("%s ended with status %d" % (" ".join(cmd), r.returncode))
    if not ok_to_fail:
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r if ok_to_fail else r.stdout


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


# A case's runs follow each other: the reference runs once per case, before the first of them; the unpadded run comes last.
RUNS = [(n, v) for n in CASES for v in VARIANTS]


@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % nv for nv in RUNS])
def test_wide_addresses_vs_reference_binary(name, variant, tmp_path_factory):
    case = mc.CASES[name]
    if not (mc.have_tools() and os.path.exists(os.path.join(BIN, "rsem-run-em"))):
        pytest.skip("generator or reference binaries not built")
    assert not _STOP, "not started: " + _STOP[0]
    R = _reference(name, tmp_path_factory)
    d = R["d"]
    for f in OUTPUTS:
        if os.path.exists(os.path.join(d, f)):
            os.remove(os.path.join(d, f))
    extra, shards, padded = VARIANTS[variant]
    out = _run_dropin(case, d, extra, {"RSEM_MODEL_STRAND_PAD": str(R["pad"])} if padded else {})
    if shards == 2:
        assert sum(l.startswith("GPU ") for l in out.split("\n")) == 2
    said = [LINE.match(l) for l in out.split("\n") if l.startswith("model: window addresses of")]
    if padded:   # once per shard, more than 32 bits, the strands' own size (the pad is not part of it)
        assert len(said) == shards and all(m and int(m.group(1)) > 32 and int(m.group(2)) == R["strand_bytes"] for m in said), (said, out[-2000:])
    else:
        assert said == [], out[-2000:]
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
    ofg = _read_ofg_fast(os.path.join(d, "temp", "s.ofg"))
    dev_ofg = _compare_ofg(ofg, R["ofg"], R["P"])
    print("DEVIATION %s %s: ofg %.3g" % (name, variant, dev_ofg))
    if variant == "default":
        _PADDED[name] = (pol, ofg[4])
    if variant == "nopad" and name in _PADDED:   # for the record, no bar: the update's LDS atomics make run-to-run noise
        ppol, pval = _PADDED.pop(name)
        print("PADDED AGAINST UNPADDED %s: theta %.3g ofg %.3g" % (name, _max_rel(ppol, pol, 1e-7), _max_rel(pval, ofg[4])))
    if (name, variant) == [nv for nv in RUNS if nv[0] == name][-1]:  # the case's last run: its files and parsed outputs are not needed again
        shutil.rmtree(d, ignore_errors=True)
        _REF[name] = None


@pytest.mark.parametrize("pad,message", [("12", "RSEM_MODEL_STRAND_PAD must be a whole number of bytes, a multiple of 8"), ("8k", "RSEM_MODEL_STRAND_PAD must be"),
                                         (str(1 << 40), "the model context addresses them with at most 40 bits")])
def test_bad_pad_and_the_remaining_limit_are_refused_with_a_message(pad, message, tmp_path_factory):
    """rsem_model_create fails with RSEM_ERR_INVALID -- before the strands are built or anything is allocated for them -- and the
    program ends with the library's message (the reference's convention: message on stderr, exit status -1)."""
    if not (mc.have_tools(need_ref=False) and os.path.exists(os.path.join(BIN, "rsem-run-em"))):
        pytest.skip("generator not built")
    assert not _STOP, "not started: " + _STOP[0]
    case = dict(rt=1, n=400, M=40, L=75, iso="2-9", opts=[])
    d = str(tmp_path_factory.mktemp("bad_pad"))
    mc.generate(case, d)
    r = _run_dropin(case, d, [], {"RSEM_MODEL_STRAND_PAD": pad}, timeout=120, ok_to_fail=True)
    assert not _STOP, _STOP[0]                      # an orderly exit, no signal
    assert r.returncode == 255 and "rsem_model_create failed" in r.stderr and message in r.stderr, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    shutil.rmtree(d, ignore_errors=True)


# ---- one reference of real size ---------------------------------------------------------------------------------------------------
XL_FILLERS, XL_LEN, XL_M, XL_READS = 2280, 1000000, 20, 67   # 67 reads: 3 unalignable, 64 alignable (tools/gen_temp.cpp)


def _write_xl(small, big):
    """The inputs of `small` (20 transcripts of ~1 Mbase, 64 alignable reads) behind XL_FILLERS transcripts of 1 Mbase that no read
    aligns to -- one random block, rotated per transcript: ref.seq / ref.ti / ref.grp rewritten, the ids of s.dat shifted, the read
    files and parameters as they are."""
    os.makedirs(os.path.join(big, "temp"))
    os.makedirs(os.path.join(big, "stat"))
    M = XL_FILLERS + XL_M
    block = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, XL_LEN)].tobytes()
    masks = " ".join(["0"] * ((XL_LEN - 1) // 32 + 1)) + "\n"
    with open(os.path.join(big, "ref.seq"), "wb") as fs, open(os.path.join(big, "ref.ti"), "w") as ft:
        ft.write("%d 1\n" % M)
        for i in range(1, XL_FILLERS + 1):
            r = (i * 7919) % XL_LEN
            fs.write(b"%d %d\nf%d\n" % (XL_LEN, XL_LEN, i))
            fs.write(block[r:])
            fs.write(block[:r])
            fs.write(b"\n" + masks.encode())
            ft.write("f%d\nfg%d\nf%d\n+ %d\n1 1 %d\n\n" % (i, i, i, XL_LEN, XL_LEN))
        with open(os.path.join(small, "ref.seq"), "rb") as f:
            shutil.copyfileobj(f, fs)
        with open(os.path.join(small, "ref.ti")) as f:
            assert f.readline().split() == [str(XL_M), "1"]
            shutil.copyfileobj(f, ft)
    with open(os.path.join(small, "ref.grp")) as f, open(os.path.join(big, "ref.grp"), "w") as g:
        g.write("".join("%d\n" % i for i in range(1, XL_FILLERS + 1)))
        g.write("".join("%d\n" % (int(x) + XL_FILLERS) for x in f.read().split()))
    with open(os.path.join(small, "temp", "s.dat")) as f, open(os.path.join(big, "temp", "s.dat"), "w") as g:
        g.write(f.readline())
        for line in f:
            t = line.split()
            k = int(t[0])
            w = (len(t) - 1) // k
            for j in range(1, len(t), w):
                v = int(t[j])
                t[j] = str(v + XL_FILLERS if v > 0 else v - XL_FILLERS)
            g.write(" ".join(t) + "\n")
    for sub in ("temp", "stat"):
        for name in os.listdir(os.path.join(small, sub)):
            if name != "s.dat":
                shutil.copy(os.path.join(small, sub, name), os.path.join(big, sub, name))


@pytest.mark.skipif(not os.environ.get("RSEM_TEST_XL"), reason="writes 2.3 GB of reference, needs ~12 GB of host memory and 6 GB of HBM: set RSEM_TEST_XL=1")
def test_reference_of_more_than_4_gib_of_strands(tmp_path_factory):
    """2 300 transcripts of 1 Mbase: 4.6 GB on both strands, no pad.  64 reads on the last 20 transcripts; the program must finish
    (before the wide path rsem_model_create refused such a reference) and give the .ofg values of the same reads run against a
    reference that holds only those 20 transcripts (rtol 1e-6)."""
    if not (mc.have_tools(need_ref=False) and os.path.exists(os.path.join(BIN, "rsem-run-em"))):
        pytest.skip("generator not built")
    assert not _STOP, "not started: " + _STOP[0]
    case = dict(rt=3, n=XL_READS, M=XL_M, L=75, iso="2-9", opts=["--gene-len", "%d-%d" % (XL_LEN, XL_LEN)])
    small = str(tmp_path_factory.mktemp("xl_small"))
    big = os.path.join(str(tmp_path_factory.mktemp("xl_big")), "d")
    mc.generate(case, small)
    _write_xl(small, big)
    _, tot = rf.read_seq_lens(os.path.join(small, "ref.seq"))
    strand_bytes = strand_layout(tot)[1] + 2 * XL_FILLERS * XL_LEN
    assert strand_bytes + 16 >= 1 << 32
    out_small = _run_dropin(case, small, [], {})
    assert "model: window addresses of" not in out_small
    out_big = _run_dropin(case, big, [], {}, timeout=1500)
    said = [LINE.match(l) for l in out_big.split("\n") if l.startswith("model: window addresses of")]
    assert len(said) == 1 and said[0] and int(said[0].group(1)) > 32 and int(said[0].group(2)) == strand_bytes, out_big[-2000:]
    M, N0, rp, sid, val = _read_ofg_fast(os.path.join(big, "temp", "s.ofg"))
    gM, gN0, grp, gsid, gval = _read_ofg_fast(os.path.join(small, "temp", "s.ofg"))
    assert (M, N0) == (gM + XL_FILLERS, gN0) and np.array_equal(rp, grp) and np.array_equal(sid, np.where(gsid > 0, gsid + XL_FILLERS, gsid))
    print("XL: strands %d bytes, %d .ofg values, max rel deviation from the 20-transcript run %.3g" % (strand_bytes, len(val), _max_rel(val, gval)))
    assert np.allclose(val, gval, rtol=1e-6, atol=0)
    shutil.rmtree(os.path.dirname(big), ignore_errors=True)
    shutil.rmtree(small, ignore_errors=True)
