"""tools/gen_temp.cpp without a GPU: (1) with none of its named options its files are byte for byte those of the generator before
the options existed (bench.py times runs on this data) -- sha256 sums recorded from that binary, for 1 and 16 host threads;
(2) every case of model_path_cases.py generates, meets the conditions of the path it is named after, does not depend on the
number of threads, and -- where oracle/_ref is built -- the reference binary accepts it and finishes."""
import hashlib
import os

import numpy as np
import pytest

import model_path_cases as mc
import rsem_files as rf

# gen_temp <dir> 40000 300 <read_type> 20250925 100 nosam 6-20 (the argv of bench.py's generate(), smaller): three tasks of reads
PARENT_SUMS = {
    1: {
        "ref.grp": "abdae108cc547e63cbc413d4c9054d5d9234bbbcc644adfa6f0151b02f6142c7",
        "ref.seq": "a13e0a0e813ecbdb4741875684ba961865a4318e5b29ad486882fbc6525e6808",
        "ref.ti": "ac2691d9caf3338684a19231e66d989555168924209e786abbb99a924f213d83",
        "stat/s.cnt": "73f9fc7410d831ddd0b254b93bf4ce6e8a071575f27fb87cb661e2159404908e",
        "temp/s.dat": "70dafd5c85b22f9a568ac91e4d9a2c64d13988bdc4dd0050151c16837ef442d9",
        "temp/s.mparams": "ea7c93d38ffa3fe8a8b640ccda7fc6579042d3079c55ba302d4287ec28951b56",
        "temp/s.omit": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "temp/s_alignable.fq": "a3d2433145aa8b235a96b70fd296b1ede3da8636449ad635a68d1fc9a58050f1",
        "temp/s_un.fq": "707732e5684c711b668ae4fc58e0e98d468efee2e5a74b27cce79a2484815e5f",
    },
    3: {
        "ref.grp": "abdae108cc547e63cbc413d4c9054d5d9234bbbcc644adfa6f0151b02f6142c7",
        "ref.seq": "a13e0a0e813ecbdb4741875684ba961865a4318e5b29ad486882fbc6525e6808",
        "ref.ti": "ac2691d9caf3338684a19231e66d989555168924209e786abbb99a924f213d83",
        "stat/s.cnt": "927af00ad1e89c163579126444fdc4b3bc56dde2591b96ee19af2ab2d96d321f",
        "temp/s.dat": "c5b0cf125633353112e2b85c375305c99758585fd72ac32d62a82d2cdafd2d39",
        "temp/s.mparams": "ea7c93d38ffa3fe8a8b640ccda7fc6579042d3079c55ba302d4287ec28951b56",
        "temp/s.omit": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "temp/s_alignable_1.fq": "f7ff171de809e92b1262691f78afc2f99de5ca2b930425f3b25d8bd250fe377b",
        "temp/s_alignable_2.fq": "f4cf798795568900cce7c42940c3e3ced62bc14c13399dcc8601d4ab81dd9dbe",
        "temp/s_un_1.fq": "4e2d23c0fe56bcb5873ffe1890eb80e66d608b92081c9dc963d49289f7c8909d",
        "temp/s_un_2.fq": "a3ab4dae9a68704dc4776b73e0328f3af09209a71edbc1b640520374441ea51f",
    },
}


def _sums(root):
    out = {}
    for dp, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dp, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = hashlib.sha256(fh.read()).hexdigest()
    return out


@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("read_type", [1, 3])
def test_default_output_is_the_parent_generators(read_type, threads, tmp_path):
    if not mc.have_tools(need_ref=False):
        pytest.skip("tools/bin/gen_temp not built")
    d = str(tmp_path)
    mc.run([mc.GEN, d, "40000", "300", str(read_type), "20250925", "100", "nosam", "6-20", "--threads", str(threads)], 120)
    assert _sums(d) == PARENT_SUMS[read_type]


def test_bad_options_are_refused(tmp_path):
    if not mc.have_tools(need_ref=False):
        pytest.skip("tools/bin/gen_temp not built")
    import subprocess
    for bad in (["--len", "80-70"], ["--no-such", "1"], ["--probF"], ["--len", "300-400", "--frag-range", "1-200"], ["--omit", "100"]):
        r = subprocess.run([mc.GEN, str(tmp_path), "1000", "100", "1", "7", "75", "nosam", "2-9"] + bad, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 1, bad


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_is_on_its_path_and_the_reference_accepts_it(name, tmp_path):
    if not mc.have_tools(need_ref=False):
        pytest.skip("tools/bin/gen_temp not built")
    case = mc.CASES[name]
    d, d1 = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    mc.generate(case, d)
    mc.generate(case, d1, threads=1)
    assert _sums(d) == _sums(d1)
    P = mc.parse_inputs(case, d)
    mc.assert_path(name, P)
    if not mc.have_tools():
        return  # (no reference binaries on this machine: the conditions above are what can be checked)
    log = mc.run_reference(case, d)
    rounds = [l for l in log.split("\n") if l.startswith("ROUND")]
    assert len(rounds) >= 20 and int(rounds[-1].split(",")[0].split("=")[1]) == len(rounds)
    raw, pol = rf.read_theta(os.path.join(d, "stat", "s.theta"))
    assert len(raw) == case["M"] + 1 and abs(raw.sum() - 1.0) < 1e-6 and np.isfinite(raw).all() and raw[1:].max() > 0
    # omitted transcripts get nothing; low-quality reads leave the sum of the counts (SUM of the ROUND line)
    assert (raw[P["omit"]] == 0).all()
    n_lq = int(np.count_nonzero(P["minlen"] < mc.SEED_LEN))
    total = float(rounds[-1].replace(",", "").split()[5])
    assert abs(total - (case["n"] - n_lq)) < 1e-3 * case["n"] + 2.0, (total, n_lq)
    M, N0, rp, sid, val = rf.read_ofg(os.path.join(d, "temp", "s.ofg")) if P["nal"].sum() < 1_000_000 else (case["M"], case["n"] // 20, None, None, None)
    assert (M, N0) == (case["M"], case["n"] // 20)
    if rp is not None:
        # a row holds the noise column and the read's alignments, less those of probability 0 (EM.cpp:435-457)
        # -- and low-quality reads have no row at all
        n_row = np.diff(rp.astype(np.int64))
        keep = P["minlen"] >= mc.SEED_LEN
        assert len(n_row) == int(keep.sum()) and (n_row <= P["nal"][keep] + 1).all() and (n_row >= 1).all() and (sid <= case["M"]).all()
        mc.assert_path_ofg(name, (M, N0, rp, sid, val))
