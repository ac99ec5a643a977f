"""Gibbs convergence diagnostics without a GPU: the numpy restatement of the definition (tests/diag_ref.py) against the theory of
AR(1) series, and tests/gibbs_diag_check.cpp -- the arithmetic the device runs (rsem_amd/csrc/gibbs_diag_math.hpp: int64 sums of
shifted values, a handful of double operations), built with AddressSanitizer and UBSan -- against the restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import diag_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++")


def write_input(path, cvs):
    with open(path, "wb") as f:
        f.write(np.array([cvs[0].shape[1], len(cvs)] + [a.shape[0] for a in cvs], np.int32).tobytes())
        for a in cvs:
            f.write(np.ascontiguousarray(a, np.int32).tobytes())


@pytest.mark.parametrize("phi", [0.0, 0.5])
def test_ref_on_ar1_series(phi):
    rng = np.random.default_rng(100 + int(phi * 10))
    cvs = [dr.ar1_counts(rng, phi, ns, 40, 1000.0, 100.0) for ns in (250, 251, 252, 253)]
    r = dr.diag_ref(cvs)
    S = 1000
    theory = S * (1 - phi) / (1 + phi)
    assert r["n_used"] == 250 and r["sequences"] == 8
    assert (r["ess"] > theory / 2).all() and (r["ess"] < theory * 2).all(), (r["ess"].min(), r["ess"].max(), theory)
    if phi == 0.0:
        assert (r["rhat"] < 1.02).all(), r["rhat"].max()


def test_ref_special_columns():
    r = dr.diag_ref(dr.synthetic())
    assert np.isnan(r["rhat"][5]) and np.isnan(r["ess"][5]) and r["lag"][5] == 0 and r["sd"][5] == 0 and r["mean"][5] == 1000
    assert np.isposinf(r["rhat"][6]) and np.isnan(r["ess"][6]) and r["lag"][6] == 0
    assert r["n_used"] == 20 and r["sequences"] == 6
    assert r["tie"] >= 1e-7


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if CXX is None:
        pytest.skip("needs g++")
    exe = os.path.join(str(tmp_path_factory.mktemp("gibbs_diag_check")), "gibbs_diag_check")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "gibbs_diag_check.cpp"), "-o", exe])
    return exe


def run_checker(checker, path, L0):
    out = subprocess.run([checker, path, str(L0)], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.strip().split("\n")]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return dict(mean=np.array([float(r[1]) for r in rows]), sd=np.array([float(r[2]) for r in rows]),
                rhat=np.array([float(r[3]) for r in rows]), ess=np.array([float(r[4]) for r in rows]),
                lag=np.array([int(r[5]) for r in rows], np.int32), long=np.array([int(r[6]) for r in rows], bool))


INPUTS = {"synthetic": lambda: dr.synthetic(), "one_chain_of_4": lambda: dr.synthetic(nsamples=(4,)),
          "counts_5e7": lambda: dr.synthetic(centre=5e7, sd=300.0)}


@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("L0", [1, 3, 63])
def test_check_program_against_ref(checker, tmp_path, name, L0):
    cvs = INPUTS[name]()
    ref = dr.diag_ref(cvs)
    assert ref["tie"] >= 1e-7, ref["tie"]  # a condition on the input: no decision of Geyer's rule sits on a tie
    path = os.path.join(str(tmp_path), "in.bin")
    write_input(path, cvs)
    got = run_checker(checker, path, L0)
    dr.compare(got, ref, (name, L0))
    assert np.array_equal(got["long"], ref["lag"] > L0)


def test_long_path_set_at_L0_3(checker, tmp_path):
    cvs = dr.synthetic()
    ref = dr.diag_ref(cvs)
    path = os.path.join(str(tmp_path), "in.bin")
    write_input(path, cvs)
    got = run_checker(checker, path, 3)
    assert got["long"].any()
    assert np.array_equal(np.nonzero(got["long"])[0], np.nonzero(ref["lag"] > 3)[0])


def test_check_program_refuses_short_chains(checker, tmp_path):
    path = os.path.join(str(tmp_path), "in.bin")
    write_input(path, dr.synthetic(nsamples=(3, 9)))
    assert subprocess.run([checker, path, "3"], capture_output=True).returncode == 3
