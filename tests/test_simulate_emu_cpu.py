"""The attempt of rsem-simulate-reads and the search for the attempts a stream of generator words holds
(rsem_amd/csrc/simulate_block.hpp -- the file simulate.hip compiles for the GPU) run on the CPU by tests/simulate_emu.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, over the tables the program's own host code
(rsem_amd/csrc/host/simulate_host.hpp) builds from recorded inputs.  Every read, its failed attempts, the counts and the resimulation
total must be the restatement's (tests/simulate_ref.py), draw for draw: on the reference's MT19937 stream, searched in chunks and
tiles small enough that chunks end inside reads and tiles hold single attempts, and on the Philox counter stream.  No GPU and no
Python process takes part in the sanitizer run."""
import os
import shutil
import subprocess

import pytest

import simulate_cases as sc
import simulate_ref as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="needs hipcc (the block header includes rng.hpp)")

# a quality model with failed attempts at the header, a paired one whose quality chain takes second uniforms (not plain), one without qualities
CASES = ["se_q_fragmean_short", "pe_q_zero_quality_row", "pe_noq_theta0_large", "pe_q_polya_rspd_zero_bins"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("simulate_emu")), "simulate_emu")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "simulate_emu.cpp"), "-o", exe, "-fsanitize=address,undefined"],
                          stdout=subprocess.DEVNULL)
    return exe


def _case(name):
    d, a = sc.case_args(name)
    return d, float(a[3]), int(a[4]), int(a[7])


_want = {}


def _restatement(name, stream, n):
    """computed once per (case, stream): the tests only read it"""
    key = (name, stream, n)
    if key not in _want:
        d, theta0, _, seed = _case(name)
        src = sim.Mt19937Source(seed) if stream == "reference" else sim.PhiloxSource(seed)
        _, _, r = sim.run_program(os.path.join(d, "ref"), os.path.join(d, "sim.model"), os.path.join(d, "sim.results"), theta0, n, src)
        _want[key] = sim.dump(r["reads"], r["counts"], r["resim"])
    return _want[key]


def _run(emu, name, stream, n, chunk, tile, tmp_path):
    d, theta0, _, seed = _case(name)
    out = os.path.join(str(tmp_path), "out.txt")
    r = subprocess.run([emu, "ref", "sim.model", "sim.results", repr(theta0), str(n), str(seed), stream, str(chunk), str(tile), out], cwd=d, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out, encoding="latin-1") as f:
        return f.read()


@pytest.mark.parametrize("chunk,tile", [(1 << 20, 2048), (1000, 64), (624, 7), (97, 1)])
@pytest.mark.parametrize("name", CASES)
def test_reference_stream_search_finds_the_reference_reads(emu, name, chunk, tile, tmp_path):
    n = 60
    assert _run(emu, name, "reference", n, chunk, tile, tmp_path) == _restatement(name, "reference", n)


@pytest.mark.parametrize("n", range(1, 61))
def test_resimulation_total_ends_with_the_last_read(emu, n, tmp_path):
    """Chunks about as long as one read's attempts (97 positions; a read of this case takes 75 to 105 uniforms and has failed attempts
    of 2 to 4 before it): for some N the last chunk holds failed attempts BEHIND read N.  They belong to a read the run never draws and
    are in no total: the reads, their failed attempts and the resimulation line are those of the first N reads of the restatement."""
    name = "se_q_fragmean_short"
    assert _run(emu, name, "reference", n, 97, 8, tmp_path) == _restatement(name, "reference", n)


# (pe_q_zero_quality_row's seed was sought for the MT19937 stream: on other draws its empty row soon gives a quality above 93, where
# both sides stop; se_q_repaired_rows has rows without mass, too)
@pytest.mark.parametrize("name", [c for c in CASES if c != "pe_q_zero_quality_row"] + ["se_q_repaired_rows"])
def test_counter_stream_is_the_philox_replay(emu, name, tmp_path):
    n = 40
    assert _run(emu, name, "counter", n, 1, 1, tmp_path) == _restatement(name, "counter", n)
