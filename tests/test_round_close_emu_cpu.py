"""The closer of an EM round (rsem_amd/csrc/round_close.hpp: slice walk, statistics, workgroup reduction, arrival and the last
arrival's publication) run on the CPU by tests/round_close_emu.cpp -- 256 OS threads as one workgroup, the closers of a round
one after another in shuffled orders of arrival -- against the reference's lines (EM.cpp:400-416) written out serially there.
The emulator has ONE workgroup: this checks the protocol's logic, not its concurrency.

Per case and order: three consecutive rounds on one Ctrl; totNum equal, bChange and the sum bit for bit (the sum the same under
every order), the stop rule, the host's line in its ring entry, bbits / tick2 left clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(CC), reason="needs hipcc (host compilation of the HIP headers)")

BUILDS = {"product": [], "tsan": ["-fsanitize=thread", "-fno-gpu-sanitize", "-g"]}
N_ORDERS = 20


@pytest.fixture(scope="module")
def emulators(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("round_close_emu"))
    procs = {}
    for name, defs in BUILDS.items():
        exe = os.path.join(d, "round_close_emu_" + name)
        procs[name] = (exe, subprocess.Popen([CC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value"] + defs +
                                             [os.path.join(ROOT, "tests", "round_close_emu.cpp"), "-o", exe, "-lpthread"],
                                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        err = p.communicate()[1]
        assert p.returncode == 0 or name == "tsan", err[-3000:]
        out[name] = exe if p.returncode == 0 else None
    return out


def _run(exe, mode, n_closers, n_orders):
    p = subprocess.run([exe, mode, str(n_closers), str(n_orders)], capture_output=True, text=True, timeout=3000)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "BAD" not in p.stdout, p.stderr[-2000:]
    return [ln for ln in p.stdout.splitlines() if ln.startswith("n ")]


@pytest.mark.parametrize("n_closers", [1, 3, 64, 128])
def test_slice_lengths(emulators, n_closers):
    """n = M + 1 in {1, 5, 127, 128, 129, 2048 n_closers, 2048 n_closers + 1}: empty slices (lo >= hi), a short last slice, the
    prefetch path at its limit and the stride path one element past it."""
    lines = _run(emulators["product"], "slices", n_closers, N_ORDERS)
    assert [int(ln.split()[1]) for ln in lines] == [1, 5, 127, 128, 129, 2048 * n_closers, 2048 * n_closers + 1]


@pytest.mark.parametrize("n_closers", [1, 3])
def test_threshold_edges(emulators, n_closers):
    """Elements with old exactly 1e-7 and just below, change exactly 0.001 and just below, old = 0."""
    assert len(_run(emulators["product"], "edges", n_closers, N_ORDERS)) == 1


def test_no_unordered_accesses(emulators, monkeypatch):
    """The same under ThreadSanitizer, as a stand-alone program (a report makes the emulator exit with 66)."""
    if emulators["tsan"] is None:
        pytest.skip("no ThreadSanitizer build with this toolchain")
    monkeypatch.setenv("TSAN_OPTIONS", "halt_on_error=0 exitcode=66")
    _run(emulators["tsan"], "edges", 3, 3)
