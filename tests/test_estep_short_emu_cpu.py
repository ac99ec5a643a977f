"""The short classes of the sliced layout (rsem_amd/csrc/sell_shape.hpp, Shape::cut: reads whose last value plane is a quarter
or more empty are sorted into shapes that store that plane compacted) checked on the CPU by tests/estep_short_emu.cpp:
the class table and the index helpers for every read length, the planes read back against the CSR, and the kernel body
(estep_block.hpp, one OS thread per lane) on layouts with the classes on -- against the oracle's E step at 1e-9 and, where
every transcript id belongs to one alignment alone (each count is then ONE product, whatever the order of the additions),
bit for bit against the same body on the layout with the classes off."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import aligner_like as al
from oracle import pyoracle as orc
from tools.q32_ref import quantize_q32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(CC), reason="needs hipcc (host compilation of the HIP headers)")

BUILDS = {"product": [], "tsan": ["-fsanitize=thread", "-fno-gpu-sanitize", "-g"]}
# the 30 classes of a format: lg = 1: q = 2; lg = 2 .. 6: q = 1, 2, 3; K = 3 and 4  (as (lg, K, cut = 4 - q))
ALL_CLASSES = {(1, K, 2) for K in (3, 4)} | {(lg, K, 4 - q) for lg in range(2, 7) for K in (3, 4) for q in (1, 2, 3)}


@pytest.fixture(scope="module")
def emulators(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("estep_short_emu"))
    procs = {}
    for name, defs in BUILDS.items():
        exe = os.path.join(d, "estep_short_emu_" + name)
        procs[name] = (exe, subprocess.Popen([CC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value"] + defs +
                                             [os.path.join(ROOT, "tests", "estep_short_emu.cpp"), "-o", exe, "-lpthread"],
                                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        err = p.communicate()[1]
        assert p.returncode == 0 or name == "tsan", err[-3000:]
        out[name] = exe if p.returncode == 0 else None
    return out


def test_class_table_and_index_helpers(emulators):
    """Every length 1..256: the chosen (lg, K, q), the lanes kept in the last plane, entries >= L; every alignment of every row
    slot has an entry of its own inside the slice's stride; ids 0..83 decode as before."""
    p = subprocess.run([emulators["product"], "--table"], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "BAD" not in p.stdout
    rows = [tuple(int(v) for v in ln.split()) for ln in p.stdout.splitlines() if len(ln.split()) == 7]
    assert [r[0] for r in rows] == list(range(1, 257))
    total = 0
    for L, lg, K, q, cut, Gk, entries in rows:
        G = 1 << lg
        assert entries >= L and q == 4 - cut and Gk == G * q // 4 and entries == (K - 1) * G + Gk
        assert K == (L if L <= 4 else -(-L // G)) and (lg == 0 or (K - 1) * G < L <= K * G)
        assert entries - L < max(1, G // 4)            # less than a quarter of a lane group is left empty
        if G <= 4:
            assert entries == L                        # exact
        total += entries
    # on average under an eighth of a lane group is empty, and a read of G lanes has more than 2 G alignments: < 1 / 16 over
    # uniform lengths (the full layout: 1.17)
    assert total / sum(range(1, 257)) < 1 + 1 / 16


def _lens_data(lens, M, seed, unique, aligner_like=False):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    rows = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(nnz) - rp[:-1].astype(np.int64)[rows]
    if unique:
        assert nnz <= M
        sid = (rng.permutation(M)[:nnz] + 1).astype(np.int32)
    else:
        start = (rng.integers(1, M - 256, len(lens)) // 40) * 40 + 1   # few distinct tuples per length: runs of identical tuples
        sid = (start[rows] + within).astype(np.int32)
    cp = np.power(10.0, rng.uniform(-30, -3, len(lens)))[rows] * np.power(2.0, rng.uniform(-6, 0, nnz))
    ncp = np.power(10.0, rng.uniform(-20, -3, len(lens)))
    theta = rng.random(M + 1)
    theta[rng.random(M + 1) < 0.1] = 1e-310   # theta * conprb under the 1e-300 clamp
    theta[0] = 0.3
    theta /= theta.sum()
    if aligner_like:   # repeated ids, ids out of order (tests/aligner_like.py)
        sid = al.aligner_like(rp, sid, seed + 100)
        al.assert_on_path(al.describe(rp, sid), repeat=0.05, all_same=0.05, not_ascending=0.05, same_plane=0.05, same_lane=0.05)
    return M, rp, sid, cp, ncp, theta


def _run(exe, M, rp, sid, cp, ncp, theta, T=4, min_units=-1, q32=0, range_bits=8):
    d = tempfile.mkdtemp()
    try:
        inp, outp = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([M, len(rp) - 1, T, min_units, q32, range_bits, 0, 0], np.int32).tobytes())
            f.write(np.array([0.0], np.float64).tobytes())
            for a, t in ((rp, np.uint64), (sid, np.int32), (cp, np.float64), (ncp, np.float64), (theta, np.float64)):
                f.write(np.ascontiguousarray(a, t).tobytes())
        p = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        out = np.fromfile(outp, np.float64)
        info = {"shapes": [], "roundtrip": None}
        for ln in p.stdout.splitlines():
            w = ln.split()
            if w[0] == "shape":
                info["shapes"].append(tuple(int(v) for v in w[1:]))   # fmt lg K cut rows
            elif w[0] == "entries":
                info["entries"] = int(w[1])
            elif w[0] == "mask":
                info["mask"] = int(w[1], 16)
            elif w[0] == "roundtrip":
                info["roundtrip"] = w[1]
        return out[:M + 1], out[M + 1], out[M + 2], info
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _mixed(seed, maxlen=60, n=3000, aligner_like=False):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.arange(1, 257), rng.integers(1, maxlen, n)])  # every length once (thin classes), then a bulk (thick ones)
    rng.shuffle(lens)
    return _lens_data(lens, 2000, seed, unique=False, aligner_like=aligner_like)


def _against_oracle(exe, seed, aligner_like=False, **kw):
    M, rp, sid, cp, ncp, theta = _mixed(seed, aligner_like=aligner_like)
    vals = quantize_q32(rp, cp, kw.get("range_bits", 8))[0] if kw.get("q32") else cp
    oc = orc.em_estep(M, rp, sid, vals, ncp, theta)
    counts, noise, neff, info = _run(exe, M, rp, sid, cp, ncp, theta, **kw)
    assert neff == len(rp) - 1
    assert np.allclose(counts[1:], oc[1:], rtol=1e-9, atol=0.0), kw
    assert abs(noise - oc[0]) <= 1e-9 * oc[0], kw
    assert info["roundtrip"] == "ok"
    return info, int(rp[-1])


def test_every_class_against_the_oracle(emulators):
    """Every (lg, K, q) present (every length 1..256 is: the reads whose last plane is exactly full keep the full shape beside
    them), F64."""
    info, nnz = _against_oracle(emulators["product"], 1, min_units=-1)
    got = {(lg, K, cut) for fmt, lg, K, cut, rows in info["shapes"] if fmt == 0 and cut}
    assert got == ALL_CLASSES
    full = {(lg, K) for fmt, lg, K, cut, rows in info["shapes"] if fmt == 0 and cut == 0}
    assert full == {(lg, K) for lg in range(0, 7) for K in range(1, 5) if lg == 0 or K >= 3}
    off = _run(emulators["product"], *_mixed(1), min_units=0)[3]
    assert not any(s[3] for s in off["shapes"]) and off["mask"] == 0
    assert info["entries"] < off["entries"] and info["entries"] < 1.05 * nnz + 64 * 4 * len(info["shapes"])


@pytest.mark.parametrize("q32", [0, 1], ids=["f64", "q32"])
def test_every_class_on_aligner_like_input(emulators, q32):
    """The classes on, every length 1..256, on reads with repeated ids and ids out of order: a compacted last plane holds a copy of an id
    of an earlier plane, or of another lane of its own."""
    info, _ = _against_oracle(emulators["product"], 1, aligner_like=True, min_units=-1, q32=q32)
    assert any(fmt == q32 and cut for fmt, lg, K, cut, rows in info["shapes"])


def test_thin_classes_fold_back(emulators):
    """With a threshold of one unit of 4 x 2 slices: the bulk (lengths < 60, some 50 reads each) fills the classes of 8 and 16
    lanes per read; of 2 and 4 lanes per read 32 / 16 reads go into a slice and a class gets 50 / 100 reads, of 32 lanes per
    read the once-each lengths give a class 8 reads = 4 slices: these keep the full shape of their (lg, K).  (64 lanes per
    read: 16 reads = 16 slices, taken.)"""
    info, _ = _against_oracle(emulators["product"], 2, min_units=1, T=2)
    got = {(lg, K, cut) for fmt, lg, K, cut, rows in info["shapes"] if cut}
    assert got == {c for c in ALL_CLASSES if c[0] in (3, 4, 6)}
    by_shape = {(lg, K): rows for fmt, lg, K, cut, rows in info["shapes"] if cut == 0}
    assert by_shape[(5, 3)] == 32 and by_shape[(5, 4)] == 32   # every length 65..96 / 97..128 once: all folded back
    assert sum(s[4] for s in info["shapes"]) == 256 + 3000


@pytest.mark.parametrize("kw", [dict(q32=1, min_units=-1), dict(q32=1, range_bits=24, min_units=1, T=3)], ids=["all", "threshold"])
def test_q32_classes_against_the_oracle(emulators, kw):
    info, _ = _against_oracle(emulators["product"], 3, **kw)
    assert any(fmt == 1 and cut for fmt, lg, K, cut, rows in info["shapes"])
    if kw["min_units"] < 0:  # (Q32 rounds the quarters up to 2 or 4: a stride of whole 128-byte lines)
        assert {(lg, K, cut) for fmt, lg, K, cut, rows in info["shapes"] if fmt == 1 and cut} == {c for c in ALL_CLASSES if c[2] == 2}


BITWISE = [list(range(1, 63)),                                                        # lg 0..3 whole, lg 4 nearly
           [63, 64, 65, 72, 73, 80, 81, 88, 89, 96, 97, 104, 105, 112, 113, 121, 128],  # lg 5: both ends of every class
           [129, 144, 145, 161, 177, 193, 209, 225, 241, 256]]                      # lg 6


@pytest.mark.parametrize("lens", BITWISE, ids=["lg0-4", "lg5", "lg6"])
@pytest.mark.parametrize("q32", [0, 1])
def test_bit_for_bit_against_the_full_layout(emulators, lens, q32):
    """Every transcript id belongs to one alignment: a count is one fraction f * (1 / normaliser), added to zero.  The per-read
    arithmetic -- the products, the butterfly over the read's lanes, the reciprocal -- is the same additions in the same order
    with the last plane compacted or not, so the counts are the same BITS."""
    data = _lens_data(lens, 2040, 11 + len(lens), unique=True)
    on = _run(emulators["product"], *data, T=1, min_units=-1, q32=q32)
    off = _run(emulators["product"], *data, T=1, min_units=0, q32=q32)
    assert any(s[3] for s in on[3]["shapes"]) and not any(s[3] for s in off[3]["shapes"])
    # (one read per class, a slice each: here the classes cost entries -- what the threshold is for)
    assert np.array_equal(on[0][1:].view(np.uint64), off[0][1:].view(np.uint64))
    assert on[2] == off[2] == len(lens)
    assert abs(on[1] - off[1]) <= 1e-12 * abs(off[1])   # (the noise total is a sum over all reads: its order is the layout's)
    vals = quantize_q32(data[1], data[3], 8)[0] if q32 else data[3]
    oc = orc.em_estep(data[0], data[1], data[2], vals, data[4], data[5])
    assert np.allclose(on[0][1:], oc[1:], rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("kw", [dict(min_units=-1, T=1), dict(min_units=1, T=2, q32=1), dict(min_units=-1, T=1, aligner_like=True)],
                         ids=["f64-all", "q32-threshold", "f64-all-aligner_like"])
def test_no_unordered_accesses_between_lanes(emulators, kw, monkeypatch):
    """The kernel body on the short classes under ThreadSanitizer (a report makes the emulator exit with 66)."""
    if emulators["tsan"] is None:
        pytest.skip("no ThreadSanitizer build with this toolchain")
    monkeypatch.setenv("TSAN_OPTIONS", "halt_on_error=0 exitcode=66")
    rng = np.random.default_rng(5)
    lens = np.concatenate([np.arange(5, 257, 3), rng.integers(1, 40, 400)])
    kw = dict(kw)
    M, rp, sid, cp, ncp, theta = _lens_data(lens, 2000, 5, unique=False, aligner_like=kw.pop("aligner_like", False))
    vals = quantize_q32(rp, cp, 8)[0] if kw.get("q32") else cp
    oc = orc.em_estep(M, rp, sid, vals, ncp, theta)
    counts, noise, neff, info = _run(emulators["tsan"], M, rp, sid, cp, ncp, theta, **kw)
    assert np.allclose(counts[1:], oc[1:], rtol=1e-9, atol=0.0)
