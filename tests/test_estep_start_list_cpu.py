"""The start list of the sliced layout (rsem_amd/csrc/sell_layout.hpp: per marked slice the ids of the lanes that start a tuple,
K * popcount(mask) entries, and the exclusive sums that say where each slice's entries begin) and the kernel body reading a new
tuple's ids from it (rsem_amd/csrc/estep_block.hpp issue()), on the CPU by tests/estep_start_emu.cpp: the list's contents against
the id planes for every marked slice, lane and plane; the loop with the list against the oracle's E step at 1e-9 and, where every
transcript id belongs to one alignment alone (each count is then ONE product, whatever the order of the additions), bit for bit
against the loop with the planes on the same layout."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import aligner_like as al
from oracle import pyoracle as orc
from tools.q32_ref import quantize_q32
from tools.synth_data import make_em_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(CC), reason="needs hipcc (host compilation of the HIP headers)")

RING = ["-DRSEM_F64_DEPTHS=3,3,3,3", "-DRSEM_Q32_DEPTHS=3,3,3,3"]   # the ring loop: the last slice of a block is issued again
BUILDS = {"product": ["-O1"], "fast": ["-O2"], "ring": ["-O1"] + RING, "tsan": ["-O1", "-fsanitize=thread", "-fno-gpu-sanitize", "-g"]}


@pytest.fixture(scope="module")
def emulators(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("estep_start_emu"))
    procs = {}
    for name, defs in BUILDS.items():
        exe = os.path.join(d, "estep_start_emu_" + name)
        procs[name] = (exe, subprocess.Popen([CC, "--offload-arch=gfx950", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value"] + defs +
                                             [os.path.join(ROOT, "tests", "estep_start_emu.cpp"), "-o", exe, "-lpthread"],
                                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        err = p.communicate()[1]
        assert p.returncode == 0 or name == "tsan", err[-3000:]
        out[name] = exe if p.returncode == 0 else None
    return out


def _lens_data(lens, M, seed, unique, per_tuple=40, aligner_like=False):
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
        start = (rng.integers(1, M - 256, len(lens)) // per_tuple) * per_tuple + 1   # few distinct tuples per length: runs of identical tuples
        sid = (start[rows] + within).astype(np.int32)
    cp = np.power(10.0, rng.uniform(-30, -3, len(lens)))[rows] * np.power(2.0, rng.uniform(-6, 0, nnz))
    ncp = np.power(10.0, rng.uniform(-20, -3, len(lens)))
    theta = rng.random(M + 1)
    theta[rng.random(M + 1) < 0.1] = 1e-310   # theta * conprb under the 1e-300 clamp
    theta[0] = 0.3
    theta /= theta.sum()
    if aligner_like:   # repeated ids, ids out of order (tests/aligner_like.py): tuples that differ in a later plane only
        sid = al.aligner_like(rp, sid, seed + 100)
        al.assert_on_path(al.describe(rp, sid), repeat=0.05, all_same=0.05, not_ascending=0.05, same_plane=0.05, same_lane=0.05)
    return M, rp, sid, cp, ncp, theta


def _run(exe, M, rp, sid, cp, ncp, theta_in, N0=0.0, T=4, min_units=0, q32=0, range_bits=8, from_counts=0, window=0, policy=0, use_list=1,
         quarter=0, far_queue=1, run=1):
    d = tempfile.mkdtemp()
    try:
        inp, outp = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([M, len(rp) - 1, T, min_units, q32, range_bits, from_counts, window, policy, use_list, quarter, far_queue, run, 0, 0, 0],
                             np.int32).tobytes())
            f.write(np.array([N0], np.float64).tobytes())
            for a, t in ((rp, np.uint64), (sid, np.int32), (cp, np.float64), (ncp, np.float64), (theta_in, np.float64)):
                f.write(np.ascontiguousarray(a, t).tobytes())
        p = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
        info = {}
        for ln in p.stdout.splitlines():
            w = ln.split()
            if len(w) == 2 and w[0] in ("slices", "marked", "entries", "maxn"):
                info[w[0]] = int(w[1])
            if len(w) == 5 and w[0] == "traffic":
                info["traffic"] = tuple(int(v) for v in w[1:])   # first-slice planes, list entries loaded, slices with an offset, far-queue planes
        # (the list entry by entry, and the byte accounting's rule -- sid_traffic_of_wave over the units -- against a slice-by-slice count)
        info["list_ok"] = "list ok" in p.stdout and "traffic ok" in p.stdout and "BAD" not in p.stdout
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
        if not run:
            return None, None, None, info
        out = np.fromfile(outp, np.float64)
        return out[:M + 1], out[M + 1], out[M + 2], info
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- 1. what the list holds -----------------------------------------------------------------------------------------------------------

def _sweep(aligner_like=False):
    """Every row length 1..256, three reads per length, two of them with the same tuple."""
    lens = np.repeat(np.arange(1, 257), 3)
    return _lens_data(lens, 2000, 3, unique=False, aligner_like=aligner_like)


def _workload(name):
    wl = make_em_workload(name, seed=21)
    return wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"], wl["theta0"]


@pytest.mark.parametrize("q32", [0, 1], ids=["f64", "q32"])
@pytest.mark.parametrize("min_units", [0, -1], ids=["full", "short"])
@pytest.mark.parametrize("name", ["sweep", "tiny", "tinyX", "small", "sweep-aligner_like"])
def test_list_holds_the_ids_of_the_lanes_that_start(emulators, name, min_units, q32):
    """For every slice, lane and plane with the mask bit set the list entry is the plane entry, at plane * n + rank from the slice's
    offset; the offsets are the exclusive sums of K * popcount(mask); the total is their sum and nothing is written behind it
    (checked entry by entry in the emulator, which builds the list with start_list_count / start_list_fill_lane)."""
    data = _sweep(name != "sweep") if name.startswith("sweep") else _workload(name)
    T = {"sweep": 3, "sweep-aligner_like": 3, "tiny": 8, "tinyX": 8, "small": 70}[name]
    kw = dict(T=T, min_units=min_units if name != "small" or min_units == 0 else 8, q32=q32, run=0)
    if name == "tinyX":
        kw.update(policy=3, window=64)   # split rows: their planes hold the in-window ids only
    info = _run(emulators["fast"], *data, **kw)[3]
    print(name, kw, info)
    assert info["list_ok"]
    n_blocks_min = -(-info["slices"] // T)
    assert info["marked"] >= n_blocks_min and info["entries"] >= 64 * n_blocks_min   # a block's first slice: every lane starts
    assert info["maxn"] == 64
    if name == "small":   # long blocks of sorted reads: most slices have no start at all
        assert info["marked"] < info["slices"] // 2
    first, listed, with_offset, fq = info["traffic"]
    assert with_offset + 0 == info["slices"] or fq > 0   # every slice outside the far-queue units fetches its offset
    assert listed <= info["entries"] - 64 * n_blocks_min   # a block's first slice is a wave's first: planes, not list
    assert first >= n_blocks_min or fq > 0


@pytest.mark.parametrize("kw", [dict(T=7), dict(T=7, quarter=1), dict(T=1), dict(T=5, window=64, far_queue=1), dict(T=5, window=64, far_queue=0),
                                dict(T=3, policy=3, window=64, far_queue=1)],
                         ids=["full-units", "quarter-units", "T1", "far-queue", "far-no-queue", "split-rows"])
def test_byte_accounting_rule(emulators, kw):
    """sid_traffic_of_wave summed over the waves of every unit -- what `sid_plane_bytes_loaded` is made of -- equals the count made
    slice by slice (checked in the emulator), for whole and quarter-size units, with and without a far-queue launch; and its terms
    behave as the layout says."""
    info = _run(emulators["fast"], *_sweep(), run=0, **kw)[3]
    print(kw, info)
    assert info["list_ok"]
    first, listed, with_offset, fq = info["traffic"]
    if kw.get("far_queue", 1) == 0 or "window" not in kw:
        assert fq == 0 and with_offset == info["slices"]
    else:
        assert fq > 0 and with_offset < info["slices"]
    if kw["T"] == 1:   # every slice is a wave's first: nothing comes from the list
        assert listed == 0 and first >= info["slices"]
    if kw.get("quarter"):   # waves that begin mid-block: more first slices than blocks
        whole = _run(emulators["fast"], *_sweep(), run=0, T=kw["T"])[3]["traffic"]
        assert first > whole[0] and listed < whole[1] and with_offset == whole[2]


# ---- 2. the loop with the list ----------------------------------------------------------------------------------------------------------

def _mixed(seed, n=1200, maxlen=60, M=500, aligner_like=False):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.arange(1, 257), rng.integers(1, maxlen, n)])   # every length once (K = 1..4, lg = 0..6), then a bulk
    rng.shuffle(lens)
    return _lens_data(lens, M, seed, unique=False, aligner_like=aligner_like)


def _from_counts(theta):
    """theta_i = (c_i + [i = 0] (noise + N0)) / (N0 + reads with a non-zero normaliser): the source of the one-launch round"""
    N0 = 37.0
    raw = theta * 1000.0
    tot = np.zeros(128)
    tot[:64] = 0.25 / 64 * 5
    tot[64:] = (1000.0 - N0) / 64
    th = raw.copy()
    th[0] += tot[:64].sum() + N0
    return N0, th / (tot[64:].sum() + N0), np.concatenate([raw, tot])


def _against_oracle(exe, data, **kw):
    M, rp, sid, cp, ncp, theta = data
    vals = quantize_q32(rp, cp, kw.get("range_bits", 8))[0] if kw.get("q32") else cp
    N0, theta_in = 0.0, theta
    if kw.get("from_counts"):
        N0, theta, theta_in = _from_counts(theta)
    oc = orc.em_estep(M, rp, sid, vals, ncp, theta)
    counts, noise, neff, info = _run(exe, M, rp, sid, cp, ncp, theta_in, N0=N0, **kw)
    assert info["list_ok"]
    assert neff == len(rp) - 1
    assert np.allclose(counts[1:], oc[1:], rtol=1e-9, atol=0.0), kw
    assert abs(noise - oc[0]) <= 1e-9 * oc[0], kw
    return info


LOOP_CASES = {
    "plain": dict(),                                          # K = 1..4, lg = 0..6
    "from-counts": dict(from_counts=1),                       # kFC
    "short-classes": dict(min_units=-1, T=3),
    "q32": dict(q32=1),
    "q32-from-counts-short": dict(q32=1, from_counts=1, min_units=-1, T=5),
    "quarter-units": dict(quarter=1, T=7),                    # a wave begins in the middle of a block: its first slice reads the planes
    "quarter-units-T4": dict(quarter=1, T=4, from_counts=1),  # ... one slice per wave: nothing but first slices
    "far-without-queue": dict(window=64, far_queue=0),        # kFar units with global atomics: they take the list
    "far-without-queue-nokey": dict(window=16, far_queue=0, T=3, from_counts=1),
    "far-queue-keeps-planes": dict(window=64, far_queue=1),   # the far-queue loop beside units that take the list
    "split-rows": dict(policy=2, window=64),
    "split-rows-all": dict(policy=3, window=16, T=3),
    "T1": dict(T=1),                                          # every slice is a first slice
}


@pytest.mark.parametrize("case", sorted(LOOP_CASES))
def test_loop_with_the_list_against_the_oracle(emulators, case):
    _against_oracle(emulators["product"], _mixed(1 + len(case)), **LOOP_CASES[case])


@pytest.mark.parametrize("case", sorted(LOOP_CASES))
def test_loop_with_the_list_on_aligner_like_input(emulators, case):
    """Reads of one (length, start) differ where the transform wrote a repeat or moved ids, often in a later plane only: a lane that
    missed such a start would go on with the ids of the read before."""
    _against_oracle(emulators["product"], _mixed(1 + len(case), aligner_like=True), **LOOP_CASES[case])


@pytest.mark.parametrize("case", ["plain", "from-counts", "q32", "quarter-units", "far-without-queue", "split-rows", "T1"])
def test_ring_loop_with_the_list_against_the_oracle(emulators, case):
    """Three register sets: the ring loop, which issues the last slice of a block again (loaded twice, reduced once)."""
    _against_oracle(emulators["ring"], _mixed(2 + len(case)), **LOOP_CASES[case])


@pytest.mark.parametrize("case", ["plain", "q32", "split-rows"])
def test_ring_loop_with_the_list_on_aligner_like_input(emulators, case):
    _against_oracle(emulators["ring"], _mixed(2 + len(case), aligner_like=True), **LOOP_CASES[case])


def _long_blocks(seed):
    """Blocks of 70 slices -- past the 64 slices whose masks and offsets a wave holds at a time -- in shapes of 64, 32 and 4 reads per
    slice; few tuples, so that most slices have a start in a few lanes only."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.full(64 * 75, 2), np.full(32 * 150, 7), np.full(4 * 72, 60)])
    rng.shuffle(lens)
    return _lens_data(lens, 1500, seed, unique=False, per_tuple=100)


@pytest.mark.parametrize("build", ["product", "ring"])
def test_blocks_longer_than_64_slices(emulators, build):
    info = _against_oracle(emulators[build], _long_blocks(9), T=70)
    assert 0 < info["marked"] < info["slices"]


BITWISE = [list(range(1, 63)),                                                        # lg 0..3 whole, lg 4 nearly
           [63, 64, 65, 72, 73, 80, 81, 88, 89, 96, 97, 104, 105, 112, 113, 121, 128],  # lg 5
           [129, 144, 145, 161, 177, 193, 209, 225, 241, 256]]                      # lg 6: one read of 64 lanes starts per slice


@pytest.mark.parametrize("lens", BITWISE, ids=["lg0-4", "lg5", "lg6"])
@pytest.mark.parametrize("q32", [0, 1])
@pytest.mark.parametrize("build", ["product", "ring"])
def test_bit_for_bit_against_the_planes(emulators, build, lens, q32):
    """Every transcript id belongs to one alignment: a count is one fraction f * (1 / normaliser), added to zero.  Ids are integers
    and a lane's arithmetic is the same whether its ids came from the list or from the planes: the same BITS.  Every read has a
    tuple of its own here, so every slice is marked, with all 64 lanes starting where the slice is full."""
    data = _lens_data(np.tile(lens, 3), 6000, 11 + len(lens), unique=True)
    on = _run(emulators[build], *data, T=3, q32=q32, use_list=1)
    off = _run(emulators[build], *data, T=3, q32=q32, use_list=0)
    assert on[3]["list_ok"] and on[3]["marked"] == on[3]["slices"] and on[3]["maxn"] == 64
    assert np.array_equal(on[0][1:].view(np.uint64), off[0][1:].view(np.uint64))
    assert on[2] == off[2] == 3 * len(lens)
    assert abs(on[1] - off[1]) <= 1e-12 * abs(off[1])   # (the noise total is a sum over all reads: its order is the threads')
    vals = quantize_q32(data[1], data[3], 8)[0] if q32 else data[3]
    oc = orc.em_estep(data[0], data[1], data[2], vals, data[4], data[5])
    assert np.allclose(on[0][1:], oc[1:], rtol=1e-9, atol=0.0)


# ---- 3. ThreadSanitizer -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(T=3, min_units=-1), dict(quarter=1, T=7, q32=1), dict(window=64, far_queue=0),
                                dict(T=3, min_units=-1, aligner_like=True), dict(window=64, far_queue=0, aligner_like=True)],
                         ids=["short", "quarter-q32", "far-without-queue", "short-aligner_like", "far-without-queue-aligner_like"])
def test_no_unordered_accesses_between_lanes(emulators, kw, monkeypatch):
    """The kernel body with the list under ThreadSanitizer (a report makes the emulator exit with 66)."""
    if emulators["tsan"] is None:
        pytest.skip("no ThreadSanitizer build with this toolchain")
    monkeypatch.setenv("TSAN_OPTIONS", "halt_on_error=0 exitcode=66")
    rng = np.random.default_rng(5)
    lens = np.concatenate([np.arange(5, 257, 3), rng.integers(1, 40, 400)])
    kw = dict(kw)
    _against_oracle(emulators["tsan"], _lens_data(lens, 2000, 5, unique=False, aligner_like=kw.pop("aligner_like", False)), **kw)
