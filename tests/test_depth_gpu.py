"""Per-base read depth on the GPU (rsem_amd/csrc/depth.hip through capi.depth_accumulate, rsem-bam2wig and rsem-bam2readdepth) against
the Python restatement (tests/depth_ref.py) and the files the unmodified reference programs wrote (tests/golden/wiggle/).  The depth
is a fold in record order: there are no tolerances, doubles are compared by their bits and files by their bytes.

T = 512 bases a tile, 256 entries an LDS chunk; every shape is small and sits on a seam of the two."""
import os
import subprocess

import numpy as np
import pytest

import depth_ref as dr
from depth_ref import BAM2READDEPTH, BAM2WIG, GOLDEN, order_sensitive_blocks

pytestmark = pytest.mark.gpu

T, CHUNK = dr.TILE, dr.CHUNK
INVALID = -1  # RSEM_ERR_INVALID
LAUNCHES_PER_BATCH = 7


def capi():
    from rsem_amd import capi as c
    return c


def check(n_bases, start, length, w, depth=None):
    start, length, w = np.asarray(start, np.uint64), np.asarray(length, np.uint32), np.asarray(w, np.float64)
    want = dr.fold(n_bases, start, length, w, depth)
    got, info = capi().depth_accumulate(n_bases, start, length, w, depth=depth)
    assert np.array_equal(dr.bits(got), dr.bits(want))
    assert info["n_entries"] == sum(dr.tiles_of(int(s), int(l)) for s, l in zip(start, length))
    return got, info


W3 = [0.1, np.float32(0.1), 2.0 ** -24]


@pytest.mark.parametrize("end", [T - 1, T, T + 1])
def test_blocks_that_end_around_a_tile_boundary(end):
    check(3 * T, [end - 40, end - 7, 0, end - 1], [40, 7, end, 1], W3 + [0.7])


@pytest.mark.parametrize("start", [T, T + 1, T - 1, 0])
def test_a_block_of_a_tile(start):
    _, info = check(3 * T, [start, start + 3], [T, 5], [0.1, 0.7])
    assert info["n_tiles_touched"] == (1 if start % T == 0 else 2)


def test_a_block_over_two_tiles_and_two_bases():
    _, info = check(4 * T, [T - 1, 0, T - 1], [2 * T + 2, 3 * T, 2 * T + 2], W3)
    assert info["n_entries"] == 4 + 3 + 4 and info["n_tiles_touched"] == 4


@pytest.mark.parametrize("n_bases", [1, T, T + 1])
def test_few_bases(n_bases):
    _, info = check(n_bases, [0, n_bases - 1, 0], [n_bases, 1, 1], W3)
    assert info["n_tiles_touched"] == (n_bases + T - 1) // T and info["n_batches"] == 1 and info["n_launches"] == LAUNCHES_PER_BATCH
    assert info["upload_ms"] > 0 and info["kernel_ms"] > 0 and info["device_bytes"] >= 8 * n_bases


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_one_tile_with_more_entries_than_a_chunk_keeps_the_order(n):
    start, length, w = order_sensitive_blocks(n)
    if n > CHUNK:  # otherwise the case proves nothing about order
        assert np.any(dr.bits(dr.fold(T, start, length, w)) != dr.bits(dr.fold(T, start[::-1], length[::-1], w[::-1])))
    _, info = check(T, start, length, w)
    assert info["n_tiles_touched"] == 1 and info["n_entries"] == n
    check(3 * T, start + np.uint64(T + 1), length, w)  # the same entries across two tiles, behind an untouched one


def test_depth_passed_in_is_continued():
    rng = np.random.default_rng(5)
    before = rng.random(2 * T + 3) * np.array([1.0, 1e-9, 0.0])[rng.integers(0, 3, 2 * T + 3)]
    before[7] = -0.0  # an untouched base keeps its bits; a touched -0.0 + w is w
    start, length, w = order_sensitive_blocks(300, seed=2, span=2 * T + 3)
    keep = ~((start <= 7) & (start + length > 7))
    got, _ = check(2 * T + 3, start[keep], length[keep], w[keep], depth=before)
    assert np.signbit(got[7])
    half = len(start) // 2  # and two calls are one
    first, _ = check(2 * T + 3, start[:half], length[:half], w[:half], depth=before)
    second, _ = check(2 * T + 3, start[half:], length[half:], w[half:], depth=first)
    assert np.array_equal(dr.bits(second), dr.bits(dr.fold(2 * T + 3, start, length, w, before)))


def test_blocks_of_no_bases():
    _, info = check(2 * T, [0, 5, 2 * T, T, T - 1], [0, 3, 0, 0, 2], [1.0, 0.1, 1.0, 1.0, 0.7])
    assert info["n_entries"] == 3


_cache = {}


def random_blocks():
    """20 000 blocks over 40 tiles, lengths like reads', some across several tiles: computed once, shared, never changed"""
    if not _cache:
        rng = np.random.default_rng(40)
        n, n_bases = 20000, 40 * T - 3
        length = rng.integers(1, 150, n)
        length[rng.integers(0, n, 40)] = rng.integers(T, 3 * T, 40)
        start = rng.integers(0, n_bases - length + 1)
        w = np.array([np.float32(1.0), np.float32(0.1), np.float32(2.0 ** -24), np.float32(3e-7), 0.7], np.float64)[rng.integers(0, 5, n)]
        _cache["in"] = (n_bases, start.astype(np.uint64), length.astype(np.uint32), w)
        _cache["want"] = dr.fold(*_cache["in"])
    return _cache["in"], _cache["want"]


@pytest.mark.parametrize("budget", [1, 7, 333, None])
def test_batches_change_nothing(monkeypatch, budget):
    """333 items a batch cut inside every tile's entry list (a tile has some 600 entries)"""
    (n_bases, start, length, w), want = random_blocks()
    if budget is None:
        monkeypatch.delenv("RSEM_DEPTH_BATCH_ITEMS", raising=False)
    else:
        monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", str(budget))
    got, info = capi().depth_accumulate(n_bases, start, length, w)
    assert np.array_equal(dr.bits(got), dr.bits(want))
    batches = dr.expected_batches(start, length, budget or 2 ** 26)
    assert info["n_batches"] == len(batches) and info["n_launches"] == LAUNCHES_PER_BATCH * len(batches)
    assert info["batch_items"] == (budget or 2 ** 26) and info["n_entries"] == sum(e for _, e in batches)
    if budget is None:
        assert len(batches) == 1 and info["n_tiles_touched"] == 40
    if budget == 333:
        assert len(batches) > 40 and info["n_tiles_touched"] > 2 * 40


def test_many_runs_cost_the_launches_of_one(monkeypatch):
    """3000 runs of 1 to 5 bases laid one after the other: the launches of a single run with as many batches"""
    monkeypatch.delenv("RSEM_DEPTH_BATCH_ITEMS", raising=False)
    targets, recs = dr.read_alignments(os.path.join(GOLDEN, "many_runs.bam"))
    runs, blocks, _ = dr.runs_and_blocks(targets, recs)
    assert len(runs) == 3000
    off, start, length, w, want = 0, [], [], [], []
    for tid, b0, b1 in runs:
        bl = blocks[b0:b1]
        start += [off + b[0] for b in bl]
        length += [b[1] for b in bl]
        w += [b[2] for b in bl]
        want.append(dr.fold(targets[tid][1], [b[0] for b in bl], [b[1] for b in bl], [b[2] for b in bl]))
        off += targets[tid][1]
    got, info = capi().depth_accumulate(off, start, length, w)
    assert np.array_equal(dr.bits(got), dr.bits(np.concatenate(want)))
    _, one = capi().depth_accumulate(off, [0], [off], [1.0])
    assert info["n_batches"] == one["n_batches"] == 1 and info["n_launches"] == one["n_launches"] == LAUNCHES_PER_BATCH


# ---- the programs ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def programs():
    assert os.path.exists(BAM2WIG) and os.path.exists(BAM2READDEPTH), "rsem-bam2wig / rsem-bam2readdepth were not built"
    return BAM2WIG, BAM2READDEPTH


@pytest.mark.parametrize("p", ["1", "4"])
@pytest.mark.parametrize("ci", dr.inputs(), ids=dr.input_id)
def test_programs_write_the_recorded_files(programs, tmp_path, ci, p):
    case, path = ci
    out = os.path.join(str(tmp_path), "out")
    r = subprocess.run([programs[1], path, out, "-p", p], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert open(out, "rb").read() == dr.recorded(case, ".readdepth")
    r = subprocess.run([programs[0], path, out, case, "-p", p], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert open(out, "rb").read() == dr.recorded(case, ".wig")
    r = subprocess.run([programs[0], path, out, case, "-p", p, "--device", "0", "-q", "--no-fractional-weight"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert open(out, "rb").read() == dr.recorded(case, ".nfw.wig")


@pytest.mark.parametrize("env", [{"RSEM_DEPTH_SPACE_BLOCKS": "1", "RSEM_HIP_BAM_CHUNK": "2000"}, {"RSEM_DEPTH_SPACE_BASES": "1"},
                                 {"RSEM_DEPTH_BATCH_ITEMS": "5"}], ids=["open_run_carried", "a_space_per_run", "batches"])
@pytest.mark.parametrize("name", ["unsorted.bam", "sorted.sam"])
def test_hand_overs_change_nothing(programs, tmp_path, name, env):
    case, path = name.split(".")[0], os.path.join(GOLDEN, name)
    out = os.path.join(str(tmp_path), "out")
    subprocess.run([programs[1], path, out, "-p", "3"], check=True, env=dict(os.environ, **env))
    assert open(out, "rb").read() == dr.recorded(case, ".readdepth")
    subprocess.run([programs[0], path, out, case, "-p", "3"], check=True, env=dict(os.environ, **env))
    assert open(out, "rb").read() == dr.recorded(case, ".wig")


def test_programs_stop_with_a_message(programs, tmp_path):
    sam = os.path.join(str(tmp_path), "past.sam")
    open(sam, "w").write("@SQ\tSN:a\tLN:30\nr_ok\t0\ta\t1\t255\t30M\t*\t0\t0\t*\t*\tZW:f:1\nr_past\t0\ta\t22\t255\t10M\t*\t0\t0\t*\t*\tZW:f:1\n")
    cram = os.path.join(str(tmp_path), "x.cram")
    open(cram, "wb").write(b"CRAM\x03\x00" + bytes(40))
    for prog, extra in ((programs[0], ["name"]), (programs[1], [])):
        r = subprocess.run([prog, sam, os.path.join(str(tmp_path), "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 255 and "r_past" in r.stderr and "past the end of a (30 bases)" in r.stderr
        r = subprocess.run([prog, cram, os.path.join(str(tmp_path), "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 255 and "CRAM" in r.stderr


def test_invalid_arguments_are_refused(monkeypatch):
    c = capi()
    ok = (np.array([0, 5], np.uint64), np.array([5, 5], np.uint32), np.array([1.0, 0.5]))
    with pytest.raises(c.RsemHipError) as e:
        c.depth_accumulate(9, *ok)
    assert e.value.status == INVALID
    for bad in ("0", "-5", "many", "12x", ""):
        monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", bad)
        with pytest.raises(c.RsemHipError) as e:
            c.depth_accumulate(10, *ok)
        assert e.value.status == INVALID and "RSEM_DEPTH_BATCH_ITEMS" in str(e.value)
    monkeypatch.delenv("RSEM_DEPTH_BATCH_ITEMS")
    got, info = c.depth_accumulate(10, *ok)
    assert got.tolist() == [1.0] * 5 + [0.5] * 5 and info["n_batches"] == 1
