"""rsem-bam2wig and rsem-bam2readdepth without a GPU: the Python restatement (tests/depth_ref.py) against the files the unmodified
reference programs wrote (tests/golden/wiggle/); tests/depth_check.cpp -- the programs' host code around the kernel's body
(rsem_amd/csrc/depth_block.hpp) on the lane emulator, built with AddressSanitizer and UBSan -- against the same files; and what the
programs and rsem_depth_accumulate do before they need a device.  Every comparison is equality: of bytes for files, of bit patterns
for doubles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_ref as dr
from depth_ref import BAM2READDEPTH, BAM2WIG, GOLDEN, ROOT, order_sensitive_blocks

CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID = -1  # RSEM_ERR_INVALID


def test_fixtures_are_there():
    assert set(dr.cases()) >= {"sorted", "cigars", "tags", "tags_d", "threshold", "unsorted", "many_runs"}
    assert len(dr.inputs()) >= 12
    targets, recs = dr.read_alignments(os.path.join(GOLDEN, "many_runs.bam"))
    assert len(dr.runs_and_blocks(targets, recs)[0]) == 3000 and max(t[1] for t in targets) <= 5
    targets, recs = dr.read_alignments(os.path.join(GOLDEN, "unsorted.bam"))
    tids = [r[0] for r in dr.runs_and_blocks(targets, recs)[0]]
    assert len(tids) > len(set(tids))  # a sequence comes back
    text = dr.recorded("tags", ".readdepth").decode()
    assert "t_no_zw_only\t30\t" + " ".join(["0"] * 30) + "\n" in text and "t_never\t5\tNA\n" in text
    assert b"t_no_zw_only" not in dr.recorded("tags", ".wig")
    assert dr.recorded("tags", ".wig") != dr.recorded("tags_d", ".wig")  # the ZW of type d counts


@pytest.mark.parametrize("ci", dr.inputs(), ids=dr.input_id)
def test_restatement_equals_recorded(ci):
    case, path = ci
    targets, recs = dr.read_alignments(path)
    run_depths, unused = dr.depths(targets, recs)
    assert dr.readdepth_text(targets, run_depths, unused) == dr.recorded(case, ".readdepth")
    assert dr.wig_text(targets, run_depths, case) == dr.recorded(case, ".wig")
    assert dr.wig_text(targets, dr.depths(targets, recs, True)[0], case) == dr.recorded(case, ".nfw.wig")


def test_sam_and_bam_hold_the_same_records():
    for case in dr.cases():
        sam, bam = (os.path.join(GOLDEN, case + e) for e in (".sam", ".bam"))
        if os.path.exists(sam):
            assert dr.read_alignments(sam) == dr.read_alignments(bam)


def test_order_sensitive_inputs_are_order_sensitive():
    """the condition on the inputs of the GPU tests' order cases: folded in reverse, at least one base has other bits"""
    for n in (dr.CHUNK + 1, 3 * dr.CHUNK + 5):
        start, length, w = order_sensitive_blocks(n)
        fwd = dr.fold(dr.TILE, start, length, w)
        rev = dr.fold(dr.TILE, start[::-1], length[::-1], w[::-1])
        assert np.any(dr.bits(fwd) != dr.bits(rev))


def test_batching_rule():
    start, length = [0, 510, 600, 5, 100], [10, 4, 0, 2 * dr.TILE + 2, 3]
    assert [dr.tiles_of(s, l) for s, l in zip(start, length)] == [1, 2, 0, 3, 1]
    assert dr.expected_batches(start, length, 100) == [(5, 7)]
    assert dr.expected_batches(start, length, 1) == [(1, 1), (1, 2), (1, 0), (1, 3), (1, 1)]
    assert dr.expected_batches(start, length, 4) == [(3, 3), (2, 4)]
    assert dr.expected_batches(start, length, 2) == [(1, 1), (1, 2), (1, 0), (1, 3), (1, 1)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CC):
        pytest.skip("needs hipcc (host compilation of the HIP headers)")
    exe = os.path.join(str(tmp_path_factory.mktemp("depth_check")), "depth_check")
    r = subprocess.run([CC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "depth_check.cpp"),
                        "-o", exe, "-lpthread", "-lz"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("ci", dr.inputs(), ids=dr.input_id)
def test_check_program_writes_the_recorded_files(checker, tmp_path, ci):
    case, path = ci
    out = os.path.join(str(tmp_path), "out")
    subprocess.run([checker, "readdepth", path, out], check=True)
    assert open(out, "rb").read() == dr.recorded(case, ".readdepth")
    subprocess.run([checker, "wig", path, out, case], check=True)
    assert open(out, "rb").read() == dr.recorded(case, ".wig")
    subprocess.run([checker, "wig", path, out, case, "--no-fractional-weight"], check=True)
    assert open(out, "rb").read() == dr.recorded(case, ".nfw.wig")


@pytest.mark.parametrize("env", [{"RSEM_DEPTH_SPACE_BLOCKS": "1", "RSEM_HIP_BAM_CHUNK": "2000"}, {"RSEM_DEPTH_SPACE_BASES": "1"},
                                 {"RSEM_DEPTH_BATCH_ITEMS": "40", "RSEM_DEPTH_SPACE_BASES": "700"}], ids=["open_run_carried", "a_space_per_run", "batches"])
@pytest.mark.parametrize("name", ["unsorted.bam", "sorted.sam", "cigars.bam"])
def test_check_program_hand_overs_change_nothing(checker, tmp_path, name, env):
    """the space handed over after every super-chunk of 2000 bytes with its last run still open; a space per run; batches of 40 items"""
    case, path = name.split(".")[0], os.path.join(GOLDEN, name)
    out = os.path.join(str(tmp_path), "out")
    subprocess.run([checker, "readdepth", path, out], check=True, env=dict(os.environ, **env))
    assert open(out, "rb").read() == dr.recorded(case, ".readdepth")
    subprocess.run([checker, "wig", path, out, case], check=True, env=dict(os.environ, **env))
    assert open(out, "rb").read() == dr.recorded(case, ".wig")


def test_check_program_fold_keeps_the_order(checker):
    """three chunks' worth of entries in one tile and a block over 2T + 2 bases, whole and in batches of 100 items (a cut inside the tile's entry list every time)"""
    start, length, w = order_sensitive_blocks(3 * dr.CHUNK + 5)
    start = np.concatenate([start, [dr.TILE - 1]]).astype(np.uint64)
    length = np.concatenate([length, [2 * dr.TILE + 2]]).astype(np.uint32)
    w = np.concatenate([w, [0.7]])
    n_bases = 3 * dr.TILE + 1
    want = dr.fold(n_bases, start, length, w)
    text = "".join("%d %d %016x\n" % (s, l, b) for s, l, b in zip(start, length, dr.bits(w)))
    for env in ({}, {"RSEM_DEPTH_BATCH_ITEMS": "100"}):
        r = subprocess.run([checker, "fold", str(n_bases)], input=text, check=True, capture_output=True, text=True, env=dict(os.environ, **env))
        got = np.array([int(x, 16) for x in r.stdout.split()], np.uint64)
        assert np.array_equal(got, dr.bits(want))
        assert ("batches 1 " in r.stderr) == (not env)


def test_check_program_tile_bits(checker):
    """the sort's end_bit: the bits of the largest tile id, one more at every 2^b + 1 tiles, never none"""
    n = [1, 2, 3, 4, 5, 2 ** 8, 2 ** 8 + 1, 2 ** 16, 2 ** 16 + 1, 2 ** 32]
    r = subprocess.run([checker, "tilebits"] + [str(x) for x in n], check=True, capture_output=True, text=True)
    assert [int(x) for x in r.stdout.split()] == [1, 1, 2, 2, 3, 8, 9, 16, 17, 32]
    assert all((x - 1).bit_length() <= b for x, b in zip(n, [1, 1, 2, 2, 3, 8, 9, 16, 17, 32]))


def test_check_program_fold_past_one_radix_digit(checker):
    """257 tiles, nine bits: order-sensitive blocks interleaved over tiles 0, 128 and 256 (tests/test_depth_limits_gpu.py's input) --
    a sort on eight bits would put tile 256's entries among tile 0's"""
    import test_depth_limits_gpu as lim
    (n_bases, start, length, w), want, touched = lim.limit_case(257)
    text = "".join("%d %d %016x\n" % (s, l, b) for s, l, b in zip(start, length, dr.bits(w)))
    for env in ({}, {"RSEM_DEPTH_BATCH_ITEMS": "100"}):
        r = subprocess.run([checker, "fold", str(n_bases)], input=text, capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array([int(x, 16) for x in r.stdout.split()], np.uint64)
        assert np.array_equal(got, dr.bits(want))
        if not env:
            assert "batches 1 " in r.stderr and "tiles %d\n" % len(touched) in r.stderr


@pytest.fixture(scope="module")
def programs():
    from rsem_amd import build
    build.build()
    assert os.path.exists(BAM2WIG) and os.path.exists(BAM2READDEPTH), "rsem-bam2wig / rsem-bam2readdepth were not built"
    return BAM2WIG, BAM2READDEPTH


WIG_USAGE = "Usage: rsem-bam2wig sorted_alignment_file wig_output wiggle_name [--no-fractional-weight]\nsorted_alignment_file\t: Can be either in SAM/BAM/CRAM format, must be sorted\n"


@pytest.mark.parametrize("argv", [[], ["in.bam"], ["in.bam", "out.wig"], ["in.bam", "out.wig", "name", "--no-fractional-weight", "more"],
                                  ["in.bam", "out.wig", "name", "-p", "2", "--bogus"]])
def test_bam2wig_wrong_argument_count(programs, tmp_path, argv):
    r = subprocess.run([programs[0]] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255
    assert r.stdout.startswith("Number of arguments is not correct!\n" + WIG_USAGE)
    assert r.stdout.endswith("Please note that this option must be at the end of the command line.\n")
    assert os.listdir(str(tmp_path)) == []


def test_bam2wig_unknown_fifth_argument(programs, tmp_path):
    r = subprocess.run([programs[0], "in.bam", "out.wig", "name", "--fractional"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255
    assert r.stdout.startswith("Cannot recognize option --fractional!\n" + WIG_USAGE)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("argv", [[], ["in.bam"], ["in.bam", "out", "extra"], ["in.bam", "out", "--device"]])
def test_bam2readdepth_usage(programs, tmp_path, argv):
    r = subprocess.run([programs[1]] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout == "Usage: rsem-bam2readdepth sorted_bam_input readdepth_output\n"
    assert os.listdir(str(tmp_path)) == []


def test_programs_missing_input(programs, tmp_path):
    for prog, extra in ((programs[0], ["name"]), (programs[1], [])):
        r = subprocess.run([prog, "missing.bam", "out"] + extra, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 255 and r.stderr == "Cannot open missing.bam!\n"


def test_programs_need_no_device_where_nothing_adds(programs, tmp_path):
    """records without ZW only: used sequences of zeros, no block, and so no device call -- the whole path around it runs here"""
    sam = os.path.join(str(tmp_path), "nozw.sam")
    open(sam, "w").write("@SQ\tSN:a\tLN:3\n@SQ\tSN:b\tLN:2\n@SQ\tSN:c\tLN:0\nr1\t0\ta\t1\t255\t2M\t*\t0\t0\t*\t*\nr2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
                         "r3\t0\tc\t1\t255\t*\t*\t0\t0\t*\t*\nr4\t0\ta\t2\t255\t1=\t*\t0\t0\t*\t*\tZW:f:1\n")
    out = os.path.join(str(tmp_path), "out")
    for p in ("1", "4"):
        subprocess.run([programs[1], sam, out, "-p", p, "-q"], check=True)
        assert open(out).read() == "a\t3\t0 0 0\nc\t0\tNA\na\t3\t0 0 0\nb\t2\tNA\n"
        r = subprocess.run([programs[0], sam, out, "a name", "-p", p], check=True, capture_output=True)
        assert open(out).read() == 'track type=wiggle_0 name="a name" description="a name" visibility=full\n' and r.stdout == b""


def test_programs_stop_at_a_block_past_the_end_and_at_cram(programs, tmp_path):
    sam = os.path.join(str(tmp_path), "past.sam")
    open(sam, "w").write("@SQ\tSN:a\tLN:30\nr_ok\t0\ta\t1\t255\t30M\t*\t0\t0\t*\t*\tZW:f:1\nr_past\t0\ta\t22\t255\t5M2D5M\t*\t0\t0\t*\t*\tZW:f:1\n")
    cram = os.path.join(str(tmp_path), "x.cram")
    open(cram, "wb").write(b"CRAM\x03\x00" + bytes(40))
    neg = os.path.join(str(tmp_path), "neg.sam")
    open(neg, "w").write("@SQ\tSN:a\tLN:30\nr_nowhere\t0\ta\t0\t255\t5M\t*\t0\t0\t*\t*\tZW:f:1\n")
    for prog, extra in ((programs[0], ["name"]), (programs[1], [])):
        r = subprocess.run([prog, sam, os.path.join(str(tmp_path), "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 255 and "r_past" in r.stderr and "past the end of a (30 bases)" in r.stderr and "r_ok" not in r.stderr
        r = subprocess.run([prog, cram, os.path.join(str(tmp_path), "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 255 and "CRAM" in r.stderr and "not supported" in r.stderr
        r = subprocess.run([prog, neg, os.path.join(str(tmp_path), "o")] + extra, capture_output=True, text=True)
        assert r.returncode == 255 and "r_nowhere" in r.stderr and "no position" in r.stderr


def test_library_refuses_invalid_arguments_without_a_device(monkeypatch):
    """the checks come before the device is touched: they answer on a machine that has none"""
    from rsem_amd import capi
    ok = (np.array([0, 5], np.uint64), np.array([5, 5], np.uint32), np.array([1.0, 0.5]))
    for n_bases, start, length in [(9, ok[0], ok[1]), (10, np.array([0, 2 ** 64 - 3], np.uint64), ok[1]), (10, np.array([0, 11], np.uint64), np.array([5, 0], np.uint32)),
                                   (0, np.array([0], np.uint64), np.array([1], np.uint32))]:
        with pytest.raises(capi.RsemHipError) as e:
            capi.depth_accumulate(n_bases, start, length, np.ones(len(start)))
        assert e.value.status == INVALID
    for bad in ("0", "-5", "many", "12x", "", "1.5"):
        monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", bad)
        with pytest.raises(capi.RsemHipError) as e:
            capi.depth_accumulate(10, *ok)
        assert e.value.status == INVALID and "RSEM_DEPTH_BATCH_ITEMS" in str(e.value)
    monkeypatch.delenv("RSEM_DEPTH_BATCH_ITEMS")
    before = np.array([0.25, -0.0, 3.0])
    for n_bases, blocks in [(3, (np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0))),         # no block
                            (3, (np.array([1, 3], np.uint64), np.zeros(2, np.uint32), np.ones(2)))]:   # blocks of no bases
        got, info = capi.depth_accumulate(n_bases, *blocks, depth=before)
        assert np.array_equal(dr.bits(got), dr.bits(before)) and info["n_entries"] == 0 and info["n_launches"] == 0 and info["device_bytes"] == 0
    got, info = capi.depth_accumulate(0, np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.ones(1))  # no base
    assert len(got) == 0 and info["n_batches"] == 0


def test_library_takes_the_batch_knob_as_strtoll_reads_it(monkeypatch):
    """the accept side of RSEM_DEPTH_BATCH_ITEMS: leading white space, a sign and leading zeros are part of a whole number"""
    from rsem_amd import capi
    for good in ("7", " 7", "+7", "007"):
        monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", good)
        got, info = capi.depth_accumulate(3, np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0))  # no block: no device needed
        assert len(got) == 3 and info["batch_items"] == 7 and info["n_batches"] == 0, good


@pytest.mark.parametrize("bad", ["99999999999999999999", "-99999999999999999999", "7x", "7 ", "", "0"])
def test_library_refuses_what_is_no_whole_number_in_range(monkeypatch, bad):
    """the reject side: a value strtoll clamps to the ends of long long, text behind the number, nothing, and 0 below lo = 1"""
    from rsem_amd import capi
    monkeypatch.setenv("RSEM_DEPTH_BATCH_ITEMS", bad)
    with pytest.raises(capi.RsemHipError) as e:
        capi.depth_accumulate(3, np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0))
    assert e.value.status == INVALID and "RSEM_DEPTH_BATCH_ITEMS" in str(e.value)
