"""rsem-scan-for-paired-end-reads without a GPU: the Python restatement (tests/pairscan_ref.py) against what the unmodified reference
program printed and wrote (tests/golden/pairscan/); the arithmetic the device code puts in the place of the reference's loops against
those loops; tests/pairscan_check.cpp -- the program's host code around the kernels' bodies (rsem_amd/csrc/pairscan_block.hpp) on the
lane emulator, built with AddressSanitizer and UBSan -- against the same files; what the program and rsem_pairscan_* do before they
need a device; and the overlay.  Every comparison is equality of bytes; the two fixtures with more than 16 properly paired records in a
group are compared with every run of records that tie under less_than sorted by the records' bytes, on both sides, and nothing else is."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import gmap_ref as gr
import pairscan_ref as pr
from pairscan_ref import GOLDEN, PROGRAM, ROOT, R1F, R2R, rec

CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID, STATE = -1, -5
USAGE = "Usage: rsem-scan-for-paired-end-reads number_of_threads input.[sam/bam/cram] output.bam\n"


def test_fixtures_are_there():
    cases = pr.cases()
    assert len(cases) >= 19 and set(pr.LARGE_CASES) <= set(cases)
    codes = {c: pr.reorder(pr.load(os.path.join(GOLDEN, c + ".bam")))[1].code for c in cases}
    assert {codes[c] for c in cases} == {pr.OK, pr.MIXED, pr.ODD_FULL, pr.ODD_PARTIAL}  # (NO_PARTNER is undefined behaviour there: no golden)
    for c in cases:
        has_out = os.path.exists(os.path.join(GOLDEN, c + ".out")) or os.path.exists(os.path.join(GOLDEN, c + ".out.gz"))
        assert (pr.status(c) == 0) == (codes[c] == pr.OK) == has_out
        assert pr.status(c) in (0, 255)
    most = lambda c: max([sum(pr.class_of(r.flag) == 0 for r in g) for g in groups_of(pr.load(os.path.join(GOLDEN, c + ".bam")))] + [0])
    assert most("both16") == 16 and most("both18") == 18 and most("both40") == 40
    assert all(most(c) <= 16 for c in cases if c not in pr.LARGE_CASES)
    shapes = set()
    for g in groups_of(pr.load(os.path.join(GOLDEN, "partials.bam"))):
        shapes.add(tuple(sum(pr.class_of(r.flag) == c for r in g) for c in (1, 2, 3)))
    assert shapes == {(1, 1, 0), (2, 2, 0), (2, 1, 1), (1, 2, 1), (0, 0, 2), (0, 0, 4), (3, 1, 2), (0, 1, 1)}
    assert b"single-end and paired-end" in pr.recorded("error_mixed", ".stderr") and b"full alignments" in pr.recorded("error_odd_full", ".stderr")
    assert b"partial alignments" in pr.recorded("error_odd_partial", ".stderr") and pr.recorded("error_mixed", ".stdout") == b".\n"


def groups_of(recs):
    return [recs[a:b] for a, b, _, _ in pr.walk(recs)]


@pytest.mark.parametrize("ci", pr.inputs(), ids=pr.input_id)
def test_restatement_against_the_recorded_files(ci):
    case, path = ci
    stdout, stderr, status, out = pr.scan(path)
    assert stdout == pr.recorded(case, ".stdout") and stderr == pr.recorded(case, ".stderr") and status == pr.status(case)
    if status == 0:
        assert pr.same_output(case, out, pr.recorded(case, ".out"))
        if case not in pr.LARGE_CASES:
            assert out == pr.recorded(case, ".out")


def test_the_large_fixtures_differ_from_the_reference_only_inside_tie_runs():
    """the reference's std::sort is not stable from 17 elements on: its order inside a tie run is its library's"""
    for case in pr.LARGE_CASES:
        out = pr.scan(os.path.join(GOLDEN, case + ".bam"))[3]
        want = pr.recorded(case, ".out")
        assert sorted(gr.split_bam(out)[2]) == sorted(gr.split_bam(want)[2]) and pr.canonical_ties(out) == pr.canonical_ties(want)
        keys = lambda b: [pr.key(pr.parse_record(d)) for d in gr.split_bam(b)[2] if pr.class_of(pr.parse_record(d).flag) == 0]
        assert keys(out) == keys(want) == sorted(keys(want))


def test_sam_and_bam_hold_the_same_records():
    for case in pr.cases():
        assert gr.read_alignments(os.path.join(GOLDEN, case + ".sam")) == gr.read_alignments(os.path.join(GOLDEN, case + ".bam"))


def test_closed_form_slots_against_the_lifo_loops():
    for n1, n2, nu in itertools.product(range(7), repeat=3):
        want = pr.lifo_order(n1, n2, nu)
        if (n1 + n2 + nu) % 2:
            continue  # (the reference stops before the loops)
        assert pr.closed_form_order(n1, n2, nu) == want, (n1, n2, nu)
        assert (want is None) == (abs(n1 - n2) > nu)


def test_prefix_count_rule_against_the_sequential_walk():
    rng = np.random.default_rng(11)
    for _ in range(400):
        recs = []
        for run in range(int(rng.integers(1, 5))):
            for _ in range(int(rng.integers(1, 9))):
                name = "n%d" % run + ("" if rng.random() < 0.5 else " w%d" % rng.integers(0, 2))
                recs.append(rec(name, int(rng.integers(0, 2)) * R1F))
        assert pr.soft_rule_starts(recs) == [a for a, _, _, _ in pr.walk(recs)]


def test_restatement_of_the_groups():
    walk = lambda *names_flags: [(a, b) for a, b, _, _ in pr.walk([rec(n, f) for n, f in names_flags])]
    assert walk(("r x", 0), ("r", 0), ("r y", 0)) == [(0, 2), (2, 3)]  # the raw name "r" continues the single-end group "r", "r y" does not
    assert walk(("r x", 1), ("r", 1), ("r y", 1)) == [(0, 3)]
    assert walk(("r", 0), ("r y", 1), ("r", 1), ("r z", 0)) == [(0, 1), (1, 4)]  # single-end, then paired to the end of the run
    perm, v, _ = pr.reorder([rec("a", R1F | 0, 0, 9, 1), rec("a", R2R, 0, 1, 9), rec("a", 0x41), rec("a", 0x41)])
    assert v == pr.Verdict(pr.NO_PARTNER, 0, 0)  # two first mates, nothing to put behind the second one


# ---- the check program: the host code and the kernels' bodies under the sanitizers ------------------------------------------------

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CC):
        pytest.skip("needs hipcc (host compilation of the HIP headers)")
    exe = os.path.join(str(tmp_path_factory.mktemp("pairscan_check")), "pairscan_check")
    r = subprocess.run([CC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pairscan_check.cpp"),
                        "-o", exe, "-lpthread", "-lz"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


KNOBS = [{}, {"RSEM_PAIRSCAN_BATCH_ITEMS": "1", "RSEM_HIP_BAM_CHUNK": "200"}, {"RSEM_PAIRSCAN_BATCH_ITEMS": "7"}]
KNOB_IDS = ["default", "a_batch_per_run_small_super_chunks", "batches_of_7"]


@pytest.mark.parametrize("env", KNOBS, ids=KNOB_IDS)
def test_check_program_against_the_recorded_files(checker, tmp_path, env):
    out = os.path.join(str(tmp_path), "out.bam")
    for case, path in pr.inputs():
        r = subprocess.run([checker, "2", path, out], capture_output=True, env=dict(os.environ, **env))
        assert (r.returncode, r.stdout, r.stderr) == (pr.status(case), pr.recorded(case, ".stdout"), pr.recorded(case, ".stderr")), (path, r.stderr[-2000:])
        if r.returncode == 0:
            got = gr.bgzf_inflate(open(out, "rb").read())
            assert got == pr.scan(path)[3] and pr.same_output(case, got, pr.recorded(case, ".out")), path


def test_check_program_sorts_by_a_workgroup_and_stops_without_a_partner(checker, tmp_path):
    """a group of 70 properly paired records takes the workgroup path of the rank sort; NO_PARTNER has no golden"""
    d = str(tmp_path)
    big = [rec("big", R1F if k % 2 == 0 else R2R, k % 3, (k * 37) % 50, (k * 11) % 40) for k in range(70)] + [rec("t", 0)]
    bad = [rec("ok", 0), rec("lonely", 0x41, 0, 1), rec("lonely", 0x41, 0, 2)]
    for name, recs in (("big", big), ("bad", bad)):
        pr.write_bam(os.path.join(d, name + ".bam"), recs)
    r = subprocess.run([checker, "3", "big.bam", "out.bam"], capture_output=True, cwd=d)
    assert (r.returncode, r.stdout) == (0, b".\nFinished!\n"), r.stderr[-2000:]
    assert gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read()) == pr.scan(os.path.join(d, "big.bam"))[3]
    r = subprocess.run([checker, "1", "bad.bam", "out.bam"], capture_output=True, cwd=d)
    assert r.returncode == 255 and r.stdout == b".\n" and r.stderr.startswith(b"Read lonely: ") and r.stderr.count(b"\n") == 1


# ---- the limit inputs of tests/pairscan_limits.py on the emulator ------------------------------------------------------------------

def emulate(checker, tmp_path, recs, env=None):
    """the records through `pairscan_check records` (a file written here): the verdict, the counts and the permutation equal the
    restatement's, and the sanitizers have nothing to say.  Returns (n_batches, n_sorted_groups)."""
    path = os.path.join(str(tmp_path), "records.txt")
    with open(path, "w") as f:
        for r in recs:
            f.write("%s %d %d %d %d\n" % (r.name.hex(), r.flag, r.tid, r.pos, r.mpos))
    e = dict(os.environ, **(env or {}))
    if env is None:
        e.pop("RSEM_PAIRSCAN_BATCH_ITEMS", None)
    r = subprocess.run([checker, "records", path], capture_output=True, text=True, env=e)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.split("\n")
    code, group, group_record, n_groups, n_batches, n_sorted = (int(x) for x in lines[0].split())
    want_perm, want, _ = pr.reorder(recs)
    assert pr.Verdict(code, group, group_record) == want
    if want.code == pr.OK:
        assert [int(x) for x in lines[1:] if x] == want_perm and n_groups == len(pr.walk(recs))
    return n_batches, n_sorted


def test_check_program_on_every_flag_byte(checker, tmp_path):
    """the sweep of tests/test_pairscan_limits_gpu.py without the two high bits"""
    import pairscan_limits as pl
    ok, failing = pl.split_flag_groups(high_bits=(0,))
    paired = [g for g in ok if g[0].flag & 1]
    assert {pr.class_of(r.flag) for g in paired for r in g[1:]} == {0, 1, 2, 3} and {r.flag for g in ok for r in g[1:]} == set(range(256))
    both = [r for g in paired for r in g if pr.class_of(r.flag) == 0]
    assert {(bool(r.flag & 0x40), pr.key(r)[3]) for r in both} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    recs, starts = pl.on_the_seams(ok)
    assert {s % 256 for s in starts} >= {0, 63, 64, 255} and 256 in starts
    emulate(checker, tmp_path, recs)
    codes = [pr.reorder(g)[1].code for g in failing]
    assert set(codes) == set(pl.FAIL_CODES) and len(failing) <= 64
    filler = sum(ok[:90], [])
    for g, code in zip(failing, codes):
        assert pr.reorder(filler + g)[1] == pr.Verdict(code, len(pr.walk(filler)), len(filler))
        emulate(checker, tmp_path, filler + g + pl.singles(3, "t%d"))


@pytest.mark.parametrize("budget", [None, "300"])
def test_check_program_on_groups_of_whole_tiles(checker, tmp_path, budget):
    """510, 512, 514 and 1024 records with the tie structure, 1024 equal ones and 1024 descending ones (the group of 4096 is the GPU's)"""
    import pairscan_limits as pl
    recs, where = pl.big_stream(sizes=pl.BIG_SIZES[:4])
    want = pr.reorder(recs)[0]
    first, n = where[4]
    assert n == 1024 and want[first:first + n] == list(range(first, first + n))
    n_batches, n_sorted = emulate(checker, tmp_path, recs, {"RSEM_PAIRSCAN_BATCH_ITEMS": budget} if budget else None)
    assert n_sorted == len(where) == 6 and n_batches == pr.expected_batches(recs, int(budget) if budget else pr.DEFAULT_BATCH_ITEMS)


def test_check_program_on_partial_groups_of_four_tiles(checker, tmp_path):
    import pairscan_limits as pl
    from test_pairscan_gpu import partial_group, shape
    even = []
    for k, (size, diff, swap) in enumerate([(1022, 0, False), (1024, 1, True), (1026, 21, False), (1024, 21, True)]):
        even += partial_group("e%d" % k, *shape(size, diff, swap), n_both=(k % 3) * 2) + pl.singles(k % 2, "t%d_" + str(k))
    assert pr.reorder(even)[1].code == pr.OK
    emulate(checker, tmp_path, even)
    for size in (1023, 1025):
        n1, n2, nu = shape(size - 1, 1, False)
        recs = pl.singles(5) + partial_group("o", n1, n2, nu + 1, n_both=4) + pl.singles(2, "b%d")
        assert pr.reorder(recs)[1] == pr.Verdict(pr.ODD_PARTIAL, 5, 5)
        emulate(checker, tmp_path, recs)


def test_check_program_on_keys_at_the_ends_of_32_bits(checker, tmp_path):
    import pairscan_limits as pl
    sub = pl.end_keys_subset()
    assert pr.reorder(sub)[0] == [3, 4, 0, 6, 5, 1, 7, 2]
    emulate(checker, tmp_path, sub + pl.singles(3))
    n_batches, n_sorted = emulate(checker, tmp_path, pl.singles(60) + pl.end_keys_group() + pl.singles(3, "t%d"))
    assert n_sorted == 1


def test_check_program_on_names_at_their_limits(checker, tmp_path):
    """names of 254 bytes, of canonical length 0, a prefix for a neighbour, a NUL inside: on the lanes 0, 63 | 64 and 255 | 256 and at
    the edges of batches of 1 and 7"""
    import pairscan_limits as pl
    for kind in sorted(pl.name_blocks()):
        for at in (0, 63, 255):
            recs = pl.name_stream(kind, at)
            assert pr.reorder(recs)[0] != list(range(len(recs)))
            emulate(checker, tmp_path, recs)
        for budget in (1, 7):
            recs = pl.name_stream(kind, 3)
            n_batches, _ = emulate(checker, tmp_path, recs, {"RSEM_PAIRSCAN_BATCH_ITEMS": str(budget)})
            assert n_batches == pr.expected_batches(recs, budget)


def test_check_program_on_names_of_254_bytes_in_a_file(checker, tmp_path):
    """the same names through the program's own reader and writer (a NUL inside a name is not something a file carries)"""
    import pairscan_limits as pl
    d = str(tmp_path)
    recs = sum((pl.name_stream(kind, at) for kind, at in (("last_byte", 0), ("behind_the_space", 63), ("prefix", 2))), [])
    for k, r in enumerate(recs):  # one stream: the fillers' names must not repeat
        if r.name[:1] in (b"u", b"t"):
            recs[k] = r._replace(name=r.name + b"_%d" % k)
    pr.write_bam(os.path.join(d, "in.bam"), recs, block=4000)
    for env in KNOBS:
        r = subprocess.run([checker, "2", "in.bam", "out.bam"], capture_output=True, cwd=d, env=dict(os.environ, **env))
        assert (r.returncode, r.stdout, r.stderr) == (0, b".\nFinished!\n", b""), r.stderr[-2000:]
        assert gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read()) == pr.scan(os.path.join(d, "in.bam"))[3]


@pytest.mark.parametrize("n_small,n_large", [(1, 0), (4, 0), (5, 0), (0, 3), (0, 0)])
def test_check_program_on_lists_of_groups_to_sort(checker, tmp_path, n_small, n_large):
    import pairscan_limits as pl
    recs = pl.list_stream(n_small, n_large)
    _, n_sorted = emulate(checker, tmp_path, recs)
    assert n_sorted == n_small + n_large


# ---- the program, before it needs a device ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def program():
    from rsem_amd import build
    build.build()
    assert os.path.exists(PROGRAM), "rsem-scan-for-paired-end-reads was not built"


def test_program_is_listed():
    from rsem_amd import build
    assert "rsem-scan-for-paired-end-reads" in build.HOST_PROGRAMS and "pairscan.hip" in build.HIP_SOURCES
    assert "rsem-scan-for-paired-end-reads" in open(os.path.join(ROOT, "tools", "make_overlay.sh")).read()


@pytest.mark.parametrize("argv", [[], ["1"], ["1", "aln"], ["1", "aln", "out.bam", "extra"], ["1", "aln", "out.bam", "--device"]])
def test_usage(program, tmp_path, argv):
    r = subprocess.run([PROGRAM] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout == USAGE and r.stderr == ""
    assert os.listdir(str(tmp_path)) == []


def test_program_refuses_before_the_device(program, tmp_path):
    d = str(tmp_path)
    r = subprocess.run([PROGRAM, "1", "missing.sam", "out.bam"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and r.stdout == "" and r.stderr == "Cannot open missing.sam !\n" and not os.path.exists(os.path.join(d, "out.bam"))
    open(os.path.join(d, "x.cram"), "wb").write(b"CRAM\3\0" + b"\0" * 30)
    r = subprocess.run([PROGRAM, "1", "x.cram", "out.bam"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and "CRAM input is not supported" in r.stderr and not os.path.exists(os.path.join(d, "out.bam"))


@pytest.mark.parametrize("name", ["header_only.sam", "header_only.bam"])
def test_program_needs_no_device_for_a_file_without_records(program, tmp_path, name):
    out = os.path.join(str(tmp_path), "out.bam")
    r = subprocess.run([PROGRAM, "3", os.path.join(GOLDEN, name), out, "--device", "0"], capture_output=True)
    assert (r.returncode, r.stdout, r.stderr) == (0, pr.recorded("header_only", ".stdout"), b"")
    assert gr.bgzf_inflate(open(out, "rb").read()) == pr.recorded("header_only", ".out")


# ---- the library, before it needs a device -----------------------------------------------------------------------------------------

def test_library_refuses_invalid_arguments_without_a_device(monkeypatch):
    import ctypes as C
    from rsem_amd import capi
    L = capi.lib()
    status = lambda f: pytest.raises(capi.RsemHipError, f).value.status
    assert status(lambda: capi._check(L.rsem_pairscan_create(None, 0))) == INVALID
    assert status(lambda: capi.Pairscan(device=-1)) == INVALID
    v, u64, u32 = capi.PairscanVerdict(), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    assert status(lambda: capi._check(L.rsem_pairscan_reorder(None, 0, *([None] * 6), 0, capi._ptr(u32), C.addressof(v)))) == INVALID  # no handle
    ps = capi.Pairscan()
    ok = pr.pack([rec("r1", R1F, 0, 5, 9), rec("r1", R2R, 0, 9, 5)])
    arrays = [capi._ptr(ok[k]) for k in ("name_off", "names", "flag", "tid", "pos", "mpos")]
    assert status(lambda: capi._check(L.rsem_pairscan_reorder(ps.h, -1, *arrays, 0, capi._ptr(u32), C.addressof(v)))) == INVALID  # a negative count
    assert status(lambda: capi._check(L.rsem_pairscan_reorder(ps.h, 2, *arrays, 0, None, C.addressof(v)))) == INVALID  # no output
    assert status(lambda: capi._check(L.rsem_pairscan_reorder(ps.h, 2, *arrays, 0, capi._ptr(u32), None))) == INVALID  # no verdict
    for change in (dict(name_off=[1, 2, 4]), dict(name_off=[0, 2, 2]), dict(name_off=[0, 3, 2])):
        assert status(lambda: ps.reorder(**dict(ok, **change))) == INVALID, change
    assert status(lambda: ps.reorder(**pr.pack([rec("n" * 255)]))) == INVALID
    for bad in ("0", "-5", "many", "12x", "", "1.5"):
        monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", bad)
        e = pytest.raises(capi.RsemHipError, lambda: ps.reorder(**ok))
        assert e.value.status == INVALID and "RSEM_PAIRSCAN_BATCH_ITEMS" in str(e.value)
    monkeypatch.delenv("RSEM_PAIRSCAN_BATCH_ITEMS")
    perm, v = ps.reorder(**pr.pack([]))  # nothing to order: no device needed
    assert len(perm) == 0 and (v["code"], v["group"], v["n_groups"], v["n_batches"], v["device_bytes"]) == (0, -1, 0, 0, 0)
    ps.reorder(last=True, **pr.pack([]))
    assert status(lambda: ps.reorder(**pr.pack([]))) == STATE  # the stream has ended
    ps.close()
    assert L.rsem_hip_abi_version() == 4


def test_library_takes_the_batch_knob_as_strtoll_reads_it(monkeypatch):
    """the accept side of RSEM_PAIRSCAN_BATCH_ITEMS: leading white space, a sign and leading zeros are part of a whole number"""
    from rsem_amd import capi
    ps = capi.Pairscan()
    for good in ("7", " 7", "+7", "007"):
        monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", good)
        perm, v = ps.reorder(**pr.pack([]))  # nothing to order: no device needed
        assert len(perm) == 0 and v["batch_items"] == 7, good
    ps.close()


@pytest.mark.parametrize("bad", ["99999999999999999999", "-99999999999999999999", "7x", "7 ", "", "0"])
def test_library_refuses_what_is_no_whole_number_in_range(monkeypatch, bad):
    """the reject side: a value strtoll clamps to the ends of long long, text behind the number, nothing, and 0 below lo = 1"""
    from rsem_amd import capi
    ps = capi.Pairscan()
    monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", bad)
    e = pytest.raises(capi.RsemHipError, lambda: ps.reorder(**pr.pack([])))
    assert e.value.status == INVALID and "RSEM_PAIRSCAN_BATCH_ITEMS" in str(e.value)
    ps.close()


# ---- the overlay -------------------------------------------------------------------------------------------------------------------

def test_overlay_copies_the_perl_drivers_that_look_next_to_themselves(program, tmp_path):
    """convert-sam-for-rsem puts its own directory (symbolic links resolved) first in PATH: linked, it would run the programs of the
    directory it came from.  A stand-in of three lines: nothing of the reference is needed."""
    src, out = os.path.join(str(tmp_path), "rsem"), os.path.join(str(tmp_path), "overlay")
    os.makedirs(src)
    for name in ("convert-sam-for-rsem", "rsem-plot-transcript-wiggles"):
        open(os.path.join(src, name), "w").write("#!/usr/bin/env perl\nuse FindBin;\nprint \"$FindBin::RealBin\\n\";\n")
        os.chmod(os.path.join(src, name), 0o755)
    open(os.path.join(src, "rsem-scan-for-paired-end-reads"), "w").write("#!/bin/sh\necho the stand-in of the installation\n")
    open(os.path.join(src, "samtools"), "w").write("#!/bin/sh\n")
    subprocess.run(["bash", os.path.join(ROOT, "tools", "make_overlay.sh"), src, out], check=True, capture_output=True)
    for name in ("convert-sam-for-rsem", "rsem-plot-transcript-wiggles"):
        p = os.path.join(out, name)
        assert os.path.isfile(p) and not os.path.islink(p) and open(p).read() == open(os.path.join(src, name)).read()
    link = os.path.join(out, "rsem-scan-for-paired-end-reads")
    assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(PROGRAM)
    assert os.path.realpath(os.path.join(out, "samtools")) == os.path.realpath(os.path.join(src, "samtools"))  # everything else is linked
    if shutil.which("perl"):
        r = subprocess.run(["perl", os.path.join(out, "convert-sam-for-rsem")], capture_output=True, text=True)
        assert r.returncode == 0 and os.path.realpath(r.stdout.strip()) == os.path.realpath(out)
