"""The reference-preparation programs without a GPU: the Python restatement (tests/refseq_ref.py) against the files, messages and
statuses the unmodified reference programs left (tests/golden/refprep/); tests/refseq_check.cpp -- the programs' host code around the
two kernel bodies (rsem_amd/csrc/refseq_block.hpp) on the lane emulator, built with AddressSanitizer and UBSan -- against the same
fixtures and on the kernels' seam shapes; and what the programs and rsem_refseq_* do before they need a device.  Every comparison is
equality of bytes."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refseq_ref as rr
from refseq_ref import BIN, PROGRAMS, ROOT

CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = rr.case_names()


def test_the_fixtures_are_there():
    assert len(CASES) >= 27
    for want in ("basic", "sources", "mapping", "dup", "skipfile", "twofiles", "err_star", "err_cr", "err_high", "err_unused_record", "err_boundary_first",
                 "err_short_second", "err_strand", "err_no_transcript_id", "err_no_transcripts", "syn_mode0", "syn_mode1", "syn_mode2", "syn_err_bad",
                 "pre_choice0", "pre_choice0_l3", "pre_choice0_l0", "pre_choice1", "pre_choice2", "pre_crlf"):
        assert want in CASES
    for dp, _, fns in os.walk(rr.GOLDEN):
        for fn in fns:
            assert os.path.getsize(os.path.join(dp, fn)) < 64 << 10


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name, tmp_path):
    c = rr.load_case(name)
    rr.stage_case(c, str(tmp_path))
    files, err, status = rr.run_program(c["program"], c["args"], str(tmp_path))
    assert status == c["status"]
    assert err == c["stderr"]
    assert sorted(files) == sorted(c["files"])
    for fn in files:
        assert files[fn] == c["files"][fn], fn


def test_recorded_clauses():
    """The clauses the issue quotes from runs of the reference, read back from the fixtures."""
    dup = rr.load_case("dup")["files"]
    assert dup["ref.chrlist"] == b"chr1\t23\nchr1\t16\nchr1\t16\nchr2\t10\n"          # a line an occurrence; the nameless header keeps chr1
    assert dup["ref.transcripts.fa"].startswith(b">t1\nGGGGGGGGGGG\n")                # the last occurrence wins
    assert b"(ASCII code 13), at line 2, position 5!" in rr.load_case("err_cr")["stderr"]
    assert b"(ASCII code -61)" in rr.load_case("err_high")["stderr"]
    assert rr.load_case("err_boundary_first")["stderr"] == b"Transcript t1 is out of chromosome chr1's boundary!\n"
    assert rr.load_case("pre_crlf")["files"]["ref.seq"] == b"9 12\na\r\nACGTNNNNNAAA\n511\n2 5\nb\nACAAA\n3\n"
    seq = rr.load_case("pre_choice0_l0")["files"]["ref.seq"].split(b"\n")
    assert seq[0] == b"1 1" and seq[3] == b"0"                                        # no tail: no mask bit


# ---- the kernels' bodies on the emulator, the programs' host code around them, under the sanitizers ---------------------------

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CC):
        pytest.skip("needs hipcc (host compilation of the HIP headers)")
    exe = os.path.join(str(tmp_path_factory.mktemp("refseq_check")), "refseq_check")
    r = subprocess.run([CC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "refseq_check.cpp"),
                        "-o", exe, "-lpthread", "-lz"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_in(cwd, argv, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def compare_with_case(c, cwd, r):
    """Files by bytes, the recorded stderr lines present, the exit status."""
    assert r.returncode == c["status"], r.stderr[-2000:]
    for line in c["stderr"].split(b"\n"):
        assert line in r.stderr, line
    got = sorted(fn for fn in os.listdir(cwd) if fn.startswith("ref."))
    assert got == sorted(c["files"])
    for fn in got:
        with open(os.path.join(cwd, fn), "rb") as f:
            assert f.read() == c["files"][fn], fn


@pytest.mark.parametrize("batch", [None, "1"])
@pytest.mark.parametrize("name", CASES)
def test_emulated_programs_reproduce_the_reference(checker, name, batch, tmp_path):
    c = rr.load_case(name)
    rr.stage_case(c, str(tmp_path))
    r = run_in(str(tmp_path), [checker, c["program"]] + c["args"], {"RSEM_REFSEQ_BATCH_BYTES": batch} if batch else None)
    assert b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
    compare_with_case(c, str(tmp_path), r)


def test_kernel_bodies_at_their_seams(checker, tmp_path):
    r = run_in(str(tmp_path), [checker, "seams"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr == b""


def test_kernel_bodies_at_their_limits(checker, tmp_path):
    """the shapes of tests/refseq_limits.py restated in the check program: every byte value in both modes and under the flag sets 0..7,
    bodies of no byte and bodies that touch, eight records in a chunk, 5000 segments, the two ends of the bases and of the store"""
    r = run_in(str(tmp_path), [checker, "limits"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr == b""


USAGE = {"extract": b"Usage: rsem-extract-reference-transcripts refName quiet gtfF sources hasMappingFile [mappingFile] chromosome_file_1 [chromosome_file_2 ...]\n",
         "synthesis": b"Usage: synthesisRef refName quiet hasMappingFile<0,no;1,yes;2,allele-specific> [mappingFile] reference_file_1 [reference_file_2 ...]\n",
         "preref": b"USAGE : rsem-preref refFastaF polyAChoice refName [-l polyALen] [-f exceptionF] [-q]\n\n"}
SHORT = {"extract": [["ref", "1", "a.gtf", "None", "0"], ["ref", "1", "a.gtf", "None", "1", "map.txt"]],
         "synthesis": [["ref", "1", "0"], ["ref", "1", "1", "map.txt"]], "preref": [["t.fa", "0"]]}
UNREADABLE = [("extract", ["ref", "1", "missing.gtf", "None", "0", "g.fa"], b"Cannot open missing.gtf! It may not exist.\n"),
              ("extract", ["ref", "1", "a.gtf", "None", "1", "missing.map", "g.fa"], b"Cannot open missing.map! It may not exist.\n"),
              ("extract", ["ref", "1", "a.gtf", "None", "0", "missing.fa"], b"Cannot open missing.fa! It may not exist.\n"),
              ("synthesis", ["ref", "1", "0", "missing.fa"], b"Cannot open missing.fa! It may not exist.\n"),
              ("synthesis", ["ref", "1", "1", "missing.map", "t.fa"], b"Cannot open missing.map! It may not exist.\n"),
              ("preref", ["missing.fa", "0", "ref", "-q"], b"Cannot open missing.fa! It may not exist.\n"),
              ("preref", ["t.fa", "2", "ref", "-f", "missing.txt"], b"Cannot open missing.txt! It may not exist.\n")]


def stage_small(tmp_path):
    c = rr.load_case("twofiles")
    rr.stage_case(c, str(tmp_path))
    shutil.copy(os.path.join(str(tmp_path), "two.fa"), os.path.join(str(tmp_path), "g.fa"))
    shutil.copy(os.path.join(str(tmp_path), "one.fa"), os.path.join(str(tmp_path), "t.fa"))


@pytest.mark.parametrize("prog", sorted(USAGE))
def test_usage_texts_and_statuses(checker, prog, tmp_path):
    """argv too short: the reference's usage line on stdout and exit(-1), from the emulated build and from the built program."""
    exes = [[checker, prog]]
    if os.path.exists(os.path.join(BIN, PROGRAMS[prog])):
        exes.append([os.path.join(BIN, PROGRAMS[prog])])
    for exe in exes:
        for args in SHORT[prog]:
            r = run_in(str(tmp_path), exe + args)
            assert r.returncode == 255 and r.stdout.startswith(USAGE[prog]) and r.stderr == b"", (exe, args, r.stderr)


@pytest.mark.parametrize("prog,args,message", UNREADABLE)
def test_unreadable_files(checker, prog, args, message, tmp_path):
    stage_small(tmp_path)
    r = run_in(str(tmp_path), [checker, prog] + args)
    assert r.returncode == 255 and r.stderr == message


def test_built_programs_are_listed_and_stop_before_the_device(tmp_path):
    """The three programs are products of the build; a GTF error ends the real program before it asks for a device."""
    from rsem_amd import build as b
    for prog in PROGRAMS.values():
        assert prog in b.HOST_PROGRAMS
        assert os.path.exists(os.path.join(BIN, prog)), "python -m rsem_amd.build"
    assert "refseq.hip" in b.HIP_SOURCES
    with open(os.path.join(ROOT, "tools", "make_overlay.sh")) as f:
        text = f.read()
    for prog in PROGRAMS.values():
        assert prog in text
    for name in ("err_strand", "err_no_transcript_id"):
        c = rr.load_case(name)
        d = tmp_path / name
        d.mkdir()
        rr.stage_case(c, str(d))
        r = run_in(str(d), [os.path.join(BIN, PROGRAMS["extract"])] + c["args"])
        assert r.returncode == 255 and r.stderr == c["stderr"]


def test_entry_points_are_declared_and_exported():
    from rsem_amd import capi
    L = capi.lib()
    with open(os.path.join(ROOT, "include", "rsem_hip.h")) as f:
        header = f.read()
    for fn in ("rsem_refseq_create", "rsem_refseq_load", "rsem_refseq_gather", "rsem_refseq_download", "rsem_refseq_get_info", "rsem_refseq_destroy"):
        assert fn + "(" in header and hasattr(L, fn)
    assert L.rsem_hip_abi_version() == capi.ABI_VERSION  # entry points were added, no signature changed


@pytest.mark.parametrize("value", ["0x10", "-16", "8", "17", "", "16 ", "1e3"])
def test_store_pad_knob_is_refused_before_a_device(value):
    """RSEM_REFSEQ_STORE_PAD: a whole number of bytes, a multiple of 16; anything else is RSEM_ERR_INVALID from rsem_refseq_create."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom rsem_amd import capi\ntry:\n    capi.Refseq(64)\nexcept capi.RsemHipError as e:\n"
            "    assert e.status == -1 and 'RSEM_REFSEQ_STORE_PAD' in str(e), e\n    print('refused')\n" % ROOT)
    e = dict(os.environ)
    e["RSEM_REFSEQ_STORE_PAD"] = value
    r = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:]
