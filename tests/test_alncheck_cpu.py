"""rsem-sam-validator and rsem-get-unique without a GPU: the Python restatement (tests/alncheck_ref.py) against what the unmodified
reference programs said and wrote (tests/golden/alncheck/); tests/alncheck_check.cpp -- the programs' host code around the kernels'
bodies (rsem_amd/csrc/alncheck_block.hpp) on the lane emulator, built with AddressSanitizer and UBSan -- against the same files; and what
the programs and rsem_alncheck_* do before they need a device.  Every comparison is equality of bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import alncheck_ref as ar
import gmap_ref as gr
from alncheck_ref import GET_UNIQUE, GOLDEN, ROOT, VALIDATOR, pair, rec

CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID, STATE = -1, -5


def test_fixtures_are_there():
    codes = {}
    for case in ar.validator_cases():
        targets, recs = ar.load(os.path.join(GOLDEN, case + ".bam"))
        codes.setdefault(ar.verdict(recs, [l for _, l in targets]).code, []).append(case)
    assert sorted(codes) == list(range(14)), codes  # valid files and a case for every code
    ops = {ar.verdict(ar.load(os.path.join(GOLDEN, "cigar_%s.bam" % c))[1], [100, 200, 50]).cigar_op for c in "nidshp"}
    assert ops == {ord(c) for c in "NIDSHP"}
    assert ar.verdict(ar.load(os.path.join(GOLDEN, "cigar_two.bam"))[1], [100, 200, 50]).cigar_op == ord("S")  # the first offending operation, not the worst
    assert set(ar.unique_cases()) >= {"uniq_se", "uniq_pe", "unmapped_only", "header_only", "valid_se", "valid_pe"}
    assert b"exceeds" not in ar.recorded("boundary_end_eq", ".stdout") and b"[91, 101)" in ar.recorded("boundary_end_plus1", ".stdout")
    assert b"[-1, 9)" in ar.recorded("boundary_pos_neg", ".stdout") and b"[100, 101)" in ar.recorded("no_cigar_mapped", ".stdout")
    assert len(ar.inputs(ar.validator_cases())) >= 2 * len(ar.validator_cases()) - 2  # SAM and BAM but for what SAM text cannot say


@pytest.mark.parametrize("ci", ar.inputs(ar.validator_cases()), ids=ar.input_id)
def test_restatement_prints_the_recorded_stdout(ci):
    case, path = ci
    targets, recs = ar.load(path)
    assert ar.validator_stdout(targets, recs).encode() == ar.recorded(case, ".stdout")


@pytest.mark.parametrize("ci", ar.inputs(ar.unique_cases()), ids=ar.input_id)
def test_restatement_writes_the_recorded_unique_file(ci):
    case, path = ci
    assert ar.get_unique(path) == ar.recorded(case, ".unique")


def test_sam_and_bam_hold_the_same_records():
    n = 0
    for case in set(ar.validator_cases()) | set(ar.unique_cases()):
        sam, bam = (os.path.join(GOLDEN, case + e) for e in (".sam", ".bam"))
        if os.path.exists(sam):
            assert gr.read_alignments(sam) == gr.read_alignments(bam)
            n += 1
    assert n >= 35


def test_restatement_of_the_set():
    """`used` holds every group before the one before: a name may come back only as the group it continues"""
    tl = [100]
    assert ar.verdict([rec("A"), rec("A"), rec("B"), rec("B")], tl).code == ar.OK
    v = ar.verdict([rec("A"), rec("B"), rec("C"), rec("B")], tl)
    assert (v.code, v.unit_record, v.units_ok) == (ar.NOT_GROUPED, 3, 3)
    v = ar.verdict(pair("A") + pair("B") + pair("A"), tl)
    assert (v.code, v.unit_record, v.units_ok) == (ar.NOT_GROUPED, 4, 2)
    assert ar.unique_keep([rec("a"), rec("b"), rec("b"), rec("a x"), rec("a y"), rec("c", 4)]) == [1, 0, 0, 1, 1, 0]


# ---- the check program: the host code and the kernels' bodies under the sanitizers ------------------------------------------------

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CC):
        pytest.skip("needs hipcc (host compilation of the HIP headers)")
    exe = os.path.join(str(tmp_path_factory.mktemp("alncheck_check")), "alncheck_check")
    r = subprocess.run([CC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "alncheck_check.cpp"),
                        "-o", exe, "-lpthread", "-lz"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


KNOBS = [{}, {"RSEM_ALNCHECK_BATCH_ITEMS": "1", "RSEM_ALNCHECK_HASH_BITS": "1", "RSEM_HIP_BAM_CHUNK": "200"}, {"RSEM_ALNCHECK_BATCH_ITEMS": "3", "RSEM_ALNCHECK_HASH_BITS": "3"}]
KNOB_IDS = ["default", "a_batch_per_unit_one_hash_bit_small_super_chunks", "batches_of_3_three_hash_bits"]


@pytest.mark.parametrize("env", KNOBS, ids=KNOB_IDS)
def test_check_program_prints_the_recorded_stdout(checker, env):
    for case, path in ar.inputs(ar.validator_cases()):
        r = subprocess.run([checker, "validate", path], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == ar.recorded(case, ".stdout"), (path, r.stderr[-2000:])


@pytest.mark.parametrize("env", KNOBS, ids=KNOB_IDS)
def test_check_program_writes_the_recorded_unique_files(checker, tmp_path, env):
    out = os.path.join(str(tmp_path), "out.bam")
    for case, path in ar.inputs(ar.unique_cases()):
        r = subprocess.run([checker, "unique", "2", path, out], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == b"done!\n", (path, r.stderr[-2000:])
        assert gr.bgzf_inflate(open(out, "rb").read()) == ar.recorded(case, ".unique"), path


# ---- the programs, before they need a device -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def programs():
    from rsem_amd import build
    build.build()
    assert os.path.exists(VALIDATOR) and os.path.exists(GET_UNIQUE), "rsem-sam-validator / rsem-get-unique were not built"


@pytest.mark.parametrize("argv", [[], ["aln", "extra"], ["aln", "-p"], ["aln", "--bogus", "1"]])
def test_validator_usage(programs, tmp_path, argv):
    r = subprocess.run([VALIDATOR] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout == "Usage: rsem-sam-validator <input.sam/input.bam/input.cram>\n"


@pytest.mark.parametrize("argv", [[], ["1"], ["1", "aln"], ["1", "aln", "out.bam", "extra"], ["1", "aln", "out.bam", "--device"]])
def test_get_unique_usage(programs, tmp_path, argv):
    r = subprocess.run([GET_UNIQUE] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout == "Usage: rsem-get-unique number_of_threads unsorted_transcript_bam_input bam_output\n"
    assert os.listdir(str(tmp_path)) == []


def test_programs_stop_with_their_own_messages(programs, tmp_path):
    d = str(tmp_path)
    r = subprocess.run([VALIDATOR, "missing.sam"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and r.stdout == "." and r.stderr == "Cannot open missing.sam! It may not exist.\n"
    open(os.path.join(d, "x.cram"), "wb").write(b"CRAM\3\0" + b"\0" * 30)
    r = subprocess.run([VALIDATOR, "x.cram"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and "CRAM input is not supported" in r.stderr
    r = subprocess.run([GET_UNIQUE, "1", "x.cram", "out.bam"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and "CRAM input is not supported" in r.stderr and not os.path.exists(os.path.join(d, "out.bam"))
    open(os.path.join(d, "unknown.sam"), "w").write("@SQ\tSN:t1\tLN:100\nr1\t0\tnobody\t1\t255\t4M\t*\t0\t0\tACGT\tIIII\n")
    r = subprocess.run([VALIDATOR, "unknown.sam"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 255 and "unknown reference nobody" in r.stderr  # (the reference says "not valid" and nothing else)


@pytest.mark.parametrize("name", ["header_only.sam", "header_only.bam"])
def test_programs_need_no_device_for_a_file_without_records(programs, tmp_path, name):
    path, out = os.path.join(GOLDEN, name), os.path.join(str(tmp_path), "out.bam")
    for extra in ([], ["-p", "4", "--device", "0"]):
        r = subprocess.run([VALIDATOR, path] + extra, capture_output=True)
        assert r.returncode == 0 and r.stdout == ar.recorded("header_only", ".stdout") == b".\nThe input file is valid!\n", r.stderr
    r = subprocess.run([GET_UNIQUE, "3", path, out], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"done!\n", r.stderr
    assert gr.bgzf_inflate(open(out, "rb").read()) == ar.recorded("header_only", ".unique")


# ---- the library, before it needs a device -----------------------------------------------------------------------------------------

def test_library_refuses_invalid_arguments_without_a_device(monkeypatch):
    """the checks come before a device is touched: they answer on a machine that has none"""
    from rsem_amd import capi
    L = capi.lib()
    status = lambda f: pytest.raises(capi.RsemHipError, f).value.status
    assert status(lambda: capi._check(L.rsem_alncheck_create(None, 0, 0, None))) == INVALID
    assert status(lambda: capi.Alncheck([100], device=-1)) == INVALID
    u64, v = np.zeros(2, np.uint64), capi.AlncheckVerdict()
    import ctypes as C
    assert status(lambda: capi._check(L.rsem_alncheck_push(None, 0, *([None] * 9), 0, C.addressof(v)))) == INVALID  # no handle
    ck = capi.Alncheck([100, 50])
    assert status(lambda: capi._check(L.rsem_alncheck_push(ck.h, -1, capi._ptr(u64), *([None] * 8), 0, C.addressof(v)))) == INVALID  # a negative count
    assert status(lambda: capi._check(L.rsem_alncheck_push(ck.h, 0, *([None] * 9), 0, None))) == INVALID  # no verdict
    ok = ar.pack([rec("r1", 0, 0, 5), rec("r2", 0, 1, 5)])
    changes = [dict(name_off=[1, 2, 4]), dict(name_off=[0, 2, 2]), dict(name_off=[0, 3, 2]), dict(names=b" 1r2\0"), dict(names=b"r1\tx\0"), dict(l_qseq=[10, 0]),
               dict(tid=[0, 2]), dict(tid=[-1, 0]), dict(cigar_off=[1, 1, 2]), dict(cigar_off=[0, 2, 1])]
    for change in changes:
        assert status(lambda: ck.push(**dict(ok, **change))) == INVALID, change
    long_name = ar.pack([rec("n" * 255)])
    assert status(lambda: ck.push(**long_name)) == INVALID
    odd = ar.pack(pair("p1") + pair("p2")[:1])
    assert status(lambda: ck.push(**odd)) == INVALID  # paired-end records, an odd number, not the last push
    for knob, bads in (("RSEM_ALNCHECK_BATCH_ITEMS", ("0", "-5", "many", "12x", "", "1.5")), ("RSEM_ALNCHECK_HASH_BITS", ("0", "65", "-1", "x", "", "8.0"))):
        for bad in bads:
            monkeypatch.setenv(knob, bad)
            e = pytest.raises(capi.RsemHipError, lambda: ck.push(**ok))
            assert e.value.status == INVALID and knob in str(e.value)
            e = pytest.raises(capi.RsemHipError, lambda: capi.alncheck_unique(ok["name_off"], ok["names"], ok["flag"]))
            assert e.value.status == INVALID and knob in str(e.value)
        monkeypatch.delenv(knob)
    v = ck.push(**ar.pack([]))  # nothing to check: no device needed
    assert (v["code"], v["unit_record"], v["units_ok"], v["n_batches"], v["device_bytes"], v["paired"]) == (0, -1, 0, 0, 0, -1)
    v = ck.push(last=True, **ar.pack([]))
    assert status(lambda: ck.push(**ar.pack([]))) == STATE  # the stream has ended
    ck.close()
    assert status(lambda: capi.alncheck_unique([0, 0], b"\0", [0])) == INVALID
    assert status(lambda: capi.alncheck_unique([0, 1], b" \0", [0])) == INVALID
    assert status(lambda: capi._check(L.rsem_alncheck_unique(0, -1, None, None, None, None, None))) == INVALID
    keep, info = capi.alncheck_unique([0], b"\0", [])
    assert len(keep) == 0 and info["n_batches"] == 0 and info["device_bytes"] == 0
    assert L.rsem_hip_abi_version() == 4


def test_library_takes_the_knobs_as_strtoll_reads_them(monkeypatch):
    """the accept side of RSEM_ALNCHECK_BATCH_ITEMS (leading white space, a sign and leading zeros are part of a whole number) and
    both sides of the upper end of RSEM_ALNCHECK_HASH_BITS"""
    from rsem_amd import capi
    ck = capi.Alncheck([100, 50])
    for good in ("7", " 7", "+7", "007"):
        monkeypatch.setenv("RSEM_ALNCHECK_BATCH_ITEMS", good)
        v = ck.push(**ar.pack([]))  # nothing to check: no device needed
        assert v["batch_items"] == 7 and v["n_batches"] == 0, good
        keep, info = capi.alncheck_unique([0], b"\0", [])
        assert len(keep) == 0 and info["batch_items"] == 7, good
    monkeypatch.setenv("RSEM_ALNCHECK_HASH_BITS", "64")
    assert ck.push(**ar.pack([]))["batch_items"] == 7
    monkeypatch.setenv("RSEM_ALNCHECK_HASH_BITS", "65")
    e = pytest.raises(capi.RsemHipError, lambda: ck.push(**ar.pack([])))
    assert e.value.status == INVALID and "RSEM_ALNCHECK_HASH_BITS" in str(e.value) and "from 1 to 64" in str(e.value)
    ck.close()


@pytest.mark.parametrize("bad", ["99999999999999999999", "-99999999999999999999", "7x", "7 ", "", "0"])
def test_library_refuses_what_is_no_whole_number_in_range(monkeypatch, bad):
    """the reject side: a value strtoll clamps to the ends of long long, text behind the number, nothing, and 0 below lo = 1"""
    from rsem_amd import capi
    ck = capi.Alncheck([100, 50])
    monkeypatch.setenv("RSEM_ALNCHECK_BATCH_ITEMS", bad)
    e = pytest.raises(capi.RsemHipError, lambda: ck.push(**ar.pack([])))
    assert e.value.status == INVALID and "RSEM_ALNCHECK_BATCH_ITEMS" in str(e.value)
    e = pytest.raises(capi.RsemHipError, lambda: capi.alncheck_unique([0], b"\0", []))
    assert e.value.status == INVALID and "RSEM_ALNCHECK_BATCH_ITEMS" in str(e.value)
    ck.close()
