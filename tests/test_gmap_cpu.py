"""rsem-tbam2gbam without a GPU: the Python restatement (tests/gmap_ref.py) against the files the unmodified reference program wrote
(tests/golden/gbam/); tests/gmap_check.cpp -- the program's host code around the kernels' bodies (rsem_amd/csrc/gmap_block.hpp) on the
lane emulator, built with AddressSanitizer and UBSan -- against the same files; and what the program and rsem_gmap_* do before they
need a device.  Every comparison is equality of bytes."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import gmap_ref as gr
from gmap_ref import GOLDEN, ROOT, TBAM2GBAM

CC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INVALID = -1  # RSEM_ERR_INVALID
COMMAND = "rsem-tbam2gbam ref aln out.bam"  # what the fixtures were recorded with


def workdir(tmp_path, in_path=None, ti="ref.ti", chrlist=True):
    d = str(tmp_path)
    shutil.copy(os.path.join(GOLDEN, ti), os.path.join(d, "ref.ti"))
    if chrlist:
        shutil.copy(os.path.join(GOLDEN, "ref.chrlist"), d)
    if in_path:
        shutil.copy(in_path, os.path.join(d, "aln"))
    return d


def test_fixtures_are_there():
    assert set(gr.cases()) >= {"se", "pe", "collapse", "collapse_pe", "tags", "tags_d", "unmapped", "unmapped_pe", "unmapped_only", "header_only"}
    assert len(gr.inputs()) >= 19
    typ, ti = gr.load_ti(gr.REF + ".ti")
    assert typ == 0 and len(ti) >= 12 and {t["strand"] for t in ti} == {"+", "-"} and len({t["seqname"] for t in ti}) == 3
    assert max(len(t["exons"]) for t in ti) == 70 and any(e[0] == e[1] for t in ti for e in t["exons"])
    assert any(a[1] + 1 == b[0] for t in ti for a, b in zip(t["exons"], t["exons"][1:]))  # two exons that touch
    assert any(t["exons"][0][0] < 2 ** 28 <= t["exons"][-1][1] for t in ti)
    text, targets, recs = gr.split_bam(gr.recorded("se"))
    assert [n for n, _ in targets] == ["chrC", "chrA", "chrB"]  # the .chrlist's order, not the order of first use
    assert "@PG\tID:rsem-tbam2gbam\tCL:" + COMMAND + "\n" in text and text.endswith("@XY\tan:unknown record")
    cig = {gr.canonical_name(r): gr.key_of(r)[3:] for r in recs}
    assert cig[b"touching_p"][2] == 0 << 4 | 3 and cig[b"touching_m"][2] == 3            # 0N is kept
    assert cig[b"all_tail_p"] == (1, 20 << 4 | 1) and cig[b"off_by_1_p"][-1] == 1 << 4 | 1  # I, not S
    assert cig[b"off_by_1_m"][1] == 1 << 4 | 1 and len(cig[b"j69_p"]) == 1 + 139
    bins = {gr.canonical_name(r): struct.unpack_from("<H", r, 10)[0] for r in recs}
    assert bins[b"all_tail_edge_p"] == 585 and bins[b"all_tail_edge_m"] == 585           # reg2bin of an empty range on a 2^14 edge
    out = gr.split_bam(gr.recorded("tags"))[2]
    mapq = {gr.canonical_name(r): r[9] for r in out}
    assert (mapq[b"sum_1"], mapq[b"sum_above_1"], mapq[b"sum_0p9"], mapq[b"sum_0"], mapq[b"no_zw"], mapq[b"no_zw_merged"]) == (100, 100, 10, 0, 255, 255)


@pytest.mark.parametrize("ci", gr.inputs(), ids=gr.input_id)
def test_restatement_equals_recorded(ci):
    case, path = ci
    assert gr.tbam2gbam(gr.REF, path, COMMAND) == gr.recorded(case)


def test_sam_and_bam_hold_the_same_records():
    n = 0
    for case in gr.cases():
        sam, bam = (os.path.join(GOLDEN, case + e) for e in (".sam", ".bam"))
        if os.path.exists(sam):
            assert gr.read_alignments(sam) == gr.read_alignments(bam)
            n += 1
    assert n >= 9


def test_restatement_stops_where_the_reference_does(tmp_path):
    d = workdir(tmp_path)
    head = "@SQ\tSN:one_p\tLN:525\n@SQ\tSN:iso1\tLN:425\n"
    open(os.path.join(d, "partial.sam"), "w").write(head + "r1\t73\tone_p\t1\t255\t4M\t=\t1\t0\tACGT\tIIII\nr1\t133\tone_p\t1\t0\t*\t=\t1\t0\tACGT\tIIII\n")
    with pytest.raises(gr.Stop, match="Detected partial alignments for read r1, which RSEM currently does not support!"):
        gr.tbam2gbam(os.path.join(d, "ref"), os.path.join(d, "partial.sam"), COMMAND)
    open(os.path.join(d, "two.sam"), "w").write(head + "r2\t99\tone_p\t1\t255\t4M\t=\t9\t12\tACGT\tIIII\nr2\t147\tiso1\t9\t255\t4M\t=\t1\t-12\tACGT\tIIII\n")
    with pytest.raises(gr.Stop, match="r2's two mates are aligned to two different transcripts!"):
        gr.tbam2gbam(os.path.join(d, "ref"), os.path.join(d, "two.sam"), COMMAND)


def test_flip_md_and_fold():
    assert gr.flip_md("10A5^AC6T7") == "7A6^GT5T10" and gr.flip_md("0n10N0^acgt3T0") == "0A3^tgca0N10n0" and gr.flip_md("29^GA") == "^TC29"
    ws = [np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)]
    assert gr.fold32(ws) == np.float32(1.0) and gr.fold32(ws[::-1]) != np.float32(1.0)  # the order of the additions shows
    assert gr.expected_batches([0, 3, 4, 9, 10], 4) == 3 and gr.expected_batches([0, 3, 4, 9, 10], 1) == 4 and gr.expected_batches([0, 3, 4, 9, 10], 100) == 1


# ---- the check program: the host code and the kernels' bodies under the sanitizers ------------------------------------------------

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(CC):
        pytest.skip("needs hipcc (host compilation of the HIP headers)")
    exe = os.path.join(str(tmp_path_factory.mktemp("gmap_check")), "gmap_check")
    r = subprocess.run([CC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DRSEM_EMU", "-Wno-unused-result", "-Wno-unused-value",
                        "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gmap_check.cpp"),
                        "-o", exe, "-lpthread", "-lz"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_convert(cmd, d, env=None):
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read())


@pytest.mark.parametrize("ci", gr.inputs(), ids=gr.input_id)
def test_check_program_writes_the_recorded_files(checker, tmp_path, ci):
    case, path = ci
    d = workdir(tmp_path, path)
    assert run_convert([checker, "convert", "ref", "aln", "out.bam"], d) == gr.recorded(case)


@pytest.mark.parametrize("env", [{"RSEM_GMAP_BATCH_ITEMS": "1"}, {"RSEM_GMAP_BATCH_ITEMS": "3", "RSEM_HIP_BAM_CHUNK": "700"}, {"RSEM_GMAP_BATCH_ITEMS": "7"}],
                         ids=["a_batch_per_group", "batches_of_3_and_groups_cut_by_super_chunks", "batches_of_7"])
@pytest.mark.parametrize("name", ["collapse.sam", "collapse_pe.bam", "tags.bam", "unmapped_pe.sam", "pe.sam"])
def test_check_program_batches_change_nothing(checker, tmp_path, name, env):
    d = workdir(tmp_path, os.path.join(GOLDEN, name))
    assert run_convert([checker, "convert", "ref", "aln", "out.bam", "-p", "2"], d, env) == gr.recorded(name.split(".")[0])


@pytest.mark.parametrize("n,run", [(63, 3), (64, 1), (65, 3), (255, 1), (256, 256), (257, 3), (700, 3)])
def test_check_program_collapse_at_the_seams(checker, n, run):
    """a wave's and a workgroup's group sizes around 64 and 256, against std::map: the kept alignments, their order, the folded floats' bits"""
    r = subprocess.run([checker, "collapse", str(n), str(run)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-2000:]


def limit_cases():
    import gmap_limits as gl
    return {"exon_cap": lambda: gl.cap_group(1), "exon_cap_mate_2": lambda: gl.cap_group(2), "exon_cap_reads": gl.cap_reads, "high_positions": gl.high_reads,
            "mixed_launch": lambda: gl.mixed_launch(5, "middle"), "mixed_launch_one_small": lambda: gl.mixed_launch(1, "last"),
            "last_word_513": lambda: gl.field_group(513, "last_word")[0], "strand_65": lambda: gl.field_group(65, "strand")[0],
            "mate2_last_word_257": lambda: gl.field_group(257, "mate2_last_word")[0]}


@pytest.mark.parametrize("name", ["exon_cap", "exon_cap_mate_2", "exon_cap_reads", "high_positions", "mixed_launch", "mixed_launch_one_small", "last_word_513",
                                  "strand_65", "mate2_last_word_257"])
def test_check_program_at_the_limits(checker, name):
    """tests/gmap_limits.py: 65532 CIGAR words whose last one decides, positions up to 2^31 - 2, wave-sized and longer groups in one batch"""
    import gmap_limits as gl
    case = limit_cases()[name]()
    r = subprocess.run([checker, "fields"], input=gl.fields_input(case), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == gl.fields_expected(case) and "batches 1\n" in r.stderr
    if name.startswith("exon_cap"):
        assert max(int(l.split()[3]) for l in r.stdout.split("\n") if l and l[0] != "o") == 65532
    if name == "high_positions":
        assert max(int(l.split()[4]) for l in r.stdout.split("\n") if l and l[0] != "o") > 65535


# ---- the program, before it needs a device ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def program():
    from rsem_amd import build
    build.build()
    assert os.path.exists(TBAM2GBAM), "rsem-tbam2gbam was not built"
    return TBAM2GBAM


USAGE = "Usage: rsem-tbam2gbam reference_name unsorted_transcript_bam_input genome_bam_output [-p number_of_threads]\n"


@pytest.mark.parametrize("argv", [[], ["ref"], ["ref", "aln"], ["ref", "aln", "out.bam", "-p"], ["ref", "aln", "out.bam", "--bogus", "1"], ["ref", "aln", "out.bam", "extra"]])
def test_usage(program, tmp_path, argv):
    r = subprocess.run([program] + argv, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 255 and r.stdout == USAGE
    assert os.listdir(str(tmp_path)) == []


def test_program_stops_with_the_reference_messages(program, tmp_path):
    d = workdir(tmp_path, os.path.join(GOLDEN, "se.sam"))
    run = lambda argv, cwd=d: subprocess.run([program] + argv, capture_output=True, text=True, cwd=cwd)
    r = run(["missing", "aln", "out.bam"])
    assert r.returncode == 255 and r.stderr == "Cannot open missing.ti! It may not exist.\n"
    shutil.copy(os.path.join(GOLDEN, "standalone.ti"), os.path.join(d, "alone.ti"))
    r = run(["alone", "aln", "out.bam"])
    assert r.returncode == 255 and r.stderr == "Genome information is not provided! RSEM cannot convert the transcript bam file!\n"
    assert r.stdout == "Start converting:\n"
    shutil.copy(os.path.join(d, "ref.ti"), os.path.join(d, "nolist.ti"))
    r = run(["nolist", "aln", "out.bam"])
    assert r.returncode == 255 and r.stderr == "Cannot open nolist.chrlist! It may not exist.\n"
    head = "@SQ\tSN:one_p\tLN:525\n@SQ\tSN:iso1\tLN:425\n"
    open(os.path.join(d, "partial.sam"), "w").write(head + "r1\t73\tone_p\t1\t255\t4M\t=\t1\t0\tACGT\tIIII\nr1\t133\tone_p\t1\t0\t*\t=\t1\t0\tACGT\tIIII\n")
    r = run(["ref", "partial.sam", "out.bam", "-q"])
    assert r.returncode == 255 and r.stderr.endswith("Detected partial alignments for read r1, which RSEM currently does not support!\n")
    open(os.path.join(d, "two.sam"), "w").write(head + "r2\t99\tone_p\t1\t255\t4M\t=\t9\t12\tACGT\tIIII\nr2\t147\tiso1\t9\t255\t4M\t=\t1\t-12\tACGT\tIIII\n")
    r = run(["ref", "two.sam", "out.bam", "-q"])
    assert r.returncode == 255 and r.stderr.endswith("r2's two mates are aligned to two different transcripts!\n")
    open(os.path.join(d, "star.sam"), "w").write(head + "r3\t0\tone_p\t1\t255\t*\t*\t0\t0\t*\t*\n")
    r = run(["ref", "star.sam", "out.bam", "-q"])
    assert r.returncode == 255 and r.stderr.endswith("One alignment line has SEQ field as *. RSEM does not support this currently!\n")
    open(os.path.join(d, "unknown.sam"), "w").write("@SQ\tSN:nobody\tLN:5\n")
    r = run(["ref", "unknown.sam", "out.bam", "-q"])
    assert r.returncode == 255 and r.stderr.endswith("RSEM can not recognize reference sequence name nobody!\n")
    open(os.path.join(d, "mixed.sam"), "w").write(head + "r4\t0\tone_p\t1\t255\t4M\t*\t0\t0\tACGT\tIIII\nr5\t77\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\nr5\t141\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    r = run(["ref", "mixed.sam", "out.bam", "-q"])
    assert r.returncode == 255 and "r5" in r.stderr and "mixes single-end and paired-end reads" in r.stderr
    open(os.path.join(d, "lonely.sam"), "w").write(head + "r6\t99\tone_p\t1\t255\t4M\t=\t9\t12\tACGT\tIIII\n")
    r = run(["ref", "lonely.sam", "out.bam", "-q"])
    assert r.returncode == 255 and "r6" in r.stderr and "adjacent" in r.stderr


@pytest.mark.parametrize("name", ["unmapped_only.sam", "unmapped_only.bam", "header_only.sam", "header_only.bam"])
def test_program_needs_no_device_where_nothing_maps(program, tmp_path, name):
    """no mapped read: the whole path around the device call runs here -- header, pass-through, BGZF"""
    d = workdir(tmp_path, os.path.join(GOLDEN, name))
    for p in ("1", "4"):
        r = subprocess.run(["rsem-tbam2gbam", "ref", "aln", "out.bam"] + (["-p", p] if p != "1" else []), executable=program, capture_output=True, text=True, cwd=d)
        assert r.returncode == 0 and r.stdout == "Start converting:\nGenome bam file is generated!\n", r.stderr
        if p == "1":
            assert gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read()) == gr.recorded(name.split(".")[0])
    # with -p the command line differs and so does the @PG line, nothing else
    got = gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read())
    assert gr.split_bam(got)[2] == gr.split_bam(gr.recorded(name.split(".")[0]))[2] and b"CL:" + COMMAND.encode() + b" -p 4\n" in got


# ---- the library, before it needs a device -----------------------------------------------------------------------------------------

def small_gmap(capi):
    return capi.Gmap("+-", [30, 20], [1, 0], [0, 2, 3], [101, 201, 501], [110, 220, 520])


def test_library_refuses_invalid_arguments_without_a_device(monkeypatch):
    """the checks come before a device is touched: they answer on a machine that has none"""
    from rsem_amd import capi
    for args in [("+x", [30, 20], [1, 0], [0, 2, 3], [101, 201, 501], [110, 220, 520]),      # a strand
                 ("+-", [31, 20], [1, 0], [0, 2, 3], [101, 201, 501], [110, 220, 520]),      # exons that do not add up to the length
                 ("+-", [30, 20], [1, -1], [0, 2, 3], [101, 201, 501], [110, 220, 520]),     # a negative tid
                 ("+-", [30, 20], [1, 0], [0, 2, 2], [101, 201, 501], [110, 220, 520]),      # a transcript without exons
                 ("+-", [30, 20], [1, 0], [0, 2, 3], [101, 105, 501], [110, 124, 520]),      # exons that overlap
                 ("+-", [30, 20], [1, 0], [0, 2, 3], [0, 201, 501], [9, 220, 520])]:         # a position before the chromosome
        with pytest.raises(capi.RsemHipError) as e:
            capi.Gmap(*args)
        assert e.value.status == INVALID
    with pytest.raises(capi.RsemHipError) as e:
        capi._check(capi.lib().rsem_gmap_create(None, 0, -1, None, None, None, None, None, None))
    assert e.value.status == INVALID
    g = small_gmap(capi)
    ok = dict(mates=1, group_off=[0, 2], tr=[0, 1], pos=[0, 5], l_qseq=[10, 10], flag=[0, 0], w=[1.0, 0.5])
    for change in [dict(mates=0), dict(mates=3), dict(tr=[0, 2]), dict(tr=[-1, 0]), dict(group_off=[0, 0, 2]), dict(group_off=[0, 2, 1, 2]), dict(group_off=[1, 2]),
                   dict(group_off=[0, 1]), dict(pos=[0, -1]), dict(l_qseq=[10, 0])]:
        with pytest.raises(capi.RsemHipError) as e:
            g.convert(**dict(ok, **change))
        assert e.value.status == INVALID, change
    u64 = np.zeros(2, np.uint64)
    with pytest.raises(capi.RsemHipError) as e:  # negative counts
        capi._check(capi.lib().rsem_gmap_convert(g.h, 1, -1, 0, capi._ptr(u64), *([None] * 11), capi._ptr(u64), None, 0, None, None, None))
    assert e.value.status == INVALID
    with pytest.raises(capi.RsemHipError) as e:  # no handle
        capi._check(capi.lib().rsem_gmap_convert(None, 1, 0, 0, capi._ptr(u64), *([None] * 11), capi._ptr(u64), None, 0, None, None, None))
    assert e.value.status == INVALID
    for bad in ("0", "-5", "many", "12x", "", "1.5"):
        monkeypatch.setenv("RSEM_GMAP_BATCH_ITEMS", bad)
        with pytest.raises(capi.RsemHipError) as e:
            g.convert(**ok)
        assert e.value.status == INVALID and "RSEM_GMAP_BATCH_ITEMS" in str(e.value)
    monkeypatch.delenv("RSEM_GMAP_BATCH_ITEMS")
    o = g.convert(1, [0], [], [], [], [], [])  # nothing to convert: no device needed
    assert o["info"]["n_alignments_out"] == 0 and o["info"]["n_batches"] == 0 and o["info"]["device_bytes"] == 0 and len(o["cigar"]) == 0
    g.close()
    assert capi.lib().rsem_hip_abi_version() == 4


def test_library_takes_the_batch_knob_as_strtoll_reads_it(monkeypatch):
    """the accept side of RSEM_GMAP_BATCH_ITEMS: leading white space, a sign and leading zeros are part of a whole number"""
    from rsem_amd import capi
    g = small_gmap(capi)
    for good in ("7", " 7", "+7", "007"):
        monkeypatch.setenv("RSEM_GMAP_BATCH_ITEMS", good)
        o = g.convert(1, [0], [], [], [], [], [])  # nothing to convert: no device needed
        assert o["info"]["batch_items"] == 7 and o["info"]["n_batches"] == 0, good
    g.close()


@pytest.mark.parametrize("bad", ["99999999999999999999", "-99999999999999999999", "7x", "7 ", "", "0"])
def test_library_refuses_what_is_no_whole_number_in_range(monkeypatch, bad):
    """the reject side: a value strtoll clamps to the ends of long long, text behind the number, nothing, and 0 below lo = 1"""
    from rsem_amd import capi
    g = small_gmap(capi)
    monkeypatch.setenv("RSEM_GMAP_BATCH_ITEMS", bad)
    with pytest.raises(capi.RsemHipError) as e:
        g.convert(1, [0], [], [], [], [], [])
    assert e.value.status == INVALID and "RSEM_GMAP_BATCH_ITEMS" in str(e.value)
    g.close()
