"""Transcript -> genome coordinates and the per-read collapse on the GPU (rsem_amd/csrc/gmap.hip through capi.Gmap, and rsem-tbam2gbam)
against the Python restatement (tests/gmap_ref.py) and the files the unmodified reference program wrote (tests/golden/gbam/).  There
are no tolerances: integers are compared for equality, floats by their bits, files by their (decompressed) bytes.

A wave takes a group of up to 64 alignments, a workgroup of 256 lanes a longer one in tiles of 256: every shape is small and sits on a
seam of the two."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gmap_ref as gr
from gmap_ref import GOLDEN, TBAM2GBAM

pytestmark = pytest.mark.gpu

LAUNCHES_PER_BATCH = 6
_cache = {}


def reference():
    """the fixtures' transcripts and a 300-exon transcript on either strand; the device handle; computed once, shared, never changed"""
    if not _cache:
        from rsem_amd import capi
        _, ti = gr.load_ti(gr.REF + ".ti")
        ex300 = [(1000 + 25 * k, 1009 + 25 * k) for k in range(300)]
        for s in "+-":
            ti.append(dict(transcript_id="x300" + s, seqname="chrA", strand=s, length=3000, exons=ex300))
        out_ids = {"chrC": 0, "chrA": 1, "chrB": 2}
        flat = gr.flat_reference(ti, out_ids)
        _cache["ti"], _cache["out_tid"], _cache["g"] = ti, flat[2], capi.Gmap(*flat)
        _cache["idx"] = {t["transcript_id"]: i for i, t in enumerate(ti)}
    return _cache["ti"], _cache["out_tid"], _cache["g"], _cache["idx"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(mates, group_off, tr, pos, l_qseq, flag, w, ref=None):
    """ref: another (ti, out_tid, handle, ...) than reference()'s"""
    ti, out_tid, g = (ref or reference())[:3]
    o = g.convert(mates, group_off, tr, pos, l_qseq, flag, w)
    want = gr.map_fields(ti, out_tid, tr, pos, l_qseq, flag)
    assert o["tid"].tolist() == [m[0] for m in want] and o["pos"].tolist() == [m[1] for m in want] and o["flag"].tolist() == [m[2] for m in want]
    assert o["n_cigar"].tolist() == [len(m[3]) for m in want] and o["bin"].tolist() == [m[4] for m in want] and o["has_n"].tolist() == [m[5] for m in want]
    assert o["cigar_off"].tolist() == np.concatenate([[0], np.cumsum([len(m[3]) for m in want])]).tolist()
    assert o["cigar"].tolist() == [x for m in want for x in m[3]]
    src, ws = gr.collapse_fields(mates, group_off, want, w)
    assert o["out_src"].tolist() == src.tolist() and np.array_equal(bits(o["out_w"]), bits(ws))
    info = o["info"]
    assert info["n_alignments_in"] == len(w) and info["n_alignments_out"] == len(src) and info["n_cigar_words"] == len(o["cigar"])
    assert info["n_groups"] == len(group_off) - 1 and info["n_launches"] == LAUNCHES_PER_BATCH * info["n_batches"]
    return o


def fixture_fields(name):
    """the mapped records of a recorded SAM input as fields: (mates, group_off, tr, pos, l_qseq, flag, w); a group per read name"""
    idx = reference()[3]
    lines = [l.split("\t") for l in open(os.path.join(GOLDEN, name)).read().split("\n") if l and l[0] != "@"]
    lines = [f for f in lines if not int(f[1]) & 4]
    mates = 2 if int(lines[0][1]) & 1 else 1
    if mates == 2:  # read 1 first
        lines = [f for k in range(0, len(lines), 2) for f in sorted(lines[k:k + 2], key=lambda f: not int(f[1]) & 0x40)]
    tr, pos, lq, flag = [idx[f[2]] for f in lines], [int(f[3]) - 1 for f in lines], [len(f[9]) for f in lines], [int(f[1]) for f in lines]
    w, names = [], []
    for f in lines[::mates]:
        zw = [t for t in f[11:] if t[:2] == "ZW"]
        w.append(np.float32(1.0) if not zw else (np.float32(float(zw[0][5:])) if zw[0][3] == "f" else np.float32(0.0)))
        names.append(f[0].split(" ")[0])
    group_off = [0] + [k for k in range(1, len(names)) if names[k] != names[k - 1]] + [len(names)]
    return mates, group_off, tr, pos, lq, flag, w


@pytest.mark.parametrize("name", ["se.sam", "pe.sam", "collapse.sam", "collapse_pe.sam", "tags.sam"])
def test_the_fixtures_fields(name):
    """every mapping seam of the synthetic reference: exon ends and starts, 1 to 69 junctions, 0N, bin edges, the poly-A tail, both strands"""
    o = check(*fixture_fields(name))
    assert o["info"]["n_batches"] == 1 and o["info"]["upload_ms"] > 0 and o["info"]["kernel_ms"] > 0 and o["info"]["device_bytes"] > 0


def test_a_transcript_of_300_exons():
    """reads on exon 1, 64, 65, 256, 257 and 300: inside the exon, over its junctions, and from there to the transcript's end"""
    idx = reference()[3]
    tr, pos, lq = [], [], []
    for name in ("x300+", "x300-"):
        for k in (1, 64, 65, 256, 257, 300):
            b = 10 * (k - 1)
            for p, n in ((b + 2, 5), (b, 10), (max(b - 1, 0), 12), (b + 9, min(12, 3000 - b - 9)), (b, 3000 - b + 3), (0, b + 1)):
                tr.append(idx[name]); pos.append(p); lq.append(n)
    n = len(tr)
    o = check(1, list(range(n + 1)), tr, pos, lq, [0] * n, [1.0] * n)
    assert o["n_cigar"].max() == 2 * 300 and o["info"]["n_alignments_out"] == n


def group_inputs(n, kind, mates, seed):
    """n alignments of one read on x300+: all with one key, all with keys of their own (in no order), or in interleaved runs of 3 equal keys"""
    idx = reference()[3]
    rng = np.random.default_rng(seed)
    places = rng.permutation(2000)[:n]
    if kind == "equal":
        p1 = np.full(n, 77)
    elif kind == "distinct":
        p1 = places
    else:
        m = (n + 2) // 3
        p1 = places[np.arange(n) % m]  # the runs' members lie m apart: rank order must still be file order
    pool = np.array([1.0, 2.0 ** -24, 0.1, 3e-7, 2.0 ** -25], np.float32)
    w = pool[rng.integers(0, len(pool), n)]
    if mates == 1:
        return [0, n], [idx["x300+"]] * n, p1.tolist(), [50] * n, [0] * n, w
    tr, pos, flag = [idx["x300+"]] * (2 * n), [], []
    for a in range(n):
        pos += [int(p1[a]) % 7, int(p1[a])]  # mate 1 has few keys, mate 2 decides
        flag += [99, 147]
    return [0, n], tr, pos, [50] * (2 * n), flag, w


@pytest.mark.parametrize("kind", ["equal", "distinct", "runs3"])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 700])
def test_collapse_at_the_wave_and_tile_seams(n, kind):
    for mates in (1, 2):
        o = check(mates, *group_inputs(n, kind, mates, n))
        assert o["info"]["n_alignments_out"] == {"equal": 1, "distinct": n, "runs3": (n + 2) // 3}[kind]


@pytest.mark.parametrize("n", [64, 700])
def test_the_fold_keeps_the_file_order(n):
    """one key, weights whose float sum depends on the order of the additions -- asserted first: otherwise the case proves nothing"""
    idx = reference()[3]
    w = np.array([1.0] + [2.0 ** -24] * (n - 2) + [0.1], np.float32)  # 1 + 2^-24 is 1 again; the small ones first add up
    assert bits(gr.fold32(list(w))) != bits(gr.fold32(list(w[::-1])))
    o = check(1, [0, n], [idx["iso1"]] * n, [10] * n, [30] * n, [0] * n, w)
    assert np.array_equal(bits(o["out_w"]), bits([gr.fold32(list(w))]))


def many_small_groups():
    if "small" not in _cache:
        idx = reference()[3]
        rng = np.random.default_rng(3000)
        sizes = rng.integers(1, 4, 3000)
        n = int(sizes.sum())
        iso = np.array([idx[x] for x in ("iso1", "iso2", "iso3", "iso4", "isoC")])
        _cache["small"] = (1, np.concatenate([[0], np.cumsum(sizes)]).tolist(), iso[rng.integers(0, 5, n)].tolist(), rng.integers(0, 150, n).tolist(), [40] * n,
                           (16 * rng.integers(0, 2, n)).tolist(), rng.random(n).astype(np.float32))
        _cache["small_out"] = check(*_cache["small"])
    return _cache["small"], _cache["small_out"]


def test_many_small_groups_in_one_launch():
    args, o = many_small_groups()
    assert o["info"]["n_groups"] == 3000 and o["info"]["n_batches"] == 1 and o["info"]["n_launches"] == LAUNCHES_PER_BATCH
    assert 3000 <= o["info"]["n_alignments_out"] < len(args[6])


@pytest.mark.parametrize("budget", [1, 7, None])
def test_batches_change_nothing(monkeypatch, budget):
    args, whole = many_small_groups()
    if budget is None:
        monkeypatch.delenv("RSEM_GMAP_BATCH_ITEMS", raising=False)
    else:
        monkeypatch.setenv("RSEM_GMAP_BATCH_ITEMS", str(budget))
    o = check(*args)
    for k in ("tid", "pos", "flag", "n_cigar", "bin", "has_n", "cigar_off", "cigar", "out_src"):
        assert np.array_equal(o[k], whole[k]), k
    assert np.array_equal(bits(o["out_w"]), bits(whole["out_w"]))
    assert o["info"]["n_batches"] == gr.expected_batches(args[1], budget or gr.DEFAULT_BATCH_ITEMS) and o["info"]["batch_items"] == (budget or gr.DEFAULT_BATCH_ITEMS)
    assert o["info"]["n_batches"] == {1: 3000, None: 1}.get(budget, o["info"]["n_batches"])
    big = group_inputs(300, "runs3", 1, 5)  # a group above the budget is a batch of its own
    assert check(1, *big)["info"]["n_batches"] == 1


# ---- the program -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", ["1", "4"])
@pytest.mark.parametrize("ci", gr.inputs(), ids=gr.input_id)
def test_program_writes_the_recorded_files(tmp_path, ci, p):
    assert os.path.exists(TBAM2GBAM), "rsem-tbam2gbam was not built"
    case, path = ci
    d = str(tmp_path)
    for n in ("ref.ti", "ref.chrlist"):
        shutil.copy(os.path.join(GOLDEN, n), d)
    shutil.copy(path, os.path.join(d, "aln"))
    r = subprocess.run(["rsem-tbam2gbam", "ref", "aln", "out.bam"] + (["-p", p, "--device", "0", "-q"] if p != "1" else []), executable=TBAM2GBAM, cwd=d, capture_output=True)
    assert r.returncode == 0 and r.stdout == (b"Start converting:\nGenome bam file is generated!\n" if p == "1" else b""), r.stderr
    got, want = gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read()), gr.recorded(case)
    if p == "1":
        assert got == want
    else:  # the command line is in the header; everything else is the recorded file
        cl = b"rsem-tbam2gbam ref aln out.bam"
        assert got.replace(cl + b" -p 4 --device 0 -q", cl, 1)[8:] == want[8:] and gr.split_bam(got)[1:] == gr.split_bam(want)[1:]


@pytest.mark.parametrize("env", [{"RSEM_GMAP_BATCH_ITEMS": "1"}, {"RSEM_GMAP_BATCH_ITEMS": "3", "RSEM_HIP_BAM_CHUNK": "700"}], ids=["a_batch_per_group", "groups_cut_by_super_chunks"])
@pytest.mark.parametrize("name", ["collapse.bam", "pe.sam"])
def test_program_batches_and_super_chunks_change_nothing(tmp_path, name, env):
    d = str(tmp_path)
    for n in ("ref.ti", "ref.chrlist"):
        shutil.copy(os.path.join(GOLDEN, n), d)
    shutil.copy(os.path.join(GOLDEN, name), os.path.join(d, "aln"))
    subprocess.run(["rsem-tbam2gbam", "ref", "aln", "out.bam"], executable=TBAM2GBAM, cwd=d, check=True, capture_output=True, env=dict(os.environ, **env))
    assert gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read()) == gr.recorded(name.split(".")[0])
