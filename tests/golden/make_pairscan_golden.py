"""Writes tests/golden/pairscan/: small name-grouped alignment files and what the UNMODIFIED reference program did with them.

    python tests/golden/make_pairscan_golden.py /path/to/rsem-scan-for-paired-end-reads

The program is compiled from the reference's untouched source (scanForPairedEndReads.cpp) against the htslib 1.3 that oracle/Makefile
builds into oracle/_ref/libhts_ref.a, outside the repository:
    g++ -std=gnu++98 -w -O3 -I$REF -I$REF/samtools-1.3/htslib-1.3 -o rsem-scan-for-paired-end-reads $REF/scanForPairedEndReads.cpp oracle/_ref/libhts_ref.a -lz -lpthread
Nothing of it is kept here.

Every case is written as SAM text and, the same records, as BAM (BGZF blocks of 300 bytes: records straddle them).  Recorded per case, the
same for both inputs: <case>.stdout, <case>.stderr, <case>.status (the exit status) and, where the program succeeds, <case>.out, the
DECOMPRESSED output of `rsem-scan-for-paired-end-reads 1 <input> out.bam`; a file above 1 KiB is kept gzip-compressed (<name>.gz, no
time stamp inside).  The expected outputs are recorded, not computed.  Every record carries a tag XI:i:<its index in the file>, so that
records with equal fields are told apart in the output.  A record with mate position -1 names no mate reference ("*"): htslib's SAM
parser would otherwise flag its mate unmapped, and the two inputs would differ.

Before anything is written the recorded result of every case is compared with the restatement (tests/pairscan_ref.py): byte for byte,
but for the two cases with more than 16 properly paired records in a group (both18, both40), where the order inside a run of records
that tie under less_than is std::sort's own and both sides are compared with those runs sorted by the records' bytes."""
import gzip
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gmap_ref as gr  # noqa: E402
import pairscan_ref as pr  # noqa: E402
from make_alncheck_golden import bgzf  # noqa: E402
from pairscan_ref import P1, P2, PU, R1F, R1R, R2F, R2R, U1, U2, proper, rec  # noqa: E402

HERE = pr.GOLDEN
TARGETS = [("t1", 1000), ("t2", 2000), ("t3", 500)]


def firsts_then_seconds(name, alignments):
    """several alignments of one read, all first mates, then all second mates: what a name-sorted aligner output looks like"""
    pairs = [proper(name, *a) for a in alignments]
    return [p[0] for p in pairs] + [p[1] for p in pairs]


def partial_group(name, n1, n2, nu, both=()):
    """a group with n1 / n2 / nu records of the three partial classes, interleaved, and the `both` records in between"""
    cls = [rec(name, P1 if k % 2 else U1, 0 if k % 2 else -1, 10 + k if k % 2 else -1) for k in range(n1)]
    cls2 = [rec(name, P2 if k % 2 == 0 else U2, 1 if k % 2 == 0 else -1, 20 + k if k % 2 == 0 else -1) for k in range(n2)]
    unk = [rec(name, PU | (4 if k % 2 else 0), -1 if k % 2 else 2, -1 if k % 2 else 30 + k) for k in range(nu)]
    out, lists = [], [cls, cls2, unk, list(both)]
    while any(lists):
        for l in lists:
            if l:
                out.append(l.pop(0))
    return out


def ties(name, n_pairs):
    """n_pairs alignments, first mates then second mates, in descending key order: pair k with k % 3 == 1 lies where pair k - 1 lies (a
    run of 4 tied records), every other pair at a place of its own (its two mates tie: a run of 2)"""
    al = []
    for k in range(n_pairs):
        p = k - 1 if k % 3 == 1 else k
        al.append((p % 2, 900 - 7 * p, 950 - 3 * p, k % 6 == 5))
    return firsts_then_seconds(name, al)


SHAPES = [(1, 1, 0), (2, 2, 0), (2, 1, 1), (1, 2, 1), (0, 0, 2), (0, 0, 4), (3, 1, 2), (0, 1, 1)]
CASES = {
    "header_only": lambda: [],
    "single_end": lambda: [rec("s1", 0, 0, 5), rec("s2", 16, 1, 7), rec("s2", 0, 0, 3), rec("s2", 0, 2, 9), rec("s3", 4, -1, -1), rec("s4", 0, 0, 1), rec("s4", R1F, 0, 2, 30),
                           rec("s4", R2R, 0, 30, 2), rec("s5", 0, 1, 1)],
    "names_single_first": lambda: [rec("r x", 0, 0, 5), rec("r", 0, 0, 6), rec("r y", 0, 0, 7), rec("r", 0, 0, 8), rec("z", 0, 0, 1)],
    "names_paired_first": lambda: [rec("r x", R1F, 0, 50, 90), rec("r", R1F, 0, 10, 40), rec("r y", R2R, 0, 90, 50), rec("r", R2R, 0, 40, 10), rec("z", 0, 0, 1)],
    "soft_after_unpaired": lambda: [rec("q", 0, 0, 1), rec("q", 0, 0, 2)] + firsts_then_seconds("q z", [(0, 50, 90), (0, 10, 40)]) + [rec("v", 0, 0, 1), rec("v 1", 0, 0, 2)]
                                   + firsts_then_seconds("v 2", [(1, 50, 90), (1, 10, 40)]) + [rec("u", 0, 0, 3)],
    "soft_after_paired": lambda: proper("w", 0, 50, 90) + proper("w k", 0, 10, 40) + [rec("y", 0, 0, 1)] + firsts_then_seconds("x", [(0, 50, 90)])
                                 + firsts_then_seconds("x j", [(0, 10, 40), (0, 5, 45)]),
    "proper_apart": lambda: [rec("p", R1F, 0, 10, 60), rec("p", U1, -1, -1), rec("p", R2R, 0, 60, 10), rec("p", U2, -1, -1)] + [rec("o", 0, 0, 1)],
    "firsts_then_seconds": lambda: firsts_then_seconds("m", [(1, 300, 400), (0, 200, 250), (1, 100, 500), (0, 20, 25, True)]) + firsts_then_seconds("n", [(2, 30, 40), (2, 3, 4)]),
    "keys": lambda: firsts_then_seconds("k", [(1, 100, 200), (0, 100, 200), (0, 100, 201), (0, 99, 200), (0, 100, 200, True), (0, 200, 100), (0, 200, 100, True)]),
    "mpos_minus_one": lambda: [rec("n", R1F, 0, 7, 3), rec("n", R1F, 0, 5, -1), rec("n", R2R, 0, 3, 7), rec("n", R2R, 0, 2, -1)],
    "partials": lambda: [r for k, s in enumerate(SHAPES) for r in partial_group("g%d" % k, *s)],
    "partials_with_both": lambda: partial_group("h", 3, 1, 2, firsts_then_seconds("h", [(0, 50, 90), (0, 10, 40), (0, 10, 40)])) + partial_group("i", 1, 2, 1, proper("i", 1, 5, 9)),
    "error_mixed": lambda: proper("a", 0, 1, 20) + [rec("b", R1F, 0, 1, 20), rec("b", 0, 0, 5), rec("b", R2R, 0, 20, 1)] + proper("c", 0, 1, 20),
    "error_odd_full": lambda: proper("a", 0, 1, 20) + proper("b", 0, 1, 20) + [rec("b", R1F, 0, 3, 30), rec("b", U1, -1, -1)] + proper("c", 0, 1, 20),
    "error_odd_partial": lambda: [rec("a", 0, 0, 1)] + proper("b", 0, 1, 20) + [rec("b", U1, -1, -1), rec("b", U2, -1, -1), rec("b", PU, 0, 4)],
    "error_mixed_before_odd": lambda: [rec("b", R1F, 0, 1, 20), rec("b x", 0, 0, 5)],
    "both16": lambda: ties("e", 8) + [rec("f", 0, 0, 1)],
    "both18": lambda: ties("e", 9) + [rec("f", 0, 0, 1)],
    "both40": lambda: [rec("d", 0, 0, 1)] + ties("e", 20),
}


def sam_line(r, k):
    unmapped = bool(r.flag & 4)
    f = [r.name.decode(), str(r.flag), TARGETS[r.tid][0] if r.tid >= 0 else "*", str(r.pos + 1), "255" if r.tid >= 0 else "0", "*" if unmapped else "4M",
         "=" if r.flag & 1 and r.tid >= 0 and r.mpos >= 0 else "*", str(r.mpos + 1), "0", "ACGT", "IIII", "XI:i:%d" % k]
    return "\t".join(f)


def keep(name, data):
    path = os.path.join(HERE, name)
    for p in (path, path + ".gz"):
        if os.path.exists(p):
            os.remove(p)
    if len(data) > 1024:
        with open(path + ".gz", "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
            g.write(data)
    else:
        open(path, "wb").write(data)


def run(prog, in_bytes):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "aln"), "wb").write(in_bytes)
        r = subprocess.run(["rsem-scan-for-paired-end-reads", "1", "aln", "out.bam"], executable=os.path.abspath(prog), cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out = gr.bgzf_inflate(open(os.path.join(tmp, "out.bam"), "rb").read()) if r.returncode == 0 else None
        return r.stdout, r.stderr, r.returncode, out


def main():
    prog = sys.argv[1]
    os.makedirs(HERE, exist_ok=True)
    head = ["@HD\tVN:1.0\tSO:queryname"] + ["@SQ\tSN:%s\tLN:%d" % t for t in TARGETS] + ["@PG\tID:aligner\tVN:1", "@CO\ta comment"]
    text = "".join(l + "\n" for l in head)
    ids = {n: i for i, (n, _) in enumerate(TARGETS)}
    results = {}
    with tempfile.TemporaryDirectory() as stage:
        for case in sorted(CASES):
            recs = CASES[case]()
            lines = [sam_line(r, k) for k, r in enumerate(recs)]
            raw = gr.bam_header(text)
            for l in lines:
                d = gr.encode_sam_line(l, ids)
                raw += struct.pack("<i", len(d)) + d
            files = {".bam": bgzf(raw), ".sam": ("\n".join(head + lines) + "\n").encode()}
            outs = {ext: run(prog, data) for ext, data in files.items()}
            assert outs[".sam"] == outs[".bam"], case
            # the restatement says the same, byte for byte (the two large cases: up to the order inside tie runs)
            for ext, data in files.items():
                path = os.path.join(stage, case + ext)
                open(path, "wb").write(data)
                assert [pr.parse_record(d) for d in gr.read_alignments(path)[2]] == recs, (case, ext)
                so, se, st, out = pr.scan(path)
                assert (so, se, st) == outs[ext][:3], (case, ext, so, se, st, outs[ext][:3])
                assert (out is None) == (outs[ext][3] is None) and (out is None or pr.same_output(case, out, outs[ext][3])), (case, ext)
                if case not in pr.LARGE_CASES:
                    assert out == outs[ext][3], (case, ext)
            results[case] = (files, outs[".bam"], len(recs))
    for case, (files, (so, se, st, out), n) in results.items():
        for ext, data in files.items():
            open(os.path.join(HERE, case + ext), "wb").write(data)
        keep(case + ".stdout", so)
        keep(case + ".stderr", se)
        keep(case + ".status", b"%d\n" % st)
        if out is not None:
            keep(case + ".out", out)
        print(case, n, "records, status", st)


if __name__ == "__main__":
    main()
