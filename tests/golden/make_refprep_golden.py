#!/usr/bin/env python3
"""Record tests/golden/refprep/: small inputs for the three reference-preparation programs and what the UNMODIFIED reference
programs write for them (files, stderr, exit status).

    python tests/golden/make_refprep_golden.py [dir with the reference programs, default oracle/_ref]

Every case runs in a scratch directory under fixed names (the reference is always `ref`), so that the recorded messages do not
depend on where this was run.  Per case: the inputs as they are, case.json (program, arguments, exit status, the names of the
outputs), stderr.txt, and the outputs under out/ -- gzip-compressed without a time stamp when above 1 KiB."""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "refprep")
PROGRAMS = {"extract": "rsem-extract-reference-transcripts", "synthesis": "rsem-synthesis-reference-transcripts", "preref": "rsem-preref"}


def wrap(seq, width):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


def ragged(seq, widths):
    out, i, k = "", 0, 0
    while i < len(seq):
        w = widths[k % len(widths)]
        out += seq[i:i + w] + "\n"
        i += w
        k += 1
    return out


def bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def gtf_line(chrom, source, feature, start, end, strand, attrs):
    return "%s\t%s\t%s\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom, source, feature, start, end, strand, attrs)


def ids(g, t, extra=""):
    return 'gene_id "%s"; transcript_id "%s";%s' % (g, t, extra)


def basic_genome():
    rng = random.Random(11)
    c1 = bases(rng, 40) + "acgtnnacgt" + bases(rng, 20) + "RYxkNNnn" + bases(rng, 42)            # 120
    c2 = bases(rng, 12) + "nNrY" + bases(rng, 14, "ACGTacgt")                                   # 30
    c3 = bases(rng, 300, "ACGTacgtNnRyx")
    return c1, c2, c3


def basic_gtf():
    g = "# a comment line\n"
    g += gtf_line("chr1", "srcA", "exon", 30, 40, "+", ids("g1", "t1"))
    g += gtf_line("chr1", "srcA", "exon", 1, 10, "+", ids("g1", "t1", ' gene_name "GeneOne";'))
    g += gtf_line("chr1", "srcA", "CDS", 1, 10, "+", ids("g1", "t1"))
    g += gtf_line("chr1", "srcA", "exon", 20, 20, "+", ids("g1", "t1", ' transcript_name "TxOne"; note "a;b";'))
    g += gtf_line("chr1", "srcA", "exon", 41, 50, "+", ids("g1", "t1"))
    g += gtf_line("chr1", "srcA", "exon", 45, 60, "+", ids("g1", "t1", ' gene_name "GeneOne";'))
    g += gtf_line("chr1", "srcB", "exon", 100, 120, "-", "  " + ids("g1", "t2"))
    g += gtf_line("chr1", "srcB", "exon", 5, 15, "-", "   " + ids("g1", "t2", " # a comment"))
    g += "chr2\tsrcB\texon\t3\t9\t.\t-\t.\t\t" + ids("g0", "t3") + "\n"  # a tab in front of the attributes
    g += gtf_line("chr2", "srcB", "exon", 12, 30, "-", ids("g0", "t3"))
    for k in range(70):
        g += gtf_line("chr3", "srcA", "exon", 1 + 4 * k, 2 + 4 * k, "+", ids("g9", "t70"))
    for k in range(5):
        g += gtf_line("chr3", "srcA", "exon", 290 - 20 * k, 300 - 20 * k, "-", ids("g9", "t71"))
    g += gtf_line("chrX", "srcA", "exon", 3, 9, "+", ids("g5", "tX"))
    g += gtf_line("chr1", "srcA", "exon", 9, 3, "+", ids("g1", "t1"))
    g += gtf_line("chr1", "srcA", "exon", 0, 3, "+", ids("g1", "t1"))
    g += gtf_line("chr1", "srcA", "exon", 70, 80, "+", ids("g1", "t0"))
    return g


def cases():
    c1, c2, c3 = basic_genome()
    genome = ">chr1 the first\n" + wrap(c1, 60) + ">chr2\n" + wrap(c2, 1) + ">chr3\tragged\n" + ragged(c3, [7, 13, 1, 25, 0, 31])
    gtf = basic_gtf()
    C = {}
    C["basic"] = ("extract", {"genome.fa": genome, "a.gtf": gtf}, ["ref", "0", "a.gtf", "None", "0", "genome.fa"])
    C["basic_quiet_nonl"] = ("extract", {"genome.fa": genome[:-1], "a.gtf": gtf}, ["ref", "1", "a.gtf", "None", "0", "genome.fa"])
    C["sources"] = ("extract", {"genome.fa": genome, "a.gtf": gtf}, ["ref", "1", "a.gtf", "srcB,srcC", "0", "genome.fa"])
    mapping = "# gene transcript\nG_A\tt1\nG_A t2\nG_B\tt3\n\nG_C\tt70\nG_C\tt71\nG_D\ttX\nG_0\tt0\n"
    C["mapping"] = ("extract", {"genome.fa": genome, "a.gtf": gtf, "map.txt": mapping}, ["ref", "1", "a.gtf", "None", "1", "map.txt", "genome.fa"])
    small_gtf = gtf_line("chr1", "s", "exon", 2, 6, "+", ids("g1", "t1")) + gtf_line("chr1", "s", "exon", 9, 14, "+", ids("g1", "t1")) + \
        gtf_line("chr2", "s", "exon", 2, 9, "-", ids("g2", "t2"))
    dup = ">chr1\nACGTACGTACGTACGTACGTACG\n>chr1 again\nTTTTGGGGCCCCAAAA\n>\nGGGGGGGGGGGGGGGG\n>chr2\nACGTTGCAAC\n"
    C["dup"] = ("extract", {"g.fa": dup, "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["skipfile"] = ("extract", {"skip.fa": "chr1\nACGTACGTACGTACGTACGT\n>chr1\nTTTTTTTTTTTTTTTTTTTT\n", "g.fa": dup, "a.gtf": small_gtf},
                     ["ref", "1", "a.gtf", "None", "0", "skip.fa", "g.fa"])
    C["twofiles"] = ("extract", {"one.fa": ">chr2\nACGTTGCAAC\n", "two.fa": ">chr1\nACGTACGTAC\nGTACGTACGTACG", "a.gtf": small_gtf},
                     ["ref", "0", "a.gtf", "None", "0", "one.fa", "two.fa"])
    ok1 = ">chr1\nACGTACGTACGTACGTACGT\n"
    C["err_star"] = ("extract", {"g.fa": ">chr1\nACGTACGT\nACG*ACGT\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_cr"] = ("extract", {"g.fa": ">chr1\r\nACGT\r\nACGT\r\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_high"] = ("extract", {"g.fa": b">chr1\nACGTACGTACGTAC\nAC\xc3\xa9GT\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_unused_record"] = ("extract", {"g.fa": ok1 + ">chrU\nAC GT\n>chr2\nACGTTGCAAC\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_boundary_first"] = ("extract", {"g.fa": ">chr1\nACGTACGTAC\n>chr2\nAC*TTGCAAC\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_short_second"] = ("extract", {"g.fa": ok1 + ">chr1\nACGTACGTAC\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_strand"] = ("extract", {"g.fa": ok1, "a.gtf": small_gtf + "chr1\ts\texon\t2\t6\t.\t.\t.\t" + ids("g1", "t9") + "\n"}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_no_transcript_id"] = ("extract", {"g.fa": ok1, "a.gtf": small_gtf + gtf_line("chr1", "s", "exon", 2, 6, "+", 'gene_id "g1"; transcript_name "x";')},
                                 ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    C["err_no_transcripts"] = ("extract", {"g.fa": ">chr7\nACGTACGTACGTACGTACGT\n", "a.gtf": small_gtf}, ["ref", "1", "a.gtf", "None", "0", "g.fa"])
    tfa = ">tA some text\nACGTacgtNNrr\nACG\n>tB\nGGGCCC\n>tA\nTTTTTTTTTTTTTTTTT\n>tC\nacgtn\n"
    C["syn_mode0"] = ("synthesis", {"t.fa": tfa}, ["ref", "0", "0", "t.fa"])
    C["syn_mode1"] = ("synthesis", {"t.fa": tfa, "map.txt": "gX\ttA\ngX\ttC\ngA\ttB\n"}, ["ref", "1", "1", "map.txt", "t.fa"])
    C["syn_mode2"] = ("synthesis", {"t.fa": tfa, "map.txt": "gX\ttr1\ttA\ngX\ttr1\ttC\ngA\ttr0\ttB\n"}, ["ref", "1", "2", "map.txt", "t.fa"])
    C["syn_err_bad"] = ("synthesis", {"t.fa": ">tA\nACGT\nAC-GT\n"}, ["ref", "1", "0", "t.fa"])
    C["syn_err_mapping"] = ("synthesis", {"t.fa": tfa, "map.txt": "gX\ttA\n"}, ["ref", "1", "1", "map.txt", "t.fa"])
    rng = random.Random(5)
    pfa = ""
    for n in (1, 24, 25, 26, 32, 33, 64):
        pfa += ">len%d\n%s\n" % (n, bases(rng, n, "ACGTacgtNnRy*"))
    pfa += ">empty entry\n>multi line entry with  blanks \n" + wrap(bases(rng, 150, "ACGTacgtn"), 60) + "\n" + ">last\nACGTN"
    C["pre_choice0"] = ("preref", {"t.fa": pfa}, ["t.fa", "0", "ref"])
    C["pre_choice0_l3"] = ("preref", {"t.fa": pfa}, ["t.fa", "0", "ref", "-l", "3", "-q"])
    C["pre_choice0_l0"] = ("preref", {"t.fa": pfa}, ["t.fa", "0", "ref", "-l", "0", "-q"])
    C["pre_choice1"] = ("preref", {"t.fa": pfa}, ["t.fa", "1", "ref", "-q"])
    C["pre_choice2"] = ("preref", {"t.fa": pfa, "exc.txt": "len24 len33\nlast\nmulti\n"}, ["t.fa", "2", "ref", "-l", "5", "-f", "exc.txt", "-q"])
    C["pre_crlf"] = ("preref", {"t.fa": ">a\r\nacgtn*\r\nRY\n>b\nAC\n"}, ["t.fa", "0", "ref", "-l", "3", "-q"])
    return C


def main():
    refdir = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "oracle", "_ref"))
    shutil.rmtree(OUT, ignore_errors=True)
    for name, (prog, files, args) in sorted(cases().items()):
        dst = os.path.join(OUT, name)
        os.makedirs(dst)
        with tempfile.TemporaryDirectory() as tmp:
            for fn, data in files.items():
                data = data if isinstance(data, bytes) else data.encode()
                for d in (tmp, dst):
                    with open(os.path.join(d, fn), "wb") as f:
                        f.write(data)
            r = subprocess.run([os.path.join(refdir, PROGRAMS[prog])] + args, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
            outs = sorted(fn for fn in os.listdir(tmp) if fn.startswith("ref."))
            if outs:
                os.makedirs(os.path.join(dst, "out"))
            for fn in outs:
                with open(os.path.join(tmp, fn), "rb") as f:
                    data = f.read()
                if len(data) > 1024:
                    with open(os.path.join(dst, "out", fn + ".gz"), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as z:
                        z.write(data)
                else:
                    with open(os.path.join(dst, "out", fn), "wb") as f:
                        f.write(data)
            with open(os.path.join(dst, "stderr.txt"), "wb") as f:
                f.write(r.stderr)
            with open(os.path.join(dst, "case.json"), "w") as f:
                json.dump({"program": prog, "args": args, "status": r.returncode, "outputs": outs}, f, indent=1)
                f.write("\n")
        print("%-24s %-9s status %3d  %d outputs, %d bytes of stderr" % (name, prog, r.returncode, len(outs), len(r.stderr)))


if __name__ == "__main__":
    main()
