"""Writes tests/golden/gbam/: a small genome-derived reference (ref.ti, ref.chrlist), transcript alignment files, and what the
UNMODIFIED reference program (tbam2gbam.cpp, BamConverter.h, bc_aux.h; g++ -O3, linked against htslib 1.3) wrote for them.

    python tests/golden/make_gbam_golden.py /path/to/rsem-tbam2gbam

Every case is written as SAM text and, the same records, as BAM (BGZF from zlib and struct; a case that holds what SAM text cannot say
-- a ZW of type d -- as BAM only).  The reference program is run in a scratch directory as
    rsem-tbam2gbam ref aln out.bam          (argv[0] the bare name, `aln` a copy of the input)
so that the @PG CL: it records is the same for both inputs and can be reproduced; on SAM and BAM input it must write the same
records.  Recorded per case: <case>.genome, the DECOMPRESSED output (header, dictionary, records); a file above 1 KiB is kept
gzip-compressed (<name>.gz, no time stamp inside).  The inputs come from fixed seeds; the expected outputs are recorded, not computed.
"""
import gzip
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gmap_ref as gr  # noqa: E402  (tests/gmap_ref.py: the SAM -> BAM record encoder and the BGZF reader)

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gbam")
POLYA = 125

# ---- the reference: structures, each on '+' (<name>_p) and on '-' (<name>_m) -------------------------------------------------------

STRUCT = [  # name, chromosome, exons
    ("one", "chrB", [(1001, 1400)]),
    ("touch", "chrB", [(5001, 5100), (5101, 5200)]),                       # two exons that touch: 0N
    ("tiny", "chrB", [(7001, 7050), (7101, 7101), (7201, 7300)]),          # a 1-base exon
    ("many", "chrC", [(1001 + 30 * k, 1010 + 30 * k) for k in range(70)]),  # 70 exons of 10 bases
    ("edge14", "chrA", [(16300, 16500)]),                                   # across the bin edge 2^14
    ("edge17", "chrA", [(130900, 131000), (131040, 131300)]),               # across 2^17
    ("edge28", "chrA", [(268435300, 268435420), (268435440, 268435520)]),   # around 2^28
    ("tail", "chrA", [(32769, 32800), (49100, 49152)]),                     # poly-A reads land on 49152 ('+') and 32768 ('-'): the bin of an empty range
]
ISO = [  # isoforms that share a locus, '+' only
    ("iso1", "chrB", [(20001, 20100), (20201, 20300), (20401, 20500)]),
    ("iso2", "chrB", [(20001, 20100), (20201, 20300)]),
    ("iso3", "chrB", [(20001, 20100), (20201, 20300), (20421, 20520)]),
    ("iso4", "chrB", [(20001, 20300)]),                                      # the intron retained
    ("isoC", "chrC", [(20001, 20100), (20201, 20300), (20401, 20500)]),     # the same structure on another chromosome
]
CHRLIST = ["chrC\t60000", "chrA\t300000000\tsecond column's quirk", "chrB\t200000"]  # not in the order of first use; a third column


def transcripts():
    out = []
    for name, chrom, exons in STRUCT:
        for s in "+-":
            out.append(dict(tid="%s_%s" % (name, "p" if s == "+" else "m"), chrom=chrom, strand=s, exons=exons))
    for name, chrom, exons in ISO:
        out.append(dict(tid=name, chrom=chrom, strand="+", exons=exons))
    for t in out:
        t["length"] = sum(e - s + 1 for s, e in t["exons"])
    return out


def ti_text(ts, typ=0):
    lines = ["%d %d" % (len(ts), typ)]
    for t in ts:
        lines += [t["tid"] + "\t" + t["tid"].upper(), "gene_" + t["tid"].split("_")[0], t["chrom"], "%s %d" % (t["strand"], t["length"]),
                  " ".join([str(len(t["exons"]))] + ["%d %d" % e for e in t["exons"]]), ""]
    return "\n".join(lines) + "\n"


# ---- records ------------------------------------------------------------------------------------------------------------------------

class Maker:
    def __init__(self, ts, seed):
        self.ts = {t["tid"]: t for t in ts}
        self.rng = random.Random(seed)
        self.lines = []
        self.raw_tags = {}  # line index -> bytes appended to the BAM record only

    def seq(self, n):
        return "".join(self.rng.choice("ACGTACGTACGTN") for _ in range(n)), "".join(chr(33 + self.rng.randrange(2, 41)) for _ in range(n))

    def aln(self, name, tr, pos, n, flag=0, tags=("ZW:f:1",), mate=None, seq=None, raw=None):
        """an alignment of n bases at 0-based pos of transcript tr; mate: (pos of the mate, tlen)"""
        s, q = seq or self.seq(n)
        f = [name, str(flag), tr, str(pos + 1), "255", "%dM" % n, "=" if mate else "*", str(mate[0] + 1) if mate else "0", str(mate[1]) if mate else "0", s, q]
        if raw is not None:
            self.raw_tags[len(self.lines)] = raw
        self.lines.append("\t".join(f + list(tags)))
        return s, q

    def unmapped(self, name, n, flag=4):
        s, q = self.seq(n)
        self.lines.append("\t".join([name, str(flag), "*", "0", "0", "*", "*", "0", "0", s, q, "YT:Z:UU"]))

    def pair(self, name, tr, p1, p2, n, tags=("ZW:f:1",), rev=False, second_first=False):
        f1, f2 = (0x1 | 0x2 | 0x40 | (0x10 if rev else 0x20)), (0x1 | 0x2 | 0x80 | (0x20 if rev else 0x10))
        tl = max(p1, p2) + n - min(p1, p2)
        a = lambda: self.aln(name, tr, p1, n, f1, tags, (p2, tl if p1 <= p2 else -tl))
        b = lambda: self.aln(name, tr, p2, n, f2, tags, (p1, -tl if p1 <= p2 else tl))
        (b(), a()) if second_first else (a(), b())


def header(ts, order_seed):
    sq = ["@SQ\tSN:%s\tLN:%d" % (t["tid"], t["length"] + POLYA) for t in ts]
    random.Random(order_seed).shuffle(sq)  # the input's ids are NOT the .ti's order: transcripts are found by name
    return ["@HD\tVN:1.0\tSO:unsorted"] + sq + ["@RG\tID:g1\tSM:s", "@PG\tID:aligner\tVN:1", "@CO\ta comment", "@XY\tan:unknown record"]


def case_se(ts):
    m = Maker(ts, 1)
    for sfx in ("_p", "_m"):
        one, tiny, many, touch = "one" + sfx, "tiny" + sfx, "many" + sfx, "touch" + sfx
        m.aln("inside" + sfx, one, 10, 30, tags=("ZW:f:1", "MD:Z:12A17"))
        m.aln("ends_on_last" + sfx, tiny, 20, 30)
        m.aln("starts_on_first" + sfx, tiny, 51, 20)
        m.aln("starts_on_tiny" + sfx, tiny, 50, 25)
        m.aln("j2" + sfx, tiny, 40, 30)
        m.aln("j3" + sfx, many, 5, 30)
        m.aln("j69" + sfx, many, 5, 690)
        m.aln("whole" + sfx, many, 0, 700)
        m.aln("touching" + sfx, touch, 90, 20)
        for k, p in enumerate((0, 399)):
            m.aln("len1_%d%s" % (k, sfx), one, p, 1)
        m.aln("len1_tiny" + sfx, tiny, 50, 1)
        for k, (p, n) in enumerate(((24, 60), (50, 34), (50, 35), (50, 36), (84, 1), (85, 1))):   # genomic 16384 = base 85 of '+'
            m.aln("e14_%d%s" % (k, sfx), "edge14" + sfx, p, n)
        for k, (p, n) in enumerate(((80, 100), (100, 32), (100, 33), (100, 34), (132, 20))):      # 131072 = base 133 of '+'
            m.aln("e17_%d%s" % (k, sfx), "edge17" + sfx, p, n)
        for k, (p, n) in enumerate(((100, 60), (121, 17), (137, 1), (138, 30), (0, 202))):        # 2^28 = 268435456 = base 138 of '+'
            m.aln("e28_%d%s" % (k, sfx), "edge28" + sfx, p, n)
        m.aln("off_by_1" + sfx, one, 371, 30, tags=("ZW:f:1", "MD:Z:30"))
        m.aln("off_by_9" + sfx, many, 680, 29)
        m.aln("all_tail" + sfx, one, 400, 20)
        m.aln("all_tail_1" + sfx, one, 410, 1)
        m.aln("all_tail_edge" + sfx, "tail" + sfx, 85, 8)
        m.aln("tail_edge_off" + sfx, "tail" + sfx, 70, 30)
        m.aln("rev_read" + sfx, tiny, 40, 30, flag=16)
    return m


def case_pe(ts):
    m = Maker(ts, 2)
    for sfx in ("_p", "_m"):
        m.pair("ov_tiny" + sfx, "tiny" + sfx, 30, 45, 30)
        m.pair("ov_many" + sfx, "many" + sfx, 100, 130, 75, rev=True)
        m.pair("ov_one" + sfx, "one" + sfx, 350, 380, 40)                # mate 2 hangs off the end
        m.pair("second_first" + sfx, "touch" + sfx, 80, 95, 25, second_first=True)
        m.pair("same_place" + sfx, "edge17" + sfx, 90, 90, 50)
    m.pair("multi", "iso1", 50, 120, 60, tags=("ZW:f:0.25",))
    m.pair("multi", "iso2", 50, 120, 60, tags=("ZW:f:0.5",))
    m.pair("multi", "iso3", 50, 120, 60, tags=("ZW:f:0.125",))
    m.pair("multi", "iso4", 50, 220, 60, tags=("ZW:f:0.125",))
    return m


def case_collapse(ts):
    m = Maker(ts, 3)
    sq = m.seq(40)
    m.aln("g1", "iso1", 10, 40, seq=sq)
    m.aln("g2", "iso1", 10, 40, tags=("ZW:f:0.6",), seq=sq)
    m.aln("g2", "iso2", 10, 40, tags=("ZW:f:0.4",), seq=sq)
    for tr, w in (("iso4", "0.0625"), ("iso1", "0.3"), ("isoC", "0.0375"), ("iso2", "0.2"), ("iso3", "0.4")):  # 3 equal, 1 other n_cigar, 1 other tid
        m.aln("g5", tr, 80, 40, tags=("ZW:f:" + w, "NM:i:1"), seq=sq)
    for w in ("0.1", "0.2", "0.3", "0.4"):
        m.aln("all_equal", "iso1", 150, 40, tags=("ZW:f:" + w,), seq=sq)
    for k, p in enumerate((70, 50, 60, 40)):  # descending and mixed: the order comes from the key
        m.aln("all_distinct", "iso1", p, 40, tags=("ZW:f:0.25", "XI:i:%d" % k), seq=sq)
    m.aln("only_tid", "isoC", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_tid", "iso1", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_pos", "iso1", 81, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_pos", "iso1", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_strand", "iso1", 80, 40, flag=16, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_strand", "iso1", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_n_cigar", "iso1", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_n_cigar", "iso4", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_last_word", "iso1", 80, 41, tags=("ZW:f:0.5",))
    m.aln("only_last_word", "iso1", 80, 40, tags=("ZW:f:0.5",), seq=sq)
    m.aln("only_an_n", "iso3", 180, 40, tags=("ZW:f:0.5",), seq=sq)   # 100N against 120N
    m.aln("only_an_n", "iso1", 180, 40, tags=("ZW:f:0.5",), seq=sq)
    for tr, w in (("iso1", "1"), ("iso4", "5.9604645e-08"), ("iso2", "5.9604645e-08"), ("iso4", "0.1"), ("iso3", "5.9604645e-08")):  # runs interleaved, order-sensitive weights
        m.aln("interleaved", tr, 80, 40, tags=("ZW:f:" + w,), seq=sq)
    m.aln("two words name", "iso1", 10, 40, tags=("ZW:f:0.5",), seq=sq)   # the group's name is its first word
    m.aln("two other", "iso2", 10, 40, tags=("ZW:f:0.5",), seq=sq)
    return m


def case_collapse_pe(ts):
    m = Maker(ts, 4)
    m.pair("only_mate2", "iso1", 10, 60, 30, tags=("ZW:f:0.5",))
    m.pair("only_mate2", "iso1", 10, 50, 30, tags=("ZW:f:0.5",))
    m.pair("equal_pairs", "iso2", 10, 120, 30, tags=("ZW:f:0.25",))
    m.pair("equal_pairs", "iso1", 10, 120, 30, tags=("ZW:f:0.5",))
    m.pair("equal_pairs", "iso3", 10, 120, 30, tags=("ZW:f:0.25",))
    # mate 1 decides before mate 2 is looked at: 100N < 120N although the second pair's mate 2 lies further left
    m.pair("mate1_first", "iso3", 180, 150, 40, tags=("ZW:f:0.5",))
    m.pair("mate1_first", "iso1", 180, 100, 40, tags=("ZW:f:0.5",))
    return m


def case_tags(ts):
    m = Maker(ts, 5)
    sq = m.seq(30)
    m.aln("no_zw", "tiny_p", 40, 30, tags=("NM:i:0",))
    m.aln("no_zw_merged", "iso1", 10, 30, tags=(), seq=sq)
    m.aln("no_zw_merged", "iso2", 10, 30, tags=(), seq=sq)
    m.aln("zw_i", "tiny_m", 40, 30, tags=("ZW:i:5", "NM:i:300", "YT:Z:UU"))      # four bytes go over a one-byte payload
    m.aln("zw_i_last", "tiny_p", 40, 30, tags=("NM:i:3", "ZW:i:5"))              # ... the XS:A that follows included
    m.aln("xs_a", "tiny_p", 40, 30, tags=("XS:A:-", "ZW:f:1"))
    m.aln("xs_i_no_n", "one_m", 40, 30, tags=("ZW:f:1", "XS:i:4", "NM:i:2"))
    m.aln("xs_twice", "tiny_m", 40, 30, tags=("XS:i:4", "ZW:f:1", "XS:A:+"))
    for sfx in ("_p", "_m"):
        m.aln("md_hat" + sfx, "one" + sfx, 40, 30, tags=("MD:Z:10A5^AC6T7", "ZW:f:1"))
        m.aln("md_lower" + sfx, "one" + sfx, 40, 30, tags=("ZW:f:1", "MD:Z:0n10N0^acgt3T0"))
        m.aln("md_letters_end" + sfx, "one" + sfx, 40, 30, tags=("ZW:f:1", "MD:Z:29R"))
        m.aln("md_hat_last" + sfx, "one" + sfx, 40, 30, tags=("ZW:f:1", "MD:Z:29^GA"))
        m.aln("md_not_z" + sfx, "one" + sfx, 40, 30, tags=("MD:i:7", "ZW:f:1", "MD:Z:30"))
    for name, ws in (("sum_1", ("0.5", "0.5")), ("sum_above_1", ("0.7", "0.4")), ("sum_0p9", ("0.4", "0.5")), ("sum_0", ("0", "0")),
                     ("sum_almost_1", ("0.5", "0.49999997")), ("sum_1_minus_1e-10", ("0.9999999", "0.0000001"))):
        for tr, w in zip(("iso1", "iso2"), ws):
            m.aln(name, tr, 10, 30, tags=("ZW:f:" + w,), seq=sq)
    m.aln("half", "one_p", 5, 30, tags=("ZW:f:0.5",))
    return m


def case_tags_d(ts):
    m = Maker(ts, 6)
    sq = m.seq(30)
    for tr, x in (("iso1", 0.1), ("iso2", 0.7)):  # narrowed to float, added, and the float written over the first half of the double
        m.aln("zw_d", tr, 10, 30, tags=("NM:i:1",), seq=sq, raw=b"ZWd" + struct.pack("<d", x) + b"YTZUU\0")
    m.aln("zw_d_minus", "tiny_m", 40, 30, tags=(), raw=b"ZWd" + struct.pack("<d", 0.3))
    return m


def case_unmapped(ts):
    m = Maker(ts, 7)
    sq = m.seq(30)
    m.unmapped("u_first", 30)
    m.unmapped("u_second", 20)
    m.aln("g_a", "iso1", 10, 30, tags=("ZW:f:0.5",), seq=sq)
    m.aln("g_a", "iso2", 10, 30, tags=("ZW:f:0.5",), seq=sq)
    m.unmapped("u_between", 30)
    m.aln("g_b", "tiny_m", 40, 30)
    m.aln("g_c", "tiny_p", 40, 30)
    m.unmapped("u_last", 25)
    return m


def case_unmapped_pe(ts):
    m = Maker(ts, 8)
    for name in ("u_first",):
        m.unmapped(name, 30, 77)
        m.unmapped(name, 30, 141)
    m.pair("g_a", "iso1", 10, 60, 30, tags=("ZW:f:0.5",))
    m.pair("g_a", "iso2", 10, 60, 30, tags=("ZW:f:0.5",))
    m.unmapped("u_between", 30, 141)  # read 2 first
    m.unmapped("u_between", 30, 77)
    m.pair("g_b", "many_m", 100, 160, 75)
    m.unmapped("u_last", 30, 77)
    m.unmapped("u_last", 30, 141)
    return m


def case_unmapped_only(ts):
    m = Maker(ts, 9)
    for k in range(5):
        m.unmapped("u%d" % k, 20 + k)
    return m


def case_header_only(ts):
    return Maker(ts, 10)


CASES = [("se", case_se), ("pe", case_pe), ("collapse", case_collapse), ("collapse_pe", case_collapse_pe), ("tags", case_tags), ("tags_d", case_tags_d),
         ("unmapped", case_unmapped), ("unmapped_pe", case_unmapped_pe), ("unmapped_only", case_unmapped_only), ("header_only", case_header_only)]


# ---- files ------------------------------------------------------------------------------------------------------------------------

def bgzf(data, block=3000):
    """small blocks: records straddle them"""
    out = b""
    for i in list(range(0, len(data), block)) + [None]:
        chunk = b"" if i is None else data[i:i + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp
        out += struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    return out


def bam_bytes(head, m):
    text = "".join(l + "\n" for l in head)
    ids = {n: i for i, (n, _) in enumerate(gr.parse_sq(text))}
    raw = gr.bam_header(text)
    for k, line in enumerate(m.lines):
        r = gr.encode_sam_line(line, ids) + m.raw_tags.get(k, b"")
        raw += struct.pack("<i", len(r)) + r
    return bgzf(raw)


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


def run_reference(prog, in_bytes):
    with tempfile.TemporaryDirectory() as tmp:
        for n in ("ref.ti", "ref.chrlist"):
            shutil.copy(os.path.join(HERE, n), tmp)
        open(os.path.join(tmp, "aln"), "wb").write(in_bytes)
        subprocess.run(["rsem-tbam2gbam", "ref", "aln", "out.bam"], executable=os.path.abspath(prog), cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        return gr.bgzf_inflate(open(os.path.join(tmp, "out.bam"), "rb").read())


def main():
    prog = sys.argv[1]
    os.makedirs(HERE, exist_ok=True)
    ts = transcripts()
    open(os.path.join(HERE, "ref.ti"), "w").write(ti_text(ts))
    open(os.path.join(HERE, "ref.chrlist"), "w").write("".join(l + "\n" for l in CHRLIST))
    open(os.path.join(HERE, "standalone.ti"), "w").write(ti_text(ts[:2], typ=1))  # a reference without a genome: the program refuses it
    for k, (case, make) in enumerate(CASES):
        m = make(ts)
        head = header(ts, 100 + k)
        bam = bam_bytes(head, m)
        open(os.path.join(HERE, case + ".bam"), "wb").write(bam)
        got = run_reference(prog, bam)
        if not m.raw_tags:
            sam = ("\n".join(head + m.lines) + "\n").encode()
            open(os.path.join(HERE, case + ".sam"), "wb").write(sam)
            assert run_reference(prog, sam) == got, case
        keep(case + ".genome", got)
        print(case, len(m.lines), "records in,", len(gr.split_bam(got)[2]), "out,", len(got), "bytes")


if __name__ == "__main__":
    main()
