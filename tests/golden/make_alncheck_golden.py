"""Writes tests/golden/alncheck/: small name-grouped alignment files and what the UNMODIFIED reference programs said about them.

    python tests/golden/make_alncheck_golden.py /path/to/rsem-sam-validator /path/to/rsem-get-unique

The two programs are compiled from the reference's untouched sources (samValidator.cpp, getUnique.cpp) against the htslib 1.3 that
oracle/Makefile builds into oracle/_ref/libhts_ref.a, outside the repository:
    g++ -std=gnu++98 -w -O3 -I$REF -I$REF/samtools-1.3/htslib-1.3 -o rsem-sam-validator $REF/samValidator.cpp oracle/_ref/libhts_ref.a -lz -lpthread
    g++ -std=gnu++98 -w -O3 -I$REF -I$REF/samtools-1.3/htslib-1.3 -o rsem-get-unique    $REF/getUnique.cpp    oracle/_ref/libhts_ref.a -lz -lpthread
Nothing of them is kept here.

Every case is written as SAM text and, the same records, as BAM (BGZF blocks of 300 bytes: records straddle them); a case that holds
what htslib's SAM parser turns into something else -- a mapped record at position 0 or without CIGAR becomes unmapped there -- as BAM
only.  Recorded: <case>.stdout, what rsem-sam-validator printed (the same for both inputs), and for the get-unique cases <case>.unique,
the DECOMPRESSED output of `rsem-get-unique 1 <input> out.bam` (the same for both inputs); a file above 1 KiB is kept gzip-compressed
(<name>.gz, no time stamp inside).  The expected outputs are recorded, not computed."""
import gzip
import os
import struct
import subprocess
import sys
import tempfile
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import alncheck_ref as ar  # noqa: E402
import gmap_ref as gr  # noqa: E402
from alncheck_ref import pair, rec  # noqa: E402

HERE = ar.GOLDEN
TARGETS = [("t1", 100), ("t2", 200), ("t3", 50)]
U1, U2 = 77, 141  # an unmapped pair's flags


def se_valid():
    r = [rec("r1", 0, 0, 5), rec("r2", 16, 1, 150, 50), rec("r2", 0, 0, 0, 50), rec("r2", 0, 2, 0, 50), rec("r3", 4, -1, -1, 12), rec("r4", 0, 0, 90, 10)]
    r += [rec("r5 first", 0, 0, 1), rec("r5 second", 0, 1, 2), rec("r5\tthird".replace("\t", " "), 0, 1, 3), rec("r6", 4, -1, -1, 7), rec("r6", 4, -1, -1, 7)]
    r += [rec("r7", 0, 1, 10, 12, [(4, "M"), (4, "="), (4, "X")]), rec("r8", 0, 2, 49, 1)]
    return r


def pe_valid():
    r = pair("p1", 0, 0, 30) + pair("p2", 1, 100, 150, 40, 50) + pair("p2", 0, 10, 40, 40, 50, rev=True) + pair("p2", 2, 0, 0, 40, 50, second_first=True)
    r += [rec("p3", U1, -1, -1, 10), rec("p3", U2, -1, -1, 10)] + [rec("p4", U2, -1, -1, 10), rec("p4", U1, -1, -1, 9)] + [rec("p4", U1, -1, -1, 9), rec("p4", U2, -1, -1, 10)]
    r += pair("p5 a", 0, 80, 90, name2="p5 b") + pair("p6", 0, 0, 90, 10, 10)
    return r


VALIDATOR = {
    "valid_se": se_valid, "valid_pe": pe_valid, "header_only": lambda: [],
    "aba": lambda: [rec("A", 0, 0, 0), rec("B", 0, 0, 0), rec("A", 0, 0, 0)],
    "aba_second_word": lambda: [rec("a 1", 0, 0, 0), rec("b", 0, 0, 0), rec("c", 0, 0, 0), rec("a 2", 0, 0, 0)],
    "aba_pe": lambda: pair("A") + pair("B") + pair("B") + pair("C") + pair("A"),
    "mixed_se": lambda: [rec("r1"), rec("r2")] + pair("r3"),
    "mixed_pe": lambda: pair("r1") + [rec("r2"), rec("r2")],
    "one_mate_end": lambda: pair("r1") + pair("r2")[:1],
    "one_mate_name": lambda: pair("r1") + pair("r2", name2="r3"),
    "one_mate_flag": lambda: pair("r1")[:1] + [rec("r1", 0x80, 0, 20)],
    "same_mate_number": lambda: [rec("r1", 0x1 | 0x40 | 0x20, 0, 0), rec("r1", 0x1 | 0x40 | 0x10, 0, 20)],
    "one_mate_aligned": lambda: pair("r0") + [rec("r1", 0x1 | 0x40 | 0x8, 0, 0), rec("r1", 0x1 | 0x80 | 0x4, -1, -1)],
    "discordant": lambda: pair("r1", 0, 0, 20, tid2=1, second_first=True),
    "same_strand_fwd": lambda: [rec("r1", 0x1 | 0x40, 1, 0), rec("r1", 0x1 | 0x80, 1, 20)],
    "same_strand_rev": lambda: [rec("r1", 0x1 | 0x80 | 0x10, 1, 0), rec("r1", 0x1 | 0x40 | 0x10, 1, 20)],
    "pair_boundary": lambda: pair("r1", 0, 60, 95, 10, 10, isize=41),
    "pair_boundary_fits": lambda: pair("r1", 0, 60, 90, 10, 10, isize=40),
    "pair_boundary_second_smaller": lambda: pair("r1", 2, 45, 10, 5, 5, isize=-41),
    "cigar_n": lambda: [rec("r0"), rec("r1", 0, 0, 0, 10, [(5, "M"), (10, "N"), (5, "M")])],
    "cigar_i": lambda: [rec("r1", 0, 0, 0, 10, [(4, "M"), (2, "I"), (4, "M")])],
    "cigar_d": lambda: [rec("r1", 0, 0, 0, 10, [(5, "M"), (2, "D"), (5, "M")])],
    "cigar_s": lambda: [rec("r1", 0, 0, 0, 10, [(2, "S"), (8, "M")])],
    "cigar_h": lambda: [rec("r1", 0, 0, 0, 10, [(2, "H"), (10, "M")])],
    "cigar_p": lambda: [rec("r1", 0, 0, 0, 10, [(5, "M"), (2, "P"), (5, "M")])],
    "cigar_two": lambda: [rec("r1", 0, 0, 0, 10, [(3, "M"), (2, "S"), (1, "I"), (4, "M")])],
    "cigar_mate2": lambda: pair("r1", 0, 0, 20, 10, 10, cigar2=[(4, "M"), (2, "I"), (4, "M")], second_first=True),
    "cigar_before_boundary": lambda: [rec("r1", 0, 0, 95, 10, [(8, "M"), (2, "S")])],
    "boundary_end_eq": lambda: [rec("r1", 0, 0, 90, 10), rec("r2", 0, 2, 40, 10, [(5, "="), (5, "X")])],
    "boundary_end_plus1": lambda: [rec("r1", 0, 0, 90, 10), rec("r2", 0, 0, 91, 10)],
    "boundary_mate2": lambda: pair("r1", 2, 0, 45, 10, 10, isize=0),
    "different_lengths_se": lambda: [rec("r1", 0, 0, 0, 10), rec("r1", 0, 1, 0, 10), rec("r1", 0, 0, 5, 11)],
    "different_lengths_pe": lambda: pair("r1", 0, 0, 20, 10, 12) + pair("r1", 1, 0, 20, 10, 11),
    "different_lengths_swapped": lambda: pair("r1", 0, 0, 20, 10, 12) + pair("r1", 1, 0, 20, 10, 12, second_first=True) + pair("r1", 1, 5, 25, 12, 10, second_first=True),
}
BAM_ONLY = {
    "boundary_pos_neg": lambda: [rec("r0"), rec("r1", 0, 0, -1, 10)],
    "no_cigar_mapped": lambda: [rec("r1", 0, 0, 99, 10, []), rec("r2", 0, 0, 100, 10, [])],
}
UNIQUE = {
    "valid_se": se_valid, "valid_pe": pe_valid, "header_only": lambda: [],
    "uniq_se": lambda: [rec("a"), rec("b"), rec("b", 0, 1), rec("c"), rec("c", 0, 1), rec("c", 0, 2), rec("d x"), rec("d y"), rec("e"), rec("e", 4, -1, -1), rec("f", 4, -1, -1),
                        rec("g"), rec("a")],
    "uniq_pe": lambda: pair("a") + pair("b") + pair("b", 1) + pair("c") + pair("c")[:1] + pair("d") + [rec("e", U1, -1, -1), rec("e", U2, -1, -1)] + pair("f", second_first=True),
    "unmapped_only": lambda: [rec("u%d" % k, 4, -1, -1, 10 + k) for k in range(5)],
}


def sam_line(r):
    cig = "".join("%d%s" % (w >> 4, ar.OPS[w & 15]) for w in r.cigar) or "*"
    paired = r.flag & 1 and r.tid >= 0
    f = [r.name.decode(), str(r.flag), TARGETS[r.tid][0] if r.tid >= 0 else "*", str(r.pos + 1), "255" if r.tid >= 0 else "0", cig, "=" if paired else "*", "1" if paired else "0",
         str(r.isize), "ACGT" * (r.lq // 4) + "ACGT"[:r.lq % 4], "I" * r.lq, "NM:i:0"]
    return "\t".join(f)


def bgzf(data, block=300):
    out = b""
    for i in list(range(0, len(data), block)) + [None]:
        chunk = b"" if i is None else data[i:i + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp
        out += struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    return out


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


def run(prog, name, argv, in_bytes, out=None):
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "aln"), "wb").write(in_bytes)
        r = subprocess.run([name] + argv, executable=os.path.abspath(prog), cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        assert r.returncode == 0, (name, r.returncode)
        return gr.bgzf_inflate(open(os.path.join(tmp, out), "rb").read()) if out else r.stdout


def main():
    validator, get_unique = sys.argv[1:3]
    os.makedirs(HERE, exist_ok=True)
    head = ["@HD\tVN:1.0\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % t for t in TARGETS] + ["@PG\tID:aligner\tVN:1", "@CO\ta comment"]
    text = "".join(l + "\n" for l in head)
    ids = {n: i for i, (n, _) in enumerate(TARGETS)}
    cases = dict(VALIDATOR, **BAM_ONLY)
    cases.update(UNIQUE)
    for case in sorted(cases):
        recs = cases[case]()
        lines = [sam_line(r) for r in recs]
        raw = gr.bam_header(text)
        for l in lines:
            d = gr.encode_sam_line(l, ids)
            raw += struct.pack("<i", len(d)) + d
        files = {".bam": bgzf(raw)}
        if case not in BAM_ONLY:
            files[".sam"] = ("\n".join(head + lines) + "\n").encode()
        for ext, data in files.items():
            open(os.path.join(HERE, case + ext), "wb").write(data)
        if case in VALIDATOR or case in BAM_ONLY:
            outs = {ext: run(validator, "rsem-sam-validator", ["aln"], data) for ext, data in files.items()}
            assert len(set(outs.values())) == 1, (case, outs)
            keep(case + ".stdout", outs[".bam"])
        if case in UNIQUE:
            outs = {ext: run(get_unique, "rsem-get-unique", ["1", "aln", "out.bam"], data, "out.bam") for ext, data in files.items()}
            assert len(set(outs.values())) == 1, case
            keep(case + ".unique", outs[".bam"])
        print(case, len(recs), "records")


if __name__ == "__main__":
    main()
