"""Writes tests/golden/wiggle/: small alignment files and the files that the UNMODIFIED reference programs (bam2wig.cpp,
bam2readdepth.cpp, wiggle.cpp; g++ -O3, linked against htslib 1.3) wrote for them.

    python tests/golden/make_wiggle_golden.py /path/to/rsem-bam2wig /path/to/rsem-bam2readdepth

Every case is written as SAM text and, the same records, as BAM (BGZF from zlib and struct); the reference programs are run on
both and must agree.  Recorded per case: <case>.wig, <case>.nfw.wig (--no-fractional-weight) and <case>.readdepth; a recorded file
above 1 KiB is kept gzip-compressed (<name>.gz, no time stamp inside).  Cases marked BAM-only hold what SAM text cannot say here (a
ZW of type d) or would only repeat at ten times the size (many_runs).
The inputs come from fixed seeds; the expected outputs are recorded, not computed here.
"""
import gzip
import os
import random
import struct
import subprocess
import sys
import zlib

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wiggle")
OPS = "MIDNSHP=X"


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def rec(name, flag, tid, pos, cigar, tags=(), mtid=-1, mpos=-1, tlen=0):
    """pos 0-based; tags: (tag, type, value) with type f, d, i, Z, A or Bc"""
    return dict(name=name, flag=flag, tid=tid, pos=pos, cigar=cigar, tags=list(tags), mtid=mtid, mpos=mpos, tlen=tlen)


def zw(x):
    return ("ZW", "f", f32(x))


def cigar_ops(c):
    out, n = [], ""
    for ch in c:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), OPS.index(ch)))
            n = ""
    return out


# ---- SAM text ----------------------------------------------------------------------------------------------------------------

def sam_text(targets, records):
    lines = ["@HD\tVN:1.0\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % t for t in targets]
    for r in records:
        rname = targets[r["tid"]][0] if r["tid"] >= 0 else "*"
        rnext = "*" if r["mtid"] < 0 else ("=" if r["mtid"] == r["tid"] else targets[r["mtid"]][0])
        f = [r["name"], str(r["flag"]), rname, str(r["pos"] + 1), "255" if r["tid"] >= 0 else "0", r["cigar"] or "*", rnext, str(r["mpos"] + 1),
             str(r["tlen"]), "*", "*"]
        for tag, ty, v in r["tags"]:
            if ty == "f":
                f.append("%s:f:%.9g" % (tag, v))
            elif ty == "d":
                raise ValueError("type d is written to BAM only")
            elif ty == "i":
                f.append("%s:i:%d" % (tag, v))
            elif ty == "Bc":
                f.append("%s:B:c,%s" % (tag, ",".join(str(x) for x in v)))
            else:
                f.append("%s:%s:%s" % (tag, ty, v))
        lines.append("\t".join(f))
    return ("\n".join(lines) + "\n").encode()


# ---- BAM -----------------------------------------------------------------------------------------------------------------------

def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def bam_record(r):
    ops = cigar_ops(r["cigar"]) if r["cigar"] else []
    rlen = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    end = r["pos"] + rlen if ops and not r["flag"] & 4 else r["pos"] + 1
    name = r["name"].encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(name), 255 if r["tid"] >= 0 else 0, reg2bin(r["pos"], end), len(ops), r["flag"], 0,
                       r["mtid"], r["mpos"], r["tlen"])
    body += name + b"".join(struct.pack("<I", n << 4 | o) for n, o in ops)
    for tag, ty, v in r["tags"]:
        body += tag.encode()
        if ty == "f":
            body += b"f" + struct.pack("<f", v)
        elif ty == "d":
            body += b"d" + struct.pack("<d", v)
        elif ty == "i":  # the smallest type that fits, as htslib's SAM parser chooses
            for code, fmt, lo, hi in (("C", "<B", 0, 255), ("c", "<b", -128, -1), ("S", "<H", 0, 65535), ("s", "<h", -32768, -1),
                                      ("I", "<I", 0, 2 ** 32 - 1), ("i", "<i", -2 ** 31, -1)):
                if lo <= v <= hi:
                    body += code.encode() + struct.pack(fmt, v)
                    break
        elif ty == "Bc":
            body += b"Bc" + struct.pack("<i", len(v)) + struct.pack("<%db" % len(v), *v)
        elif ty == "A":
            body += b"A" + v.encode()
        else:
            body += b"Z" + v.encode() + b"\0"
    return struct.pack("<i", len(body)) + body


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


def bam_bytes(targets, records):
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % t for t in targets)
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(targets))
    for name, ln in targets:
        raw += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return bgzf(raw + b"".join(bam_record(r) for r in records))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

WEIGHTS = [1.0, 0.1, 2.0 ** -24, 3e-7, 0.5, 0.25, 0.33333334, 0.9999999, 0.0123]


def case_sorted():
    r = random.Random(20240901)
    targets = [("unused_first", 50), ("chrA", 700), ("one", 1), ("chrB", 1300), ("unused_mid", 10), ("chrC", 513), ("unused_last", 2000)]
    recs = []
    for tid in (1, 2, 3, 5):
        ln = targets[tid][1]
        if ln == 1:
            recs += [rec("s_one_%d" % i, 0, tid, 0, "1M", [zw(w)]) for i, w in enumerate((0.3, 0.1, 0.7))]
            continue
        rows = []
        for i in range(30):
            w = r.choice(WEIGHTS)
            L = r.randint(20, 76)
            p = r.randint(0, ln - L)
            if r.random() < 0.5:
                rows.append((p, [rec("s%d_%d" % (tid, i), 16 * r.randint(0, 1), tid, p, "%dM" % L, [zw(w)])]))
            else:  # a pair; the mates overlap in one case of two
                L2 = r.randint(20, 76)
                p2 = min(ln - L2, p + (r.randint(0, L - 1) if r.random() < 0.5 else L + r.randint(0, 60)))
                t = p2 + L2 - p
                rows.append((p, [rec("p%d_%d" % (tid, i), 99, tid, p, "%dM" % L, [zw(w)], tid, p2, t),
                                 rec("p%d_%d" % (tid, i), 147, tid, p2, "%dM" % L2, [zw(w)], tid, p, -t)]))
        rows.sort(key=lambda x: x[0])
        for _, rr in rows:  # (mates stay next to each other, as in RSEM's own transcript.bam before sorting by coordinate)
            recs += rr
        recs.append(rec("s%d_first_base" % tid, 0, tid, 0, "1M", [zw(0.5)]))
        recs.append(rec("s%d_last_base" % tid, 0, tid, ln - 1, "1M", [zw(0.5)]))
    return targets, recs


def case_cigars():
    r = random.Random(5)
    targets = [("long", 6000), ("short", 40)]
    cigs = ["10M", "5S10M", "10M5S", "5H10M5H", "2H3S10M3S2H", "10M2I10M", "10M3D10M", "3M1P1I3M", "10=", "5X", "4=3M2X4M", "2S3M1I2M4D3M200N5M2S",
            "1I10M", "10M1I", "3D10M", "10M3D", "5N10M", "10M5N", "1P10M", "10M1P", "2=10M", "10M2=", "3X10M", "10M3X", "1M1I1M1D1M1N1M1S",
            "10M2100N10M", "7M600N7M1100N7M", "8=8X", "0M5M", "4M0M4M", "3I", "6S"]
    recs = []
    for i, c in enumerate(cigs * 2):
        rlen = sum(n for n, o in cigar_ops(c) if o in (0, 2, 3, 7, 8))
        p = r.randint(0, 6000 - rlen) if i >= len(cigs) else min(6000 - rlen, 37 * i)
        recs.append(rec("c%d" % i, 0, 0, p, c, [zw(r.choice(WEIGHTS))]))
    recs.append(rec("c_tile_edges", 0, 0, 500, "12M500N12M500N12M", [zw(0.75)]))
    recs.append(rec("c_short_eq", 0, 1, 0, "40=", [zw(1.0)]))       # adds nothing: the sequence is used, all zeros
    recs.append(rec("c_short_x", 0, 1, 3, "10X5=", [zw(1.0)]))
    return targets, recs


def case_tags():
    targets = [("t_mixed", 120), ("t_no_zw_only", 30), ("t_after", 64), ("t_never", 5)]
    u = lambda n: rec(n, 4, -1, -1, "", [])
    recs = [rec("g_f", 0, 0, 0, "50M", [zw(0.25)]),
            u("g_unmapped_1"),
            rec("g_other_tags_first", 0, 0, 10, "50M", [("NH", "i", 3), ("XS", "A", "+"), ("XB", "Bc", [1, -2, 3]), ("XZ", "Z", "ZW:f:9"), zw(0.1)]),
            rec("g_int", 0, 0, 20, "50M", [("ZW", "i", 1)]),
            rec("g_int_big", 0, 0, 20, "50M", [("ZW", "i", 70000)]),
            rec("g_zero", 0, 0, 30, "50M", [zw(0.0)]),
            rec("g_none", 0, 0, 40, "50M", [("NH", "i", 1)]),
            rec("g_string", 0, 0, 40, "50M", [("ZW", "Z", "0.5")]),
            u("g_unmapped_2"),
            rec("g_unmapped_with_place", 4, 0, 60, "50M", [zw(1.0)]),
            rec("g_twice", 0, 0, 60, "60M", [zw(0.5), zw(0.125)]),
            rec("g_negative", 0, 0, 70, "20M", [zw(-0.25)]),
            rec("g_only_1", 0, 1, 0, "30M", []),
            u("g_unmapped_3"),
            rec("g_only_2", 16, 1, 5, "10M", [("NH", "i", 2)]),
            rec("g_after", 0, 2, 0, "64M", [zw(1.0)]),
            u("g_unmapped_4")]
    return targets, recs


def case_tags_d():
    targets, recs = case_tags()
    recs = recs[:3] + [rec("g_double", 0, 0, 15, "50M", [("ZW", "d", 0.7)]), rec("g_double_small", 0, 0, 15, "50M", [("ZW", "d", 1e-17)])] + recs[3:]
    recs.append(rec("g_double_after", 0, 2, 1, "10M", [("ZW", "d", 1e-17)]))
    return targets, recs


def case_threshold():
    targets = [("edges", 30), ("single", 9), ("sums", 24)]
    recs = [rec("h_at_start", 0, 0, 0, "4M", [zw(0.0095)]), rec("h_below", 0, 0, 6, "3M", [zw(0.0094)]), rec("h_above", 0, 0, 11, "3M", [zw(0.00951)]),
            rec("h_one_base", 0, 0, 20, "1M", [zw(0.02)]), rec("h_at_end", 0, 0, 27, "3M", [zw(1.0)]),
            rec("h_whole", 0, 1, 0, "9M", [zw(0.00949)]), rec("h_middle", 0, 1, 4, "1M", [zw(0.00002)]),
            rec("h_half_1", 0, 2, 0, "12M", [zw(0.005)]), rec("h_half_2", 0, 2, 4, "12M", [zw(0.0045)]), rec("h_half_3", 0, 2, 8, "12M", [zw(0.0044)]),
            rec("h_tiny", 0, 2, 20, "4M", [zw(0.00475)]), rec("h_tiny_2", 0, 2, 22, "2M", [zw(0.00475)])]
    return targets, recs


def case_unsorted():
    r = random.Random(77)
    targets = [("u0", 600), ("u1", 90), ("u2", 1030), ("u3", 7)]
    recs = []
    for run, tid in enumerate([2, 0, 2, 1, 0, 0, 3, 2, 1]):
        ln = targets[tid][1]
        ps = sorted((r.randint(0, ln - 1) for _ in range(r.randint(1, 25))), reverse=run % 2 == 0)
        for i, p in enumerate(ps):
            L = r.randint(1, min(60, ln - p))
            recs.append(rec("u%d_%d" % (run, i), 0, tid, p, "%dM" % L, [zw(r.choice(WEIGHTS))]))
        if run % 3 == 0:
            recs.append(rec("u%d_unmapped" % run, 4, -1, -1, "", []))
    return targets, recs


def case_many_runs():
    r = random.Random(3000)
    targets = [("m%d" % i, r.randint(1, 5)) for i in range(64)]
    recs, last = [], -1
    for run in range(3000):
        tid = r.randrange(64)
        while tid == last:
            tid = r.randrange(64)
        last = tid
        for i in range(r.choice((1, 1, 1, 2, 3))):
            ln = targets[tid][1]
            p = r.randint(0, ln - 1)
            recs.append(rec("m%d_%d" % (run, i), 0, tid, p, "%dM" % r.randint(1, ln - p), [zw(r.choice(WEIGHTS))]))
    return targets, recs


CASES = [("sorted", case_sorted, True), ("cigars", case_cigars, True), ("tags", case_tags, True), ("tags_d", case_tags_d, False),
         ("threshold", case_threshold, True), ("unsorted", case_unsorted, True), ("many_runs", case_many_runs, False)]


def main():
    bam2wig, bam2readdepth = sys.argv[1], sys.argv[2]
    os.makedirs(HERE, exist_ok=True)
    for name, make, with_sam in CASES:
        targets, recs = make()
        inputs = []
        if with_sam:
            inputs.append(os.path.join(HERE, name + ".sam"))
            open(inputs[-1], "wb").write(sam_text(targets, recs))
        inputs.append(os.path.join(HERE, name + ".bam"))
        open(inputs[-1], "wb").write(bam_bytes(targets, recs))
        got = []
        for k, path in enumerate(inputs):
            pre = os.path.join(HERE, name) if k == len(inputs) - 1 else os.path.join(HERE, "_from_sam")
            subprocess.check_call([bam2wig, path, pre + ".wig", name], stdout=subprocess.DEVNULL)
            subprocess.check_call([bam2wig, path, pre + ".nfw.wig", name, "--no-fractional-weight"], stdout=subprocess.DEVNULL)
            subprocess.check_call([bam2readdepth, path, pre + ".readdepth"], stdout=subprocess.DEVNULL)
            got.append([open(pre + e, "rb").read() for e in (".wig", ".nfw.wig", ".readdepth")])
        if len(got) == 2:
            assert got[0] == got[1], "%s: the reference programs disagree between SAM and BAM" % name
            for e in (".wig", ".nfw.wig", ".readdepth"):
                os.remove(os.path.join(HERE, "_from_sam" + e))
        for e, data in zip((".wig", ".nfw.wig", ".readdepth"), got[-1]):
            path = os.path.join(HERE, name + e)
            if os.path.exists(path + ".gz"):
                os.remove(path + ".gz")
            if len(data) > 1024:
                with open(path + ".gz", "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
                    z.write(data)
                os.remove(path)
        print(name, len(recs), "records;", ", ".join("%d bytes" % len(x) for x in got[-1]))


if __name__ == "__main__":
    main()
