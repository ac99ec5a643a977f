"""TEST INFRASTRUCTURE: rsem-sam-validator and rsem-get-unique restated in Python, record by record as the reference programs go
(samValidator.cpp:26-59,82-190 with its std::set of names as a Python set; getUnique.cpp:25-30,55-80), on records given as tuples; and
what the tests share: the fixtures of tests/golden/alncheck/, records <-> BAM bytes <-> the arrays of rsem_alncheck_push.
Nothing here is fast and nothing here is used by the product."""
import collections
import gzip
import os
import struct

import numpy as np

import gmap_ref as gr

ROOT = gr.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "alncheck")
VALIDATOR = os.path.join(ROOT, "rsem_amd", "bin", "rsem-sam-validator")
GET_UNIQUE = os.path.join(ROOT, "rsem_amd", "bin", "rsem-get-unique")
DEFAULT_BATCH_ITEMS = 1 << 22

(OK, MIXED, ONE_MATE, SAME_MATE_NUMBER, ONE_MATE_ALIGNED, DISCORDANT, SAME_STRAND, PAIR_BOUNDARY, CIGAR_SKIP, CIGAR_INDEL, CIGAR_CLIP, BOUNDARY, NOT_GROUPED,
 DIFFERENT_LENGTHS) = range(14)
CODE_NAMES = ["OK", "MIXED", "ONE_MATE", "SAME_MATE_NUMBER", "ONE_MATE_ALIGNED", "DISCORDANT", "SAME_STRAND", "PAIR_BOUNDARY", "CIGAR_SKIP", "CIGAR_INDEL",
              "CIGAR_CLIP", "BOUNDARY", "NOT_GROUPED", "DIFFERENT_LENGTHS"]

# name: the raw read name (bytes, no NUL); cigar: BAM words
Rec = collections.namedtuple("Rec", "name flag tid pos isize lq cigar")
Verdict = collections.namedtuple("Verdict", "code mate unit_record units_ok cigar_op")
OPS = "MIDNSHP=XB"


def rec(name, flag=0, tid=0, pos=0, lq=10, cigar=None, isize=0):
    """a record for the synthetic cases; cigar: None = lq M, else a list of (length, letter)"""
    if isinstance(name, str):
        name = name.encode()
    words = [lq << 4] if cigar is None else [n << 4 | OPS.index(op) for n, op in cigar]
    return Rec(name, flag, tid, pos, isize, lq, tuple(words))


def pair(name, tid=0, p1=0, p2=20, lq=10, lq2=None, rev=False, second_first=False, cigar1=None, cigar2=None, isize=None, tid2=None, name2=None):
    """a properly aligned pair: read 1 and read 2 on opposite strands"""
    lq2 = lq if lq2 is None else lq2
    tl = max(p1 + lq, p2 + lq2) - min(p1, p2) if isize is None else isize
    a = rec(name, 0x1 | 0x2 | 0x40 | (0x10 if rev else 0x20), tid, p1, lq, cigar1, tl if p1 <= p2 else -tl)
    b = rec(name if name2 is None else name2, 0x1 | 0x2 | 0x80 | (0x20 if rev else 0x10), tid if tid2 is None else tid2, p2, lq2, cigar2, -tl if p1 <= p2 else tl)
    return [b, a] if second_first else [a, b]


def parse_record(d):
    tid, pos, l_name, _, _, n_cigar, flag, l_seq, _, _, isize = struct.unpack_from(gr.CORE, d, 0)
    name = d[32:32 + l_name].split(b"\0")[0]
    return Rec(name, flag, tid, pos, isize, l_seq, struct.unpack_from("<%dI" % n_cigar, d, 32 + l_name))


def record_bytes(r):
    """a BAM record (without block_size) of a Rec: bases A, qualities 30, no tags"""
    name = r.name + b"\0"
    rlen = sum(w >> 4 for w in r.cigar if (w & 15) in (0, 2, 3, 7, 8))
    end = r.pos + rlen if r.cigar and not r.flag & 4 else r.pos + 1
    body = struct.pack(gr.CORE, r.tid, r.pos, len(name), 255, gr.reg2bin(max(r.pos, 0), max(end, 0)) & 0xffff, len(r.cigar), r.flag, r.lq, r.tid if r.flag & 1 else -1, -1, r.isize)
    return body + name + struct.pack("<%dI" % len(r.cigar), *r.cigar) + bytes([0x11] * ((r.lq + 1) // 2)) + bytes([30] * r.lq)


def canonical(name):
    for i, c in enumerate(name):
        if c in b" \t\n\r\f\v\0":  # (bam_get_canonical_name works on the C string: a NUL ends it)
            return name[:i]
    return name


def pack(recs):
    """the arrays of rsem_alncheck_push"""
    name_off = np.zeros(len(recs) + 1, np.uint64)
    cigar_off = np.zeros(len(recs) + 1, np.uint64)
    if recs:
        name_off[1:] = np.cumsum([len(r.name) for r in recs])
        cigar_off[1:] = np.cumsum([len(r.cigar) for r in recs])
    names = np.frombuffer(b"".join(r.name for r in recs) + b"\0", np.uint8).copy()
    cigar = np.array([w for r in recs for w in r.cigar] + [0], np.uint32)
    f = lambda k, t: np.array([getattr(r, k) for r in recs], t)
    return dict(name_off=name_off, names=names, flag=f("flag", np.uint32), tid=f("tid", np.int32), pos=f("pos", np.int32), isize=f("isize", np.int32),
                l_qseq=f("lq", np.int32), cigar_off=cigar_off, cigar=cigar)


# ---- rsem-sam-validator ------------------------------------------------------------------------------------------------------------

def check_read(b, mate, tlen):
    for w in b.cigar:
        op = OPS[w & 15] if (w & 15) < len(OPS) else "?"
        if op == "N":
            return CIGAR_SKIP, mate, ord(op)
        if op in "ID":
            return CIGAR_INDEL, mate, ord(op)
        if op in "SHP":
            return CIGAR_CLIP, mate, ord(op)
    if b.pos < 0 or endpos(b) > tlen[b.tid]:
        return BOUNDARY, mate, 0
    return None


def endpos(b):
    if not b.flag & 4 and b.cigar:
        return b.pos + sum(w >> 4 for w in b.cigar if (w & 15) in (0, 2, 3, 7, 8))
    return b.pos + 1


def verdict(recs, tlen):
    """the loop of samValidator.cpp:82-183: where it stops and why, and its cnt"""
    used, cq, cl, paired, cnt, i = set(), b"", None, None, 0, 0
    while i < len(recs):
        unit, b = i, recs[i]
        fail = lambda code, mate=0, op=0: Verdict(code, mate, unit, cnt, op)
        q = canonical(b.name)
        if paired is None:
            paired = b.flag & 1
        elif paired != (b.flag & 1):
            return fail(MIXED)
        if paired:
            b2 = recs[i + 1] if i + 1 < len(recs) else None
            if b2 is None or canonical(b2.name) != q or not b2.flag & 1:
                return fail(ONE_MATE)
            if not ((b.flag & 0x40 and b2.flag & 0x80) or (b2.flag & 0x40 and b.flag & 0x80)):
                return fail(SAME_MATE_NUMBER)
            value = (not b.flag & 4) + (not b2.flag & 4)
            if value == 1:
                return fail(ONE_MATE_ALIGNED)
            m1 = 0
            if not b.flag & 0x40:
                b, b2, m1 = b2, b, 1
            if value == 2:
                if b.tid != b2.tid:
                    return fail(DISCORDANT, m1)
                if ((b.flag >> 4 & 1) << 1) + (b2.flag >> 4 & 1) not in (1, 2):
                    return fail(SAME_STRAND, m1)
                tb = b if b.pos < b2.pos else b2
                if not (tb.pos >= 0 and tb.pos + abs(tb.isize) <= tlen[tb.tid]):
                    return fail(PAIR_BOUNDARY, m1)
                for x, m in ((b, m1), (b2, 1 - m1)):
                    c = check_read(x, m, tlen)
                    if c:
                        return fail(*c)
            lens = (b.lq, b2.lq)
            i += 2
        else:
            if not b.flag & 4:
                c = check_read(b, 0, tlen)
                if c:
                    return fail(*c)
            lens = (b.lq,)
            i += 1
        if cq != q:
            if q in used:
                return fail(NOT_GROUPED)
            used.add(cq)
            cq, cl = q, lens
        elif cl != lens:
            return fail(DIFFERENT_LENGTHS)
        cnt += 1
    return Verdict(OK, 0, -1, cnt, 0)


def message(v, recs, targets):
    """what the reference prints for the verdict (its printf lines, in its words)"""
    if v.code == OK:
        return ""
    r0 = v.unit_record
    a = recs[r0 + v.mate]
    b = recs[r0 + 1 - v.mate] if r0 + 1 - v.mate < len(recs) else None
    q, q0 = a.name.decode(), recs[r0].name.decode()
    tn = lambda t: targets[t][0]
    if v.code == MIXED:
        return "\nWe detected both single-end and paired-end reads in the data!\nRSEM currently does not support a mixture of single-end/paired-end reads.\n"
    if v.code == ONE_MATE:
        return "\nOnly find one mate for paired-end read %s!\nPlease make sure that the two mates of a paired-end read are adjacent to each other.\n" % q0
    if v.code == SAME_MATE_NUMBER:
        return "\nThe two mates of paired-end read %s are marked as both mate1 or both mate2!\n" % q0
    if v.code == ONE_MATE_ALIGNED:
        return "\nPaired-end read %s has an alignment with only one mate aligned!\nCurrently RSEM does not handle mixed alignments for paired-end reads.\n" % q0
    if v.code == DISCORDANT:
        return ("\nPaired-end read %s has a discordant alignment (two mates aligned to different reference sequences)!\nMate 1 aligns to %s and mate 2 aligns to %s\n"
                "Currently RSEM does not handle discordant alignments.\n" % (q, tn(a.tid), tn(b.tid)))
    if v.code == SAME_STRAND:
        return ("\nPaired-end read %s has an alignment in which two mates aligned to the same strand!\nIts two mates aligned to %s in %s direction.\n"
                % (q, tn(a.tid), "reverse" if a.flag & 16 else "forward"))
    if v.code == PAIR_BOUNDARY:
        t = a if a.pos < b.pos else b
        return ("\nPaired-end read %s aligns to [%d, %d) of transcript %s, which exceeds the transcript's boundary [0, %d)!\n"
                % (q, t.pos, t.pos + abs(t.isize), tn(t.tid), targets[t.tid][1]))
    if v.code == CIGAR_SKIP:
        return "\nSkipped region is detected (cigar N) for read %s!\nTo use RSEM, please align your reads to a set of transcript sequences instead of a genome.\n" % q
    if v.code == CIGAR_INDEL:
        return "\nIndel alignment is detected (cigar %c) for read %s!\nRSEM currently does not support indel alignments.\n" % (v.cigar_op, q)
    if v.code == CIGAR_CLIP:
        return "\nClipping or padding is detected (cigar %c) for read %s!\nRSEM currently doest not support clipping or padding.\n" % (v.cigar_op, q)
    if v.code == BOUNDARY:
        who = "Mate %d of paired-end read %s" % (1 if a.flag & 0x40 else 2, q) if a.flag & 1 else "Read %s" % q
        return "\n%s aligns to [%d, %d) of transcript %s, which exceeds the transcript's boundary [0, %d)!\n" % (who, a.pos, endpos(a), tn(a.tid), targets[a.tid][1])
    name = canonical(recs[r0].name).decode()
    if v.code == NOT_GROUPED:
        return "\nThe alignments of read %s are not grouped together!\n" % name
    return "\nRead %s have alignments showing different read/mate lengths!\n" % name


def validator_stdout(targets, recs):
    v = verdict(recs, [l for _, l in targets])
    out = "." + "." * (v.units_ok // 1000000) + message(v, recs, targets)
    return out + ("\nThe input file is valid!\n" if v.code == OK else "The input file is not valid!\n")


# ---- rsem-get-unique ---------------------------------------------------------------------------------------------------------------

def unique_keep(recs):
    """getUnique.cpp:25-30,55-65: per record whether it is written"""
    keep, i = [0] * len(recs), 0
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j].name == recs[i].name:
            j += 1
        if not any(r.flag & 4 for r in recs[i:j]) and j - i == (2 if recs[i].flag & 1 else 1):
            keep[i:j] = [1] * (j - i)
        i = j
    return keep


def header_bytes(path):
    """the header as the reference writes back what it read: a BAM's own bytes, a SAM's text and the dictionary of its @SQ lines"""
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        raw = gr.bgzf_inflate(data)
        l_text = struct.unpack_from("<i", raw, 4)[0]
        p = 8 + l_text
        n_ref = struct.unpack_from("<i", raw, p)[0]
        p += 4
        for _ in range(n_ref):
            p += 8 + struct.unpack_from("<i", raw, p)[0]
        return raw[:p]
    return gr.bam_header("".join(l + "\n" for l in data.decode().split("\n") if l and l[0] == "@"))


def get_unique(path):
    """the decompressed output of rsem-get-unique for an alignment file"""
    _, _, raw = gr.read_alignments(path)
    keep = unique_keep([parse_record(d) for d in raw])
    return header_bytes(path) + b"".join(struct.pack("<i", len(d)) + d for d, k in zip(raw, keep) if k)


# ---- the library ---------------------------------------------------------------------------------------------------------------------

def device_verdict(recs, tlen, cuts=()):
    """the records through capi.Alncheck in pushes cut at the record indices `cuts`: (the verdict in the file's coordinates, the pushes' dicts)"""
    from rsem_amd import capi
    ck = capi.Alncheck(tlen)
    bounds = [0] + list(cuts) + [len(recs)]
    units, pushes = 0, []
    try:
        for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
            v = ck.push(last=(k == len(bounds) - 2), **pack(recs[a:b]))
            pushes.append(v)
            assert v["n_records"] == b - a and 3 * v["n_batches"] <= v["n_launches"] <= 5 * v["n_batches"]
            if v["code"]:
                assert v["unit_record"] >= 0
                return Verdict(v["code"], v["mate"], a + v["unit_record"], units + v["units_ok"], v["cigar_op"]), pushes
            assert v["unit_record"] == -1 and v["units_ok"] == v["n_units"]
            units += v["units_ok"]
    finally:
        ck.close()
    return Verdict(OK, 0, -1, units, 0), pushes


def device_keep(recs):
    from rsem_amd import capi
    p = pack(recs)
    return capi.alncheck_unique(p["name_off"], p["names"], p["flag"])


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------

def _cases(suffix):
    return sorted({f[:-len(suffix)] for f in os.listdir(GOLDEN) if f.endswith(suffix)} | {f[:-len(suffix) - 3] for f in os.listdir(GOLDEN) if f.endswith(suffix + ".gz")})


def validator_cases():
    return _cases(".stdout")


def unique_cases():
    return _cases(".unique")


def inputs(cases):
    return [(c, os.path.join(GOLDEN, c + e)) for c in cases for e in (".sam", ".bam") if os.path.exists(os.path.join(GOLDEN, c + e))]


def input_id(ci):
    return os.path.basename(ci[1])


def recorded(case, suffix):
    p = os.path.join(GOLDEN, case + suffix)
    if os.path.exists(p + ".gz"):
        return gzip.open(p + ".gz", "rb").read()
    return open(p, "rb").read()


def load(path):
    """(targets, [Rec]) of an alignment file"""
    _, targets, raw = gr.read_alignments(path)
    return targets, [parse_record(d) for d in raw]
