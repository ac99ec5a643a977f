"""rsem-tbam2gbam restated in plain Python: what the program computes, said from its behaviour.

A transcript BAM (records in read order, the alignments of a read next to each other, for paired reads mate 1 and mate 2 next to each
other) becomes a genome BAM:
  header    the text regrouped HD, SQ, RG, PG, CO, other (unknown records lose their newline); every @SQ replaced by one line per
            line of <ref>.chrlist; @PG ID:rsem-tbam2gbam CL:<argv> appended unless that ID is there;
  per mate  the range pos + 1 .. pos + l_seq of the transcript (found by NAME of the input tid), mirrored on a '-' transcript, walked
            over the exon list: tid of the chromosome, 0-based pos, M / N words, I for what hangs off either end, one I for a read
            wholly in the poly-A tail; MAPQ 255; flags, SEQ, QUAL, MD flipped on '-'; XS deleted, XS:A added where the CIGAR has an N;
  per read  alignments with the same (tid, pos, reverse, n_cigar, words) of mate 1 then mate 2 collapse into the first one; weights
            (ZW; 1 without) add up in float32 in file order; the read's alignments are written in key order; MAPQ from the sum
            where the kept mate 1 carries a ZW.
The exon walk here is the linear one; the device bisects.  Unmapped reads pass through unchanged.
"""
import glob
import gzip
import math
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gbam")
TBAM2GBAM = os.path.join(ROOT, "rsem_amd", "bin", "rsem-tbam2gbam")
REF = os.path.join(GOLDEN, "ref")  # ref.ti, ref.chrlist
OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
WAVE, GROUP_THREADS = 64, 256  # rsem_amd/csrc/gmap_block.hpp: kWave, kGroupThreads
DEFAULT_BATCH_ITEMS = 1 << 22


class Stop(Exception):
    """the program stops with this message"""


# ---- the reference files ------------------------------------------------------------------------------------------------------------

def load_ti(path):
    """(type, [dict(transcript_id, seqname, strand, length, exons=[(start, end)])])"""
    lines = open(path).read().split("\n")
    M, typ = (int(x) for x in lines[0].split())
    out = []
    for i in range(M):
        l = lines[1 + 6 * i: 7 + 6 * i]
        strand, length = l[3].split()
        v = [int(x) for x in l[4].split()]
        out.append(dict(transcript_id=l[0].split("\t")[0], seqname=l[2], strand=strand, length=int(length),
                        exons=[(v[1 + 2 * k], v[2 + 2 * k]) for k in range(v[0])]))
    return typ, out


def parse_sq(text):
    out = []
    for line in text.split("\n"):
        if line[:3] == "@SQ":
            name, ln = "", 0
            for f in line.split("\t")[1:]:
                if f[:3] == "SN:":
                    name = f[3:]
                if f[:3] == "LN:":
                    ln = int(f[3:])
            out.append((name, ln))
    return out


def out_header_text(text, chrlist_lines, command):
    hd = sq = rg = pg = co = other = ""
    has = False
    for line in text.split("\n"):
        if not line or line[0] != "@":
            continue
        tag = line[1:3]
        if tag == "HD":
            hd = line + "\n"
        elif tag == "SQ":
            pass
        elif tag == "RG":
            rg += line + "\n"
        elif tag == "PG":
            has = has or any(f == "ID:rsem-tbam2gbam" for f in line.split("\t")[1:])
            pg += line + "\n"
        elif tag == "CO":
            co += line + "\n"
        else:
            other += line  # the newline of an unknown record is lost
    for line in chrlist_lines:
        pos = line.index("\t")
        nxt = line.find("\t", pos + 1)
        ln = line[pos + 1:] if nxt < 0 else line[pos + 1: pos + 1 + nxt]  # the COUNT of the substring is the second tab's index
        sq += "@SQ\tSN:" + line[:pos] + "\tLN:" + ln + "\n"
    if not has:
        pg += "@PG\tID:rsem-tbam2gbam\tCL:" + command + "\n"
    return hd + sq + rg + pg + co + other


def bam_header(text):
    b = b"BAM\1" + struct.pack("<i", len(text)) + text.encode()
    sq = parse_sq(text)
    b += struct.pack("<i", len(sq))
    for name, ln in sq:
        b += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return b


# ---- alignment files ----------------------------------------------------------------------------------------------------------------

def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def encode_sam_line(line, ids):
    """one SAM text line as a BAM record (without block_size), as htslib 1.3 encodes it"""
    f = line.split("\t")
    flag, pos, mapq = int(f[1]), int(f[3]) - 1, int(f[4])
    tid = -1 if f[2] == "*" else ids[f[2]]
    mtid = tid if f[6] == "=" else (-1 if f[6] == "*" else ids[f[6]])
    ops, n = [], ""
    for ch in f[5] if f[5] != "*" else "":
        if ch.isdigit():
            n += ch
        else:
            ops.append(int(n) << 4 | OPS.index(ch))
            n = ""
    rlen = sum(w >> 4 for w in ops if (w & 15) in (0, 2, 3, 7, 8))
    end = pos + rlen if ops and not flag & 4 else pos + 1
    seq = "" if f[9] == "*" else f[9]
    name = f[0].encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, reg2bin(pos, end), len(ops), flag, len(seq), mtid, int(f[7]) - 1, int(f[8]))
    body += name + b"".join(struct.pack("<I", w) for w in ops)
    nib = [NT16.index(c.upper()) if c.upper() in NT16 else 15 for c in seq] + [0]
    body += bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))
    body += bytes([0xff] * len(seq)) if f[10] == "*" else bytes(ord(c) - 33 for c in f[10])
    for t in f[11:]:
        tag, ty, v = t[:2].encode(), t[3], t[5:]
        if ty == "i":
            x = int(v)
            for code, fmt, lo, hi in ((b"c", "<b", -128, -1), (b"s", "<h", -32768, -1), (b"i", "<i", -2 ** 31, -1), (b"C", "<B", 0, 255),
                                      (b"S", "<H", 0, 65535), (b"I", "<I", 0, 2 ** 32 - 1)):
                if lo <= x <= hi:
                    body += tag + code + struct.pack(fmt, x)
                    break
        elif ty == "f":
            body += tag + b"f" + struct.pack("<f", float(v))
        elif ty == "A":
            body += tag + b"A" + v.encode()
        elif ty in "ZH":
            body += tag + ty.encode() + v.encode() + b"\0"
        else:
            raise ValueError("tag type %s" % ty)
    return body


def bgzf_inflate(data):
    out, o = [], 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = struct.unpack_from("<H", data, o + 16)[0]  # (the BC field comes first in every file here)
        out.append(zlib.decompress(data[o + 12 + xlen: o + bsize + 1 - 8], -15))
        o += bsize + 1
    return b"".join(out)


def split_bam(raw):
    """decompressed BAM -> (header text, [(name, length)], [record without block_size])"""
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].rstrip(b"\0").decode()
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    targets = []
    for _ in range(n_ref):
        l = struct.unpack_from("<i", raw, p)[0]
        targets.append((raw[p + 4:p + 4 + l - 1].decode(), struct.unpack_from("<i", raw, p + 4 + l)[0]))
        p += 8 + l
    recs = []
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        recs.append(raw[p + 4:p + 4 + bs])
        p += 4 + bs
    return text, targets, recs


def read_alignments(path):
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        return split_bam(bgzf_inflate(data))
    lines = [l for l in data.decode().split("\n") if l]
    text = "".join(l + "\n" for l in lines if l[0] == "@")
    targets = parse_sq(text)
    ids = {n: i for i, (n, _) in enumerate(targets)}
    return text, targets, [encode_sam_line(l, ids) for l in lines if l[0] != "@"]


# ---- a record ---------------------------------------------------------------------------------------------------------------------

CORE = "<iiBBHHHiiii"  # tid pos l_name mapq bin n_cigar flag l_seq mtid mpos isize
AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}


def aux_fields(d, p):
    """[(offset of the tag, tag, type, offset behind the field)]"""
    out = []
    while p + 3 <= len(d):
        tag, ty, q = d[p:p + 2], chr(d[p + 2]), p + 3
        if ty in AUX_SIZE:
            q += AUX_SIZE[ty]
        elif ty in "ZH":
            q = d.index(b"\0", q) + 1
        elif ty == "B":
            sub, n = chr(d[q]), struct.unpack_from("<i", d, q + 1)[0]
            q += 5 + n * AUX_SIZE[sub]
        else:
            raise ValueError("aux type %r" % ty)
        out.append((p, tag, ty, q))
        p = q
    return out


def canonical_name(d):
    name = d[32:32 + d[8] - 1]
    for i, c in enumerate(name):
        if c in b" \t\n\r\f\v":
            return name[:i]
    return name


def tr2chr(t, sp, ep):
    """(0-based pos, [cigar words]) of the transcript range sp .. ep (1-based); the linear walk"""
    L, ex = t["length"], t["exons"]
    if t["strand"] == "-":
        sp, ep = L - ep + 1, L - sp + 1
    if ep < 1 or sp > L:
        return (ex[-1][1] if sp > L else ex[0][0] - 1), [(ep - sp + 1) << 4 | 1]
    words = []
    if sp < 1:
        words.append((1 - sp) << 4 | 1)
        sp = 1
    cur, i = 0, 0
    while True:
        old = cur
        cur += ex[i][1] - ex[i][0] + 1
        if cur >= sp:
            break
        i += 1
    pos = ex[i][0] + (sp - old - 1) - 1
    while cur < ep and i < len(ex):
        words.append((cur - sp + 1) << 4 | 0)
        i += 1
        if i >= len(ex):
            break
        words.append(((ex[i][0] - ex[i - 1][1] - 1) << 4 | 3) & 0xffffffff)  # a CIGAR word has 32 bits: an intron of 2^28 bases or more wraps
        sp = cur + 1
        cur += ex[i][1] - ex[i][0] + 1
    words.append((ep - L) << 4 | 1 if i >= len(ex) else (ep - sp + 1) << 4 | 0)
    return pos, words


COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def flip_md(s):
    segs = []
    for ch in s:
        if segs and segs[-1][0].isdigit() == ch.isdigit():
            segs[-1] += ch
        else:
            segs.append(ch)
    out = ""
    for g in reversed(segs):
        if g[0].isdigit():
            out += g
        else:
            hat = g[0] == "^"
            body = g[1:] if hat else g
            out += ("^" if hat else "") + "".join(COMP.get(c, c) for c in reversed(body))
    return out


def convert(d, t, out_tid):
    """one mapped mate -> its record on the genome (mpos still the input's)"""
    tid, pos, l_name, _, _, n_cigar, flag, l_seq, mtid, mpos, isize = struct.unpack_from(CORE, d, 0)
    if l_seq <= 0:
        raise Stop("One alignment line has SEQ field as *. RSEM does not support this currently!")
    paired = flag & 1
    minus = t["strand"] == "-"
    if minus:
        flag ^= 0x10
        if paired:
            flag ^= 0x20
            isize = -isize
    p = 32 + l_name + 4 * n_cigar
    seq, qual, aux = bytearray(d[p:p + (l_seq + 1) // 2]), d[p + (l_seq + 1) // 2: p + (l_seq + 1) // 2 + l_seq], bytearray(d[p + (l_seq + 1) // 2 + l_seq:])
    if minus:
        nib = [(seq[i >> 1] >> (4 * (1 - i % 2))) & 15 for i in range(l_seq)]
        if any(x not in (1, 2, 4, 8, 15) for x in nib):
            raise Stop("SEQ holds a base other than A, C, G, T, N")
        nib = [{1: 8, 2: 4, 4: 2, 8: 1, 15: 15}[x] for x in reversed(nib)] + [0]
        seq = bytearray(nib[i] << 4 | nib[i + 1] for i in range(0, l_seq, 2))
        qual = qual[::-1]
        for off, tag, ty, end in aux_fields(aux, 0):
            if tag == b"MD":
                if ty == "Z":
                    aux[off + 3:end - 1] = flip_md(aux[off + 3:end - 1].decode()).encode()
                break
    new_pos, words = tr2chr(t, pos + 1, pos + l_seq)
    for off, tag, ty, end in aux_fields(aux, 0):
        if tag == b"XS":
            del aux[off:end]
            break
    if any(w & 15 == 3 for w in words):
        aux += b"XSA" + t["strand"].encode()
    rlen = sum(w >> 4 for w in words if (w & 15) in (0, 3))
    core = struct.pack(CORE, out_tid, new_pos, l_name, 255, reg2bin(new_pos, new_pos + rlen), len(words), flag, l_seq, out_tid if paired else mtid, mpos, isize)
    return core + d[32:32 + l_name] + b"".join(struct.pack("<I", w) for w in words) + bytes(seq) + bytes(qual) + bytes(aux)


def set_field(d, off, fmt, v):
    """the bytes of v over d[off:]; what would fall behind the record is not written"""
    b = struct.pack(fmt, v)[:len(d) - off]
    return d[:off] + b + d[off + len(b):]


def key_of(d):
    tid, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", d, 0)
    return (tid, pos, (flag >> 4) & 1, n_cigar) + struct.unpack_from("<%dI" % n_cigar, d, 32 + l_name)


def zw_of(d):
    """(offset of the ZW payload or None, the weight as (float)bam_aux2f gives it)"""
    _, _, l_name, _, _, n_cigar, _, l_seq = struct.unpack_from("<iiBBHHHi", d, 0)
    for off, tag, ty, end in aux_fields(d, 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq):
        if tag == b"ZW":
            if ty == "f":
                return off + 3, np.float32(struct.unpack_from("<f", d, off + 3)[0])
            if ty == "d":
                return off + 3, np.float32(struct.unpack_from("<d", d, off + 3)[0])
            return off + 3, np.float32(0.0)
    return None, np.float32(1.0)


def prb_to_mapq(val):
    err = 1.0 - float(val)
    if err <= 1e-10:
        return 100
    return int(-10 * math.log10(err) + .5) & 255


def fold32(ws):
    acc = np.float32(ws[0])
    for x in ws[1:]:
        acc = np.float32(acc + np.float32(x))
    return acc


def collapse(items):
    """items: [(key, weight, payload)] of one read in file order -> [(payload of the first with the key, folded weight)] in key order"""
    first, ws = {}, {}
    for k, w, x in items:
        if k not in first:
            first[k] = x
            ws[k] = [w]
        else:
            ws[k].append(w)
    return [(first[k], fold32(ws[k])) for k in sorted(first)]


def write_group(out, group):
    for (a, b), w in collapse(group):
        off, _ = zw_of(a)
        if off is not None:
            a = set_field(a, off, "<f", w)
            a = set_field(a, 9, "<B", prb_to_mapq(w))
        out.append(a)
        if b is not None:
            if off is not None:
                off2, _ = zw_of(b)
                if off2 is not None:
                    b = set_field(b, off2, "<f", w)
            out.append(set_field(b, 9, "<B", a[9]))


def tbam2gbam(ref, in_path, command):
    """the decompressed genome BAM for the transcript alignments of in_path"""
    typ, ti = load_ti(ref + ".ti")
    if typ != 0:
        raise Stop("Genome information is not provided! RSEM cannot convert the transcript bam file!")
    text, targets, recs = read_alignments(in_path)
    by_name = {t["transcript_id"]: t for t in ti}
    for name, _ in targets:
        if name not in by_name:
            raise Stop("RSEM can not recognize reference sequence name %s!" % name)
    if not os.path.exists(ref + ".chrlist"):
        raise Stop("Cannot open %s.chrlist! It may not exist." % ref)
    new_text = out_header_text(text, [l for l in open(ref + ".chrlist").read().split("\n") if l], command)
    out_ids = {n: i for i, (n, _) in enumerate(parse_sq(new_text))}
    out, group, cq, i = [], [], b"", 0
    while i < len(recs):
        a, b = recs[i], None
        i += 1
        fa = struct.unpack_from("<H", a, 14)[0]
        if fa & 1:
            b = recs[i]
            i += 1
            if not fa & 0x40:
                a, b = b, a
            fa, fb = struct.unpack_from("<H", a, 14)[0], struct.unpack_from("<H", b, 14)[0]
            if bool(fa & 4) != bool(fb & 4):
                raise Stop("Detected partial alignments for read %s, which RSEM currently does not support!" % canonical_name(a).decode())
        q = canonical_name(a)
        if not fa & 4:
            tid = struct.unpack_from("<i", a, 0)[0]
            if b is not None and struct.unpack_from("<i", b, 0)[0] != tid:
                raise Stop("%s's two mates are aligned to two different transcripts!" % q.decode())
            t = by_name[targets[tid][0]]
            a = convert(a, t, out_ids[t["seqname"]])
            if b is not None:
                b = convert(b, t, out_ids[t["seqname"]])
                a, b = set_field(a, 24, "<i", struct.unpack_from("<i", b, 4)[0]), set_field(b, 24, "<i", struct.unpack_from("<i", a, 4)[0])
            if q != cq:
                write_group(out, group)
                group, cq = [], q
            group.append((key_of(a) + (key_of(b) if b is not None else ()), zw_of(a)[1], (a, b)))
        else:
            write_group(out, group)
            group, cq = [], q
            out.append(a)
            if b is not None:
                out.append(b)
    write_group(out, group)
    return bam_header(new_text) + b"".join(struct.pack("<i", len(r)) + r for r in out)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------

def cases():
    return sorted(os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(GOLDEN, "*.genome*")))


def inputs():
    return [(c, p) for c in cases() for p in (os.path.join(GOLDEN, c + ".sam"), os.path.join(GOLDEN, c + ".bam")) if os.path.exists(p)]


def input_id(ci):
    return os.path.basename(ci[1])


def recorded(case):
    """what the reference program wrote, decompressed; a file above 1 KiB is kept gzip-compressed"""
    path = os.path.join(GOLDEN, case + ".genome")
    return gzip.open(path + ".gz", "rb").read() if os.path.exists(path + ".gz") else open(path, "rb").read()


def command_of(in_name):
    """the argv the fixtures were recorded with (tests/golden/make_gbam_golden.py), run inside tests/golden/gbam/"""
    return "rsem-tbam2gbam ref %s out.bam" % in_name


# ---- the device's view: fields in, fields out --------------------------------------------------------------------------------------

def flat_reference(ti, out_ids):
    """the arrays of capi.Gmap for the transcripts ti"""
    strand = "".join(t["strand"] for t in ti)
    length = [t["length"] for t in ti]
    out_tid = [out_ids[t["seqname"]] for t in ti]
    off, st, en = [0], [], []
    for t in ti:
        st += [e[0] for e in t["exons"]]
        en += [e[1] for e in t["exons"]]
        off.append(len(st))
    return strand, length, out_tid, off, st, en


def map_fields(ti, out_tid, tr, pos, l_qseq, flag):
    """per mate (tid, pos, flag, words, bin, has_n), the restatement of k_gmap_count / k_gmap_fill"""
    out = []
    for t, p, l, f in zip(tr, pos, l_qseq, flag):
        T = ti[t]
        np_, words = tr2chr(T, p + 1, p + l)
        if T["strand"] == "-":
            f ^= 0x10
            if f & 1:
                f ^= 0x20
        rlen = sum(w >> 4 for w in words if (w & 15) in (0, 3))
        out.append((out_tid[t], np_, f, words, reg2bin(np_, np_ + rlen), int(any(w & 15 == 3 for w in words))))
    return out


def collapse_fields(mates, group_off, mapped, w):
    """(out_src, out_w) of the groups, from the mapped mates"""
    src, ws = [], []
    for g in range(len(group_off) - 1):
        items = []
        for a in range(int(group_off[g]), int(group_off[g + 1])):
            k = ()
            for m in range(mates):
                tid, p, f, words, _, _ = mapped[a * mates + m]
                k += (tid, p, (f >> 4) & 1, len(words)) + tuple(words)
            items.append((k, np.float32(w[a]), a))
        for a, x in collapse(items):
            src.append(a)
            ws.append(x)
    return np.array(src, np.uint64), np.array(ws, np.float32)


def expected_batches(group_off, budget):
    out, items = 0, 0
    for g in range(len(group_off) - 1):
        it = int(group_off[g + 1]) - int(group_off[g])
        if items > 0 and items + it > budget:
            out += 1
            items = 0
        items += it
    return out + (1 if items else 0)
