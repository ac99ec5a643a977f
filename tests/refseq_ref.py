"""The contract of the three reference-preparation programs (rsem-extract-reference-transcripts, rsem-synthesis-reference-transcripts,
rsem-preref) restated in plain Python, clause by clause from the reference's code (extractRef.cpp, synthesisRef.cpp, preRef.cpp,
GTFItem.h, Transcript.h, Refs.h, RefSeq.h, PolyARules.h), and the two device operations behind them (rsem_refseq_load,
rsem_refseq_gather).  Everything is bytes; every comparison made with it is equality.  tests/golden/refprep/ holds what the unmodified
reference programs wrote; test_refprep_cpu.py holds this module to those files, test_refseq_gpu.py holds the product to both."""
import gzip
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refprep")
BIN = os.path.join(ROOT, "rsem_amd", "bin")
PROGRAMS = {"extract": "rsem-extract-reference-transcripts", "synthesis": "rsem-synthesis-reference-transcripts", "preref": "rsem-preref"}
MAX_WARNS = 50
SPACE = b" \t\n\v\f\r"
RC, UPPER_N, N2G, FILL = 1, 2, 4, 8


class Stop(Exception):
    """The program ends here: what it wrote to stderr so far is in the run's buffer, the status is 255 (exit(-1))."""


# ---- the device operations ---------------------------------------------------------------------------------------------------

def check_map(c):
    """check() of extractRef.cpp:297-303 on a letter."""
    if c in b"ACGTacgt":
        return c
    return ord("N") if 65 <= c <= 90 else ord("n")


def is_letter(c):
    return 65 <= c <= 90 or 97 <= c <= 122


def load_ref(raw, lo, hi, checked):
    """Per record: (bases, offset into raw of the first byte of the body that is no letter or -1)."""
    out = []
    for a, b in zip(lo, hi):
        body, bad, seq = raw[a:b], -1, bytearray()
        for k, c in enumerate(body):
            if c == 10:
                continue
            if checked and not is_letter(c):
                if bad < 0:
                    bad = a + k
                seq.append(c)
            else:
                seq.append(check_map(c) if checked else c)
        out.append((bytes(seq), bad))
    return out


OPP = bytes.maketrans(b"acgtACGT", b"tgcaTGCA")  # getOpp (utils.h:78-94); n and N stay


def upper_n(seq):
    """RefSeqPolicy::convert: toupper, then N for anything but A, C, G, T."""
    return bytes(c & ~0x20 if c in b"ACGTacgt" else 78 for c in seq)


def segment_ref(bases, first, length, flags):
    if flags & FILL:
        return b"A" * length
    s = bases[first:first + length]
    assert len(s) == length
    if flags & RC:
        s = s[::-1].translate(OPP)
    if flags & UPPER_N:
        s = upper_n(s)
    if flags & N2G:
        s = s.replace(b"N", b"G")
    return s


def gather_ref(store, bases, segments):
    """segments: (record, first base, length, destination, flags); store: a bytearray."""
    for src, first, length, dst, flags in segments:
        store[dst:dst + length] = segment_ref(None if flags & FILL else bases[src], first, length, flags)
    return store


# ---- FASTA ---------------------------------------------------------------------------------------------------------------------

def frame_fasta(data):
    """[(header behind '>', body_lo, body_hi)]: nothing unless the first line starts with '>'; a body is every line up to the next
    line that starts with '>'."""
    recs = []
    if not data.startswith(b">"):
        return recs
    h = 0
    while h < len(data):
        nl = data.find(b"\n", h)
        head_hi = nl if nl >= 0 else len(data)
        lo = head_hi + 1 if nl >= 0 else len(data)
        q = lo
        if not data.startswith(b">", lo):
            q = data.find(b"\n>", lo)
            q = len(data) if q < 0 else q + 1
        recs.append((data[h + 1:head_hi], lo, q))
        h = q
    return recs


def first_token(s):
    t = s.split()
    return t[0] if t else None


def bad_character(run, fname, data, off):
    line = data.count(b"\n", 0, off) + 1
    start = data.rfind(b"\n", 0, off) + 1
    c = data[off]
    run.err += b"FASTA file %s contains an unknown character, %s (ASCII code %d), at line %d, position %d!\n" % (
        fname.encode(), bytes([c]), c - 256 if c >= 128 else c, line, off - start + 1)
    raise Stop


class Run:
    def __init__(self, cwd):
        self.cwd, self.err, self.files = cwd, b"", {}

    def read(self, name):
        try:
            with open(os.path.join(self.cwd, name), "rb") as f:
                return f.read()
        except OSError:
            self.err += b"Cannot open %s! It may not exist.\n" % name.encode()
            raise Stop


def lines_of(data):
    ls = data.split(b"\n")
    if ls and ls[-1] == b"":
        ls.pop()
    return ls


def load_mapping(run, file_type, name):
    t1, t2 = {}, {}
    key = value = value2 = b""
    for line in lines_of(run.read(name)):
        line = line.strip(SPACE)
        if line.startswith(b"#"):
            continue
        tok = line.split()
        want = 3 if file_type == 2 else 2
        got = tok[:want]
        if len(got) >= 1:
            value = got[0]
        if file_type == 2:
            if len(got) >= 2:
                value2 = got[1]
            if len(got) >= 3:
                key = got[2]
        elif len(got) >= 2:
            key = got[1]
        t1[key] = value
        if file_type == 2:
            t2[key] = value2
    return t1, t2


# ---- the GTF ---------------------------------------------------------------------------------------------------------------

def gtf_stop(run, line, msg):
    run.err += b"The GTF file might be corrupted!\nStop at line : " + line + b"\nError Message: " + msg + b"\n"
    raise Stop


def c_atoi(s):
    s = s.lstrip(SPACE)
    k = 1 if s[:1] in (b"+", b"-") else 0
    e = k
    while e < len(s) and 48 <= s[e] <= 57:
        e += 1
    return int(s[:e]) if e > k else 0


class Item:
    def __init__(self):
        self.seqname = self.source = self.feature = self.score = self.frame = self.left = b""
        self.gene_id = self.transcript_id = self.gene_name = self.transcript_name = b""
        self.start = self.end = 0
        self.strand = b""

    def parse(self, run, line):
        """Nine getlines on one stream: behind the line's end a field keeps what it held."""
        st = {"cur": 0, "eof": False}

        def get(old, delim=b"\t"):
            if st["eof"]:
                return old
            p = line.find(delim, st["cur"]) if delim else -1
            if p < 0:
                st["eof"] = True
                return line[st["cur"]:]
            f = line[st["cur"]:p]
            st["cur"] = p + 1
            return f
        self.seqname, self.source, self.feature = get(self.seqname), get(self.source), get(self.feature)
        tmp = get(b"")
        self.start = c_atoi(tmp)
        tmp = get(tmp)
        self.end = c_atoi(tmp)
        self.score = get(self.score)
        tmp = get(tmp)
        if tmp not in (b"+", b"-"):
            gtf_stop(run, line, b"Strand is neither '+' nor '-'!")
        self.strand = tmp
        self.frame = get(self.frame)
        self.left = get(self.left, None)

    def parse_attributes(self, run, line):
        left, n = self.left, len(self.left)
        at = lambda i: left[i:i + 1] if 0 <= i < n else b"\0"
        sp = lambda i: at(i) in (b" ", b"\t", b"\n", b"\v", b"\f", b"\r")
        self.gene_id = self.transcript_id = self.gene_name = self.transcript_name = b""
        nleft, lpos = 4, 0
        while nleft > 0:
            while lpos < n and sp(lpos):
                lpos += 1
            rpos, in_quote = lpos, False
            while rpos < n and (at(rpos) != b";" or in_quote):
                if at(rpos) == b'"':
                    in_quote = not in_quote
                rpos += 1
            if not rpos < n:
                break
            pos = lpos
            while pos < rpos and not sp(pos):
                pos += 1
            if not sp(pos):
                gtf_stop(run, line, b"Cannot locate the identifier from attribute " + left[lpos:rpos + 1] + b"!")
            ident = left[lpos:pos]
            lpos = rpos + 1
            pos += 1
            while pos < rpos and sp(pos):
                pos += 1
            if at(pos) != b'"':
                pos = rpos
            rpos -= 1
            while rpos > pos and sp(rpos):
                rpos -= 1
            if rpos > pos and at(rpos) != b'"':
                rpos = pos
            val = left[pos + 1:rpos] if rpos - pos > 1 else b""
            empty = b"Attribute " + ident + b"'s value should be surrounded by double quotes and cannot be empty!"
            if ident == b"gene_id":
                if self.gene_id:
                    gtf_stop(run, line, b"gene_id appear more than once!")
                if not rpos - pos > 1:
                    gtf_stop(run, line, empty)
                self.gene_id = val
                nleft -= 1
            elif ident == b"transcript_id":
                if self.transcript_id:
                    gtf_stop(run, line, b"transcript_id appear more than once!")
                if not rpos - pos > 1:
                    gtf_stop(run, line, empty)
                self.transcript_id = val
                nleft -= 1
            elif ident == b"gene_name" and not self.gene_name and rpos - pos > 1:
                self.gene_name = val
                nleft -= 1
            elif ident == b"transcript_name" and not self.transcript_name and rpos - pos > 1:
                self.transcript_name = val
                nleft -= 1
        if not self.gene_id:
            gtf_stop(run, line, b"Cannot find gene_id!")
        if not self.transcript_id:
            gtf_stop(run, line, b"Cannot find transcript_id!")


def general_stop(run, msg):
    run.err += msg + b"\n"
    raise Stop


def parse_gtf(run, name, sources, mi_table):
    import copy
    items, item, n_warns = [], Item(), 0
    for line in lines_of(run.read(name)):
        if line.startswith(b"#"):
            continue
        item.parse(run, line)
        if item.feature == b"exon" and (not sources or item.source in sources):
            if item.start > item.end or item.start < 1:
                n_warns += 1
                if n_warns <= MAX_WARNS:
                    run.err += (b"Warning: exon's start position is larger than its end position! This exon is discarded.\n" if item.start > item.end
                                else b"Warning: exon's start position is less than 1! This exon is discarded.\n") + b"\t" + line + b"\n\n"
            else:
                item.parse_attributes(run, line)
                if mi_table is not None:
                    if item.transcript_id not in mi_table:
                        general_stop(run, b"Mapping Info is not correct, cannot find " + item.transcript_id + b"'s gene_id!")
                    item.gene_id = mi_table[item.transcript_id]
                items.append(copy.copy(item))
    if n_warns:
        run.err += b"Warning: In total, %d exons are discarded." % n_warns
    items.sort(key=lambda i: (i.gene_id, i.transcript_id, i.start))  # stable
    trs, sp = [], 0
    while sp < len(items):
        ep = sp + 1
        while ep < len(items) and items[ep].transcript_id == items[sp].transcript_id:
            ep += 1
        f = items[sp]
        t = {"tid": f.transcript_id, "gid": f.gene_id, "seqname": f.seqname, "strand": f.strand, "left": f.left.lstrip(b" "), "gname": b"", "tname": b"", "structure": []}
        cur_s = cur_e = -1
        for it in items[sp:ep]:
            if it.strand != t["strand"]:
                general_stop(run, b"According to the GTF file given, transcript " + t["tid"] + b" has exons from different orientations!")
            if it.seqname != t["seqname"]:
                general_stop(run, b"According to the GTF file given, transcript " + t["tid"] + b" has exons on multiple chromosomes!")
            if it.gene_name:
                if not t["gname"]:
                    t["gname"] = it.gene_name
                elif t["gname"] != it.gene_name:
                    general_stop(run, b"Transcript " + t["tid"] + b" is associated with multiple gene names!")
            if it.transcript_name:
                if not t["tname"]:
                    t["tname"] = it.transcript_name
                elif t["tname"] != it.transcript_name:
                    general_stop(run, b"Transcript " + t["tid"] + b" is associated with multiple transcript names!")
            if cur_e + 1 < it.start:
                if cur_s > 0:
                    t["structure"].append((cur_s, cur_e))
                cur_s = it.start
            cur_e = max(cur_e, it.end)
        if cur_s > 0:
            t["structure"].append((cur_s, cur_e))
        t["length"] = sum(e + 1 - s for s, e in t["structure"])
        trs.append(t)
        sp = ep
    if not trs:
        general_stop(run, b"The reference contains no transcripts!")
    return trs


def ti_text(trs, typ):
    out = b"%d %d\n" % (len(trs), typ)
    for t in trs:
        out += t["tid"] + (b"\t" + t["tname"] if t["tname"] else b"") + b"\n" + t["gid"] + (b"\t" + t["gname"] if t["gname"] else b"") + b"\n"
        out += t["seqname"] + b"\n" + t["strand"] + b" %d\n" % t["length"] + b"%d" % len(t["structure"])
        out += b"".join(b" %d %d" % se for se in t["structure"]) + b"\n" + t["left"] + b"\n"
    return out


def numbers(v):
    return b"".join(b"%d\n" % x for x in v)


# ---- the programs: argv as the reference takes it (without argv[0]), files relative to cwd -------------------------------------

def extract(run, a):
    has_mapping = c_atoi(a[4].encode()) if len(a) > 4 else 0
    if len(a) < 6 or (has_mapping and len(a) < 7):
        raise Stop
    mi = load_mapping(run, 1, a[5])[0] if has_mapping else None
    sources = set() if a[3] == "None" else set(s for s in a[3].encode().split(b",") if s)
    trs = parse_gtf(run, a[2], sources, mi)
    seqs, chrvec, seqname = [None] * len(trs), [], b""
    for fname in a[6 if has_mapping else 5:]:
        data = run.read(fname)
        for head, lo, hi in frame_fasta(data):
            seqname = first_token(head) or seqname
            (gseq, bad), = load_ref(data, [lo], [hi], True)
            if bad >= 0:
                bad_character(run, fname, data, bad)
            if not gseq:
                raise Stop  # (the reference's assert; the drop-in's own message)
            mine = [k for k, t in enumerate(trs) if t["seqname"] == seqname]
            if not mine:
                continue
            chrvec.append((seqname, len(gseq)))
            for k in mine:
                t = trs[k]
                st = t["structure"]
                if st[0][0] < 1 or st[-1][1] > len(gseq):
                    run.err += b"Transcript " + t["tid"] + b" is out of chromosome " + t["seqname"] + b"'s boundary!\n"
                    raise Stop
                if t["strand"] == b"+":
                    seqs[k] = b"".join(segment_ref(gseq, s - 1, e - s + 1, 0) for s, e in st)
                else:
                    seqs[k] = b"".join(segment_ref(gseq, s - 1, e - s + 1, RC) for s, e in reversed(st))
    chrvec.sort(key=lambda c: c[0])  # stable: occurrences of a name keep file order
    kept, n_warns = [], 0
    for k, t in enumerate(trs):
        if seqs[k] is None:
            n_warns += 1
            if n_warns <= MAX_WARNS:
                run.err += b"Warning: Cannot extract transcript " + t["tid"] + b"'s sequence since the chromosome it locates, " + t["seqname"] + b", is absent!\n"
        else:
            kept.append(k)
    if n_warns:
        run.err += b"Warning: %d transcripts are failed to extract because their chromosome sequences are absent.\n" % n_warns
    if not kept:
        general_stop(run, b"The reference contains no transcripts!")
    starts, cur = [], b""
    for i, k in enumerate(kept):
        if trs[k]["gid"] != cur:
            starts.append(i + 1)
            cur = trs[k]["gid"]
    starts.append(len(kept) + 1)
    ref = a[0]
    run.files[ref + ".grp"] = numbers(starts)
    run.files[ref + ".ti"] = ti_text([trs[k] for k in kept], 0)
    run.files[ref + ".chrlist"] = b"".join(n + b"\t%d\n" % l for n, l in chrvec)
    run.files[ref + ".transcripts.fa"] = b"".join(b">" + trs[k]["tid"] + b"\n" + seqs[k] + b"\n" for k in kept)


def synthesis(run, a):
    mode = c_atoi(a[2].encode()) if len(a) > 2 else 0
    if len(a) < 4 or (mode and len(a) < 5):
        raise Stop
    t1, t2 = load_mapping(run, mode, a[3]) if mode else ({}, {})
    trs, name2seq, seqname = [], {}, b""
    for fname in a[4 if mode else 3:]:
        data = run.read(fname)
        for head, lo, hi in frame_fasta(data):
            seqname = first_token(head) or seqname
            (gseq, bad), = load_ref(data, [lo], [hi], True)
            if bad >= 0:
                bad_character(run, fname, data, bad)
            if not gseq:
                raise Stop
            name2seq[seqname] = gseq
            gid = tid = seqname
            if mode:
                if seqname not in t1:
                    general_stop(run, b"Mapping Info is not correct, cannot find " + seqname + b"'s gene_id!")
                gid = t1[seqname]
                if mode == 2:
                    if seqname not in t2:
                        general_stop(run, b"Mapping Info is not correct, cannot find allele " + seqname + b"'s transcript_id!")
                    tid = t2[seqname]
            trs.append({"tid": tid, "gid": gid, "seqname": seqname, "strand": b"+", "left": b"", "gname": b"", "tname": b"", "structure": [(1, len(gseq))], "length": len(gseq)})
    if not trs:
        general_stop(run, b"Number of transcripts in the reference is less than 1!")
    trs.sort(key=lambda t: (t["gid"], t["tid"], t["seqname"]))
    gi, gt, ta, cg, ct = [], [], [], b"", b""
    for i, t in enumerate(trs, 1):
        if cg != t["gid"]:
            gi.append(i)
            gt.append(len(ta))
            cg = t["gid"]
        if mode == 2 and ct != t["tid"]:
            ta.append(i)
            ct = t["tid"]
    gi.append(len(trs) + 1)
    gt.append(len(ta))
    ta.append(len(trs) + 1)
    ref = a[0]
    run.files[ref + ".ti"] = ti_text(trs, 2 if mode == 2 else 1)
    run.files[ref + ".grp"] = numbers(gi)
    if mode == 2:
        run.files[ref + ".gt"] = numbers(gt)
        run.files[ref + ".ta"] = numbers(ta)
    run.files[ref + ".transcripts.fa"] = b"".join(b">" + t["seqname"] + b"\n" + name2seq[t["seqname"]] + b"\n" for t in trs)


def preref(run, a):
    if len(a) < 3:
        raise Stop
    choice, poly_a, exc_f = c_atoi(a[1].encode()), 125, ""
    for i in range(3, len(a)):
        if a[i] == "-l" and i + 1 < len(a):
            poly_a = c_atoi(a[i + 1].encode())
        if a[i] == "-f" and i + 1 < len(a):
            exc_f = a[i + 1]
    exceptions = set(run.read(exc_f).split()) if choice == 2 else set()
    data = run.read(a[0])
    seq_txt = idx = n2g = b""
    for tag, lo, hi in frame_fasta(data):
        (raw, _), = load_ref(data, [lo], [hi], False)
        if not raw:
            run.err += b"Warning: Fasta entry " + tag + b" has an empty sequence! It is omitted!\n"
            continue
        tail = poly_a if choice == 0 else 0 if choice == 1 else (0 if tag in exceptions else poly_a)
        full = len(raw)
        seq = segment_ref(raw, 0, full, UPPER_N) + segment_ref(None, 0, tail, FILL)
        masks = [0] * ((full - 1) // 32 + 1)
        if tail > 0:
            for i in range(max(full - 24, 0), full):
                masks[i // 32] |= 1 << (i % 32)
        seq_txt += b"%d %d\n" % (full, full + tail) + tag + b"\n" + seq + b"\n" + b" ".join(b"%d" % m for m in masks) + b"\n"
        idx += b">" + tag + b"\n" + seq + b"\n"
        n2g += b">" + tag + b"\n" + segment_ref(raw, 0, full, UPPER_N | N2G) + segment_ref(None, 0, tail, FILL) + b"\n"
    ref = a[2]
    run.files[ref + ".seq"], run.files[ref + ".idx.fa"], run.files[ref + ".n2g.idx.fa"] = seq_txt, idx, n2g


def run_program(prog, args, cwd):
    """-> (files written: name -> bytes, stderr bytes, exit status).  A program that stops has written none of its files (all the
    writes come last)."""
    run = Run(cwd)
    try:
        {"extract": extract, "synthesis": synthesis, "preref": preref}[prog](run, list(args))
    except Stop:
        return {}, run.err, 255
    return run.files, run.err, 0


# ---- the fixtures --------------------------------------------------------------------------------------------------------------

def case_names():
    return sorted(d for d in os.listdir(GOLDEN) if os.path.isfile(os.path.join(GOLDEN, d, "case.json")))


def load_case(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "case.json")) as f:
        c = json.load(f)
    c["dir"] = d
    with open(os.path.join(d, "stderr.txt"), "rb") as f:
        c["stderr"] = f.read()
    c["files"] = {}
    for fn in c["outputs"]:
        p = os.path.join(d, "out", fn)
        if os.path.exists(p + ".gz"):
            with gzip.open(p + ".gz", "rb") as f:
                c["files"][fn] = f.read()
        else:
            with open(p, "rb") as f:
                c["files"][fn] = f.read()
    return c


def stage_case(case, tmp):
    """The case's inputs into tmp (the programs run there under the recorded names)."""
    import shutil
    for fn in os.listdir(case["dir"]):
        p = os.path.join(case["dir"], fn)
        if os.path.isfile(p) and fn not in ("case.json", "stderr.txt"):
            shutil.copy(p, os.path.join(tmp, fn))
