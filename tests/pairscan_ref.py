"""TEST INFRASTRUCTURE: rsem-scan-for-paired-end-reads restated in Python, record by record as the reference program goes
(scanForPairedEndReads.cpp:24-51,78-126), with a STABLE sort where the reference calls std::sort; and what the tests share: the
fixtures of tests/golden/pairscan/, records <-> BAM bytes <-> the arrays of rsem_pairscan_reorder.
Nothing here is fast and nothing here is used by the product."""
import collections
import gzip
import os
import struct
import zlib

import numpy as np

import gmap_ref as gr
from alncheck_ref import canonical, header_bytes

ROOT = gr.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "pairscan")
PROGRAM = os.path.join(ROOT, "rsem_amd", "bin", "rsem-scan-for-paired-end-reads")
DEFAULT_BATCH_ITEMS = 1 << 22
OK, MIXED, ODD_FULL, ODD_PARTIAL, NO_PARTNER = range(5)
LARGE_CASES = ("both18", "both40")  # groups of more than 16 `both` records: compared up to the order inside runs of tied records

# name: the raw read name (bytes, no NUL)
Rec = collections.namedtuple("Rec", "name flag tid pos mpos")
Verdict = collections.namedtuple("Verdict", "code group group_record")

# flags of the synthetic records: proper pairs (read 1 / read 2, forward / reverse), partial and unknown records
R1F, R1R, R2F, R2R = 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x40 | 0x10, 0x1 | 0x2 | 0x80 | 0x20, 0x1 | 0x2 | 0x80 | 0x10
P1, P2, PU = 0x1 | 0x40 | 0x8, 0x1 | 0x80 | 0x8, 0x1
U1, U2 = 0x1 | 0x4 | 0x8 | 0x40, 0x1 | 0x4 | 0x8 | 0x80


def rec(name, flag=0, tid=0, pos=0, mpos=-1):
    if isinstance(name, str):
        name = name.encode()
    return Rec(name, flag, tid, pos, mpos)


def proper(name, tid, p1, p2, rev=False, name2=None):
    """the two records of a properly aligned pair: read 1 at p1, read 2 at p2"""
    return [rec(name, R1R if rev else R1F, tid, p1, p2), rec(name if name2 is None else name2, R2F if rev else R2R, tid, p2, p1)]


def parse_record(d):
    tid, pos, l_name, _, _, _, flag, _, _, mpos, _ = struct.unpack_from(gr.CORE, d, 0)
    return Rec(d[32:32 + l_name].split(b"\0")[0], flag, tid, pos, mpos)


def record_bytes(r, k=0):
    """a BAM record (without block_size) of a Rec: 4 bases, one tag that tells records with equal fields apart"""
    name = r.name + b"\0"
    unmapped = bool(r.flag & 4)
    body = struct.pack(gr.CORE, r.tid, r.pos, len(name), 255, gr.reg2bin(max(r.pos, 0), max(r.pos, 0) + 1) & 0xffff, 0 if unmapped else 1, r.flag, 4, r.tid if r.flag & 1 else -1,
                       r.mpos, 0)
    return body + name + (b"" if unmapped else struct.pack("<I", 4 << 4)) + bytes([0x12, 0x48]) + bytes([30] * 4) + b"XIi" + struct.pack("<i", k)


HEADER_TEXT = "@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:t1\tLN:1000\n@SQ\tSN:t2\tLN:2000\n@SQ\tSN:t3\tLN:500\n"


def write_bam(path, recs, block=300, text=HEADER_TEXT, raw=None):
    """the records (or the BAM records `raw`, without block_size) as a BAM file in BGZF blocks of `block` bytes"""
    raw = [record_bytes(r, k) for k, r in enumerate(recs)] if raw is None else raw
    data = gr.bam_header(text) + b"".join(struct.pack("<i", len(b)) + b for b in raw)
    with open(path, "wb") as f:
        for i in list(range(0, len(data), block)) + [None]:
            chunk = b"" if i is None else data[i:i + block]
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            comp = co.compress(chunk) + co.flush()
            f.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))


def pack(recs):
    """the arrays of rsem_pairscan_reorder"""
    name_off = np.zeros(len(recs) + 1, np.uint64)
    if recs:
        name_off[1:] = np.cumsum([len(r.name) for r in recs])
    names = np.frombuffer(b"".join(r.name for r in recs) + b"\0", np.uint8).copy()
    f = lambda k, t: np.array([getattr(r, k) for r in recs], t)
    return dict(name_off=name_off, names=names, flag=f("flag", np.uint32), tid=f("tid", np.int32), pos=f("pos", np.int32), mpos=f("mpos", np.int32))


# ---- the program, record by record ---------------------------------------------------------------------------------------------------

def i32(x):
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


def key(r):
    """less_than (:39-51): signed 32-bit fields, then the pattern code"""
    rev = r.flag >> 4 & 1
    return (i32(r.tid), min(i32(r.pos), i32(r.mpos)), max(i32(r.pos), i32(r.mpos)), rev if r.flag & 0x40 else 1 - rev)


def class_of(flag):
    if not flag & 4 and flag & 2:
        return 0
    return 1 if flag & 0x40 else (2 if flag & 0x80 else 3)


def walk(recs):
    """the sequential walk of :78-87,117-122: [(first, end, paired, mixed)] -- mixed: the first record of a paired group without bit 0x1"""
    out, i, n = [], 0, len(recs)
    while i < n:
        q, paired, j, mixed = canonical(recs[i].name), recs[i].flag & 1, i + 1, None
        if paired:
            while j < n and canonical(recs[j].name) == q:
                if mixed is None and not recs[j].flag & 1:
                    mixed = j
                j += 1
        else:
            while j < n and recs[j].name.split(b"\0")[0] == q:  # (:119 compares C strings)
                j += 1
        out.append((i, j, paired, mixed))
        i = j
    return out


def lifo_order(n1, n2, nu):
    """:98-115 with the vectors holding 0 .. n - 1: [(class, index)] in output order, or None where back() meets an empty vector"""
    a, b, u, out = list(range(n1)), list(range(n2)), list(range(nu)), []
    while a or b:
        if a and b:
            out += [(1, a.pop()), (2, b.pop())]
        else:
            left, c = (a, 1) if a else (b, 2)
            out.append((c, left.pop()))
            if not u:
                return None
            out.append((3, u.pop()))
    while u:
        out.append((3, u.pop()))
    return out


def group_order(recs, first, end):
    """a paired group's output order and the first check it fails"""
    arr = [[], [], [], []]
    for i in range(first, end):
        arr[class_of(recs[i].flag)].append(i)
    if len(arr[0]) % 2:
        return None, ODD_FULL
    if (len(arr[1]) + len(arr[2]) + len(arr[3])) % 2:
        return None, ODD_PARTIAL
    order = lifo_order(len(arr[1]), len(arr[2]), len(arr[3]))
    if order is None:
        return None, NO_PARTNER
    return sorted(arr[0], key=lambda i: key(recs[i])) + [arr[c][k] for c, k in order], OK  # (sorted is stable)


def reorder(recs):
    """(perm, verdict, groups): perm[k] = the input index of the k-th output record (None from the failing group on)"""
    perm, groups = [], walk(recs)
    for g, (first, end, paired, mixed) in enumerate(groups):
        if not paired:
            perm += range(first, end)
            continue
        if mixed is not None:
            return perm, Verdict(MIXED, g, first), g
        order, code = group_order(recs, first, end)
        if code:
            return perm, Verdict(code, g, first), g
        perm += order
    return perm, Verdict(OK, -1, -1), len(groups)


MESSAGES = {MIXED: "Read %s is detected as both single-end and paired-end read!",
            ODD_FULL: "Number of first and second mates in read %s's full alignments (both mates are aligned) are not matched!",
            ODD_PARTIAL: "Number of first and second mates in read %s's partial alignments (at most one mate is aligned) are not matched!"}


def scan(path):
    """(stdout, stderr, exit status, decompressed output or None) of the program for an alignment file"""
    _, _, raw = gr.read_alignments(path)
    recs = [parse_record(d) for d in raw]
    perm, v, done = reorder(recs)
    dots = "." + "." * (done // 1000000)
    if v.code:
        q = canonical(recs[v.group_record].name).decode()
        return (dots + "\n").encode(), ((MESSAGES[v.code] % q) + "\n").encode() if v.code in MESSAGES else None, 255, None
    return (dots + "\nFinished!\n").encode(), b"", 0, header_bytes(path) + b"".join(struct.pack("<i", len(raw[i])) + raw[i] for i in perm)


# ---- the order inside runs of tied records -------------------------------------------------------------------------------------------

def canonical_ties(out_bytes):
    """a decompressed output with every maximal run of records that tie under less_than inside a group sorted by the records' bytes
    (the two large fixtures: the reference's order there is its library's)"""
    text, targets, raw = gr.split_bam(out_bytes)
    recs = [parse_record(d) for d in raw]
    out, k = [], 0
    for first, end, paired, _ in walk(recs):
        i = first
        while i < end:
            j = i + 1
            if paired and class_of(recs[i].flag) == 0:
                while j < end and class_of(recs[j].flag) == 0 and key(recs[j]) == key(recs[i]):
                    j += 1
            out += sorted(raw[i:j])
            i = j
    p = len(out_bytes) - sum(4 + len(d) for d in raw)
    return out_bytes[:p] + b"".join(struct.pack("<i", len(d)) + d for d in out)


# ---- the library ---------------------------------------------------------------------------------------------------------------------

def run_cuts(recs, cuts):
    """the calls' boundaries moved to where a canonical name starts (the library takes whole runs)"""
    out = []
    for c in cuts:
        while 0 < c < len(recs) and canonical(recs[c].name) == canonical(recs[c - 1].name):
            c += 1
        if 0 < c < len(recs) and c not in out:
            out.append(c)
    return out


def device_perm(recs, cuts=(), handle=None):
    """the records through capi.Pairscan in calls cut at the record indices `cuts` (each at a run's start): (perm or the part before
    the failing call, verdict in the file's coordinates, the calls' dicts)"""
    from rsem_amd import capi
    ps = handle or capi.Pairscan()
    bounds = [0] + list(cuts) + [len(recs)]
    perm, groups, calls = [], 0, []
    try:
        for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
            p, v = ps.reorder(last=(handle is None and k == len(bounds) - 2), **pack(recs[a:b]))
            calls.append(v)
            assert v["n_records"] == b - a and 10 * v["n_batches"] <= v["n_launches"] <= 11 * v["n_batches"]
            if v["code"]:
                assert v["group"] >= 0 and v["group_record"] >= 0
                return perm, Verdict(v["code"], groups + v["group"], a + v["group_record"]), calls
            assert v["group"] == -1 and v["group_record"] == -1
            assert sorted(p.tolist()) == list(range(b - a))
            perm += [a + int(x) for x in p]
            groups += v["n_groups"]
    finally:
        if handle is None:
            ps.close()
    return perm, Verdict(OK, -1, -1), calls


def expected_batches(recs, budget):
    """whole runs of equal canonical names within the budget; a run above it is a batch of its own"""
    starts = [i for i in range(len(recs)) if i == 0 or canonical(recs[i].name) != canonical(recs[i - 1].name)] + [len(recs)]
    n, lo = 0, 0
    while lo < len(recs):
        if len(recs) - lo <= budget:
            hi = len(recs)
        else:
            within = [s for s in starts if lo < s <= lo + budget]
            hi = within[-1] if within else min(s for s in starts if s > lo)
        n, lo = n + 1, hi
    return n


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------

def cases():
    return sorted(f[:-len(".status")] for f in os.listdir(GOLDEN) if f.endswith(".status"))


def inputs(which=None):
    return [(c, os.path.join(GOLDEN, c + e)) for c in (which or cases()) for e in (".sam", ".bam")]


def input_id(ci):
    return os.path.basename(ci[1])


def recorded(case, suffix):
    p = os.path.join(GOLDEN, case + suffix)
    if os.path.exists(p + ".gz"):
        return gzip.open(p + ".gz", "rb").read()
    return open(p, "rb").read()


def status(case):
    return int(recorded(case, ".status").decode())


def load(path):
    """[Rec] of an alignment file"""
    return [parse_record(d) for d in gr.read_alignments(path)[2]]


def same_output(case, got, want):
    """the comparison the fixtures are held to: bytes, but for the two large cases' tie runs"""
    if case in LARGE_CASES:
        return canonical_ties(got) == canonical_ties(want)
    return got == want


def closed_form_order(n1, n2, nu):
    """lifo_order through the arithmetic of partial_slot (rsem_amd/csrc/pairscan_block.hpp), restated"""
    m, L = min(n1, n2), abs(n1 - n2)
    if (n1 + n2 + nu) % 2 or L > nu:
        return None
    out = [None] * (n1 + n2 + nu)
    for r in range(n1):
        out[2 * (n1 - 1 - r)] = (1, r)
    for r in range(n2):
        b = n2 - 1 - r
        out[2 * b + 1 if b < m else 2 * b] = (2, r)
    for r in range(nu):
        b = nu - 1 - r
        out[2 * m + 2 * b + 1 if b < L else 2 * m + L + b] = (3, r)
    return out


def soft_rule_starts(recs):
    """group starts by the prefix-count rule of the device code: a hard start, or a soft candidate with no paired hard start or soft
    candidate before it in its run"""
    starts, paired_seen = [], 0
    for i, r in enumerate(recs):
        hard = i == 0 or canonical(r.name) != canonical(recs[i - 1].name)
        soft = not hard and len(r.name.split(b"\0")[0]) > len(canonical(r.name))
        if hard:
            paired_seen = 0
        if hard or (soft and paired_seen == 0):
            starts.append(i)
        if hard or soft:
            paired_seen += r.flag & 1
    return starts
