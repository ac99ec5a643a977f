"""Inputs at the limits rsem_amd/csrc/gmap_block.hpp names, shared by tests/test_gmap_limits_gpu.py (the device) and tests/test_gmap_cpu.py
(tests/gmap_check.cpp, the same source on the lane emulator): the exon cap kMaxExons = 32766 that keeps n_cigar inside rev_ncigar's low
16 bits, positions up to 2^31 - 2 whose bins leave 16 bits, keys that differ in one field only, and a launch that mixes wave-sized and
longer groups.  A case is (mates, group_off, tr, pos, l_qseq, flag, w) as capi.Gmap.convert takes them."""
import numpy as np

import gmap_ref as gr

MAX_EXONS = 32766  # kMaxExons
EDGES = (14, 17, 20, 23, 26)  # the bin levels of reg2bin
N_VALUES = 240  # distinct values a key field takes: above (700 + 2) // 3
POOL = np.array([1.0, 2.0 ** -24, 0.1, 3e-7, 2.0 ** -25], np.float32)

_cache = {}


def transcripts():
    """the transcripts of every case here, by name; computed once, never changed"""
    if "ti" not in _cache:
        ti = []

        def add(name, seqname, strand, exons):
            ti.append(dict(transcript_id=name, seqname=seqname, strand=strand, length=sum(e - s + 1 for s, e in exons), exons=exons))

        cap = [(1 + 2 * k, 1 + 2 * k) for k in range(MAX_EXONS)]
        hi = [(2 ** 29 - 9, 2 ** 29 + 10), (2 ** 31 - 21, 2 ** 31 - 2)]
        for s in "+-":
            add("cap" + s, "chrA", s, cap)
            add("hi" + s, "chrA", s, hi)
            for b in EDGES:
                add("e%d%s" % (b, s), "chrA", s, [(2 ** b - 29, 2 ** b), (2 ** b + 11, 2 ** b + 40)])  # an exon's end on the edge
                add("s%d%s" % (b, s), "chrA", s, [(2 ** b - 29, 2 ** b + 30)])                           # an exon across it
            add("x300" + s, "chrA", s, [(1000 + 25 * k, 1009 + 25 * k) for k in range(300)])
            add("one" + s, "chrA", s, [(1000, 3999)])
        add("last", "chrA", "+", [(1000, 1009), (1100, 1399)])
        for v in range(N_VALUES):
            add("tid%d" % v, "chr%d" % v, "+", [(1000, 3999)])                      # the same local place on another sequence
            add("first%d" % v, "chrA", "+", [(1000, 1000 + v), (2000, 2099)])      # the same start, another first exon
        _cache["ti"] = ti
        _cache["idx"] = {t["transcript_id"]: i for i, t in enumerate(ti)}
        names = ["chrA"] + ["chr%d" % v for v in np.random.default_rng(1).permutation(N_VALUES)]  # output ids in no order of the transcripts
        _cache["out_ids"] = {n: i for i, n in enumerate(names)}
    return _cache["ti"], _cache["idx"], _cache["out_ids"]


def flat():
    ti, _, out_ids = transcripts()
    return gr.flat_reference(ti, out_ids)


# ---- the exon cap ---------------------------------------------------------------------------------------------------------------

def cap_reads():
    """single reads, a group each: the whole transcript and a poly-A tail of 5 on either strand (on '-' the tail is the lead: the
    largest n_cigar there is), the whole transcript, the last exon alone"""
    idx, L = transcripts()[1], MAX_EXONS
    rows = [("cap+", 0, L + 5), ("cap-", 0, L + 5), ("cap+", 0, L), ("cap-", 0, L), ("cap+", L - 1, 1), ("cap-", 0, 1), ("cap+", L - 1, 4), ("cap+", L, 3)]
    n = len(rows)
    return 1, list(range(n + 1)), [idx[r[0]] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [0] * n, [1.0] * n


CAP_GROUP = [("cap+", 5), ("cap+", 5), ("cap+", 6), ("cap-", 5), ("cap+", 0), ("cap-", 0), ("cap+", 5)]
CAP_GROUP_KEPT = 5  # the three with tail 5 are one


def cap_group(mates):
    """one group at one position: two identical alignments and a third further on (they collapse, the weights fold in file order), one with
    tail 6 for 5 (the LAST of 65532 words differs), the '-' twin (the strand bit decides before any word), and without a tail either strand
    (65531 equal words, the strand bit alone).  mates == 2: each as mate 2 of a pair whose mate 1 is constant."""
    idx, L = transcripts()[1], MAX_EXONS
    tr, pos, lq, flag = [], [], [], []
    for name, tail in CAP_GROUP:
        if mates == 2:
            tr.append(idx["cap+"]); pos.append(L - 1); lq.append(1); flag.append(99)
        tr.append(idx[name]); pos.append(0); lq.append(L + tail); flag.append(147 if mates == 2 else 0)
    w = np.array([1.0, 2.0 ** -24, 0.1, 3e-7, 0.1, 0.1, 2.0 ** -24], np.float32)
    assert gr.fold32([w[0], w[1], w[6]]) != gr.fold32([w[6], w[1], w[0]])  # the order of the fold shows
    return mates, [0, len(CAP_GROUP)], tr, pos, lq, flag, w


# ---- high positions ----------------------------------------------------------------------------------------------------------------

def high_reads():
    """reads that end one base before, on and one base after every exon edge and bin edge, over the junctions, into and inside the tail"""
    idx = transcripts()[1]
    rows = []
    for s in "+-":
        for b in EDGES:
            rows += [("e%d%s" % (b, s), p, n) for p, n in ((20, 9), (20, 10), (20, 11), (30, 5), (29, 1), (0, 60), (55, 8), (60, 2))]
            rows += [("s%d%s" % (b, s), p, n) for p, n in ((20, 9), (20, 10), (20, 11), (30, 5), (29, 1), (29, 2), (0, 60))]
        rows += [("hi" + s, p, n) for p, n in ((0, 9), (0, 10), (0, 11), (9, 1), (10, 1), (5, 14), (5, 15), (5, 16), (19, 2), (20, 5), (20, 20), (35, 5), (35, 10),
                                               (40, 3), (0, 40), (0, 47))]
    n = len(rows)
    return 1, list(range(n + 1)), [idx[r[0]] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [0] * n, [1.0] * n


# ---- one key field at a time -------------------------------------------------------------------------------------------------------

FIELDS = ["tid", "strand", "n_cigar", "first_word", "last_word", "mate2_pos", "mate2_last_word"]


def field_group(n, field, seed=None):
    """n alignments of one read in interleaved runs of 3 equal keys (the members of a run lie (n + 2) // 3 apart); two keys differ in
    `field` alone -- for `strand`, which has two values, in the position or in the strand bit alone.  Returns the case and the number
    of mates."""
    idx = transcripts()[1]
    rng = np.random.default_rng(n if seed is None else seed)
    m = (n + 2) // 3
    assert m <= N_VALUES
    # the value of alignment a, in no order; for the strand the values 0 .. m - 1, so that both strands of a place are there
    v = (rng.permutation(m) if field == "strand" else rng.permutation(N_VALUES)[:m])[np.arange(n) % m]
    w = POOL[rng.integers(0, len(POOL), n)]
    one = idx["one+"]
    if field == "tid":
        mate = [(idx["tid%d" % x], 77, 50, 0) for x in v]
    elif field == "strand":  # 50 bases at genome 1000 + 10 * (x // 2) on either strand's transcript
        mate = [(idx["one+"], 10 * (x // 2), 50, 0) if x % 2 == 0 else (idx["one-"], 3000 - 10 * (x // 2) - 50, 50, 0) for x in v]
    elif field == "n_cigar":  # from one start over x junctions
        mate = [(idx["x300+"], 0, 5 + 10 * x, 0) for x in v]
    elif field == "first_word":  # (x + 1)M, an N, 10M
        mate = [(idx["first%d" % x], 0, x + 1 + 10, 0) for x in v]
    elif field in ("last_word", "mate2_last_word"):  # 10M 90N (x + 1)M
        mate = [(idx["last"], 0, 10 + x + 1, 0) for x in v]
    else:
        mate = [(one, 7 * x, 50, 0) for x in v]
    mates = 2 if field.startswith("mate2") else 1
    tr, pos, lq, flag = [], [], [], []
    for t, p, l, f in mate:
        if mates == 2:
            tr.append(one); pos.append(5); lq.append(50); flag.append(99)
        tr.append(t); pos.append(p); lq.append(l); flag.append(147 if mates == 2 else f)
    return (mates, [0, n], tr, pos, lq, flag, w), m


def keys_of(case):
    """the alignments' keys as the collapse compares them: per mate tid, pos, strand bit, n_cigar, the words"""
    ti, _, out_ids = transcripts()
    mates, _, tr, pos, lq, flag, _ = case
    mapped = gr.map_fields(ti, flat()[2], tr, pos, lq, flag)
    keys = []
    for a in range(len(tr) // mates):
        k = ()
        for mm in range(mates):
            tid, p, f, words, _, _ = mapped[a * mates + mm]
            k += (tid, p, (f >> 4) & 1, len(words)) + tuple(words)
        keys.append(k)
    return keys, mapped


def first_differences(case, field):
    """where two neighbours among the sorted distinct keys first differ, as names of fields"""
    keys, mapped = keys_of(case)
    mates = case[0]
    out = set()
    ks = sorted(set(keys))
    for a, b in zip(ks, ks[1:]):
        i = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
        n1 = 4 + a[3]  # the fields of mate 1
        pre, j, nc = ("", i, a[3]) if i < n1 or mates == 1 else ("mate2_", i - n1, a[n1 + 3])
        out.add(pre + (["tid", "pos", "strand", "n_cigar"][j] if j < 4 else "first_word" if j == 4 else "last_word" if j == 4 + nc - 1 else "word"))
    return out


# ---- a launch of wave-sized and longer groups --------------------------------------------------------------------------------------

def mixed_launch(n_small, where):
    """n_small groups of 1, 2, 64, 1, ... alignments and two longer ones (65 and 300), the longer ones first, in the middle or last"""
    idx = transcripts()[1]
    small = [(1, 2, 64)[k % 3] for k in range(n_small)]
    sizes = {"first": [65, 300] + small, "middle": small[:(n_small + 1) // 2] + [65, 300] + small[(n_small + 1) // 2:], "last": small + [65, 300]}[where]
    if where == "middle" and n_small == 1:
        sizes = [65] + small + [300]
    rng = np.random.default_rng(100 * n_small + len(where))
    pos = []
    for n in sizes:
        m = (n + 2) // 3
        pos += rng.permutation(2000)[:m][np.arange(n) % m].tolist()
    n = sum(sizes)
    return 1, np.concatenate([[0], np.cumsum(sizes)]).tolist(), [idx["x300+"]] * n, pos, [50] * n, [0] * n, POOL[rng.integers(0, len(POOL), n)]


# ---- tests/gmap_check.cpp's `fields` mode ------------------------------------------------------------------------------------------

def fields_input(case):
    """the text the check program reads: the transcripts, then the case"""
    strand, length, out_tid, off, st, en = flat()
    mates, group_off, tr, pos, lq, flag, w = case
    out = ["%d %d" % (len(length), len(st))]
    out.append(" ".join("%d %d %d %d" % (ord(strand[t]), length[t], out_tid[t], off[t + 1]) for t in range(len(length))))
    out.append(" ".join("%d %d" % se for se in zip(st, en)))
    out.append("%d %d %d" % (mates, len(w), len(group_off) - 1))
    out.append(" ".join(str(int(g)) for g in group_off))
    out.append(" ".join("%d %d %d %d" % x for x in zip(tr, pos, lq, flag)))
    out.append(" ".join("%08x" % b for b in np.ascontiguousarray(w, np.float32).view(np.uint32)))
    return "\n".join(out) + "\n"


def fields_expected(case):
    """what the check program prints for the case, from the restatement"""
    ti, _, _ = transcripts()
    mates, group_off, tr, pos, lq, flag, w = case
    mapped = gr.map_fields(ti, flat()[2], tr, pos, lq, flag)
    src, ws = gr.collapse_fields(mates, group_off, mapped, w)
    out = ["%d %d %d %d %d %d %s" % (m[0], m[1], m[2], len(m[3]), m[4], m[5], " ".join(str(x) for x in m[3])) for m in mapped]
    out += ["out %d %08x" % (s, b) for s, b in zip(src, ws.view(np.uint32))]
    return "\n".join(out) + "\n"
