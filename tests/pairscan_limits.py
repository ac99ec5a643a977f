"""TEST INFRASTRUCTURE: the inputs of tests/test_pairscan_limits_gpu.py and of the limit cases of tests/test_pairscan_cpu.py --
rsem_pairscan_reorder where the value domain ends: every value of the flag's low byte, groups of whole tiles and of more than three,
keys at the two ends of 32 bits, names of kMaxName bytes, of canonical length 0, with a prefix for a neighbour and with a NUL inside.
Plain lists of pairscan_ref.Rec; the expectation is always pairscan_ref's."""
import pairscan_ref as pr
from pairscan_ref import P2, R1F, R1R, R2R, rec

MAX_NAME = 254  # kMaxName of rsem_amd/csrc/alncheck_block.hpp
FAIL_CODES = (pr.MIXED, pr.ODD_FULL, pr.ODD_PARTIAL, pr.NO_PARTNER)
HIGH_BITS = (0, 0x100, 0x800, 0x900)  # secondary and supplementary: no code reads them


def singles(n, name="u%d"):
    return [rec(name % k, 16 * (k % 2), k % 3, k) for k in range(n)]


# ---- every flag byte -------------------------------------------------------------------------------------------------------------------

# A group is a fixed first record and records whose flags are drawn from f: f itself, f with the strand bit turned and f with the two
# mate bits turned.  A first record of class `both` (R1F) lets a group of `both` records come out OK and sorted; a partial first record
# (P2) lets the partial and unknown ones come out OK -- a group of one `both` record and partial ones has an odd number of full
# alignments whatever f is -- so there are two fixed paired first records, and 0 as the unpaired one.
SHAPES = [(R1F, lambda f: [f, f ^ 0x10, f ^ 0xc0]), (P2, lambda f: [f]), (P2, lambda f: [f, f ^ 0x10]), (P2, lambda f: [f, f ^ 0xc0, f ^ 0x10])]


def flag_group(name, first, flags):
    """the first record, then the others: places of their own, but the first two of the others share theirs (they differ in the strand
    bit alone: where they are `both` records the pattern code orders them)"""
    out = [rec(name, first, 1, 300, 700)]
    for k, f in enumerate(flags):
        j = max(k, 1)
        out.append(rec(name, f, 1, 100 + 10 * j, 900 - j))
    return out


def flag_groups(paired, high_bits=HIGH_BITS):
    """[(f | high bits, group)] for every f, every high-bit combination and every shape; with `paired` false the first record is unpaired:
    the group is single-end whatever its other records say"""
    out = []
    for f in range(256):
        for hb in high_bits:
            for s, (first, others) in enumerate(SHAPES):
                name = "%s%02x_%x_%d" % ("p" if paired else "s", f, hb >> 8, s)
                out.append((f | hb, flag_group(name, first if paired else 0, [x | hb for x in others(f)])))
    return out


def split_flag_groups(high_bits=HIGH_BITS):
    """(ok, failing): the groups that pr.reorder puts in order, and of the failing ones one per (code, set of classes among its records)
    where there are more than 64 -- the first such group in the order of flag_groups"""
    ok, failing = [], []
    for paired in (True, False):
        for f, g in flag_groups(paired, high_bits):
            code = pr.reorder(g)[1].code
            if code == pr.OK:
                ok.append(g)
            else:
                failing.append((code, frozenset(pr.class_of(r.flag) for r in g), g))
    if len(failing) > 64:
        seen, few = set(), []
        for code, classes, g in failing:
            if (code, classes) not in seen:
                seen.add((code, classes))
                few.append((code, classes, g))
        failing = few
    return ok, [g for _, _, g in failing]


def on_the_seams(groups):
    """one stream of the groups with single-end fillers, so that a group starts on each of the lanes 0, 63, 64, 255 and on record 256;
    returns (records, the groups' first records)"""
    targets = [0, 63, 256, 256 + 64, 512 + 255]
    recs, starts = [], []
    for k, g in enumerate(groups):
        if targets and len(recs) + len(g) > targets[0] > len(recs):
            recs += singles(targets[0] - len(recs), "f%d_" + str(k))
        if targets and targets[0] <= len(recs):
            targets.pop(0)
        starts.append(len(recs))
        recs += g
    return recs, starts


# ---- group sizes -----------------------------------------------------------------------------------------------------------------------

TILE_EDGES = (255, 511, 1023)
BIG_SIZES = [510, 512, 514, 1024, 4096]


def tied_group(name, n):
    """n properly paired records in descending key order; of every 8, four tie, two tie and two stand alone; the records at 255 | 256,
    511 | 512 and 1023 | 1024 share a place and differ in the pattern code only, the larger one first"""
    out = []
    for i in range(n):
        blk, j = divmod(i, 8)
        sub = 0 if j < 4 else (1 if j < 6 else j - 4)
        pos = 100000 - (blk * 4 + sub) * 3
        out.append(rec(name, R1F if i % 2 == 0 else R2R, blk % 3, pos, pos + 50))
    for a in TILE_EDGES:
        if a + 1 < n:
            out[a] = rec(name, R1R, 1, 7, 9 + a)      # pattern code 1
            out[a + 1] = rec(name, R1F, 1, 7, 9 + a)  # pattern code 0: goes first
    return out


def equal_group(name, n):
    return [rec(name, R1F if i % 2 == 0 else R2R, 2, 40, 90) for i in range(n)]  # (R1F and R2R have one pattern code)


def descending_group(name, n):
    return [rec(name, R1F if i % 2 == 0 else R2R, 0, 3 * (n - i), 3 * (n - i) + 1) for i in range(n)]


def big_stream(sizes=BIG_SIZES, extra=1024):
    """(records, [(first, n)] of the groups): the tied groups, one of `extra` equal records and one of `extra` descending ones"""
    recs, where = [], []
    for k, n in enumerate(sizes):
        where.append((len(recs), n))
        recs += tied_group("g%d" % k, n) + singles(k % 3, "s%d_" + str(k))
    for name, make in (("eq", equal_group), ("desc", descending_group)):
        where.append((len(recs), extra))
        recs += make(name, extra) + singles(2, name + "%d")
    return recs, where


# ---- keys at the ends of 32 bits -------------------------------------------------------------------------------------------------------

ENDS = [-2 ** 31, -1, 0, 1, 2 ** 31 - 1]


def end_keys_group(name="k"):
    """all 25 (pos, mpos) pairs on the two outermost tid values: 50 `both` records, the larger keys first"""
    out = []
    for tid in (2 ** 31 - 1, -2 ** 31):
        for pos in reversed(ENDS):
            for mpos in reversed(ENDS):
                out.append(rec(name, R1F if len(out) % 2 == 0 else R2R, tid, pos, mpos))
    return out


def end_keys_subset(name="k"):
    """eight records whose order is written out in the test"""
    lo, hi = -2 ** 31, 2 ** 31 - 1
    return [rec(name, R1F, 0, hi, lo), rec(name, R2R, 0, -1, hi), rec(name, R1F, hi, lo, lo), rec(name, R2R, lo, hi, hi), rec(name, R1F, 0, lo, lo), rec(name, R2R, 0, 1, -1),
            rec(name, R1F, 0, lo, hi), rec(name, R2R, 0, hi, hi)]


# ---- names -----------------------------------------------------------------------------------------------------------------------------

def paired_four(n1, n2, n3, n4, tid=0):
    """two proper pairs, the first mates before the second ones, under four raw names of one canonical name: one group, reordered"""
    a, b = pr.proper(n1, tid, 50, 90, name2=n3), pr.proper(n2, tid, 10, 40, name2=n4)
    return [a[0], b[0], a[1], b[1]]


def name_blocks():
    """{kind: records}: every kind once in paired groups and once single-end, each block closed in itself (its first and last canonical
    names occur nowhere else)"""
    base = b"N" * (MAX_NAME - 1)
    soft = b"S" * (MAX_NAME - 2)
    blocks = {
        # 254 bytes that differ in the last one: two runs, two groups each way
        "last_byte": paired_four(*[base + b"a"] * 4) + paired_four(*[base + b"b"] * 4) + [rec(base + b"c"), rec(base + b"c"), rec(base + b"d")],
        # 254 bytes that share their canonical name and differ behind the space: one run with soft starts
        "behind_the_space": paired_four(soft + b" a", soft + b" b", soft + b" a", soft + b" b") + [rec(b"T" * (MAX_NAME - 2) + b" a"), rec(b"T" * (MAX_NAME - 2) + b" b"),
                                                                                                 rec(b"T" * (MAX_NAME - 2) + b" b")],
        # a name that is a proper prefix of the next
        "prefix": paired_four(*[b"pre"] * 4) + paired_four(*[b"pref"] * 4) + [rec(b"q"), rec(b"qq"), rec(b"qqq"), rec(b"qqq")],
        # canonical length 0 (the first byte is a space), next to each other and to a name of one byte
        "no_canonical_name": [rec(b"a")] + paired_four(b" a", b" b", b" ", b" a") + [rec(b"b"), rec(b"\tx"), rec(b" y"), rec(b" y"), rec(b"c")],
        # a NUL inside: it ends the name as a space does, and the raw name with it
        "nul": paired_four(b"z\0a", b"z\0b", b"z", b"z\0a") + [rec(b"y\0a"), rec(b"y\0b"), rec(b"y"), rec(b"y x"), rec(b"y\0 x"), rec(b"w\0a", R1F, 0, 5, 9), rec(b"w\0b", R2R, 0, 9, 5)],
    }
    return blocks


def name_stream(kind, at):
    """the block of `kind` with its first record on record `at` of a stream of single-end records"""
    b = name_blocks()[kind]
    return singles(at) + b + singles(5, "t%d")


# ---- list shapes -----------------------------------------------------------------------------------------------------------------------

def list_stream(n_small, n_large):
    """n_small groups of 2 to 64 `both` records and n_large longer ones, single-end and partial-only groups between them"""
    recs = singles(3)
    for k in range(n_small):
        recs += tied_group("w%d" % k, (2, 64, 18, 40, 6)[k % 5]) + singles(1, "a%d_" + str(k))
        recs += [rec("p%d" % k, pr.P1, 0, 4), rec("p%d" % k, pr.P2, 0, 9)]  # a paired group with nothing to sort
    for k in range(n_large):
        recs += tied_group("l%d" % k, (66, 300)[k % 2]) + singles(2, "b%d_" + str(k))
    return recs
