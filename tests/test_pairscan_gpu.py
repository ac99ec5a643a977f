"""rsem-scan-for-paired-end-reads on the GPU (rsem_amd/csrc/pairscan.hip through capi.Pairscan, and the program) against the Python
restatement (tests/pairscan_ref.py) and what the unmodified reference program printed and wrote (tests/golden/pairscan/).  There are no
tolerances: permutations, verdicts and files are compared for equality (the two fixtures with more than 16 properly paired records in
a group: with the runs of tied records sorted by their bytes on both sides, tests/golden/make_pairscan_golden.py).

A lane takes a record, a wave reduces to one atomic and sorts a group of up to 64, a workgroup of 256 lanes sorts a longer one in tiles
of 256: every stream is a few hundred to a few thousand records and puts its events on lanes 0, 63, 64, 255, 256 and the last one."""
import os
import struct
import subprocess

import pytest

import alncheck_ref as ar
import gmap_ref as gr
import pairscan_ref as pr
from pairscan_ref import GOLDEN, P1, P2, PROGRAM, PU, R1F, R1R, R2F, R2R, U1, U2, proper, rec

pytestmark = pytest.mark.gpu

SEAMS = [0, 63, 64, 255, 256]
N = 600


def check(recs, cuts=(), handle=None):
    """the library's order and verdict equal the restatement's; returns (verdict, the calls' dicts)"""
    want_perm, want, _ = pr.reorder(recs)
    perm, got, calls = pr.device_perm(recs, cuts, handle)
    assert got == want
    if want.code == pr.OK:
        assert perm == want_perm
        assert sum(c["n_groups"] for c in calls) == len(pr.walk(recs))
    return got, calls


def singles(n, name="u%d"):
    return [rec(name % k, 16 * (k % 2), k % 3, k) for k in range(n)]


def firsts_then_seconds(name, alignments):
    pairs = [proper(name, *a) for a in alignments]
    return [p[0] for p in pairs] + [p[1] for p in pairs]


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------

def run_program(tmp_path, case, path, threads, env=None):
    assert os.path.exists(PROGRAM), "rsem-scan-for-paired-end-reads was not built"
    out = os.path.join(str(tmp_path), "out.bam")
    r = subprocess.run([PROGRAM, threads, path, out] + (["--device", "0"] if path.endswith(".bam") else []), capture_output=True, env=dict(os.environ, **(env or {})))
    assert (r.returncode, r.stdout, r.stderr) == (pr.status(case), pr.recorded(case, ".stdout"), pr.recorded(case, ".stderr"))
    if r.returncode == 0:
        got = gr.bgzf_inflate(open(out, "rb").read())
        assert got == pr.scan(path)[3]  # the stable order
        assert pr.same_output(case, got, pr.recorded(case, ".out"))
        if case not in pr.LARGE_CASES:
            assert got == pr.recorded(case, ".out")


@pytest.mark.parametrize("ci", pr.inputs(), ids=pr.input_id)
def test_program_against_the_recorded_files(tmp_path, ci):
    case, path = ci
    run_program(tmp_path, case, path, "4" if path.endswith(".bam") else "1")


@pytest.mark.parametrize("budget", ["1", "7", "64"])
@pytest.mark.parametrize("case", pr.cases())
def test_program_batches_and_super_chunks_change_nothing(tmp_path, case, budget):
    """super-chunks of 200 bytes cut through every group: the run of equal canonical names at a chunk's end waits for the next one"""
    for ext in (".sam", ".bam"):
        run_program(tmp_path, case, os.path.join(GOLDEN, case + ext), "2", {"RSEM_PAIRSCAN_BATCH_ITEMS": budget, "RSEM_HIP_BAM_CHUNK": "200"})


@pytest.mark.parametrize("case", pr.cases())
def test_fixtures_through_the_library(case):
    recs = pr.load(os.path.join(GOLDEN, case + ".bam"))
    got, calls = check(recs)
    assert (got.code == pr.OK) == (pr.status(case) == 0)
    if recs:
        assert calls[0]["n_batches"] == 1 and calls[0]["upload_ms"] > 0 and calls[0]["kernel_ms"] > 0 and calls[0]["device_bytes"] > 0


# ---- the rank sort -------------------------------------------------------------------------------------------------------------------

SORT_SIZES = [2, 16, 18, 62, 64, 66, 254, 256, 258, 600]


def sort_group(name, n):
    """n properly paired records in descending key order.  Of every 8, four tie (a run of 4), two tie (a run of 2) and two stand alone;
    the records at 63 | 64 and 255 | 256 share a place and differ in the pattern code only, the larger one first."""
    out = []
    for i in range(n):
        blk, j = divmod(i, 8)
        sub = 0 if j < 4 else (1 if j < 6 else j - 4)
        pos = 100000 - (blk * 4 + sub) * 3
        out.append(rec(name, R1F if i % 2 == 0 else R2R, blk % 3, pos, pos + 50))
    for a in (63, 255):
        if a + 1 < n:
            out[a] = rec(name, R1R, 1, 7, 9 + a)      # pattern code 1
            out[a + 1] = rec(name, R1F, 1, 7, 9 + a)  # pattern code 0: goes first
    return out


@pytest.mark.parametrize("budget", [None, 300])
def test_both_groups_of_every_size_in_one_call(monkeypatch, budget):
    if budget:
        monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", str(budget))
    recs = []
    for k, n in enumerate(SORT_SIZES):
        recs += sort_group("g%d" % k, n) + singles(k % 3, "s%d_" + str(k))
    got, calls = check(recs)
    assert got.code == pr.OK and calls[0]["n_sorted_groups"] == len(SORT_SIZES)
    assert calls[0]["n_batches"] == pr.expected_batches(recs, budget or pr.DEFAULT_BATCH_ITEMS) and calls[0]["batch_items"] == (budget or pr.DEFAULT_BATCH_ITEMS)
    perm = pr.device_perm(recs)[0]
    for a in (63, 255):  # the pairs that differ in the pattern code only have changed places
        first = sum(n + k % 3 for k, n in enumerate(SORT_SIZES[:SORT_SIZES.index(600)]))
        assert perm.index(first + a + 1) + 1 == perm.index(first + a)


def test_the_comparison_is_signed():
    big = 2 ** 31 - 2
    g = [rec("s", R1F, 0, big, 5), rec("s", R2R, 0, 3, -1), rec("s", R1F, 0, 5, big), rec("s", R2R, 0, -1, big), rec("s", R1R, -1, 0, 0), rec("s", R2F, 0, big, big),
         rec("s", R1F, 1, -1, -1), rec("s", R2R, 0, 0, 0)]
    got, _ = check(g + singles(3))
    assert got.code == pr.OK
    assert pr.device_perm(g)[0] == [4, 1, 3, 7, 0, 2, 5, 6]  # tid -1 first; then min(pos, mpos) = -1 twice (max 3, then 2^31 - 2), 0, 5 (a tie), 2^31 - 2; tid 1 last


# ---- partial records -----------------------------------------------------------------------------------------------------------------

def partial_group(name, n1, n2, nu, n_both=0):
    """the classes interleaved (three records of one, then of the next, ...), every record with a place of its own"""
    lists = [[rec(name, P1 if k % 2 else U1, 0, 10 + k) for k in range(n1)], [rec(name, P2 if k % 3 else U2, 1, 20 + k) for k in range(n2)],
             [rec(name, PU | (4 if k % 2 else 0), 2, 30 + k) for k in range(nu)],
             [rec(name, R1F if k % 2 == 0 else R2R, 0, 5000 - k // 2, 6000) for k in range(n_both)]]
    out = []
    while any(lists):
        for l in lists:
            out += l[:3]
            del l[:3]
    return out


def shape(size, diff, swap):
    """(n1, n2, nu) of `size` records with n1 - n2 = diff (n2 - n1 where swap)"""
    nu = diff + 2 * (size // 16)  # at least as many unknown records as are left over, and an even rest for the pairs (size is even)
    n2 = (size - nu - diff) // 2
    n1 = n2 + diff
    assert n1 + n2 + nu == size and n2 >= 0
    return (n2, n1, nu) if swap else (n1, n2, nu)


@pytest.mark.parametrize("diff", [0, 1, 21], ids=["equal", "one_left_over", "many_left_over"])
def test_partial_groups_at_the_seams(diff):
    """groups of 62 to 66 and 254 to 258 records: the even ones are put in order, the odd ones are what the reference stops at"""
    even, k = [], 0
    for size in (62, 64, 66, 254, 256, 258):
        for swap in (False, True):
            even += partial_group("e%d" % k, *shape(size, diff, swap), n_both=(k % 3) * 2) + singles(k % 2, "t%d_" + str(k))
            k += 1
    got, _ = check(even)
    assert got.code == pr.OK
    for size in (63, 65, 255, 257):
        n1, n2, nu = shape(size - 1, diff, False)
        recs = singles(5) + partial_group("o", n1, n2, nu + 1, n_both=4) + singles(2, "b%d")
        got, _ = check(recs)
        assert (got.code, got.group, got.group_record) == (pr.ODD_PARTIAL, 5, 5)


# ---- group starts --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["hard", "soft_after_unpaired", "soft_after_paired", "soft_after_unpaired_soft"])
def test_group_starts_on_every_seam(kind):
    al = [(0, 50, 90), (0, 10, 40)]
    for at in SEAMS + [N - 4]:
        recs = singles(N)
        if kind == "hard":
            recs[at:at + 4] = firsts_then_seconds("x", al)
        elif kind == "soft_after_unpaired" and at >= 1:
            recs[at - 1:at + 4] = [rec("x", 0, 0, 1)] + firsts_then_seconds("x s", al)  # the record on the seam opens a paired group
        elif kind == "soft_after_paired" and at >= 1:
            recs[at - 1:at + 4] = [rec("x", R1F, 0, 70, 95)] + firsts_then_seconds("x s", al) + [rec("x", R2R, 0, 95, 70)]  # it does not: one group of six
        elif kind == "soft_after_unpaired_soft" and at >= 2:
            recs[at - 2:at + 4] = [rec("x", 0, 0, 1), rec("x a", 0, 0, 2)] + firsts_then_seconds("x s", al)
        else:
            continue
        got, calls = check(recs)
        assert got.code == pr.OK and calls[0]["n_sorted_groups"] == 1
        assert pr.device_perm(recs)[0] != list(range(len(recs)))


# ---- verdicts ------------------------------------------------------------------------------------------------------------------------

def failing_group(code, name):
    if code == pr.MIXED:
        return [rec(name, R1F, 0, 1, 20), rec(name, 0, 0, 5), rec(name, R2R, 0, 20, 1)]
    if code == pr.ODD_FULL:
        return proper(name, 0, 1, 20) + [rec(name, R1F, 0, 3, 30), rec(name, U1, -1, -1)]
    if code == pr.ODD_PARTIAL:
        return proper(name, 0, 1, 20) + [rec(name, U1, -1, -1), rec(name, U2, -1, -1), rec(name, PU, 0, 4)]
    return proper(name, 0, 1, 20) + [rec(name, P1, 0, 4), rec(name, U1, -1, -1)]  # two first mates, nothing to put behind the second


@pytest.mark.parametrize("code", [pr.MIXED, pr.ODD_FULL, pr.ODD_PARTIAL, pr.NO_PARTNER])
def test_every_code_alone(code):
    for at in (0, 63, 300):
        recs = singles(at) + failing_group(code, "bad") + singles(7, "t%d")
        got, _ = check(recs)
        assert (got.code, got.group, got.group_record) == (code, at, at)
    mixed_and_odd = singles(3) + [rec("m", R1F, 0, 1, 20), rec("m", U1, -1, -1), rec("m x", 0, 0, 5)]  # the reference meets the mixed record first
    assert check(mixed_and_odd)[0].code == pr.MIXED


@pytest.mark.parametrize("where", ["one_launch", "batches_of_100", "batches_of_1", "calls"])
def test_the_smaller_of_two_failing_groups_wins(monkeypatch, where):
    """two failing groups on lanes of different waves, workgroups, batches and calls: the verdict is the first one's"""
    if where.startswith("batches"):
        monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", where.split("_")[-1])
    places = SEAMS + [N - 1]
    codes = [pr.MIXED, pr.ODD_FULL, pr.ODD_PARTIAL, pr.NO_PARTNER]
    for i, (a, b) in enumerate(zip(places, places[1:])):
        first, second = failing_group(codes[(i + 1) % 4], "bad_a"), failing_group(codes[i % 4], "bad_b")  # (the later one often has the smaller code)
        recs = singles(a) + first + singles(b - a - 1, "m%d") + second + singles(5, "t%d")
        cuts = [a + len(first)] if where == "calls" else []
        got, calls = check(recs, cuts)
        assert (got.code, got.group, got.group_record) == (codes[(i + 1) % 4], a, a)
        if where == "batches_of_100":
            assert calls[0]["n_batches"] == a // 100 + 1  # nothing is run behind the batch that fails
        if where == "calls":
            assert len(calls) == 1 if a == 0 else True


# ---- the handle ----------------------------------------------------------------------------------------------------------------------

def test_the_handle_keeps_its_buffers():
    from rsem_amd import capi
    ps = capi.Pairscan()
    streams = [singles(10) + sort_group("a", 18), singles(100) + sort_group("b", 66) + partial_group("c", 3, 1, 2), singles(700) + sort_group("d", 258) + partial_group("e", 5, 5, 0)]
    held = []
    for recs in streams:
        _, calls = check(recs, handle=ps)
        held.append(calls[0]["device_bytes"])
    assert held[0] > 0 and held == sorted(held) and held[2] > held[0]
    _, calls = check(streams[0], handle=ps)  # a small call after the large ones: nothing shrinks, nothing changes
    assert calls[0]["device_bytes"] == held[2]
    ps.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_a_file_with_separated_mates_becomes_valid(tmp_path):
    """a valid paired-end file, each read's first mates before its second mates: rsem-sam-validator refuses it, takes what this program
    makes of it"""
    targets = [("t1", 1000), ("t2", 2000), ("t3", 500)]
    raw = []
    for k in range(400):
        pairs = [ar.pair("read%d" % k, (k + a) % 3, 5 + 11 * a, 200 + 7 * a, 10, 12, rev=bool((k + a) % 2)) for a in range(1 + k % 5)]
        mates = []
        for m1, m2 in pairs:
            b1, b2 = bytearray(ar.record_bytes(m1)), bytearray(ar.record_bytes(m2))
            struct.pack_into("<i", b1, 24, m2.pos)
            struct.pack_into("<i", b2, 24, m1.pos)
            mates.append((bytes(b1), bytes(b2)))
        raw += [m[0] for m in mates] + [m[1] for m in mates]
    d = str(tmp_path)
    pr.write_bam(os.path.join(d, "in.bam"), None, 60000, "".join("@SQ\tSN:%s\tLN:%d\n" % t for t in targets), raw)
    r = subprocess.run([ar.VALIDATOR, "in.bam"], capture_output=True, cwd=d)
    assert r.returncode == 0 and r.stdout.endswith(b"The input file is not valid!\n")
    r = subprocess.run([PROGRAM, "4", "in.bam", "out.bam"], capture_output=True, cwd=d, env=dict(os.environ, RSEM_HIP_BAM_CHUNK="30000"))
    assert (r.returncode, r.stdout, r.stderr) == (0, b".\nFinished!\n", b"")
    out = gr.bgzf_inflate(open(os.path.join(d, "out.bam"), "rb").read())
    assert out == pr.scan(os.path.join(d, "in.bam"))[3] and sorted(gr.split_bam(out)[2]) == sorted(raw)
    r = subprocess.run([ar.VALIDATOR, "out.bam"], capture_output=True, cwd=d)
    assert r.returncode == 0 and r.stdout.endswith(b"\nThe input file is valid!\n"), r.stdout
