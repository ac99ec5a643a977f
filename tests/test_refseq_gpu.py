"""rsem_refseq_load / rsem_refseq_gather and the three reference-preparation programs on the GPU: the kernels at their seams against
the plain restatement (tests/refseq_ref.py), the programs against the fixtures the unmodified reference programs left
(tests/golden/refprep/) and, live, against the reference programs in oracle/_ref/ on a seeded genome.  Equality of bytes throughout."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refseq_ref as rr
from refseq_ref import BIN, PROGRAMS, ROOT

pytestmark = pytest.mark.gpu

T, C, W, WAVE_SPAN = 4096, 1024, 16384, 4096  # kTile, kChunk, kGroupSpan, kSpan of rsem_amd/csrc/refseq_block.hpp
ALPHABET = b"ACGTacgtNnRyXk"


@pytest.fixture(scope="module")
def capi():
    from rsem_amd import capi as c
    if c.device_count() < 1:
        pytest.skip("needs a GPU")
    return c


def letters(rng, n):
    return bytes(rng.choice(ALPHABET) for _ in range(n))


def lines(rng, raw_len, width):
    """raw_len bytes: lines of `width` letters."""
    out = bytearray()
    col = 0
    while len(out) < raw_len:
        if col == width:
            out.append(10)
            col = 0
        else:
            out.append(rng.choice(ALPHABET))
            col += 1
    return bytes(out)


def load_file():
    """One file whose records put every load seam somewhere: (bytes, body_lo, body_hi).  The first body starts at byte 3, so with
    all records in one batch the tiles are those of the file."""
    rng = random.Random(3)
    f = bytearray()
    lo, hi = [], []

    def record(name, body):
        f.extend(b">" + name + b"\n")
        lo.append(len(f))
        f.extend(body)
        hi.append(len(f))
        f.extend(b"\n")

    for n in (1, 15, 16, 17, C - 1, C, C + 1, T - 1, T, T + 1, 2 * T + 3):
        record(b"len%d" % n, lines(rng, n, 60))
        record(b"w1_%d" % n, lines(rng, min(n, 300), 1))
    # a line end as the last and as the first byte of a tile; empty lines over a tile's edge
    while (len(f) + 4) % T > T - 200:
        record(b"fill", b"ACGT")
    f.extend(b">edge\n")
    lo.append(len(f))
    to_edge = T - len(f) % T
    f.extend(letters(rng, to_edge - 1) + b"\n" + letters(rng, 50) + b"\n")                 # '\n' last in a tile
    f.extend(letters(rng, T - 51) + b"\n" + letters(rng, 30) + b"\n")                       # '\n' first in the next but one
    f.extend(letters(rng, T - 31 - 10) + b"\n" * 20 + letters(rng, 40))                      # empty lines over an edge
    hi.append(len(f))
    f.extend(b"\n")
    record(b"a", b"AC")          # two records whose header sits inside one 16-byte chunk
    record(b"b", b"G")
    record(b"c", b"T")
    record(b"last", lines(rng, 100, 60).rstrip(b"\n"))
    del f[-1]                    # no final line end
    return bytes(f), lo, hi


def batches_of(lo, hi, budget):
    n, first = 0, 0
    while first < len(lo):
        r = first
        while r < len(lo) and (r == first or hi[r] - lo[first] <= budget):
            r += 1
        first = r
        n += 1
    return n


@pytest.fixture(scope="module")
def loadcase():
    raw, lo, hi = load_file()
    return raw, lo, hi, rr.load_ref(raw, lo, hi, True), rr.load_ref(raw, lo, hi, False)


def run_load(capi, raw, lo, hi, mode, monkeypatch, budget):
    """Every record loaded and copied out again: (n_bases, bad, the records' bases, n_batches)."""
    if budget is None:
        monkeypatch.delenv("RSEM_REFSEQ_BATCH_BYTES", raising=False)
    else:
        monkeypatch.setenv("RSEM_REFSEQ_BATCH_BYTES", str(budget))
    place = np.concatenate([[0], np.cumsum([(b - a + 15) & ~15 for a, b in zip(lo, hi)])])
    h = capi.Refseq(int(place[-1]))
    n = len(lo)
    first, n_bases, bad = 0, np.zeros(n, np.uint64), np.zeros(n, np.int64)
    while first < n:
        taken, nb, bd = h.load(mode, raw, lo, hi, None, first)
        assert taken >= 1
        sl = slice(first, first + taken)
        n_bases[sl], bad[sl] = nb[sl], bd[sl]
        idx = [r for r in range(first, first + taken) if nb[r] > 0]
        h.gather(idx, [0] * len(idx), [int(nb[r]) for r in idx], [int(place[r]) for r in idx], [0] * len(idx))
        first += taken
    store = h.download()
    info = h.info()
    h.close()
    return n_bases, bad, [store[int(place[r]):int(place[r]) + int(n_bases[r])] for r in range(n)], info["n_batches"]


@pytest.mark.parametrize("budget", [None, "smallest", 1])
@pytest.mark.parametrize("mode", [1, 0])
def test_load_at_its_seams(capi, loadcase, mode, budget, monkeypatch):
    raw, lo, hi, checked, plain = loadcase
    want = checked if mode else plain
    b = min(y - x for x, y in zip(lo, hi)) if budget == "smallest" else budget
    n_bases, bad, seqs, n_batches = run_load(capi, raw, lo, hi, mode, monkeypatch, b)
    assert n_bases.tolist() == [len(s) for s, _ in want]
    assert bad.tolist() == [-1] * len(lo)
    for r, (s, _) in enumerate(want):
        assert seqs[r] == s, r
    assert n_batches == (1 if b is None else batches_of(lo, hi, b))
    assert n_batches == (1 if b is None else len(lo))  # (no two bodies and the header between them fit the smallest body)


@pytest.mark.parametrize("budget", [None, "smallest", 1])
def test_load_reports_each_records_first_bad_byte(capi, budget, monkeypatch):
    rng = random.Random(9)
    body = bytearray(letters(rng, 3 * T))
    f = bytearray(b">a*\n") + body + b"\n>b *-\nACGT\n>c\n" + letters(rng, 2 * T) + b"\n"
    raw0 = bytes(f)
    lo = [4, 4 + 3 * T + 7, 4 + 3 * T + 7 + 5 + 3]
    hi = [4 + 3 * T, lo[1] + 4, lo[2] + 2 * T]
    assert raw0[lo[1]:hi[1]] == b"ACGT" and raw0[lo[2] - 3:lo[2]] == b">c\n"
    b = min(y - x for x, y in zip(lo, hi)) if budget == "smallest" else budget
    for places in ([], [T - 1], [T], [2 * T + 5, T + 9], [lo[2] + T, lo[2] + 3, 2 * T - 1]):  # last / first byte of a tile; two tiles of one record
        f2 = bytearray(raw0)
        for k, p in enumerate(places):
            f2[p] = b"*-\r\xc3 "[k]
        raw = bytes(f2)
        want = rr.load_ref(raw, lo, hi, True)
        n_bases, bad, _, n_batches = run_load(capi, raw, lo, hi, 1, monkeypatch, b)
        assert bad.tolist() == [x for _, x in want], places   # a bad byte in a header: none is reported
        assert n_bases.tolist() == [len(s) for s, _ in want]
        assert n_batches == (1 if b is None else batches_of(lo, hi, b)) == (1 if b is None else 3)
        n_bases, bad, seqs, _ = run_load(capi, raw, lo, hi, 0, monkeypatch, b)  # raw mode: the bytes stay, nothing is reported
        assert bad.tolist() == [-1, -1, -1]
        assert seqs == [s for s, _ in rr.load_ref(raw, lo, hi, False)]


def test_records_that_are_not_kept_are_checked(capi, monkeypatch):
    monkeypatch.delenv("RSEM_REFSEQ_BATCH_BYTES", raising=False)
    raw = b">a\nACGT\n>b\nAC*T\nGG\n>c\nTTTT\n"
    lo, hi = [3, 11, 22], [7, 18, 26]
    h = capi.Refseq(64)
    taken, nb, bad = h.load(1, raw, lo, hi, [1, 0, 1])
    assert taken == 3 and nb.tolist() == [4, 0, 4] and bad.tolist() == [-1, 13, -1]
    h.gather([0, 2], [0, 0], [4, 4], [0, 16], [0, 1])
    assert h.download(0, 4) == b"ACGT" and h.download(16, 4) == b"AAAA"
    h.close()


# ---- gather ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chromosomes():
    rng = random.Random(21)
    seqs = [letters(rng, 3 * W + 500), letters(rng, 700), letters(rng, 3100)]
    raw, lo, hi = bytearray(), [], []
    for k, s in enumerate(seqs):
        raw.extend(b">chr%d\n" % k)
        lo.append(len(raw))
        raw.extend(b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)))
        hi.append(len(raw))
        raw.extend(b"\n")
    bases = [s for s, _ in rr.load_ref(bytes(raw), lo, hi, True)]
    return bytes(raw), lo, hi, bases


def gather_segments():
    """(record, first base, length, destination, flags), ascending in the store."""
    segs, d = [], 5
    for flags in (0, rr.RC, rr.UPPER_N, rr.UPPER_N | rr.N2G, rr.RC | rr.UPPER_N | rr.N2G):
        for sm in range(16):                       # every source misalignment against every destination misalignment
            for dm in range(16):
                for n in (1, 15, 16, 17, 40):
                    d = ((d + 15) & ~15) + dm
                    segs.append((0, 32 + sm, n, d, flags))
                    d += n
    for strand in (0, rr.RC):                      # 300 exons of 10 bases on both strands
        order = range(300) if not strand else range(299, -1, -1)
        for k in order:
            segs.append((2, 10 * k + 3, 10, d, strand))
            d += 10
    d += 7
    shared = (1, 100, 333)                          # two transcripts that share an exon; mixed case with n and N on '-'
    for _ in range(2):
        segs.append(shared + (d, rr.RC))
        d += 333
        segs.append((1, 500, 50, d, rr.RC))
        d += 50
    for flags in (rr.RC, rr.UPPER_N, rr.N2G | rr.UPPER_N, rr.FILL):  # the four flags, each alone
        segs.append((1, 11, 97, d + 3, flags))
        d += 100
    segs.append((1, 0, 700, d, rr.UPPER_N))        # fill after a copy: an entry and its tail
    segs.append((0, 0, 125, d + 700, rr.FILL))
    return segs, d + 825 + 64


def seam_segments():
    """Segments whose ends fall on W - 1, W, W + 1 (and on a wave's span) of the cumulative length."""
    out = []
    for end in (WAVE_SPAN - 1, WAVE_SPAN, WAVE_SPAN + 1, W - 1, W, W + 1):
        for flags in (0, rr.RC):
            out.append(([(0, 7, end - 9, 3, flags), (0, 1, 9, end + 3, 0), (0, 50, 2 * W + 100, end + 40, flags), (0, 0, 5, end + 2 * W + 200, rr.FILL)],
                        end + 2 * W + 300))
    return out


def run_gather(capi, chromosomes, segs, size, monkeypatch, budget, pad=None):
    """The store is first filled with 'A' from end to end (one fill segment), then the segments are gathered over it: the whole
    store is compared, so a byte written outside every segment shows.  Returns (store, info, what the store must hold)."""
    raw, lo, hi, bases = chromosomes
    for k, v in (("RSEM_REFSEQ_BATCH_BYTES", budget), ("RSEM_REFSEQ_STORE_PAD", pad)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    h = capi.Refseq(size)
    h.gather([0], [0], [size], [0], [rr.FILL])
    h.run(1, raw, lo, hi, segs)
    got, info = h.download(), h.info()
    h.close()
    return got, info, bytes(rr.gather_ref(bytearray(b"A" * size), bases, segs))


def budget_of(budget, lo, hi):
    return min(y - x for x, y in zip(lo, hi)) if budget == "smallest" else budget


BUDGETS = [None, "smallest", 1]


@pytest.mark.parametrize("budget", BUDGETS)
def test_gather_at_its_seams(capi, chromosomes, budget, monkeypatch):
    raw, lo, hi, bases = chromosomes
    b = budget_of(budget, lo, hi)
    for sg, sz in [gather_segments()] + seam_segments():
        got, info, want = run_gather(capi, chromosomes, sg, sz, monkeypatch, b)
        assert got == want
        assert info["n_batches"] == (1 if b is None else batches_of(lo, hi, b)) == (1 if b is None else 3)
        assert info["gathered_bytes"] == sz + sum(s[2] for s in sg)


@pytest.mark.parametrize("budget", BUDGETS)
def test_a_transcript_astride_two_to_the_32(capi, chromosomes, budget, monkeypatch):
    """RSEM_REFSEQ_STORE_PAD = 2^32 - 64: the store's byte 64 is the device allocation's byte 2^32."""
    raw, lo, hi, bases = chromosomes
    b = budget_of(budget, lo, hi)
    segs = [(1, 5, 40, 3, 0), (1, 200, 90, 43, rr.RC), (1, 0, 60, 133, rr.UPPER_N | rr.N2G), (0, 0, 30, 193, rr.FILL)]
    got, info, want = run_gather(capi, chromosomes, segs, 256, monkeypatch, b, pad=(1 << 32) - 64)
    assert got == want
    assert info["store_pad"] == (1 << 32) - 64
    assert info["n_batches"] == (1 if b is None else 3)


def test_refusals_come_back_as_errors(capi, chromosomes, monkeypatch):
    """Checked before any launch: knob values, segments outside their record or the store, destinations that overlap, an over-long record."""
    raw, lo, hi, bases = chromosomes
    monkeypatch.delenv("RSEM_REFSEQ_STORE_PAD", raising=False)
    h = capi.Refseq(1000)
    for bad in ("0", "-1", "1.5", "x", ""):
        monkeypatch.setenv("RSEM_REFSEQ_BATCH_BYTES", bad)
        with pytest.raises(capi.RsemHipError) as e:
            h.load(1, raw, lo, hi)
        assert e.value.status == -1 and "RSEM_REFSEQ_BATCH_BYTES" in str(e.value)
    monkeypatch.delenv("RSEM_REFSEQ_BATCH_BYTES")
    with pytest.raises(capi.RsemHipError) as e:
        h.gather([0], [0], [4], [0], [0])  # nothing is loaded
    assert e.value.status == -1
    h.load(1, raw, lo, hi)
    for seg in ([1], [690], [20], [0], [0]), ([1], [0], [20], [990], [0]), ([3], [0], [20], [0], [0]), ([1, 1], [0, 0], [20, 20], [0, 19], [0, 0]), ([1], [0], [0], [0], [0]), \
            ([1], [0], [4], [0], [16]):
        with pytest.raises(capi.RsemHipError) as e:
            h.gather(*seg)
        assert e.value.status == -1, seg
    with pytest.raises(capi.RsemHipError) as e:  # a body of 2^31 bytes without a line end: refused before anything is uploaded
        big = np.zeros((1 << 31) + 8, np.uint8)
        h.load(1, big, [4], [4 + (1 << 31)])
    assert e.value.status == -1 and "2^31 - 1" in str(e.value)
    h.close()


# ---- the programs -------------------------------------------------------------------------------------------------------------

def run_in(cwd, argv, env=None):
    e = dict(os.environ)
    e.pop("RSEM_REFSEQ_BATCH_BYTES", None)
    e.pop("RSEM_REFSEQ_STORE_PAD", None)
    e.update(env or {})
    return subprocess.run(argv, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("name", rr.case_names())
def test_programs_reproduce_the_recorded_fixtures(capi, name, tmp_path):
    c = rr.load_case(name)
    for k, env in enumerate((None, {"RSEM_REFSEQ_BATCH_BYTES": "1"})):
        d = tmp_path / str(k)
        d.mkdir()
        rr.stage_case(c, str(d))
        r = run_in(str(d), [os.path.join(BIN, PROGRAMS[c["program"]])] + c["args"], env)
        assert r.returncode == c["status"], r.stderr[-2000:]
        for line in c["stderr"].split(b"\n"):
            assert line in r.stderr, line
        got = sorted(fn for fn in os.listdir(str(d)) if fn.startswith("ref."))
        assert got == sorted(c["files"])
        for fn in got:
            assert (d / fn).read_bytes() == c["files"][fn], fn


def test_quiet_silences_stdout(capi, tmp_path):
    for name, quiet in (("basic", False), ("basic_quiet_nonl", True), ("pre_choice0", False), ("pre_choice1", True)):
        c = rr.load_case(name)
        d = tmp_path / name
        d.mkdir()
        rr.stage_case(c, str(d))
        r = run_in(str(d), [os.path.join(BIN, PROGRAMS[c["program"]])] + c["args"])
        assert (r.stdout == b"") == quiet


def test_programs_against_the_reference_programs_live(capi, tmp_path):
    """A seeded genome of three chromosomes of about 40 kbases and 200 transcripts on both strands, some on an absent chromosome:
    the three programs and the reference's, one after the other, every output file equal."""
    ref_bin = os.path.join(ROOT, "oracle", "_ref")
    if not all(os.path.exists(os.path.join(ref_bin, p)) for p in PROGRAMS.values()):
        pytest.skip("reference binaries not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_genome
    gen_genome.write(str(tmp_path), seed=4, n_chromosomes=3, chromosome_bases=40000, n_transcripts=200, absent_fraction=0.05)
    for side, bindir in (("ref", ref_bin), ("new", BIN)):
        d = tmp_path / side
        d.mkdir()
        r = run_in(str(d), [os.path.join(bindir, PROGRAMS["extract"]), "out", "1", "../genes.gtf", "None", "0", "../genome.fa"])
        assert r.returncode == 0, r.stderr[-2000:]
        r = run_in(str(d), [os.path.join(bindir, PROGRAMS["preref"]), "out.transcripts.fa", "0", "out", "-l", "125", "-q"])
        assert r.returncode == 0, r.stderr[-2000:]
        r = run_in(str(d), [os.path.join(bindir, PROGRAMS["synthesis"]), "syn", "1", "0", "out.transcripts.fa"])
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(str(tmp_path / "ref")))
    assert names == sorted(os.listdir(str(tmp_path / "new"))) and len(names) == 10
    for fn in names:
        assert (tmp_path / "ref" / fn).read_bytes() == (tmp_path / "new" / fn).read_bytes(), fn
    assert 150 <= int((tmp_path / "new" / "out.ti").read_bytes().split()[0]) < 200  # some of the 200 lie on a chromosome that is absent
