"""rsem_pairscan_reorder on the GPU where its value domain ends (inputs: tests/pairscan_limits.py), through the check() of
tests/test_pairscan_gpu.py: the permutation, the verdict and the number of groups equal the restatement's (tests/pairscan_ref.py).

  every flag byte    class_of, the pattern code and "paired is the group's first record" read bits 0x1, 0x2, 0x4, 0x10, 0x40, 0x80: all
                     256 values of the low byte, with 0x100 and 0x800 set and clear, behind a paired and an unpaired first record
  group sizes        whole tiles of 256 (512, 1024), 16 tiles (4096), a group of equal keys, a descending one; partial groups of 1022 .. 1026
  32 bits            tid, pos and mpos at -2^31, -1, 0, 1 and 2^31 - 1
  names              kMaxName bytes, canonical length 0, a proper prefix for a neighbour, a NUL inside; on the lanes 0, 63 | 64, 255 | 256
                     and at batch edges
  list shapes        1, 4 and 5 wave-sized groups, workgroup-sized ones alone, nothing to sort"""
import pytest

import pairscan_limits as pl
import pairscan_ref as pr
from test_pairscan_gpu import check, partial_group, shape

pytestmark = pytest.mark.gpu


# ---- every flag byte -------------------------------------------------------------------------------------------------------------------

_split = []


def split():
    if not _split:
        _split.append(pl.split_flag_groups())
    return _split[0]


def test_every_flag_byte_in_groups_that_come_out_in_order():
    ok, failing = split()
    paired = [g for g in ok if g[0].flag & 1]
    assert {pr.class_of(r.flag) for g in paired for r in g[1:]} == {0, 1, 2, 3}
    both = [r for g in paired for r in g if pr.class_of(r.flag) == 0]
    assert {(bool(r.flag & 0x40), pr.key(r)[3]) for r in both} == {(True, 0), (True, 1), (False, 0), (False, 1)}  # both pattern codes, first and second mates
    assert {r.flag & 0xff for g in ok for r in g[1:]} == set(range(256)) and {r.flag & 0x900 for g in ok for r in g[1:]} == set(pl.HIGH_BITS)
    assert any(r.flag & 0xc0 == 0xc0 and pr.class_of(r.flag) == 1 for g in paired for r in g) and any(r.flag & 0xc6 == 0x02 for r in both)
    assert any(r.flag & 0x06 == 0x06 and pr.class_of(r.flag) != 0 for g in paired for r in g)  # unmapped and "proper": not a full alignment
    recs, starts = pl.on_the_seams(ok)
    assert {s % 256 for s in starts} >= {0, 63, 64, 255} and 256 in starts
    got, calls = check(recs)
    assert got.code == pr.OK and calls[0]["n_sorted_groups"] == sum(sum(pr.class_of(r.flag) == 0 for r in g) >= 2 for g in paired)


def test_every_code_among_the_flag_groups_that_fail():
    ok, failing = split()
    codes = [pr.reorder(g)[1].code for g in failing]
    assert set(codes) == set(pl.FAIL_CODES) and len(failing) <= 64
    filler = sum(ok[:90], [])
    n_before = len(pr.walk(filler))
    assert 200 <= len(filler) <= 400
    for g, code in zip(failing, codes):
        got, _ = check(filler + g + pl.singles(3, "t%d"))
        assert (got.code, got.group, got.group_record) == (code, n_before, len(filler))


# ---- group sizes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget", [None, 300])
def test_groups_of_whole_tiles_and_of_sixteen(monkeypatch, budget):
    if budget:
        monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", str(budget))
    else:
        monkeypatch.delenv("RSEM_PAIRSCAN_BATCH_ITEMS", raising=False)
    recs, where = pl.big_stream()
    assert [n for _, n in where] == [510, 512, 514, 1024, 4096, 1024, 1024]
    want = pr.reorder(recs)[0]
    first, n = where[4]
    for a in pl.TILE_EDGES:  # the pairs that differ in the pattern code only change places
        assert want.index(first + a + 1) + 1 == want.index(first + a)
    first, n = where[5]
    assert want[first:first + n] == list(range(first, first + n))      # equal keys: the stable order is the file's
    first, n = where[6]
    assert want[first:first + n] == list(range(first + n - 1, first - 1, -1))
    got, calls = check(recs)
    assert got.code == pr.OK and calls[0]["n_sorted_groups"] == len(where)
    assert calls[0]["n_batches"] == pr.expected_batches(recs, budget or pr.DEFAULT_BATCH_ITEMS)
    perm = pr.device_perm(recs)[0]
    first, n = where[5]
    assert perm[first:first + n] == list(range(first, first + n))


@pytest.mark.parametrize("diff", [0, 1, 21], ids=["equal", "one_left_over", "many_left_over"])
def test_partial_groups_of_four_tiles(diff):
    even, k = [], 0
    for size in (1022, 1024, 1026):
        for swap in (False, True):
            even += partial_group("e%d" % k, *shape(size, diff, swap), n_both=(k % 3) * 2) + pl.singles(k % 2, "t%d_" + str(k))
            k += 1
    assert max(b - a for a, b, _, _ in pr.walk(even)) == 1026 + 4
    got, _ = check(even)
    assert got.code == pr.OK
    for size in (1023, 1025):
        n1, n2, nu = shape(size - 1, diff, False)
        recs = pl.singles(5) + partial_group("o", n1, n2, nu + 1, n_both=4) + pl.singles(2, "b%d")
        got, _ = check(recs)
        assert (got.code, got.group, got.group_record) == (pr.ODD_PARTIAL, 5, 5)


# ---- keys at the ends of 32 bits ---------------------------------------------------------------------------------------------------------

def test_keys_at_the_ends_of_32_bits():
    lo, hi = -2 ** 31, 2 ** 31 - 1
    sub = pl.end_keys_subset()
    # tid -2^31 first; tid 0 by (min, max): (-2^31, -2^31), (-2^31, 2^31 - 1) twice in file order, (-1, 1), (-1, 2^31 - 1), (2^31 - 1, 2^31 - 1); tid 2^31 - 1 last
    assert pr.reorder(sub)[0] == [3, 4, 0, 6, 5, 1, 7, 2]
    assert [pr.key(sub[i])[:3] for i in (3, 4, 0, 2)] == [(lo, hi, hi), (0, lo, lo), (0, lo, hi), (hi, lo, lo)]
    got, _ = check(sub + pl.singles(3))
    assert got.code == pr.OK and pr.device_perm(sub)[0] == [3, 4, 0, 6, 5, 1, 7, 2]
    g = pl.end_keys_group()
    assert len(g) == 50 and {(r.pos, r.mpos) for r in g} == {(a, b) for a in pl.ENDS for b in pl.ENDS} and {r.tid for r in g} == {lo, hi}
    want = pr.reorder(g)[0]
    assert want[0] == 49 and want != list(range(50))  # (tid, pos, mpos) = (-2^31, -2^31, -2^31) is the file's last record
    got, calls = check(pl.singles(60) + g + pl.singles(3, "t%d"))
    assert got.code == pr.OK and calls[0]["n_sorted_groups"] == 1


# ---- names -----------------------------------------------------------------------------------------------------------------------------

KINDS = sorted(pl.name_blocks())


def test_the_name_blocks_reach_their_limits():
    b = pl.name_blocks()
    assert {len(r.name) for r in b["last_byte"]} == {pl.MAX_NAME} and len({r.name[:-1] for r in b["last_byte"]}) == 1
    assert {len(r.name) for r in b["behind_the_space"]} == {pl.MAX_NAME} and {len(pr.canonical(r.name)) for r in b["behind_the_space"]} == {pl.MAX_NAME - 2}
    assert any(y.name.startswith(x.name) and len(y.name) > len(x.name) for x, y in zip(b["prefix"], b["prefix"][1:]))
    zero = [len(pr.canonical(r.name)) == 0 for r in b["no_canonical_name"]]
    assert any(p and q for p, q in zip(zero, zero[1:])) and any(p != q and 1 in (len(x.name), len(y.name)) for p, q, x, y in zip(zero, zero[1:], b["no_canonical_name"], b["no_canonical_name"][1:]))
    assert any(0 in r.name for r in b["nul"]) and [(e - a) for a, e, _, _ in pr.walk(b["nul"])] == [4, 3, 2, 2]
    for kind in KINDS:
        assert pr.reorder(b[kind])[1].code == pr.OK and pr.soft_rule_starts(b[kind]) == [a for a, _, _, _ in pr.walk(b[kind])]


@pytest.mark.parametrize("at", [0, 63, 255])
@pytest.mark.parametrize("kind", KINDS)
def test_names_on_the_seams(monkeypatch, kind, at):
    monkeypatch.delenv("RSEM_PAIRSCAN_BATCH_ITEMS", raising=False)
    recs = pl.name_stream(kind, at)
    got, calls = check(recs)
    assert got.code == pr.OK and calls[0]["n_groups"] == len(pr.walk(recs))
    assert pr.device_perm(recs)[0] != list(range(len(recs)))


@pytest.mark.parametrize("budget", [1, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_names_at_batch_edges(monkeypatch, kind, budget):
    monkeypatch.setenv("RSEM_PAIRSCAN_BATCH_ITEMS", str(budget))
    for at in (0, 3, 6):  # the block's runs against batches of 7 in three phases
        recs = pl.name_stream(kind, at)
        got, calls = check(recs)
        assert got.code == pr.OK
        assert calls[0]["n_groups"] == len(pr.walk(recs)) and calls[0]["n_batches"] == pr.expected_batches(recs, budget)


# ---- list shapes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_small,n_large", [(1, 0), (4, 0), (5, 0), (0, 3), (0, 0), (5, 2)])
def test_lists_of_groups_to_sort(monkeypatch, n_small, n_large):
    monkeypatch.delenv("RSEM_PAIRSCAN_BATCH_ITEMS", raising=False)
    recs = pl.list_stream(n_small, n_large)
    if not n_small + n_large:
        recs += [pr.rec("p", pr.P1, 0, 4), pr.rec("p", pr.P2, 0, 9), pr.rec("q", pr.P1, 0, 4), pr.rec("q", pr.PU, 0, 5), pr.rec("q", pr.P2, 0, 9), pr.rec("q", pr.PU, 0, 7)] + pl.singles(300, "z%d")
    sizes = [sum(pr.class_of(r.flag) == 0 for r in recs[a:b]) for a, b, paired, _ in pr.walk(recs) if paired]
    assert sum(2 <= s <= 64 for s in sizes) == n_small and sum(s > 64 for s in sizes) == n_large
    got, calls = check(recs)
    assert got.code == pr.OK and calls[0]["n_sorted_groups"] == n_small + n_large and calls[0]["n_batches"] == 1
