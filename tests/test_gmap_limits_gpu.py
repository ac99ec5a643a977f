"""Transcript -> genome coordinates and the collapse on the GPU at the limits rsem_amd/csrc/gmap_block.hpp names (inputs: tests/gmap_limits.py),
through the check() of tests/test_gmap_gpu.py: equality with the Python restatement (tests/gmap_ref.py) of every field, every CIGAR
word, the kept alignments, their order and their folded weights' bits.

  the exon cap      kMaxExons = 32766 keeps n_cigar <= 65533 inside the low 16 bits of rev_ncigar; compare_keys then walks 65532 words
  high positions    up to 2^31 - 2: bins above 37448 (no valid bin) and above 65535 (the 16 bits of a BAM record)
  one field         keys that differ in one field alone, at the wave, workgroup and tile seams
  a mixed launch    wave-sized groups in a partly filled block next to workgroup-sized ones"""
import numpy as np
import pytest

import gmap_limits as gl
import gmap_ref as gr
from test_gmap_gpu import bits, check

pytestmark = pytest.mark.gpu

INVALID = -1  # RSEM_ERR_INVALID
_cache = {}


def ref():
    """(ti, out_tid, handle): made once, shared, never changed"""
    if not _cache:
        from rsem_amd import capi
        flat = gl.flat()
        _cache["ref"] = (gl.transcripts()[0], flat[2], capi.Gmap(*flat))
    return _cache["ref"]


def test_a_transcript_of_32766_exons_whole():
    case = gl.cap_reads()
    want = gr.map_fields(ref()[0], ref()[1], *case[2:6])
    top = max(len(m[3]) for m in want)
    assert 65532 <= top <= 65533 and [len(m[3]) for m in want[:4]] == [65532, 65532, 65531, 65531]  # the path: asserted before the device runs
    o = check(*case, ref=ref())
    assert o["n_cigar"].max() == top and o["info"]["n_alignments_out"] == len(case[6])


@pytest.mark.parametrize("mates", [1, 2])
def test_a_group_whose_keys_differ_behind_65531_words(mates):
    case = gl.cap_group(mates)
    keys, mapped = gl.keys_of(case)
    assert len(set(keys)) == gl.CAP_GROUP_KEPT and keys[0] == keys[1] == keys[6] and max(len(m[3]) for m in mapped) == 65532
    a, b = mapped[mates - 1][3], mapped[3 * mates - 1][3]  # tail 5 and tail 6: the last word alone
    assert len(a) == len(b) == 65532 and a[:-1] == b[:-1] and a[-1] != b[-1]
    o = check(*case, ref=ref())
    assert o["info"]["n_alignments_out"] == gl.CAP_GROUP_KEPT
    w = case[6]
    assert int(bits([gr.fold32([w[0], w[1], w[6]])])[0]) in bits(o["out_w"]).tolist()  # 0, 1 and 6 folded in file order


def test_a_transcript_of_32767_exons_is_refused():
    from rsem_amd import capi
    n = gl.MAX_EXONS + 1
    st = [1 + 2 * k for k in range(n)]
    with pytest.raises(capi.RsemHipError) as e:
        capi.Gmap("+", [n], [0], [0, n], st, st)
    assert e.value.status == INVALID
    capi.Gmap("+", [n - 1], [0], [0, n - 1], st[:-1], st[:-1]).close()


def test_positions_up_to_the_last_one_and_their_bins():
    case = gl.high_reads()
    want = gr.map_fields(ref()[0], ref()[1], *case[2:6])
    bins, pos = [m[4] for m in want], [m[1] for m in want]
    assert max(pos) == 2 ** 31 - 2 and any(37448 < b <= 65535 for b in bins) and any(b > 65535 for b in bins)
    for e in gl.EDGES:  # a read that ends on the last base of a bin, one that starts on the first of the next
        assert any(p + sum(x >> 4 for x in m[3] if x & 15 in (0, 3)) == 2 ** e for p, m in zip(pos, want)) and 2 ** e in pos
    assert any(x >= 2 ** 31 for m in want for x in m[3])  # the intron of 2^28 bases or more, wrapped into its word
    o = check(*case, ref=ref())
    assert o["bin"].max() == max(bins) > 65535


@pytest.mark.parametrize("field", gl.FIELDS)
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 512, 513, 700])
def test_keys_that_differ_in_one_field_at_the_seams(n, field):
    case, m = gl.field_group(n, field)
    diffs = gl.first_differences(case, field)
    assert diffs == ({"pos", "strand"} if field == "strand" else {field})  # the precondition: no other field tells two keys apart
    o = check(*case, ref=ref())
    assert o["info"]["n_alignments_out"] == m == (n + 2) // 3


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("n_small", [1, 2, 3, 5])
def test_wave_sized_and_longer_groups_in_one_launch(monkeypatch, n_small, where):
    monkeypatch.delenv("RSEM_GMAP_BATCH_ITEMS", raising=False)
    case = gl.mixed_launch(n_small, where)
    sizes = np.diff(case[1]).tolist()
    assert sorted(s for s in sizes if s > gr.WAVE) == [65, 300] and sum(s <= gr.WAVE for s in sizes) == n_small
    o = check(*case, ref=ref())
    assert o["info"]["n_batches"] == 1 and o["info"]["n_groups"] == n_small + 2
    assert o["info"]["n_alignments_out"] == sum((s + 2) // 3 for s in sizes)
