"""EM on reads whose ids lie at and above the anchor cap of the sliced layout (rsem_amd/csrc/sell_layout.hpp: kKeyMinSidCap =
2^23 - 1; the input and what the cap does to it: tests/em_id_cap.py).  M = cap + 12000, some 2300 reads: anchors below the cap,
across it and above it, of the kinds of tests/test_em_units_gpu.py.

Every test asserts its path before it compares a number: the split rows the rule of row_key_of gives (reads whose anchor lies above
the cap stay whole), units with ids outside their window, one read left in the CSR, host and device unit tables that agree.  The
numbers are the oracle's (oracle/pyoracle.py) within the bars of tests/test_em_units_gpu.py.  MAX_ROUND = 30: an M step of the
oracle walks 8.4 M entries, 30 rounds take it two seconds; the runs end at that round, the oracle's and the device's alike."""
import numpy as np
import pytest

import em_id_cap as cap
from oracle import pyoracle as orc
from tools.q32_ref import quantize_q32

pytestmark = pytest.mark.gpu

MAX_ROUND = 30
_cache = {}


def capi():
    from rsem_amd import capi as c
    return c


def reads():
    if "d" not in _cache:
        _cache["d"] = cap.reads()
    return _cache["d"]


def oracle(bits):
    """(step counts incl. N0, weights, noise weights, theta, rounds, totNum): computed once per format, shared, never changed"""
    if bits not in _cache:
        d = reads()
        cp = d["conprb"] if bits == 64 else quantize_q32(d["row_ptr"], d["conprb"], 8)[0]
        oc, ow, own = orc.em_estep(d["M"], d["row_ptr"], d["sid"], cp, d["ncp"], d["theta0"], want_weights=True)
        oc = oc.copy()
        oc[0] += d["N0"]
        oth, orounds, _, ot = orc.em_run(d["M"], d["row_ptr"], d["sid"], cp, d["ncp"], d["N0"], d["theta0"], max_round=MAX_ROUND)
        _cache[bits] = (oc, ow, own, oth, orounds, ot)
    return _cache[bits]


def context(bits, policy):
    d = reads()
    ctx = capi().EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])
    if bits == 32:
        ctx.set_option("value_bits", 32)
    ctx.set_option("split_policy", policy)
    return ctx


def assert_path(ctx, bits, policy, tag):
    d = reads()
    N1 = len(d["row_ptr"]) - 1
    split, kept_by_cap = cap.expected_split_rows(d, policy)
    # (the layout takes split rows only where one read in twenty would split, sell_build; Q32 planes take whole reads, em.hip build_layout)
    assert 20 * split >= N1 and kept_by_cap > 0
    info = {k: ctx.info(k) for k in ("split_rows", "far_units", "unit_tables_agree", "reads_long", "reads_q32", "units")}
    print(tag, info)
    assert info["split_rows"] == (split if bits == 64 else 0), (tag, info, split)
    assert info["far_units"] >= 1 and info["unit_tables_agree"] == 1 and info["reads_long"] == 1, (tag, info)
    if bits == 32:
        assert info["reads_q32"] == N1 - 1, (tag, info)  # all but the read of 300 alignments


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("bits", [64, 32])
def test_step_and_weights(bits, policy):
    d = reads()
    assert d["anchor"].min() < cap.CAP - 8000 and (d["anchor"] == cap.CAP).any() and (d["anchor"] == cap.CAP + 1).any() and d["anchor"].max() > cap.CAP + 2 * cap.WINDOW
    ctx = context(bits, policy)
    tag = "value_bits=%d split_policy=%d" % (bits, policy)
    assert_path(ctx, bits, policy, tag)
    oc, ow, own, *_ = oracle(bits)
    N1 = len(d["row_ptr"]) - 1
    counts, theta_new, s, _, _ = ctx.step(d["theta0"], d["N0"])
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-9), tag
    assert abs(s - (d["N0"] + N1)) < 1e-6 and np.allclose(theta_new, oc / oc.sum(), rtol=1e-9, atol=1e-12), tag
    assert np.count_nonzero(counts[1:]) == np.count_nonzero(oc[1:])  # no count on an id that no read has
    c2, w, wn = ctx.expected_weights(d["theta0"], d["N0"])
    assert np.allclose(c2, oc, rtol=1e-9, atol=1e-9), tag
    if bits == 64:  # (the weights pass walks the caller's values)
        assert np.allclose(w, ow, rtol=1e-12, atol=0) and np.allclose(wn, own, rtol=1e-12, atol=0), tag
    assert ctx.info("unit_tables_agree") == 1
    ctx.close()


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("bits", [64, 32])
def test_every_loop(bits, policy, monkeypatch):
    d = reads()
    ctx = context(bits, policy)
    tag = "value_bits=%d split_policy=%d" % (bits, policy)
    assert_path(ctx, bits, policy, tag)
    _, _, _, oth, orounds, ot = oracle(bits)
    runs = {}
    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        out = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
        assert out["rounds"] == orounds and out["totNum"] == ot, (tag, loop, out["rounds"], orounds, out["totNum"], ot)
        assert np.allclose(out["theta"], oth, rtol=1e-9, atol=1e-12), (tag, loop)
        assert ctx.info("unit_tables_agree") == 1, (tag, loop)
        runs[loop] = out
    for loop in ("1", "2"):
        assert np.allclose(runs[loop]["theta"], runs["0"]["theta"], rtol=1e-10, atol=1e-18), (tag, loop)
    ctx.close()


def test_values_come_back_after_release_csr():
    """without the read of 300 alignments and with whole reads only (split rows and reads in the CSR keep the caller's arrays): the
    rounds stream the planes alone, the values are read back out of them bit for bit, above the cap as below"""
    d = cap.reads(with_long=False)
    ctx = capi().EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])
    ctx.set_option("split_rows", 0)
    assert ctx.info("split_rows") == 0 and ctx.info("reads_long") == 0 and ctx.info("far_units") >= 1 and ctx.info("unit_tables_agree") == 1
    ref = ctx.run(d["theta0"], d["N0"], max_round=25)
    ctx.set_option("release_csr", 1)
    assert ctx.info("csr_released") == 1
    again = ctx.run(d["theta0"], d["N0"], max_round=25)
    assert again["rounds"] == ref["rounds"] and np.allclose(again["theta"], ref["theta"], rtol=1e-12, atol=0)
    cp, ncp = ctx.get_values()
    assert ctx.info("csr_released") == 0
    assert np.array_equal(cp.view(np.uint64), d["conprb"].view(np.uint64)) and np.array_equal(ncp.view(np.uint64), d["ncp"].view(np.uint64))
    ctx.close()
