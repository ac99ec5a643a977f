"""Option "sid_start_list" of the EM context (rsem_amd/csrc/sell_layout.hpp: the start list; estep_block.hpp issue()): in every slice
of a wave but its first, the lanes that start a tuple take its ids from a compact list -- K * popcount(mask) entries -- instead of
K planes of 64.  One step and 200 rounds with the option on against off IN THE SAME CONTEXT (no relayout: the kernels are handed
the list or a null pointer) and against the oracle at 1e-9, under the three loops, with blocks longer than the 64 slices whose masks
and offsets a wave holds at a time, with Q32 planes, with the CSR released, through the other entry points, and the byte accounting."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tools.synth_data import make_em_workload

pytestmark = pytest.mark.gpu

_CACHE = {}


def _wl(name):
    if name not in _CACHE:
        if name == "C3x0.06":
            wl = make_em_workload("C3", scale=0.06)
        else:
            wl = make_em_workload(name, seed=21)
        _CACHE[name] = wl
    return _CACHE[name]


def _oracle_step(name, vals_key="conprb", vals=None):
    key = (name, "step", vals_key)
    if key not in _CACHE:
        wl = _wl(name)
        oc = orc.em_estep(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"] if vals is None else vals, wl["ncp"], wl["theta0"])
        _CACHE[key] = orc.em_mstep(wl["M"], wl["N0"], oc, wl["theta0"])[:2]
    return _CACHE[key]


def _ctx(name, **opts):
    from rsem_amd import capi
    wl = _wl(name)
    ctx = capi.EmContext(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
    for k, v in opts.items():
        ctx.set_option(k, v)
    return wl, ctx


def _closed_form(ctx):
    """sid_plane_bytes_loaded with the list on, from the layout's own counts: the full planes (256 B) of every wave's first slice and of
    the far-queue units' marked slices, 4 B per list entry of the other marked slices, 4 B of offset per slice of the list launches."""
    return (256 * (ctx.info("sid_first_slice_planes") + ctx.info("sid_marked_planes_far_queue")) +
            4 * (ctx.info("start_list_entries_loaded") + ctx.info("start_list_slices")))


def _step_on_off(name, ctx, wl, oracle, small_atol=1e-9):
    assert ctx.info("sid_start_list") == 1 and ctx.info("start_list_entries") > 0     # the default
    on = ctx.step(wl["theta0"], wl["N0"])
    ctx.set_option("sid_start_list", 0)
    assert ctx.info("sid_start_list") == 0
    off = ctx.step(wl["theta0"], wl["N0"])
    ctx.set_option("sid_start_list", 1)
    for d in (on, off):
        assert np.allclose(d[0], oracle[0], rtol=1e-9, atol=small_atol)
        assert np.allclose(d[1], oracle[1], rtol=1e-9, atol=1e-15)
    assert np.allclose(on[0], off[0], rtol=1e-12, atol=1e-9)
    return on, off


def _runs_on_off(ctx, wl, monkeypatch):
    """200 rounds under each loop (RSEM_EM_FUSED 0: kernel sequence, 1: statistics on a second stream, 2: one launch per round)"""
    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        ctx.set_option("sid_start_list", 1)
        on = ctx.run(wl["theta0"], wl["N0"], min_round=200, max_round=200)
        ctx.set_option("sid_start_list", 0)
        off = ctx.run(wl["theta0"], wl["N0"], min_round=200, max_round=200)
        ctx.set_option("sid_start_list", 1)
        assert on["rounds"] == off["rounds"] == 200, loop
        assert np.allclose(on["theta"], off["theta"], rtol=1e-9, atol=1e-15), loop


@pytest.mark.parametrize("T", [0, 70], ids=["T-default", "T70"])
@pytest.mark.parametrize("name", ["small", "smallX"])
def test_step_and_runs_on_against_off_and_oracle(name, T, monkeypatch):
    """`small`: every unit compact; `smallX`: split rows, units with ids outside their window, the far-queue launch beside the others.
    T = 70: a block crosses the 64-slice reload of masks and offsets."""
    if T:
        monkeypatch.setenv("RSEM_HIP_T", str(T))
    wl, ctx = _ctx(name)
    _step_on_off(name, ctx, wl, _oracle_step(name))
    _runs_on_off(ctx, wl, monkeypatch)
    ctx.close()


def test_q32_planes_and_a_switch_of_formats(monkeypatch):
    """value_bits 64 -> 32 -> 64 on one context: every switch that lays the reads out again builds the list again."""
    from tools.q32_ref import quantize_q32
    wl, ctx = _ctx("small")
    e64 = ctx.info("start_list_entries")
    _step_on_off("small", ctx, wl, _oracle_step("small"))
    ctx.set_option("value_bits", 32)
    assert ctx.info("reads_q32") > 0 and ctx.info("start_list_entries") > 0
    vals = quantize_q32(wl["row_ptr"], wl["conprb"], ctx.info("value_range_bits"))[0]
    _step_on_off("small", ctx, wl, _oracle_step("small", "q32", vals))
    _runs_on_off(ctx, wl, monkeypatch)
    assert ctx.info("sid_plane_bytes_loaded") == _closed_form(ctx)
    ctx.set_option("value_bits", 64)
    assert ctx.info("reads_q32") == 0 and ctx.info("start_list_entries") == e64
    _step_on_off("small", ctx, wl, _oracle_step("small"))
    ctx.close()


def test_q32_planes_with_long_blocks(monkeypatch):
    from tools.q32_ref import quantize_q32
    monkeypatch.setenv("RSEM_HIP_T", "70")
    wl, ctx = _ctx("small", value_bits=32)
    vals = quantize_q32(wl["row_ptr"], wl["conprb"], ctx.info("value_range_bits"))[0]
    _step_on_off("small", ctx, wl, _oracle_step("small", "q32", vals))
    _runs_on_off(ctx, wl, monkeypatch)
    ctx.close()


@pytest.mark.parametrize("T", [0, 70], ids=["T-default", "T70"])
def test_with_the_csr_released(T, monkeypatch):
    """The caller-order ids are freed; the planes they are read back from are untouched by the list."""
    if T:
        monkeypatch.setenv("RSEM_HIP_T", str(T))
    wl, ctx = _ctx("small", split_rows=0)
    ctx.set_option("release_csr", 1)
    assert ctx.info("csr_released") == 1
    _step_on_off("small", ctx, wl, _oracle_step("small"))
    _runs_on_off(ctx, wl, monkeypatch)
    assert ctx.info("csr_released") == 1
    cp, ncp = ctx.get_values()
    assert np.array_equal(cp, wl["conprb"]) and np.array_equal(ncp, wl["ncp"])
    c1, w1, wn1 = ctx.expected_weights(wl["theta0"], wl["N0"])   # walks the restored ids
    assert np.allclose(c1, _oracle_step("small")[0], rtol=1e-9, atol=1e-9)
    ctx.close()


@pytest.mark.parametrize("name", ["small", "smallX"])
def test_expected_weights(name):
    wl, ctx = _ctx(name)
    ref = _oracle_step(name)
    got = {}
    for on in (1, 0):
        ctx.set_option("sid_start_list", on)
        got[on] = ctx.expected_weights(wl["theta0"], wl["N0"])
        assert np.allclose(got[on][0], ref[0], rtol=1e-9, atol=1e-9)
    assert np.allclose(got[1][1], got[0][1], rtol=1e-12, atol=1e-300) and np.allclose(got[1][2], got[0][2], rtol=1e-12, atol=1e-300)
    ctx.close()


def test_step_after_a_tuned_run():
    """A layout of more than 2048 units: the first run re-sorts the unit table by measured lifetimes.  The list does not depend on the
    units' order, the accounting follows it."""
    wl, ctx = _ctx("C3x0.06")
    assert ctx.info("units") >= 2048
    before = ctx.info("sid_plane_bytes_loaded")
    assert before == _closed_form(ctx)
    ctx.run(wl["theta0"], wl["N0"], min_round=3, max_round=3)
    assert ctx.info("unit_tables_agree") == 1
    assert ctx.info("sid_plane_bytes_loaded") == _closed_form(ctx)
    _step_on_off("C3x0.06", ctx, wl, _oracle_step("C3x0.06"))
    ctx.close()


@pytest.mark.parametrize("T", [0, 70], ids=["T-default", "T70"])
@pytest.mark.parametrize("name", ["small", "smallX"])
def test_byte_accounting(name, T, monkeypatch):
    if T:
        monkeypatch.setenv("RSEM_HIP_T", str(T))
    wl, ctx = _ctx(name)
    on, phys_on = ctx.info("sid_plane_bytes_loaded"), ctx.info("physical_bytes_per_launch")
    entries, listed, first = ctx.info("start_list_entries"), ctx.info("start_list_entries_loaded"), ctx.info("sid_first_slice_planes")
    ctx.set_option("sid_start_list", 0)
    off, phys_off = ctx.info("sid_plane_bytes_loaded"), ctx.info("physical_bytes_per_launch")
    ctx.set_option("sid_start_list", 1)
    print("%s T %d: sid bytes loaded %d with the list, %d without; list of %d entries, %d bytes" % (name, T, on, off, entries, ctx.info("start_list_bytes")))
    assert entries > 0 and ctx.info("start_list_bytes") >= 4 * entries + 4 * ctx.info("slices")
    assert on == _closed_form(ctx)
    assert phys_on - phys_off == on - off
    assert 0 < listed < entries and first > 0
    # a block's first slice is the first slice of a wave (units are whole blocks): its K planes are loaded as planes, its 64 K list
    # entries never; a layout of `slices` slices has at least slices / T blocks
    T_now = T if T else 8   # (inputs this small take the shortest block: 8 slices)
    blocks_min = -(-ctx.info("slices") // T_now)
    assert listed <= entries - 64 * blocks_min
    if ctx.info("sid_marked_planes_far_queue") == 0:   # (a far-queue unit's first slices are counted with its marked planes)
        assert first >= blocks_min
    assert first * 256 <= ctx.info("sid_plane_bytes") and ctx.info("start_list_slices") <= ctx.info("slices")
    assert on < off
    if name == "small":   # no far-queue launch: every slice's offset is fetched, no unit keeps the planes
        assert ctx.info("units_compact") == ctx.info("units") and ctx.info("start_list_slices") == ctx.info("slices")
        assert ctx.info("sid_marked_planes_far_queue") == 0
    ctx.close()


@pytest.mark.parametrize("name", ["small", "smallX"])
def test_byte_accounting_when_every_slice_is_a_first_slice(name, monkeypatch):
    """Blocks of ONE slice: every slice is the first slice of its wave, so outside the far-queue units the launch loads exactly the id
    planes of the layout -- a figure the layout states on its own ("sid_plane_bytes" = 256 B per plane of every slice) -- and not one
    list entry; the answers are those of the planes path."""
    monkeypatch.setenv("RSEM_HIP_T", "1")
    wl, ctx = _ctx(name)
    assert ctx.info("start_list_entries") > 0 and ctx.info("start_list_entries_loaded") == 0
    if ctx.info("sid_marked_planes_far_queue") == 0 and ctx.info("start_list_slices") == ctx.info("slices"):
        assert 256 * ctx.info("sid_first_slice_planes") == ctx.info("sid_plane_bytes")
        assert ctx.info("sid_plane_bytes_loaded") == ctx.info("sid_plane_bytes") + 4 * ctx.info("slices")
    else:   # (units of the far-queue launch keep the planes of their marked slices)
        assert 256 * ctx.info("sid_first_slice_planes") < ctx.info("sid_plane_bytes") and ctx.info("start_list_slices") < ctx.info("slices")
    assert name != "small" or ctx.info("start_list_slices") == ctx.info("slices")
    _step_on_off(name, ctx, wl, _oracle_step(name))
    ctx.close()

