"""Option "short_last_plane" of the EM context (rsem_amd/csrc/sell_shape.hpp, Shape::cut): reads whose last value plane is a
quarter or more empty are sorted into short classes that store that plane compacted.  One step and a 200-round run with the
option on against off IN THE SAME CONTEXT and against the oracle at 1e-9, F64 and Q32 planes; the values read back from the
planes after "release_csr"; a model round written straight into the planes (rsem-run-em) against the same run with the option
off; the byte accounting.  The small inputs lower the class threshold ("short_class_min_units") so that classes are taken."""
import os
import subprocess

import numpy as np
import pytest

import rsem_files as rf
from oracle import pyoracle as orc
from tools.synth_data import make_em_workload

pytestmark = pytest.mark.gpu

PARTS = ("value_plane_bytes", "sid_plane_bytes_loaded", "slots", "slices", "units", "window_entries")


def _fixture_csr(name):
    fx = rf.fixture(name)
    M, N0ofg, rpi, sidi, vali = rf.read_ofg(os.path.join(fx, "temp", "s.ofg"))
    rp, sid, cp, ncp = rf.split_noise(rpi, sidi, vali)
    raw, pol = rf.read_theta(os.path.join(fx, "stat", "s.theta"))
    N0, N1, N2, Ntot = rf.read_cnt(os.path.join(fx, "stat", "s.cnt"))
    return dict(M=M, N0=float(N0), row_ptr=rp, sid=sid, conprb=cp, ncp=ncp, theta0=raw)


def _inputs(name):
    if name == "C3x0.1":
        return make_em_workload("C3", scale=0.1)
    if name == "small":
        return make_em_workload("small", seed=21)   # 400 000 reads of up to 12 alignments: four classes fill 8 units, a fifth one unit
    return _fixture_csr(name)


def _oracle_run(wl, vals, rounds):
    th = wl["theta0"]
    for _ in range(rounds):
        oc = orc.em_estep(wl["M"], wl["row_ptr"], wl["sid"], vals, wl["ncp"], th)
        th = orc.em_mstep(wl["M"], wl["N0"], oc, th)[1]
    return th


def _bytes_by_parts(ctx, q32):
    """physical_bytes_per_launch of a layout without split rows and long reads, from its parts (em.hip rsem_em_get_info)."""
    i = {k: ctx.info(k) for k in PARTS}
    unit_bytes = ctx.info("unit_bytes")
    return (i["value_plane_bytes"] + i["sid_plane_bytes_loaded"] + i["slots"] * (10 if q32 else 8) + i["slices"] * 8 + i["window_entries"] * 16,
            i["units"], unit_bytes)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name", ["se_q", "pe_q_polya_rspd", "small", "C3x0.1"])
def test_step_and_run_on_against_off_and_oracle(name, bits):
    """The fixtures' few hundred reads fill no unit of any class (on and off are then the same layout: that the option and the
    threshold do no harm there is all they show); `small` (400 000 reads of up to 12 alignments) and configs[2] at a tenth of its
    size take classes at the default threshold, asserted, and their step AND their 200 rounds are held against the oracle."""
    from rsem_amd import capi
    from tools.q32_ref import quantize_q32
    wl = _inputs(name)
    M = wl["M"]
    small = name in ("se_q", "pe_q_polya_rspd")   # the fixtures
    takes_classes = not small
    ctx = capi.EmContext(M, wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
    assert ctx.info("short_last_plane") == 1                     # the default
    if small:
        ctx.set_option("short_class_min_units", 1)
    ctx.set_option("value_bits", bits)
    vals = quantize_q32(wl["row_ptr"], wl["conprb"], ctx.info("value_range_bits"))[0] if bits == 32 else wl["conprb"]
    if bits == 32:
        assert ctx.info("reads_q32") > 0
    nnz_sliced = int(sum(np.diff(wl["row_ptr"].astype(np.int64))[np.diff(wl["row_ptr"].astype(np.int64)) <= 256]))
    on = dict(step=ctx.step(wl["theta0"], wl["N0"]), run=ctx.run(wl["theta0"], wl["N0"], min_round=200, max_round=200),
              bytes=ctx.info("value_plane_bytes"), entries=ctx.info("value_plane_entries"), classes=ctx.info("short_classes"),
              phys=ctx.info("physical_bytes_per_launch"), parts=_bytes_by_parts(ctx, bits == 32), long=ctx.info("reads_long"), x=ctx.info("split_rows"))
    ctx.set_option("short_last_plane", 0)
    assert ctx.info("short_last_plane") == 0 and ctx.info("short_classes") == 0
    off = dict(step=ctx.step(wl["theta0"], wl["N0"]), run=ctx.run(wl["theta0"], wl["N0"], min_round=200, max_round=200),
               bytes=ctx.info("value_plane_bytes"), entries=ctx.info("value_plane_entries"),
               phys=ctx.info("physical_bytes_per_launch"), parts=_bytes_by_parts(ctx, bits == 32))
    print("%s bits %d: classes %d, value plane bytes %d -> %d, entries per alignment %.4f -> %.4f" %
          (name, bits, on["classes"], off["bytes"], on["bytes"], off["entries"] / nnz_sliced, on["entries"] / nnz_sliced))
    assert off["entries"] == ctx.info("sid_plane_bytes") // 4      # the full layout: 64 entries per plane
    if takes_classes:
        assert on["classes"] > 0 and on["bytes"] < off["bytes"] and on["entries"] < off["entries"]
    else:
        assert on["classes"] == 0 and on["bytes"] == off["bytes"]
    assert on["entries"] >= nnz_sliced
    # the accounting is the sum of its parts (no split rows, no long reads in these inputs: their terms are zero)
    for d in (on, off):
        if not on["long"] and not on["x"]:
            s, units, ub = d["parts"]
            assert d["phys"] == s + units * ub + 16 * (M + 1), (d["phys"], s, units)
    # one step: on == off == oracle at 1e-9
    oc = orc.em_estep(M, wl["row_ptr"], wl["sid"], vals, wl["ncp"], wl["theta0"])
    oc, oth, *_ = orc.em_mstep(M, wl["N0"], oc, wl["theta0"])
    for d in (on, off):
        assert np.allclose(d["step"][0], oc, rtol=1e-9, atol=1e-9 if not small else 1e-12)
        assert np.allclose(d["step"][1], oth, rtol=1e-9, atol=1e-15)
    assert np.allclose(on["step"][0], off["step"][0], rtol=1e-12, atol=1e-9)
    # 200 rounds
    assert on["run"]["rounds"] == off["run"]["rounds"] == 200
    assert np.allclose(on["run"]["theta"], off["run"]["theta"], rtol=1e-9, atol=1e-15)
    oth200 = _oracle_run(wl, vals, 200)
    assert np.allclose(on["run"]["theta"], oth200, rtol=1e-9, atol=1e-15)
    assert np.allclose(off["run"]["theta"], oth200, rtol=1e-9, atol=1e-15)
    ctx.close()


@pytest.mark.parametrize("name", ["small", "C3x0.1"])
def test_release_csr_gives_the_csr_back(name):
    """The caller-order values are freed and read back from planes whose last plane is compacted: the doubles that went in."""
    from rsem_amd import capi
    wl = _inputs(name)
    if int(np.max(np.diff(wl["row_ptr"].astype(np.int64)))) > 256:
        pytest.skip("reads with more than 256 alignments live in the CSR alone")
    ctx = capi.EmContext(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
    ctx.set_option("split_rows", 0)
    if name == "small":
        n8 = ctx.info("short_classes")
        ctx.set_option("short_class_min_units", 1)          # (the fixtures' few hundred reads fill no unit of any class: not used here)
        assert ctx.info("short_classes") > n8 > 0
    assert ctx.info("short_classes") > 0
    ref = ctx.step(wl["theta0"], wl["N0"])
    ctx.set_option("release_csr", 1)
    assert ctx.info("csr_released") == 1
    again = ctx.step(wl["theta0"], wl["N0"])
    assert np.allclose(again[0], ref[0], rtol=1e-12, atol=1e-9)
    cp, ncp = ctx.get_values()
    assert ctx.info("csr_released") == 0
    assert np.array_equal(cp, wl["conprb"]) and np.array_equal(ncp, wl["ncp"])
    c1, w1, wn1 = ctx.expected_weights(wl["theta0"], wl["N0"])   # walks the restored ids and values
    assert np.allclose(c1, ref[0], rtol=1e-9, atol=1e-9)
    ctx.set_option("release_csr", 1)
    ctx.set_option("short_last_plane", 0)                        # a rebuild of the layout needs the CSR: restored first
    assert ctx.info("csr_released") == 0 and ctx.info("short_classes") == 0
    cp, ncp = ctx.get_values()
    assert np.array_equal(cp, wl["conprb"])
    ctx.close()


def test_model_round_written_through_the_planes(tmp_path):
    """rsem-run-em: the model rounds' kernel writes every alignment probability straight into the value planes (model_block.hpp
    plane_put).  With the classes on (threshold 1 unit: 20 000 reads) the .theta, .model and .ofg (--lean-device: read back from
    the planes) are those of the run with the option off."""
    import model_path_cases as mc
    if not mc.have_tools(need_ref=False):
        pytest.skip("needs tools/bin/gen_temp and rsem_amd/bin/rsem-run-em (build())")
    case = mc.CASES["chunks_pe_q"]
    d = str(tmp_path)
    mc.generate(case, d)
    outs = {}
    for tag, env in (("on", {"RSEM_HIP_SHORT_LAST_PLANE": "1", "RSEM_HIP_SHORT_MIN_UNITS": "1"}), ("off", {"RSEM_HIP_SHORT_LAST_PLANE": "0"})):
        cmd = [os.path.join(mc.ROOT, "rsem_amd", "bin", "rsem-run-em")] + mc.em_args(case, d) + ["--lean-device"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, (tag, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs[tag] = dict(rounds=[l for l in r.stdout.split("\n") if l.startswith("ROUND")],
                         theta=rf.read_theta(os.path.join(d, "stat", "s.theta"))[0], model=rf.read_model(os.path.join(d, "stat", "s.model")),
                         ofg=rf.read_ofg(os.path.join(d, "temp", "s.ofg")))
    a, b = outs["on"], outs["off"]
    # the `on` run did take classes: the same row lengths (all F64 while the model rounds run) under the same threshold
    M_, N0_, rp_, sid_, val_ = b["ofg"]
    rp2, sid2, cp2, ncp2 = rf.split_noise(rp_, sid_, val_)
    from rsem_amd import capi
    ctx = capi.EmContext(M_, rp2, sid2, cp2, ncp2)
    ctx.set_option("short_class_min_units", 1)
    n_classes, e_on = ctx.info("short_classes"), ctx.info("value_plane_entries")
    ctx.set_option("short_last_plane", 0)
    assert n_classes > 0 and e_on < ctx.info("value_plane_entries")
    ctx.close()
    assert len(a["rounds"]) == len(b["rounds"]) > 11
    assert np.allclose(a["theta"], b["theta"], rtol=1e-9, atol=1e-12)
    for key in ("qd_init", "qd_tran", "qpro", "nqpro", "pro", "npro", "rspd", "mw"):
        if key in b["model"] and b["model"][key] is not None:
            assert np.allclose(a["model"][key], b["model"][key], rtol=1e-9, atol=1e-12), key
    assert np.allclose(a["model"]["gld"][3], b["model"]["gld"][3], rtol=1e-9, atol=1e-12)
    assert a["ofg"][0] == b["ofg"][0] and np.array_equal(a["ofg"][2], b["ofg"][2]) and np.array_equal(a["ofg"][3], b["ofg"][3])
    assert np.allclose(a["ofg"][4], b["ofg"][4], rtol=1e-9, atol=1e-300)
