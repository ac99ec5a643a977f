"""Which units of the sliced layout go to which E-step launch, under every EM loop.

partition_units (em.hip, by the rules of unit_groups.hpp) puts the units of the lane kernel in up to three groups: the compact
units [0, units_compact), the units with a few ids outside their LDS window [units_compact, units_main) -- the far-queue
instantiation, taken only where they are at least one main unit in 25 --, and the split rows [units_main, units).
plan_lane_launches (unit_groups.hpp; enumerated without a GPU by test_unit_groups_cpu.py) deals these ranges to launches its own
way for each of rsem_em_run's three loops (RSEM_EM_FUSED = 0 kernel sequence, 1 statistics on a second stream, 2 one launch per
round).  The
inputs here are built by hand so that each lands in one grouping, G0-G7; every test first asserts the grouping through the
info keys (a layout change that moves an input elsewhere fails here instead of quietly testing something else), then the
step against the oracle, whole runs of all three loops against the oracle and each other, and that the host and the device
copies of the unit table agree.

How the inputs steer the layout (sell_layout.hpp): a block is 8 slices for inputs this small, a unit 1, 2 or 4 blocks -- as
many as fit one window of 2048 ids.  Reads of one length share a shape; their anchors (the smallest id near the median) are
spaced so that one block of reads spans 1280 ids and two blocks more than a window: every unit is one block.  Reads of 16
alignments take 16 per slice, so a unit of reads with ONE id outside has 16 such entries per slice (the far-queue launch
takes up to 48).  The kinds of reads:
  compact   consecutive ids from the anchor: every id inside its unit's window;
  apart     15 ids from the anchor and one 3000 above it: outside the read's own window, sorted behind the compact reads
            of its shape (the apart bit), split only by split_policy 2;
  stray     15 ids from the anchor and one 2000 above it: inside the read's own window but outside its unit's; the second
            layout pass sorts them apart like the others, and no split policy splits them;
  outside   4 ids, two of them 3000 above the other two: mostly outside its window, a split row under either policy;
  long      300 alignments: stays in the CSR (k_estep_long);
  single    one alignment (the bulk of G6, 512 reads per unit).
G7 is the layout of split rows alone (units_main == 0): every read is mostly outside its window.  Split and long rows make
rsem_em_run fall back to the kernel sequence (loop_wanted); the three loops still run there: the fallback must be correct too.
"""
import threading

import numpy as np
import pytest

from oracle import pyoracle as orc
from tools.q32_ref import quantize_q32

pytestmark = pytest.mark.gpu

MAX_ROUND = 1000
INFO_KEYS = ("units", "units_compact", "units_main", "units_queued", "far_units", "split_rows", "reads_long", "unit_tables_agree")


def capi():
    from rsem_amd import capi as c
    return c


def _reads_per_slice(L):
    if L <= 4:
        return 64
    lg, cap = 1, 8
    while L > cap:
        cap, lg = cap * 2, lg + 1
    return 64 >> lg


def _group(kind, n, a0, L=16):
    """-> (lengths, ids) of n reads of one kind whose anchors start at id a0, and the first id above all of them."""
    if kind == "single":
        L = 1
    elif kind == "outside":
        L = 4
    elif kind == "long":
        L = 300
    rpb = 8 * max(_reads_per_slice(L), 1)                # reads per block of 8 slices
    anchor = a0 + (np.arange(n, dtype=np.int64) * 1280) // rpb
    if kind in ("compact", "single", "long"):
        offs = np.arange(L)
    elif kind == "apart":
        offs = np.concatenate([np.arange(15), [3000]])
    elif kind == "stray":
        offs = np.concatenate([np.arange(15), [2000]])
    elif kind == "outside":
        offs = np.array([0, 1, 3000, 3001])
    ids = (anchor[:, None] + offs[None, :]).ravel()
    return np.full(n, len(offs), np.int64), ids, int(ids.max()) + 1


def _build(groups, seed):
    lens, ids, a0 = [], [], 1
    for kind, n in groups:
        ln, sd, top = _group(kind, n, a0)
        lens.append(ln)
        ids.append(sd)
        a0 = top + 4000
    lens, sid = np.concatenate(lens), np.concatenate(ids)
    M = int(sid.max()) + 7
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    # one likely alignment per read, the others 5-20 times less likely: EM stops by its own rule within a few hundred rounds;
    # a read's values lie within 2^8 of each other, so every read (up to 256 alignments) takes Q32 planes with value_bits 32
    cp = rng.uniform(0.05, 0.2, len(sid))
    cp[rp[:-1].astype(np.int64) + rng.integers(0, 1 << 30, len(lens)) % lens] = rng.uniform(0.5, 1.0, len(lens))
    ncp = rng.uniform(0.01, 1.0, len(lens)) * 1e-5
    theta0 = np.full(M + 1, 0.95 / M)
    theta0[0] = 0.05
    return dict(M=M, N0=100, row_ptr=rp, sid=sid.astype(np.int32), conprb=cp, ncp=ncp, theta0=theta0)


G2_READS = [("compact", 1280), ("stray", 256), ("apart", 256)]
INPUTS = {
    "G0": [("compact", 1280)],                               # compact only
    "G1": [("compact", 3840), ("apart", 20)],                # 30 compact units, 1 far one: below 1 in 25, run inline
    "G2": G2_READS,                                          # far group adopted beside compact units
    "G3": [("apart", 300)],                                  # every main unit far-queued
    "G4": G2_READS + [("outside", 200)],                     # split rows plus a far group
    "G5": G2_READS + [("long", 4)],                          # long rows beside a far group
    "G6": [("single", 2000 * 512), ("apart", 90 * 128)],     # >= 2048 units: tune_unit_order runs on the first run()
    "G7": [("outside", 256)],                                # split rows only (Q32: whole reads, far units run inline)
}
_DATA, _ORACLE, _WEIGHTS = {}, {}, {}


def _input(g):
    if g not in _DATA:
        _DATA[g] = _build(INPUTS[g], seed=sorted(INPUTS).index(g) + 1)
    return _DATA[g]


def _oracle(g, bits):
    """(step counts incl. N0, theta, rounds, totNum) of the oracle; Q32: on the values the Q32 planes hold."""
    key = (g, bits)
    if key not in _ORACLE:
        d = _input(g)
        cp = d["conprb"] if bits == 64 else quantize_q32(d["row_ptr"], d["conprb"], 8)[0]
        oc = orc.em_estep(d["M"], d["row_ptr"], d["sid"], cp, d["ncp"], d["theta0"])
        oc[0] += d["N0"]
        oth, orounds, _, ot = orc.em_run(d["M"], d["row_ptr"], d["sid"], cp, d["ncp"], d["N0"], d["theta0"], max_round=MAX_ROUND)
        _ORACLE[key] = (oc, oth, orounds, ot)
    return _ORACLE[key]


def _ctx(d, bits=64):
    ctx = capi().EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])
    if bits == 32:
        ctx.set_option("value_bits", 32)
    return ctx


def _info(ctx, tag):
    i = {k: ctx.info(k) for k in INFO_KEYS}
    print(tag, " ".join("%s=%d" % kv for kv in i.items()))
    return i


def _assert_grouping(g, i, far_queue=1, bits=64):
    n, nc, nm, nq = i["units"], i["units_compact"], i["units_main"], i["units_queued"]
    assert i["unit_tables_agree"] == 1, i
    assert 0 <= nc <= nm <= n and nq <= nm, i
    # the far-queue launch takes exactly the queued units, and only where they are one main unit in 25
    adopted = far_queue == 1 and nq > 0 and nq * 25 >= nm
    assert nc == (nm - nq if adopted else nm), i
    split = g in ("G4", "G7") and bits == 64
    assert (i["split_rows"] > 0) == split and (nm < n) == split, i
    assert (i["reads_long"] > 0) == (g == "G5"), i
    if g == "G0":
        assert i["far_units"] == 0 and nq == 0 and nc == nm == n, i
    elif g == "G1":
        assert 0 < nq and nq * 25 < nm and nc == nm == n, i
    elif g == "G3":
        assert nq == nm > 0 and nc == (0 if far_queue else nm), i
    elif g == "G6":
        assert n >= 2048 and 0 < nq, i
    elif g == "G7":
        assert (nm == 0 < n if bits == 64 else i["far_units"] > 0 and nq == 0 and nc == nm == n), i
    else:  # G2, G4 (Q32: the same without its split rows), G5
        assert 0 < nq < nm and (0 < nc < nm if far_queue else nc == nm), i
    if g in ("G2", "G4", "G5", "G6"):
        assert adopted == bool(far_queue), i


def _check_runs(ctx, d, oracle, tag, monkeypatch):
    """Whole runs of all three loops against the oracle (same ROUND count, theta to 1e-6) and each other (1e-10); the ROUND
    lines of the device loops; the unit tables after every run."""
    _, oth, orounds, ot = oracle
    N1 = len(d["row_ptr"]) - 1
    runs = {}
    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        lines = []
        ctx.set_progress((lambda r, s, b, t: lines.append((r, s, b, t))) if loop != "0" else None)
        out = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
        assert out["rounds"] == orounds and out["totNum"] == ot, (tag, loop, out["rounds"], orounds)
        assert np.allclose(out["theta"], oth, rtol=1e-6, atol=1e-12), (tag, loop)
        if loop != "0":
            assert [l[0] for l in lines] == list(range(1, out["rounds"] + 1)), (tag, loop)
            assert abs(lines[-1][1] - (d["N0"] + N1)) < 1e-6 and lines[-1][3] == out["totNum"], (tag, loop)
        assert ctx.info("unit_tables_agree") == 1, (tag, loop)
        runs[loop] = out
    ctx.set_progress(None)
    monkeypatch.delenv("RSEM_EM_FUSED")
    for loop in ("1", "2"):
        assert runs[loop]["rounds"] == runs["0"]["rounds"] and runs[loop]["totNum"] == runs["0"]["totNum"], (tag, loop)
        assert np.allclose(runs[loop]["theta"], runs["0"]["theta"], rtol=1e-10, atol=1e-18), (tag, loop)
    return runs


def _check_step(ctx, d, oracle, tag):
    counts, *_ = ctx.step(d["theta0"], d["N0"])
    assert np.allclose(counts, oracle[0], rtol=1e-9, atol=1e-9), tag


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("far_queue", [1, 0])
@pytest.mark.parametrize("g", sorted(INPUTS))
def test_grouping_step_and_every_loop(g, far_queue, bits, monkeypatch):
    d = _input(g)
    monkeypatch.setenv("RSEM_HIP_FAR_QUEUE", str(far_queue))  # (read when the layout is built)
    ctx = _ctx(d, bits)
    tag = "%s far_queue=%d value_bits=%d" % (g, far_queue, bits)
    _assert_grouping(g, _info(ctx, tag), far_queue, bits)
    oracle = _oracle(g, bits)
    _check_step(ctx, d, oracle, tag)
    _check_runs(ctx, d, oracle, tag, monkeypatch)
    # after the runs (G6: after the measured-lifetime reordering of the first one) the same grouping, the same tables
    _assert_grouping(g, _info(ctx, tag + " after the runs"), far_queue, bits)
    _check_step(ctx, d, oracle, tag)
    ctx.close()


def _oracle_weights(g):
    if g not in _WEIGHTS:
        d = _input(g)
        _WEIGHTS[g] = orc.em_estep(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"], d["theta0"], want_weights=True)[1:]
    return _WEIGHTS[g]


@pytest.mark.parametrize("g", ["G2", "G4"])
def test_entry_points_in_turn_on_one_context(g, monkeypatch):
    """run -> step -> expected_weights -> run on ONE context, under each loop: every entry point has the E-step workgroups add the
    two device-wide totals (noise fraction, reads with a non-zero normaliser) into the slots beside the counts, and each finds that
    [counts | totals] scratch clear and leaves it clear -- the M-step kernel or a memset does.  Totals or counts left behind by one
    entry point would show in the next one's noise bin, sum and theta: the step's here, or the second run's.  G2: three lane
    launches per round; G4: split rows, every loop falls back to the kernel sequence."""
    d = _input(g)
    oc, oth, orounds, ot = _oracle(g, 64)
    ow, own = _oracle_weights(g)
    N1 = len(d["row_ptr"]) - 1
    ctx = _ctx(d)
    _assert_grouping(g, _info(ctx, g))

    def run(tag):
        out = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
        assert out["rounds"] == orounds and out["totNum"] == ot, (tag, out["rounds"], orounds)
        assert np.allclose(out["theta"], oth, rtol=1e-6, atol=1e-12), tag
        return out

    for loop in ("0", "1", "2"):
        monkeypatch.setenv("RSEM_EM_FUSED", loop)
        tag = "%s loop %s" % (g, loop)
        first = run(tag + " first run")
        counts, theta_new, s, _, _ = ctx.step(d["theta0"], d["N0"])
        assert np.allclose(counts, oc, rtol=1e-9, atol=1e-9), tag
        assert abs(s - (d["N0"] + N1)) < 1e-6, (tag, s)
        assert np.allclose(theta_new, oc / oc.sum(), rtol=1e-9, atol=1e-12), tag
        c2, w, wn = ctx.expected_weights(d["theta0"], d["N0"])
        assert np.allclose(c2, oc, rtol=1e-9, atol=1e-9), tag
        assert np.allclose(w, ow, rtol=1e-12, atol=0) and np.allclose(wn, own, rtol=1e-12, atol=0), tag
        second = run(tag + " second run")
        assert np.allclose(second["theta"], first["theta"], rtol=1e-10, atol=1e-18), tag
    assert ctx.info("unit_tables_agree") == 1
    ctx.close()


def test_tuned_unit_order_keeps_the_groups_and_the_results(monkeypatch):
    """G6: the first run() of a context with 2048 units or more times one E step per workgroup and re-sorts the units
    longest-first (tune_unit_order); the partition that follows puts the queued units behind the compact ones again, on the
    host and on the device.  The second run equals a run of a context that never reordered."""
    d = _input("G6")
    oracle = _oracle("G6", 64)
    monkeypatch.setenv("RSEM_HIP_TUNE", "0")
    ctx0 = _ctx(d)
    ref = ctx0.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
    i0 = _info(ctx0, "G6 untuned")
    ctx0.close()
    monkeypatch.delenv("RSEM_HIP_TUNE")
    ctx = _ctx(d)
    before = _info(ctx, "G6 built")
    _assert_grouping("G6", before)
    first = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
    # the tuning launches of that run added to the totals like every E step: nothing of them is left for the next entry points
    _check_step(ctx, d, oracle, "G6 step after the tuned run")
    c2, _, _ = ctx.expected_weights(d["theta0"], d["N0"], want_weights=False)
    assert np.allclose(c2, oracle[0], rtol=1e-9, atol=1e-9)
    after = _info(ctx, "G6 tuned")
    _assert_grouping("G6", after)
    assert after == before == i0
    second = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
    for out in (first, second):
        assert out["rounds"] == ref["rounds"] == oracle[2] and out["totNum"] == ref["totNum"]
        assert np.allclose(out["theta"], ref["theta"], rtol=1e-10, atol=1e-18)
        assert np.allclose(out["counts"], ref["counts"], rtol=1e-10, atol=1e-9)
    ctx.close()


def test_step_after_a_traced_launch():
    """G2: rsem_em_debug_trace runs three E-step launches that add to the counts and the totals; the step that follows must find
    both clear."""
    d = _input("G2")
    oc, *_ = _oracle("G2", 64)
    ctx = _ctx(d)
    _assert_grouping("G2", _info(ctx, "G2"))
    t = ctx.debug_trace(d["theta0"])
    assert t.shape == (ctx.info("units"), 2) and np.all(t[:, 1] >= t[:, 0]) and np.all(t[:, 0] > 0)
    counts, theta_new, s, _, _ = ctx.step(d["theta0"], d["N0"])
    assert np.allclose(counts, oc, rtol=1e-9, atol=1e-9)
    assert abs(s - (d["N0"] + len(d["row_ptr"]) - 1)) < 1e-6, s
    assert np.allclose(theta_new, oc / oc.sum(), rtol=1e-9, atol=1e-12)
    ctx.close()


def test_rebuilds_in_one_context_move_between_groupings():
    """One context through G2 -> G4 -> G2 (split_policy 1 -> 2 -> 1: the apart reads split under 2, the stray reads stay a far
    group) and through value_bits 64 -> 32 -> 64; each rebuild of the layout re-checked: grouping, tables, step."""
    d = _input("G2")
    ctx = _ctx(d)
    _assert_grouping("G2", _info(ctx, "G2"))
    _check_step(ctx, d, _oracle("G2", 64), "G2")
    ctx.set_option("split_policy", 2)
    i = _info(ctx, "G2 input, split_policy 2")
    _assert_grouping("G4", i)
    assert i["split_rows"] == 256
    _check_step(ctx, d, _oracle("G2", 64), "split_policy 2")
    ctx.set_option("split_policy", 1)
    _assert_grouping("G2", _info(ctx, "split_policy 1 again"))
    _check_step(ctx, d, _oracle("G2", 64), "split_policy 1 again")
    ctx.set_option("value_bits", 32)
    i = _info(ctx, "value_bits 32")
    _assert_grouping("G2", i, bits=32)
    assert ctx.info("reads_q32") == len(d["row_ptr"]) - 1
    _check_step(ctx, d, _oracle("G2", 32), "value_bits 32")
    ctx.set_option("value_bits", 64)
    _assert_grouping("G2", _info(ctx, "value_bits 64 again"))
    _check_step(ctx, d, _oracle("G2", 64), "value_bits 64 again")
    ctx.close()


def test_sharded_fused_with_one_rank_all_far_queued(monkeypatch):
    """Two ranks of the LOCAL communicator on one GPU, RSEM_EM_FUSED=1 (the loop sharded runs take on large inputs): the shard
    rule (rsem_em_shard_rows) gives rank 0 the apart reads alone -- every unit far-queued, no compact unit (G3) -- and rank 1
    the compact reads alone (G0).  Every rank equals the single-context run and the oracle."""
    c = capi()
    from rsem_amd import dist as rd
    d = _build([("apart", 300), ("compact", 300)], seed=11)
    M, rp = d["M"], d["row_ptr"]
    oth, orounds, _, ot = orc.em_run(M, rp, d["sid"], d["conprb"], d["ncp"], d["N0"], d["theta0"], max_round=MAX_ROUND)
    single = _ctx(d)
    ref = single.run(d["theta0"], d["N0"], max_round=MAX_ROUND)
    single.close()
    assert ref["rounds"] == orounds and np.allclose(ref["theta"], oth, rtol=1e-6, atol=1e-12)
    world = 2
    bounds = c.em_shard_rows(rp, world)
    assert bounds == [0, 300, 600]
    monkeypatch.setenv("RSEM_EM_FUSED", "1")
    comms = c.Comm.create_local([0] * world)
    outs, infos, lines = [None] * world, [None] * world, []

    def rank(k):
        srp, ssid, scp, sncp = rd.take_shard(rp, d["sid"], d["conprb"], d["ncp"], bounds[k], bounds[k + 1])
        ctx = c.EmContext(M, srp, np.ascontiguousarray(ssid), np.ascontiguousarray(scp), np.ascontiguousarray(sncp))
        ctx.set_comm(comms[k])
        infos[k] = {key: ctx.info(key) for key in INFO_KEYS}
        if k == 0:
            ctx.set_progress(lambda r, s, b, t: lines.append((r, s, b, t)))
        outs[k] = ctx.run(d["theta0"], d["N0"], max_round=MAX_ROUND)  # GLOBAL N0 on every rank
        infos[k]["unit_tables_agree_after"] = ctx.info("unit_tables_agree")
        ctx.close()

    ts = [threading.Thread(target=rank, args=(k,)) for k in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for cm in comms:
        cm.close()
    print("sharded FUSED:", infos)
    assert all(o is not None for o in outs)
    _assert_grouping("G3", infos[0])
    _assert_grouping("G0", infos[1])
    assert infos[0]["unit_tables_agree_after"] == infos[1]["unit_tables_agree_after"] == 1
    for o in outs:
        assert o["rounds"] == ref["rounds"] and o["totNum"] == ot
        assert np.allclose(o["theta"], ref["theta"], rtol=1e-9, atol=1e-18)
    assert np.array_equal(outs[0]["theta"], outs[1]["theta"])
    assert [l[0] for l in lines] == list(range(1, ref["rounds"] + 1))
    assert abs(lines[-1][1] - (d["N0"] + len(rp) - 1)) < 1e-6
