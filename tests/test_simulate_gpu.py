"""rsem-simulate-reads on the GPU (rsem_amd/csrc/simulate.hip through the program and through capi.Simulate) against what the
unmodified reference program wrote (tests/golden/simulate/) and against the restatement (tests/simulate_ref.py).  Reads, counts and
files are compared for equality; the one statistical test takes its bound from the chi-square distribution and the reference's own
statistic lies inside it (tests/test_simulate_cpu.py).

A lane takes a read (an attempt); the stream search works in chunks, tiles and a prefix sum over positions.  Sizes: 1, 63, 64, 65 and
257 reads (a lane, a wave and a workgroup, each with one more), knobs that put a chunk's end inside a read's header and inside its
bases (chunks of 5 and 97 positions under attempts of 37 and more uniforms), on the last word of a 624-word generator block (624), and
a tile around a single attempt (tiles of 1 and 8)."""
import json
import os
import subprocess

import numpy as np
import pytest

import simulate_cases as sc
import simulate_ref as sim

pytestmark = pytest.mark.gpu

SMALL_KNOBS = [dict(RSEM_SIM_BATCH_READS="7", RSEM_SIM_CHUNK_WORDS="5", RSEM_SIM_TILE="1"),
               dict(RSEM_SIM_BATCH_READS="64", RSEM_SIM_CHUNK_WORDS="97", RSEM_SIM_TILE="8"),
               dict(RSEM_SIM_BATCH_READS="33", RSEM_SIM_CHUNK_WORDS="624", RSEM_SIM_TILE="624"),
               dict(RSEM_SIM_BATCH_READS="1000", RSEM_SIM_CHUNK_WORDS="4099", RSEM_SIM_TILE="2048", RSEM_SIM_LDS_TABLES="0")]
KNOB_CASES = ["se_q_fragmean_short", "pe_q_zero_quality_row", "pe_noq_theta0_large", "pe_q_polya_rspd_zero_bins", "se_noq_reverse_only"]
N_KNOBS = 60


def run_program(tmp_path, name, extra=(), n=None, seed=None, env=None):
    """the program on a recorded case's inputs -> ({file name: bytes}, stdout, stderr)"""
    assert os.path.exists(sc.PROGRAM), "rsem-simulate-reads was not built"
    d, a = sc.case_args(name)
    a = list(a)
    a[5] = os.path.join(str(tmp_path), "out")
    if n is not None:
        a[4] = str(n)
    if seed is not None:
        a[7] = str(seed)
    r = subprocess.run([sc.PROGRAM] + a + list(extra), cwd=d, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files = {}
    for fn in sorted(os.listdir(str(tmp_path))):
        if fn.startswith("out"):
            with open(os.path.join(str(tmp_path), fn), "rb") as f:
                files[fn] = f.read()
            os.remove(os.path.join(str(tmp_path), fn))
    return files, r.stdout, r.stderr


# ---- the program, the reference's stream ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_program_default_stream_writes_the_reference_files(tmp_path, name):
    want_files, want_stdout = sc.recorded(name)
    files, stdout, stderr = run_program(tmp_path, name)
    assert stdout == want_stdout
    assert sorted(files) == sorted(want_files)
    for fn in want_files:
        assert files[fn] == want_files[fn], fn
    assert stderr.count(b"--sim-stream reference") == 1


_mt = {}


def _restated_mt(name):
    if name not in _mt:
        _mt[name] = sc.restated(name, sim.Mt19937Source(sc.seed_of(name)), n=N_KNOBS)[:2]
    return _mt[name]


@pytest.mark.parametrize("knobs", SMALL_KNOBS, ids=lambda k: "b%s_c%s_t%s" % (k["RSEM_SIM_BATCH_READS"], k["RSEM_SIM_CHUNK_WORDS"], k["RSEM_SIM_TILE"]))
@pytest.mark.parametrize("name", KNOB_CASES)
def test_program_files_do_not_depend_on_batch_chunk_and_tile(tmp_path, name, knobs):
    want_files, want_stdout = _restated_mt(name)
    files, stdout, _ = run_program(tmp_path, name, n=N_KNOBS, env=knobs)
    assert stdout == want_stdout
    assert files == want_files


# ---- the program, the counter stream ------------------------------------------------------------------------------------------------

COUNTER_CASES = ["se_noq", "se_q_repaired_rows", "pe_noq_theta0_large", "pe_q", "se_q_fragmean_short", "pe_q_polya_rspd_zero_bins", "se_q_allele"]
N_COUNTER = 150
_ph = {}


def _restated_philox(name, seed):
    if (name, seed) not in _ph:
        _ph[(name, seed)] = sc.restated(name, sim.PhiloxSource(seed), n=N_COUNTER)[:2]
    return _ph[(name, seed)]


@pytest.mark.parametrize("name", COUNTER_CASES)
def test_program_counter_stream_is_the_philox_replay(tmp_path, name):
    want_files, want_stdout = _restated_philox(name, 77)
    files, stdout, stderr = run_program(tmp_path, name, extra=["--sim-stream", "counter"], n=N_COUNTER, seed=77)
    assert stdout == want_stdout
    assert files == want_files
    assert stderr.count(b"--sim-stream counter") == 1


@pytest.mark.parametrize("batch,threads", [(1, 1), (7, 4), (64, 1), (100000, 4)])
def test_program_counter_files_do_not_depend_on_batch_and_threads(tmp_path, batch, threads):
    name = "pe_q"
    want_files, want_stdout = _restated_philox(name, 77)
    files, stdout, _ = run_program(tmp_path, name, extra=["--sim-stream", "counter", "-p", str(threads)], n=N_COUNTER, seed=77, env={"RSEM_SIM_BATCH_READS": str(batch)})
    assert (stdout, files) == (want_stdout, want_files)


def test_program_counter_seeds_give_different_files(tmp_path):
    a, _, _ = run_program(tmp_path, "se_q", extra=["--sim-stream", "counter"], n=50, seed=1)
    b, _, _ = run_program(tmp_path, "se_q", extra=["--sim-stream", "counter"], n=50, seed=2)
    assert a["out.fq"] != b["out.fq"]


# ---- capi.Simulate, hand-made tables ------------------------------------------------------------------------------------------------

def hand_tables(model_type, rng_seed=3, **kw):
    rng = np.random.default_rng(rng_seed)
    lens = kw.pop("lens", [40, 75, 40, 120, 64])
    full, tot, seq = sc.transcripts(rng, lens, kw.pop("tails", None))
    theta = kw.pop("theta", sc.theta_of([2] + [1 + i for i in range(len(lens))]))
    return sim.build_tables(sc.hand_model(model_type, **kw), full, tot, seq, theta)


# lengths 1 and the longest; a transcript (1 and 3) exactly as long as the longest fragment: effL = 1, pos = 0 on both strands
LENGTHS = {1: 1.0, 17: 2.0, 40: 3.0}
HAND = {
    "se_noq": dict(model_type=0, lengths=LENGTHS),
    "se_q": dict(model_type=1, lengths=LENGTHS),
    "se_q_mld": dict(model_type=1, lengths={30: 1.0, 40: 1.0}, mate_lengths={1: 1.0, 25: 1.0, 35: 1.0}),
    "pe_noq": dict(model_type=2, lengths={30: 1.0, 40: 2.0}, mate_lengths={1: 1.0, 30: 1.0}),
    "pe_q_rspd": dict(model_type=3, lengths={30: 1.0, 40: 2.0}, mate_lengths={1: 1.0, 30: 1.0}, est_bins=[0.0, 0.0, 0.3, 0.3, 0.4], tails=[0, 10, 0, 25, 5]),
}


def check_counter(t, n, seed=11, first=0):
    from rsem_amd import capi
    want, counts, resim = sim.simulate(t, sim.PhiloxSource(seed), n, first_read=first)
    h = capi.Simulate(sc.capi_tables(t))
    try:
        b = h.counter_batch(seed, first, n)
        assert b["status"] == capi.SIM_OK and b["n_reads"] == n
        assert sc.reads_of_batch(b, t["type"]) == sc.strip(want)
        got_counts, got_resim = h.totals()
        assert got_counts.tolist() == counts and got_resim == resim == b["resimulations"]
    finally:
        h.close()
    return want


def check_reference(t, n, seed=11, parts=(1.0,)):
    from rsem_amd import capi
    want, counts, resim = sim.simulate(t, sim.Mt19937Source(seed), n)
    h = capi.Simulate(sc.capi_tables(t))
    try:
        h.reference_begin(seed)
        got, left = [], n
        for k, share in enumerate(parts):
            take = left if k == len(parts) - 1 else min(left, max(1, int(n * share)))
            b = h.reference_batch(take)
            assert b["status"] == capi.SIM_OK and b["n_reads"] == take
            got += sc.reads_of_batch(b, t["type"])
            left -= take
        assert got == sc.strip(want)
        got_counts, got_resim = h.totals()
        assert got_counts.tolist() == counts and got_resim == resim
    finally:
        h.close()
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("model", sorted(HAND))
def test_counter_batch_is_the_restatement(model, n):
    t = hand_tables(**dict(HAND[model]))
    want = check_counter(t, n)
    if n == 257:  # what the tables were made for is in the reads: lengths 1 and the longest, the noise and the last transcript
        lens = {len(m[0]) for r in want for m in r["mates"]}
        assert 1 in lens and max(lens) == (t["mld"].ub if t["mld"] is not None else t["gld"].ub)
        assert {0, t["M"]} <= {r["sid"] for r in want}
    if n == 257 and model in ("se_noq", "se_q"):  # a fragment as long as its transcript (1 and 3): effL = 1, pos = 0 on both strands
        whole = [r for r in want if r["sid"] in (1, 3) and len(r["mates"][0][0]) == 40]
        assert {r["dir"] for r in whole} == {0, 1} and {r["pos"] for r in whole} == {0}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("model", sorted(HAND))
def test_reference_batch_is_the_restatement(model, n, monkeypatch):
    monkeypatch.setenv("RSEM_SIM_CHUNK_WORDS", "1000")
    monkeypatch.setenv("RSEM_SIM_TILE", "32")
    t = hand_tables(**dict(HAND[model]))
    check_reference(t, n, parts=(0.3, 0.3, 1.0))


def test_counter_batch_first_read_offsets_the_counter():
    """reads 100 .. 139 of a run are those reads whatever batch they come in; a read id above 2^32 reaches the counter's second word"""
    t = hand_tables(**dict(HAND["se_q"]))
    check_counter(t, 40, first=100)
    check_counter(t, 3, first=(1 << 32) + 5)


@pytest.mark.parametrize("stream", ["counter", "reference"])
def test_tie_goes_right(stream):
    """theta's running sum is made so that u * total of read 0's first uniform IS its entries 0 and 1 (the total is 1.0): an entry equal to
    the probe is passed, a zero-width entry is never picked: the read comes from transcript 2"""
    src = sim.PhiloxSource(11) if stream == "counter" else sim.Mt19937Source(11)
    src.begin(0, 0)
    u = src.next()
    t = hand_tables(**dict(HAND["se_noq"]))
    t["theta_cdf"] = [u, u, (u + 1.0) / 2, (u + 1.0) / 2, 1.0, 1.0]
    assert u * t["theta_cdf"][-1] == t["theta_cdf"][0]
    want = check_counter(t, 64) if stream == "counter" else check_reference(t, 64)
    assert want[0]["sid"] == 2


def test_resimulation_total_ends_with_the_last_read(monkeypatch):
    """Chunks about as long as one read's attempts: for some N the last chunk holds failed attempts behind read N.  The run never makes
    them (simulation.cpp:121-126 stops after read N): the batch's and the handle's totals are the failed attempts of the first N reads,
    for every N from 1 to 60; and a second batch claims what the first one left behind it."""
    from rsem_amd import capi
    monkeypatch.setenv("RSEM_SIM_CHUNK_WORDS", "70")
    monkeypatch.setenv("RSEM_SIM_TILE", "8")
    # most fragments (20) are below the reads of 25 and 35: four uniforms and a failed attempt; a read takes 55 to 75 uniforms
    t = hand_tables(**dict(HAND["se_q_mld"], lengths={20: 3.0, 30: 1.0, 40: 1.0}, mate_lengths={25: 1.0, 35: 1.0}))
    want = sim.simulate(t, sim.Mt19937Source(11), 70)[0]
    fails = [r["attempts"] for r in want]
    assert sum(fails) > 30
    for n in range(1, 61):
        h = capi.Simulate(sc.capi_tables(t))
        try:
            h.reference_begin(11)
            b = h.reference_batch(n)
            assert b["attempts"].tolist() == fails[:n]
            assert b["resimulations"] == sum(fails[:n]) == h.totals()[1], n
            b2 = h.reference_batch(10)
            assert b2["attempts"].tolist() == fails[n:n + 10] and h.totals()[1] == sum(fails[:n + 10]), n
        finally:
            h.close()


def _empty_quality_row(m):
    """Quality 20 becomes rare and its row empty; the second uniform then reaches every value: those below 94 lead back to 10 and have a
    profile (one above 93 stops the reference at an assertion, the restatement and the device with a status)."""
    m["p_init"][20] *= 0.05
    for q in range(94):
        m["p_tran"][q][20] *= 0.05
        if q not in (10, 20, 30, 40):
            m["p_tran"][q][10] = 1.0
            m["p"][q] = m["p"][10]
            m["np"][q] = m["np"][10]
    m["p_tran"][20] = [0.0] * 100


def _visits_the_empty_row(t, src, n):
    """the restatement gets through n reads (no quality above 93) and some quality is one only the second uniform gives"""
    try:
        reads = sim.simulate(t, src, n)[0]
    except sim.Undefined:
        return False
    return any(ord(c) - 33 not in (10, 20, 30, 40) for r in reads for c in r["mates"][0][1])


def test_quality_row_without_mass_takes_a_second_uniform():
    """the row of quality 20 is empty: sample() takes a second uniform there, which shifts every later position of the reference's stream"""
    full, tot, seq = sc.transcripts(np.random.default_rng(5), [40, 75, 64])
    m = sc.hand_model(1, lengths={12: 1.0, 20: 1.0})
    _empty_quality_row(m)
    t = sim.build_tables(m, full, tot, seq, sc.theta_of([1, 2, 3, 4]))
    seed = next(s for s in range(1, 400) if _visits_the_empty_row(t, sim.Mt19937Source(s), 30) and _visits_the_empty_row(t, sim.PhiloxSource(s), 30))
    from rsem_amd import capi
    h = capi.Simulate(sc.capi_tables(t))
    assert not h.plain
    h.close()
    check_reference(t, 30, seed=seed)
    check_counter(t, 30, seed=seed)


def test_profile_rows_without_mass_are_repaired_by_the_caller_and_sampled():
    """rows that startSimulation repairs (QProfile.h:160-191): the repaired running sums are what the device samples from"""
    full, tot, seq = sc.transcripts(np.random.default_rng(6), [40, 75, 64])
    m = sc.hand_model(1, lengths={20: 1.0, 30: 1.0})
    m["p"][10][1] = [0.0] * 5
    m["p"][30][4] = [0.0] * 5
    t = sim.build_tables(m, full, tot, seq, sc.theta_of([0, 2, 3, 4]))
    assert t["pc"][10][1][4] > 0.0 and t["pc"][30][4][4] > 0.0
    check_counter(t, 257)
    check_reference(t, 257)


@pytest.mark.parametrize("stream", ["counter", "reference"])
def test_a_read_that_never_succeeds_returns_the_attempt_cap(stream, monkeypatch):
    """every transcript is shorter than the shortest fragment and theta[0] is 0: every attempt fails at its header (two uniforms)"""
    from rsem_amd import capi
    monkeypatch.setenv("RSEM_SIM_ATTEMPT_CAP", "50")
    monkeypatch.setenv("RSEM_SIM_CHUNK_WORDS", "64")
    full, tot, seq = sc.transcripts(np.random.default_rng(7), [10, 12])
    t = sim.build_tables(sc.hand_model(0, {20: 1.0, 30: 1.0}), full, tot, seq, sc.theta_of([0, 1, 1]))
    h = capi.Simulate(sc.capi_tables(t))
    try:
        if stream == "counter":
            b = h.counter_batch(1, 0, 5)
        else:
            h.reference_begin(1)
            b = h.reference_batch(5)
        assert b["status"] == capi.SIM_ATTEMPT_CAP and b["n_reads"] == 0
        assert h.totals()[0].sum() == 0
        with pytest.raises(capi.RsemHipError):  # the handle takes no more batches
            h.counter_batch(1, 0, 1)
    finally:
        h.close()


def test_a_short_insert_is_a_status():
    """PairedEndQModel.h:415-417: an insert shorter than every mate length is undefined in the reference, a status here"""
    from rsem_amd import capi
    full, tot, seq = sc.transcripts(np.random.default_rng(8), [60, 80])
    t = sim.build_tables(sc.hand_model(2, lengths={10: 1.0, 40: 1.0}, mate_lengths={20: 1.0, 30: 1.0}), full, tot, seq, sc.theta_of([0, 1, 1]))
    h = capi.Simulate(sc.capi_tables(t))
    try:
        assert h.counter_batch(1, 0, 64)["status"] == capi.SIM_SHORT_INSERT
    finally:
        h.close()


# ---- the counter stream's distribution ------------------------------------------------------------------------------------------------

def test_counter_stream_counts_follow_theta(tmp_path):
    """20 000 reads of the smallest model: Pearson's chi-square of the per-transcript counts against N theta stays below the 99.9 %
    quantile for its degrees of freedom -- the bound the reference's own counts at this N and seed meet (reference.json)"""
    from scipy.stats import chi2
    d = sc.inputs("chisq")
    with open(os.path.join(sim.GOLDEN, "chisq", "reference.json")) as f:
        ref = json.load(f)
    out = os.path.join(str(tmp_path), "out")
    r = subprocess.run([sc.PROGRAM, "ref", "sim.model", "sim.results", repr(ref["theta0"]), str(ref["N"]), out, "--seed", str(ref["seed"]), "-q", "--sim-stream", "counter",
                        "-p", "4"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    full, tot, _ = sim.load_refs(os.path.join(d, "ref.seq"))
    M = len(full) - 1
    counts = [0] * (M + 1)
    with open(out + ".fa") as f:
        for line in f:
            if line[0] == ">":
                counts[int(line.split("_")[2])] += 1
    model = sim.load_model(os.path.join(d, "sim.model"))
    theta = sim.theta_from_results(os.path.join(d, "sim.results"), M, sim.calc_eel(model["gld"], full, tot), ref["theta0"], False)
    x, df = sc.chi_square(counts, theta, ref["N"])
    print("chi-square %.2f on %d degrees of freedom; the reference's %.2f; bound %.2f" % (x, df, ref["chi_square"], chi2.ppf(0.999, df)))
    assert sum(counts) == ref["N"] and df == ref["degrees_of_freedom"]
    assert x < chi2.ppf(0.999, df)
