"""rsem-simulate-reads without a GPU: the restatement (tests/simulate_ref.py) on MT19937 against what the unmodified reference program
wrote (tests/golden/simulate/, made by tests/golden/make_simulate_golden.py) -- every read file, every .sim.*.results file and stdout
with its resimulation line, byte for byte: this is what ties the restatement, and through it the counter stream, to the reference --
and what the program and the library do before they touch a device: the usage text, the message for a model file that is not there,
the argument checks of rsem_sim_create."""
import json
import os
import subprocess

import pytest

import simulate_cases as sc
import simulate_ref as sim


def test_the_cases_the_issue_names_are_recorded():
    types = set()
    resim = 0
    for name in sc.CASES:
        d, a = sc.case_args(name)
        types.add(sim.load_model(os.path.join(d, "sim.model"))["type"])
        resim += int(sc.recorded(name)[1].split()[-1]) > 0
    assert types == {0, 1, 2, 3} and resim >= 2 and len(sc.CASES) >= 11


@pytest.mark.parametrize("name", sc.CASES)
def test_restatement_on_mt19937_writes_the_reference_files(name):
    want_files, want_stdout = sc.recorded(name)
    got_files, got_stdout, _ = sc.restated(name, sim.Mt19937Source(sc.seed_of(name)))
    assert got_stdout == want_stdout
    assert sorted(got_files) == sorted(want_files)
    for fn in want_files:
        assert got_files[fn] == want_files[fn], fn


def test_no_paired_case_has_an_insert_below_the_shortest_mate():
    for name in sc.CASES:
        m = sim.load_model(os.path.join(sc.case_args(name)[0], "sim.model"))
        if m["type"] >= 2:
            assert m["gld"].lb >= m["mld"].lb, name


def test_reference_chi_square_is_inside_its_bound():
    """the bound the counter stream is held to (tests/test_simulate_gpu.py) holds for the reference's own counts at that N and seed"""
    from scipy.stats import chi2
    d = sc.inputs("chisq")
    with open(os.path.join(sim.GOLDEN, "chisq", "reference.json")) as f:
        ref = json.load(f)
    full, tot, _ = sim.load_refs(os.path.join(d, "ref.seq"))
    model = sim.load_model(os.path.join(d, "sim.model"))
    theta = sim.theta_from_results(os.path.join(d, "sim.results"), len(full) - 1, sim.calc_eel(model["gld"], full, tot), ref["theta0"], False)
    x, df = sc.chi_square(ref["counts"], theta, ref["N"])
    assert sum(ref["counts"]) == ref["N"] and df == ref["degrees_of_freedom"]
    assert abs(x - ref["chi_square"]) < 1e-9 * x
    assert x < chi2.ppf(0.999, df)


def test_philox_source_is_the_counter_layout():
    """uniform k of attempt a of read r: word k % 4 of the block at counter (r low, r high, a, k / 4), keyed by the seed's halves"""
    import sampler_ref as sr
    seed, read, att = (7 << 32) | 9, (3 << 32) | 5, 2
    s = sim.PhiloxSource(seed)
    s.begin(read, att)
    got = [s.next() for _ in range(9)]
    for k in (0, 3, 4, 8):
        w = sr.philox4x32_10(9, 7, 5, 3, att, k // 4)
        assert got[k] == int(w[k % 4][0]) * sim.TWO32


# ---- the program, before any device use ---------------------------------------------------------------------------------------------

def _message(name):
    rd = lambda ext: open(os.path.join(sim.GOLDEN, "messages", name + ext), "rb").read()  # noqa: E731
    return sc.inputs("se_noq"), rd(".args").decode().split(), int(rd(".status")), rd(".stdout"), rd(".stderr")


@pytest.mark.parametrize("name", ["usage", "missing_model"])
def test_program_messages_and_status_are_the_reference_ones(name):
    assert os.path.exists(sc.PROGRAM), "rsem-simulate-reads was not built"
    d, args, status, out, err = _message(name)
    r = subprocess.run([sc.PROGRAM] + args, cwd=d, capture_output=True)
    assert (r.returncode & 0xff, r.stdout, r.stderr) == (status & 0xff, out, err)
    assert not [f for f in os.listdir(d) if f.startswith("out")]


def test_program_takes_its_own_options_out_of_the_argument_count():
    """--device, -p and --sim-stream are not counted: six arguments and they are still the usage case, and a bad stream name is refused"""
    d, _, status, out, _ = _message("usage")
    r = subprocess.run([sc.PROGRAM, "ref", "sim.model", "sim.results", "0.1", "10"], cwd=d, capture_output=True)
    assert (r.returncode & 0xff, r.stdout) == (status & 0xff, out)
    r = subprocess.run([sc.PROGRAM, "ref", "no_such.model", "sim.results", "0.1", "10", "out", "--sim-stream", "fast"], cwd=d, capture_output=True)
    assert r.returncode != 0 and b"--sim-stream" in r.stderr


def test_library_checks_the_model_before_any_device():
    """RSEM_ERR_INVALID (-1), not RSEM_ERR_NODEVICE: the checks come first (this machine has no GPU; on one with a GPU they come first too)"""
    from rsem_amd import capi
    import numpy as np
    rng = np.random.default_rng(1)
    full, tot, seq = sc.transcripts(rng, [60, 80])
    t = sim.build_tables(sc.hand_model(0, {20: 1.0, 30: 1.0}), full, tot, seq, sc.theta_of([1, 2, 3]))
    good = sc.capi_tables(t)
    for key, bad in (("type", 4), ("theta_cdf", [0.5, 0.2, 1.0]), ("g_cdf", [0.1] + list(t["gld"].cdf[1:])), ("prob_f", 1.5), ("tot_len", [0, 10, 80]),
                     ("g_lb", 40), ("npc", [0.1, 0.2, float("nan"), 0.4, 1.0])):
        with pytest.raises(capi.RsemHipError) as e:
            capi.Simulate(dict(good, **{key: bad}))
        assert e.value.status == -1, (key, e.value)
