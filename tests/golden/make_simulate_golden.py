#!/usr/bin/env python3
"""Writes tests/golden/simulate/: small inputs of rsem-simulate-reads and what the UNMODIFIED reference program wrote for them.

    make -C oracle ref && python tests/golden/make_simulate_golden.py

TEST INFRASTRUCTURE (needs oracle/_ref/rsem-simulate-reads).  A case takes the reference files of one of the fixtures of
make_fixtures.py (its tiny transcriptome: ref.seq, ref.ti, ref.grp and, allele-specific, ref.ta / ref.gt) and the .model that
rsem-run-em learned on it (stat/s.model), edits the model's tables where the case asks for it (data: a length distribution, the RSPD's
bins, a row of the quality chain), writes a results table with the TPM column and runs, inside the case's directory,

    rsem-simulate-reads ref sim.model sim.results <theta0> <N> out --seed <seed>       (the line is kept in cmd.txt)

Kept per case: sim.results, cmd.txt, every out.* file and stdout.txt; the reference files and the model are not copied: the tests lay a
case's directory out again from the fixture it came from and the same edit (tests/simulate_cases.py: inputs).  Before anything is kept, the restatement (tests/simulate_ref.py on
MT19937) must reproduce every file byte for byte.  The generator also asserts what the cases are there for: at least two cases with
a resimulation count above 0 (a fragment shorter than every read length; an estimated RSPD whose leading bins are 0), no paired-end
case whose shortest insert is below its shortest mate (PairedEndQModel.h:415-417 is undefined there), and that the reference's own
chi-square of counts against N theta lies inside the bound the counter stream is held to (chisq/)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import simulate_cases as sc  # noqa: E402
import simulate_ref as sim  # noqa: E402

REFBIN = os.path.join(REPO, "oracle", "_ref", "rsem-simulate-reads")
OUT = sim.GOLDEN


def tpm_table(rng, M, zeros_at_ends=False):
    tpm = np.exp(rng.normal(0, 2, M))
    tpm[rng.random(M) < 0.3] = 0.0
    if zeros_at_ends:
        tpm[:3] = 0.0
        tpm[-2:] = 0.0
        tpm[M // 2:M // 2 + 4] = 0.0
    return tpm / tpm.sum() * 1e6


N = 60  # reads a case: the files stay small, and the stream search has chunk ends in every part of an attempt all the same
CASES = [  # src and edit of a case: simulate_cases.SPECS
    dict(name="se_noq", seed=101, theta0=0.06),
    dict(name="se_q", seed=102, theta0=0.06),
    dict(name="pe_noq_theta0_large", seed=111, theta0=0.9),
    dict(name="pe_q", seed=104, theta0=0.06),
    dict(name="pe_q_polya_rspd_zero_bins", seed=106, theta0=0.05, resim=True),
    dict(name="se_noq_reverse_only", seed=107, theta0=0.06),
    dict(name="se_q_allele", seed=108, theta0=0.06),
    dict(name="se_q_fragmean_short", seed=109, theta0=0.06, resim=True),
    dict(name="se_noq_zero_tpm_runs_theta0_zero", seed=112, theta0=0.0, zeros_at_ends=True),
    dict(name="pe_q_zero_quality_row", seed=113, theta0=0.1, seek_seed=True, unseen_quality=True),
    dict(name="se_q_repaired_rows", seed=114, theta0=0.06),
]
CHISQ = dict(name="chisq", seed=201, N=20000, theta0=0.06)


def prepare(case):
    """the inputs of a case in a work directory (simulate_cases.inputs lays it out; the TPM table is written here and kept) -> (directory, M)"""
    src = os.path.join(HERE, sc.SPECS[case["name"]][0])
    allele = os.path.exists(os.path.join(src, "ref.ta"))
    tr = sim.load_transcripts(os.path.join(src, "ref.ti"))
    M = len(tr) - 1
    tpm = tpm_table(np.random.default_rng(case["seed"]), M, case.get("zeros_at_ends", False))
    keep = os.path.join(OUT, case["name"])
    shutil.rmtree(keep, ignore_errors=True)
    os.makedirs(keep)
    with open(os.path.join(keep, "sim.results"), "w") as f:
        if allele:  # alleles.results: TPM is the 7th column (simulation.cpp:190)
            f.write("allele_id\ttranscript_id\tgene_id\tlength\teffective_length\texpected_count\tTPM\tFPKM\tAlleleIsoPct\tAlleleGenePct\n")
            for i in range(1, M + 1):
                f.write("%s\t%s\t%s\t%d\t0\t0\t%.4f\t0\t0\t0\n" % (tr[i][2], tr[i][0], tr[i][1], tr[i][3], tpm[i - 1]))
        else:
            f.write("transcript_id\tgene_id\tlength\teffective_length\texpected_count\tTPM\tFPKM\tIsoPct\n")
            for i in range(1, M + 1):
                f.write("%s\t%s\t%d\t0\t0\t%.4f\t0\t0\n" % (tr[i][0], tr[i][1], tr[i][3], tpm[i - 1]))
    return sc.inputs(case["name"], fresh=True), M


def run_reference(d, args):
    r = subprocess.run([REFBIN] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r.returncode, r.stdout, r.stderr


def build_case(case):
    d, _ = prepare(case)
    keep = os.path.join(OUT, case["name"])
    case.setdefault("N", N)
    args = ["ref", "sim.model", "sim.results", repr(case["theta0"]), str(case["N"]), "out", "--seed", str(case["seed"])]
    model = sim.load_model(os.path.join(d, "sim.model"))
    if model["type"] >= 2:
        assert model["gld"].lb >= model["mld"].lb, "%s: an insert can be shorter than every mate" % case["name"]
    rc, out, err = run_reference(d, args)
    for _ in range(40):  # (zero_quality_row: see simulate_cases; a case that is there for its failed attempts needs some among its few reads)
        if (rc == 0 or not case.get("seek_seed")) and not (rc == 0 and case.get("resim") and int(out.strip().split()[-1]) == 0):
            break
        case["seed"] += 1000
        args[-1] = str(case["seed"])
        rc, out, err = run_reference(d, args)
    assert rc == 0, (case["name"], rc, err)
    with open(os.path.join(keep, "stdout.txt"), "w") as f:
        f.write(out)
    with open(os.path.join(keep, "cmd.txt"), "w") as f:
        f.write(" ".join(["rsem-simulate-reads"] + args) + "\n")
    resim = int(out.strip().split()[-1])
    files, stdout, _ = sim.run_program(os.path.join(d, "ref"), os.path.join(d, "sim.model"), os.path.join(d, "sim.results"), case["theta0"], case["N"],
                                       sim.Mt19937Source(case["seed"]), quiet=False)
    assert stdout == out, (case["name"], stdout, out)
    for suffix, text in files.items():
        with open(os.path.join(d, "out" + suffix), "rb") as f:  # (a quality above 93 is a byte above 126: QualDist.h:42 has 100 values)
            assert f.read() == text.encode("latin-1"), "%s: out%s differs from the restatement" % (case["name"], suffix)
    if case.get("unseen_quality"):  # the second uniform was taken: a quality no read of the learned model had
        seen = {33 + v for v in range(100) if model["p_init"][v] > 0.0 or any(row[v] > 0.0 for row in model["p_tran"])}
        quals = files["_1.fq"].split("\n")[3::4]
        assert any(ord(c) not in seen for line in quals for c in line), case["name"]
    n_out = len([f for f in os.listdir(d) if f.startswith("out")])
    assert n_out == len(files), (case["name"], n_out, sorted(files))
    for f in os.listdir(d):
        if f.startswith("out"):
            shutil.move(os.path.join(d, f), os.path.join(keep, f))
    size = sum(os.path.getsize(os.path.join(keep, f)) for f in os.listdir(keep))
    print("%-28s type %d  resimulations %5d  %.0f KB" % (case["name"], model["type"], resim, size / 1024))
    if case.get("resim"):
        assert resim > 0, "%s is there for its failed attempts and has none" % case["name"]
    return resim


def build_chisq():
    from scipy.stats import chi2
    c = dict(CHISQ)
    d, M = prepare(c)
    args = ["ref", "sim.model", "sim.results", repr(c["theta0"]), str(c["N"]), "out", "--seed", str(c["seed"]), "-q"]
    rc, out, err = run_reference(d, args)
    assert rc == 0, err
    counts = [0] * (M + 1)
    with open(os.path.join(d, "out.fa")) as f:
        for line in f:
            if line[0] == ">":
                counts[int(line.split("_")[2])] += 1
    full, tot, seq = sim.load_refs(os.path.join(d, "ref.seq"))
    model = sim.load_model(os.path.join(d, "sim.model"))
    theta = sim.theta_from_results(os.path.join(d, "sim.results"), M, sim.calc_eel(model["gld"], full, tot), c["theta0"], False)
    # a read of a transcript is kept only if its attempt succeeds; this model has no failing attempts, so counts ~ multinomial(N, theta)
    assert int(out.strip().split()[-1]) == 0
    x, df = sc.chi_square(counts, theta, c["N"])
    bound = float(chi2.ppf(0.999, df))
    assert x < bound, (x, bound)
    for f in os.listdir(d):
        if f.startswith("out"):
            os.remove(os.path.join(d, f))
    with open(os.path.join(OUT, "chisq", "reference.json"), "w") as f:
        json.dump({"cmd": " ".join(["rsem-simulate-reads"] + args), "N": c["N"], "seed": c["seed"], "theta0": c["theta0"], "counts": counts, "chi_square": x,
                   "degrees_of_freedom": df, "quantile_0.999": bound}, f, indent=1)
        f.write("\n")
    print("chisq: reference %.2f on %d degrees of freedom, bound %.2f" % (x, df, bound))


def build_messages():
    """what the reference prints for a wrong argument count and for a model file that is not there, with its exit status"""
    d = os.path.join(OUT, "messages")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    work = sc.inputs("se_noq")
    for name, args in (("usage", ["ref", "sim.model"]), ("missing_model", ["ref", "no_such.model", "sim.results", "0.1", "10", "out"])):
        rc, out, err = run_reference(work, args)
        for suffix, text in ((".stdout", out), (".stderr", err), (".status", "%d\n" % rc), (".args", " ".join(args) + "\n")):
            with open(os.path.join(d, name + suffix), "w") as f:
                f.write(text)
    assert not [f for f in os.listdir(work) if f.startswith("out")]


if __name__ == "__main__":
    only = set(sys.argv[1:])
    n_resim = 0
    for case in CASES:
        if not only or case["name"] in only:
            n_resim += build_case(case) > 0
    if not only:
        assert n_resim >= 2, "at least two cases must record failed attempts"
        build_chisq()
        build_messages()
