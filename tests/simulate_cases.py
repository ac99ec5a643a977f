"""Hand-made models for the tests of rsem-simulate-reads (tests/test_simulate_cpu.py, tests/test_simulate_gpu.py): tiny tables in the
restatement's form (tests/simulate_ref.py) and the same tables in the form capi.Simulate takes, and the recorded cases."""
import atexit
import os
import shutil
import tempfile

import numpy as np

import simulate_ref as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "rsem_amd", "bin", "rsem-simulate-reads")
CASES = sorted(d for d in os.listdir(sim.GOLDEN) if os.path.exists(os.path.join(sim.GOLDEN, d, "cmd.txt"))) if os.path.isdir(sim.GOLDEN) else []


# ---- the recorded cases: a fixture of make_fixtures.py (its reference files and the model rsem-run-em learned on it) and an edit ---------

def fmt(v):
    return " ".join("%.10g" % x for x in v)


def parse_raw(path):
    """the .model file as its sections, nothing trimmed or summed"""
    with open(path) as f:
        tok = f.read().split()
    p = [0]

    def nxt(n, conv=float):
        v = [conv(x) for x in tok[p[0]:p[0] + n]]
        p[0] += n
        return v

    def lendist():
        lb, ub, span = nxt(3, int)
        return [lb, ub, nxt(span)]

    m = {"type": nxt(1, int)[0], "probF": nxt(1)[0], "gld": lendist()}
    if m["type"] < 2:
        m["mld"] = lendist() if nxt(1, int)[0] > 0 else None
    else:
        m["mld"] = lendist()
    m["rspd"] = nxt(nxt(1, int)[0]) if nxt(1, int)[0] else None
    if m["type"] in (1, 3):
        assert nxt(1, int)[0] == 100
        m["p_init"] = nxt(100)
        m["p_tran"] = [nxt(100) for _ in range(100)]
        assert nxt(2, int) == [100, 5]
        m["p"] = [[nxt(5) for _ in range(5)] for _ in range(100)]
        assert nxt(2, int) == [100, 5]
        m["np"] = [nxt(5) for _ in range(100)]
    else:
        L = nxt(2, int)[0]
        m["p"] = [[nxt(5) for _ in range(5)] for _ in range(L)]
        assert nxt(1, int)[0] == 5
        m["np"] = nxt(5)
    return m


def write_raw(m, path):
    """model_file_description.txt's layout; the mask weights at the end are left out (the simulator does not read them)"""
    def lendist(d):
        return ["%d %d %d" % (d[0], d[1], len(d[2])), fmt(d[2]), ""]

    out = [str(m["type"]), "", "%.10g" % m["probF"], ""] + lendist(m["gld"])
    if m["type"] < 2:
        out += (["1"] + lendist(m["mld"])) if m["mld"] else ["0", ""]
    else:
        out += lendist(m["mld"])
    out += (["1", str(len(m["rspd"])), fmt(m["rspd"]), ""]) if m["rspd"] else ["0", ""]
    if m["type"] in (1, 3):
        out += ["100", fmt(m["p_init"])] + [fmt(r) for r in m["p_tran"]] + ["", "100 5"]
        for q in range(100):
            out += [fmt(r) for r in m["p"][q]] + [""]
        out += ["100 5"] + [fmt(r) for r in m["np"]]
    else:
        out += ["%d 5" % len(m["p"])]
        for rows in m["p"]:
            out += [fmt(r) for r in rows] + [""]
        out += ["5", fmt(m["np"])]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


# ---- edits of a model's tables (data) ----------------------------------------------------------------------------------------------

def short_fragments(m):
    """single-end with a mate-length distribution: fragments from 20 bases on, most of them below the shortest read (36)"""
    lo = 20
    hi = m["gld"][1]
    x = range(lo, hi + 1)
    p = [3.0 if v < m["mld"][0] + 1 else 1.0 for v in x]
    m["gld"] = [lo - 1, hi, [v / sum(p) for v in p]]


def rspd_leading_zeros(m):
    """an estimated RSPD whose first 13 bins of 20 are empty: a fragment that leaves a transcript only its first positions cannot start"""
    v = [0.0] * 13 + list(m["rspd"][13:])
    m["rspd"] = [x / sum(v) for x in v]


def zero_quality_row(m):
    """The quality chain reaches, now and then, a value whose row is empty: sample() takes its second uniform there and the next quality
    is any of the 100 values.  One above 93 ends the reference at an assertion (c2q), so the value is made rare (a handful of visits in
    the run; the generator looks for a seed at which the reference gets through), and the rows of the values no read had, which the
    second uniform can now reach, lead back to the most likely first value instead of being empty themselves."""
    home = int(np.argmax(m["p_init"]))
    q = home - 3
    for v in range(100):
        if sum(m["p_tran"][v]) == 0.0:
            m["p_tran"][v][home] = 1.0
        m["p_tran"][v][q] *= 0.02
    m["p_init"][q] *= 0.02
    m["p_tran"][q] = [0.0] * 100


def zero_profile_rows(m):
    """profile rows that startSimulation repairs (reference base C: no observation at a fifth of the rows), and one whole quality empty"""
    rows = m["p"]
    for i in range(0, len(rows), 5):
        rows[i][1] = [0.0] * 5
    if m["type"] in (1, 3):
        q = int(np.argmax(m["p_init"])) + 1
        rows[q] = [[0.0] * 5 for _ in range(5)]


# case -> (the fixture under tests/golden/ it takes ref.* and stat/s.model from, the edit of the model's tables).
# The recorded outputs under tests/golden/simulate/ belong to THESE inputs: whoever runs make_fixtures.py again (new ref.* or
# stat/s.model in a fixture named here) or changes an edit above has to run make_simulate_golden.py again, or all the cases fail.
SPECS = {
    "se_noq": ("se_noq", None), "se_q": ("se_q", None), "pe_noq_theta0_large": ("pe_noq", None), "pe_q": ("pe_q", None),
    "pe_q_polya_rspd_zero_bins": ("pe_q_polya_rspd", rspd_leading_zeros), "se_noq_reverse_only": ("se_noq_rev_rspd_omit", None),
    "se_q_allele": ("se_q_allele", None), "se_q_fragmean_short": ("se_q_fragmean", short_fragments),
    "se_noq_zero_tpm_runs_theta0_zero": ("se_noq", None), "pe_q_zero_quality_row": ("pe_q", zero_quality_row),
    "se_q_repaired_rows": ("se_q", zero_profile_rows), "chisq": ("se_noq", None),
}
_inputs = {}


def inputs(name, fresh=False):
    """A directory (made once per process, removed at exit) that holds what the recorded command line of a case names: ref.seq, ref.ti,
    ref.grp [, ref.ta, ref.gt] of the case's fixture, sim.model -- the fixture's learned model with the case's edit, written as the
    generator wrote it -- and the recorded sim.results."""
    if name in _inputs and not fresh:
        return _inputs[name]
    src = os.path.join(os.path.dirname(sim.GOLDEN), SPECS[name][0])
    d = tempfile.mkdtemp(prefix="rsem_sim_" + name + "_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    for ext in ("seq", "ti", "grp", "ta", "gt"):
        if os.path.exists(os.path.join(src, "ref." + ext)):
            shutil.copy(os.path.join(src, "ref." + ext), os.path.join(d, "ref." + ext))
    m = parse_raw(os.path.join(src, "stat", "s.model"))
    if SPECS[name][1]:
        SPECS[name][1](m)
    write_raw(m, os.path.join(d, "sim.model"))
    shutil.copy(os.path.join(sim.GOLDEN, name, "sim.results"), os.path.join(d, "sim.results"))
    _inputs[name] = d
    return d


def case_args(name):
    """-> (the directory of the case's inputs, the recorded argument list after the program's name)"""
    with open(os.path.join(sim.GOLDEN, name, "cmd.txt")) as f:
        return inputs(name), f.read().split()[1:]


def recorded(name):
    """{file name: bytes} of what the reference wrote for a case, and its stdout"""
    d = os.path.join(sim.GOLDEN, name)
    files = {}
    for fn in sorted(os.listdir(d)):
        if fn.startswith("out"):
            with open(os.path.join(d, fn), "rb") as f:
                files[fn] = f.read()
    with open(os.path.join(d, "stdout.txt"), "rb") as f:
        return files, f.read()


def restated(name, src, n=None, quiet=False):
    """the restatement's files of a recorded case's inputs, as bytes under the names the program gives them"""
    d, a = case_args(name)
    files, stdout, r = sim.run_program(os.path.join(d, "ref"), os.path.join(d, "sim.model"), os.path.join(d, "sim.results"), float(a[3]), int(a[4]) if n is None else n, src, quiet)
    return {"out" + k: v.encode("latin-1") for k, v in files.items()}, stdout.encode(), r


def seed_of(name):
    return int(case_args(name)[1][7])


# ---- hand-made models ----------------------------------------------------------------------------------------------------------------

def _profile(rows, err=0.05):
    p = []
    for _ in range(rows):
        p.append([[(1.0 - err) if k == r else err / 4 for k in range(5)] if r < 4 else [0.2499, 0.2499, 0.2499, 0.2499, 0.0004] for r in range(5)])
    return p


def hand_model(model_type, lengths, mate_lengths=None, est_bins=None, prob_f=0.5):
    """lengths: {length: weight} of the fragment (read) length distribution; mate_lengths: the same for mates / reads"""
    def lendist(w):
        lo, hi = min(w), max(w)
        tot = float(sum(w.values()))
        return sim.LenDist(lo - 1, hi, [w.get(x, 0.0) / tot for x in range(lo, hi + 1)])

    m = {"type": model_type, "probF": prob_f, "gld": lendist(lengths), "mld": lendist(mate_lengths) if mate_lengths else None}
    m["est"] = est_bins is not None
    B = len(est_bins) if est_bins is not None else 20
    m["B"] = B
    pdf, cdf = [0.0] * (B + 2), [0.0] * (B + 2)
    for i in range(1, B + 1):
        pdf[i] = est_bins[i - 1] if est_bins is not None else 1.0 / B
        cdf[i] = cdf[i - 1] + pdf[i] if est_bins is not None else i * 1.0 / B
    m["r_pdf"], m["r_cdf"] = pdf, cdf
    if model_type in (1, 3):
        init = [0.0] * 100
        tran = [[0.0] * 100 for _ in range(100)]
        for q in (10, 20, 30, 40):
            init[q] = 0.25
            for w in (10, 20, 30, 40):
                tran[q][w] = 0.4 if w == q else 0.2
        m["p_init"], m["p_tran"] = init, tran
        m["p"] = [[[0.0] * 5 for _ in range(5)] for _ in range(100)]
        for q in (10, 20, 30, 40):
            m["p"][q] = _profile(1, 10 ** (-q / 10.0))[0]
        m["np"] = [[0.3, 0.2, 0.2, 0.2999, 0.0001] if q in (10, 20, 30, 40) else [0.0] * 5 for q in range(100)]
    else:
        m["p"] = _profile(max(lengths) if not mate_lengths else max(mate_lengths), 0.03)
        m["np"] = [0.3, 0.2, 0.2, 0.2999, 0.0001]
    return m


def transcripts(rng, lens, tails=None):
    """-> full, tot, seq (index 0 unused); tails: poly(A) letters behind transcript i"""
    full, tot, seq = [0], [0], [""]
    for i, n in enumerate(lens):
        t = (tails or [0] * len(lens))[i]
        full.append(n)
        tot.append(n + t)
        seq.append("".join(rng.choice(list("ACGTN"), size=n, p=[0.26, 0.24, 0.24, 0.25, 0.01])) + "A" * t)
    return full, tot, seq


def theta_of(weights):
    s = float(sum(weights))
    return [w / s for w in weights]


def capi_tables(t):
    """the restatement's tables as the dict capi.Simulate takes"""
    d = {"type": t["type"], "prob_f": t["probF"], "theta_cdf": t["theta_cdf"], "full_len": t["full"], "tot_len": t["tot"], "seqs": t["seq"],
         "g_lb": t["gld"].lb, "g_ub": t["gld"].ub, "g_cdf": t["gld"].cdf, "est_rspd": t["est"], "r_pdf": t["r_pdf"], "r_cdf": t["r_cdf"], "pc": t["pc"], "npc": t["npc"]}
    if t["mld"] is not None:
        d.update({"m_lb": t["mld"].lb, "m_ub": t["mld"].ub, "m_cdf": t["mld"].cdf})
    if t["type"] in (1, 3):
        d.update({"qc_init": t["qc_init"], "qc_trans": t["qc_trans"]})
    return d


def reads_of_batch(b, model_type):
    """a batch of capi.Simulate as the restatement's list of reads (without rid)"""
    fastq, paired = model_type in (1, 3), model_type >= 2
    out = []
    for i in range(len(b["sid"])):
        mates = []
        for k in range(2 if paired else 1):
            n = int(b["len%d" % (k + 1)][i])
            letters = bytes(b["seq%d" % (k + 1)][i][:n]).decode("latin-1")
            quals = bytes(b["qual%d" % (k + 1)][i][:n]).decode("latin-1") if fastq else None
            mates.append((letters, quals))
        out.append({"sid": int(b["sid"][i]), "dir": int(b["dir"][i]), "pos": int(b["pos"][i]), "insertL": int(b["insert_l"][i]), "mates": mates,
                    "attempts": int(b["attempts"][i])})
    return out


def strip(reads):
    return [{k: v for k, v in r.items() if k != "rid"} for r in reads]


def chi_square(counts, theta, n):
    """Pearson's statistic of counts against n theta over the cells with theta > 0 -> (statistic, degrees of freedom)"""
    x, df = 0.0, -1
    for c, t in zip(counts, theta):
        if t > 0.0:
            x += (c - n * t) ** 2 / (n * t)
            df += 1
        else:
            assert c == 0
    return x, df

