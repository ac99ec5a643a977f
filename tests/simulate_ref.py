"""A plain restatement of rsem-simulate-reads: the draw program of one attempt (SingleModel.h:413-452, SingleQModel.h:428-471,
PairedEndModel.h:372-415, PairedEndQModel.h:386-433 with simul.h:17-35, Orientation.h:36, LenDist.h:255-263, RSPD.h:182-198,
QualDist.h:116-145, Profile.h:163-214, QProfile.h:151-202, NoiseProfile.h:137-153, NoiseQProfile.h:153-175), the loop around it
(simulation.cpp:86-130) and the files it writes (WriteResults.h:481-635), with a pluggable source of uniforms:

    Mt19937Source(seed)     ONE stream for the whole run, boost::random::mt19937 as simul.h:11 seeds it: the reference's own draws;
    PhiloxSource(seed)      uniform k of attempt a of read r is word k % 4 of Philox4x32-10 (tests/sampler_ref.py) keyed
                            (seed low, seed high) at counter (r low, r high, a, k / 4): the program's --sim-stream counter.

Every uniform is a 32-bit word times 2^-32.  Written from the algorithm, read by read, with Python floats (IEEE doubles: the same bits
as the reference where the order of operations is kept, which it is).  Nothing here is fast and nothing needs to be."""
import os

import numpy as np

import sampler_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulate")
Q, NCODES = 100, 5
EPS = 1e-300
MINEEL = 1.0
TWO32 = 1.0 / 4294967296.0
ATTEMPT_CAP = 1 << 20
BASE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
LETTER = "ACGTN"


# ---- sources of uniforms -----------------------------------------------------------------------------------------------------------

def mt19937_words(seed):
    """the outputs of boost::random::mt19937(seed), 624 at a time"""
    mt = np.zeros(624, np.uint64)
    mt[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        mt[i] = (1812433253 * (int(mt[i - 1]) ^ (int(mt[i - 1]) >> 30)) + i) & 0xFFFFFFFF
    mt = [int(x) for x in mt]
    while True:
        for k in range(624):
            y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
            mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        for y in mt:
            y ^= y >> 11
            y ^= (y << 7) & 0x9D2C5680
            y ^= (y << 15) & 0xEFC60000
            y ^= y >> 18
            yield y


class Mt19937Source:
    """one stream for the run: an attempt begins where the attempt before it ended"""

    def __init__(self, seed):
        self.gen = mt19937_words(seed)
        self.words = 0      # words taken so far
        self.k = 0          # ... by the current attempt

    def begin(self, read, attempt):
        self.k = 0

    def next(self):
        self.words += 1
        self.k += 1
        return next(self.gen) * TWO32


class WordsSource:
    """the uniforms of a given list of words (tests that place a tie or a zero row at a chosen draw)"""

    def __init__(self, words):
        self.list = list(words)
        self.words = 0
        self.k = 0

    def begin(self, read, attempt):
        self.k = 0

    def next(self):
        w = self.list[self.words]
        self.words += 1
        self.k += 1
        return w * TWO32


class PhiloxSource:
    def __init__(self, seed):
        self.k0, self.k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
        self.k = 0
        self.buf = []

    def begin(self, read, attempt):
        self.c = (read & 0xFFFFFFFF, (read >> 32) & 0xFFFFFFFF, attempt)
        self.k = 0
        self.buf = []

    def next(self):
        if self.k >= len(self.buf):
            b0 = len(self.buf) // 4
            w = sr.philox4x32_10(self.k0, self.k1, self.c[0], self.c[1], self.c[2], np.arange(b0, b0 + 64))
            self.buf += [int(x) for x in np.stack(w, axis=1).reshape(-1)]
        u = self.buf[self.k] * TWO32
        self.k += 1
        return u


# ---- input files --------------------------------------------------------------------------------------------------------------------

def load_refs(path):
    """ref.seq (RefSeq.h:108-138) -> fullLen, totLen, seq, each [M + 1] with index 0 unused"""
    full, tot, seq = [0], [0], [""]
    with open(path) as f:
        lines = f.read().split("\n")
    for i in range(0, len(lines) - 3, 4):
        a, b = lines[i].split()
        full.append(int(a))
        tot.append(int(b))
        seq.append(lines[i + 2])
    return full, tot, seq


def load_transcripts(path):
    """ref.ti (Transcripts.h:81-94, Transcript.h:119-148) -> [(transcript_id, gene_id, seqname, length)], index 0 unused"""
    with open(path) as f:
        lines = f.read().split("\n")
    M = int(lines[0].split()[0])
    out = [None]
    for i in range(M):
        rec = lines[1 + 6 * i: 7 + 6 * i]
        out.append((rec[0].split("\t")[0], rec[1].split("\t")[0], rec[2], int(rec[3].split()[1])))
    return out


def load_groups(path):
    with open(path) as f:
        return [int(x) for x in f.read().split()]


class LenDist:
    def __init__(self, lb, ub, pdf):
        self.lb, self.ub, self.span = lb, ub, ub - lb
        self.pdf = [0.0] + list(pdf)
        self.cdf = [0.0] * (self.span + 1)
        for i in range(1, self.span + 1):
            self.cdf[i] = self.cdf[i - 1] + self.pdf[i]
        self.trim()

    def trim(self):  # LenDist.h:265-294
        newlb = 1
        while newlb <= self.span and self.pdf[newlb] < EPS:
            newlb += 1
        newlb -= 1
        newub = self.span
        while newub > newlb and self.pdf[newub] < EPS:
            newub -= 1
        assert newlb < newub
        if newlb == 0 and newub == self.span:
            return
        span = newub - newlb
        self.pdf = [0.0] + [self.pdf[i + newlb] for i in range(1, span + 1)]
        self.cdf = [0.0] + [self.cdf[i + newlb] for i in range(1, span + 1)]
        self.span = span
        self.lb += newlb
        self.ub = self.lb + span


def load_model(path):
    """the .model file (model_file_description.txt; the read() members of the four models) -> dict"""
    with open(path) as f:
        tok = f.read().split()
    p = [0]

    def nxt(n, conv=float):
        v = [conv(x) for x in tok[p[0]:p[0] + n]]
        p[0] += n
        return v

    def lendist():
        lb, ub, span = nxt(3, int)
        return LenDist(lb, ub, nxt(span))

    m = {"type": nxt(1, int)[0], "probF": nxt(1)[0]}
    m["gld"] = lendist()
    if m["type"] < 2:
        m["mld"] = lendist() if nxt(1, int)[0] > 0 else None
    else:
        m["mld"] = lendist()
    m["est"] = nxt(1, int)[0] != 0
    m["B"] = nxt(1, int)[0] if m["est"] else 20
    B = m["B"]
    pdf = [0.0] * (B + 2)
    cdf = [0.0] * (B + 2)
    vals = nxt(B) if m["est"] else [1.0 / B] * B
    for i in range(1, B + 1):
        pdf[i] = vals[i - 1]
        cdf[i] = cdf[i - 1] + pdf[i] if m["est"] else i * 1.0 / B
    m["r_pdf"], m["r_cdf"] = pdf, cdf
    if m["type"] in (1, 3):
        assert nxt(1, int)[0] == Q
        m["p_init"] = nxt(Q)
        m["p_tran"] = [nxt(Q) for _ in range(Q)]
        assert nxt(2, int) == [Q, NCODES]
        m["p"] = [[nxt(NCODES) for _ in range(NCODES)] for _ in range(Q)]
        assert nxt(2, int) == [Q, NCODES]
        m["np"] = [nxt(NCODES) for _ in range(Q)]
    else:
        L, nc = nxt(2, int)
        assert nc == NCODES
        m["p"] = [[nxt(NCODES) for _ in range(NCODES)] for _ in range(L)]
        assert nxt(1, int)[0] == NCODES
        m["np"] = nxt(NCODES)
    return m


# ---- startSimulation: the running sums --------------------------------------------------------------------------------------------

def running(v):
    out = list(v)
    for i in range(1, len(out)):
        out[i] += out[i - 1]
    return out


def repaired_profile(p):
    """QProfile::startSimulation / Profile::startSimulation: running sums, all-zero rows replaced by the table's average behaviour"""
    pc = []
    for rows in p:
        c = [running(r) for r in rows]
        cp_sum = cp_d = cp_n = 0.0
        for j in range(NCODES - 1):
            cp_sum += c[j][NCODES - 1]
            cp_d += rows[j][j]
            cp_n += rows[j][NCODES - 1]
        if cp_sum != 0.0:
            p_d = cp_d / cp_sum
            p_n = cp_n / cp_sum
            p_o = (1.0 - p_d - p_n) / (NCODES - 2)
            for j in range(NCODES - 1):
                if c[j][NCODES - 1] > 0.0:
                    continue
                c[j] = running([p_d if k == j else (p_n if k == NCODES - 1 else p_o) for k in range(NCODES)])
            if c[NCODES - 1][NCODES - 1] == 0.0:
                p_o = (1.0 - p_n) / (NCODES - 1)
                c[NCODES - 1] = running([p_o if k < NCODES - 1 else p_n for k in range(NCODES)])
        pc.append(c)
    return pc


def build_tables(model, full, tot, seq, theta):
    """everything an attempt reads: the model after startSimulation, flat lists"""
    t = {"type": model["type"], "M": len(full) - 1, "probF": model["probF"], "full": full, "tot": tot, "seq": seq,
         "gld": model["gld"], "mld": model["mld"], "est": model["est"], "B": model["B"], "r_pdf": model["r_pdf"], "r_cdf": model["r_cdf"]}
    t["theta_cdf"] = running(theta)
    if model["type"] in (1, 3):
        t["qc_init"] = running(model["p_init"])
        t["qc_trans"] = [running(r) for r in model["p_tran"]]
        t["pc"] = repaired_profile(model["p"])
        npc = []
        for r in model["np"]:
            c = running(r)
            if abs(c[NCODES - 1]) < 1e-8:
                c = [0.25, 0.5, 0.75, 1.0, 1.0]
            npc.append(c)
        t["npc"] = npc
    else:
        t["pc"] = repaired_profile(model["p"])
        t["npc"] = running(model["np"])
    return t


# ---- one attempt ---------------------------------------------------------------------------------------------------------------------

class Undefined(Exception):
    """where the reference runs into undefined behaviour (the program stops with a message of its own)"""


def sample(src, at, n):
    prb = src.next() * at(n - 1)
    lo, hi = 0, n - 1
    while lo <= hi:
        mid = (lo + hi) // 2
        if at(mid) <= prb:
            lo = mid + 1
        else:
            hi = mid - 1
    if lo >= n:
        lo = int(src.next() * n)
    return lo


def sample_list(src, arr, n=None):
    return sample(src, arr.__getitem__, len(arr) if n is None else n)


def draw_length(src, d, ref_l):
    if ref_l == -1:
        ref_l = d.ub
    if ref_l <= d.lb:
        return -1
    dlen = min(d.ub, ref_l) - d.lb
    if d.cdf[dlen] <= 0.0:
        return -1
    return d.lb + 1 + sample(src, lambda i: d.cdf[1 + i], dlen)


def eval_cdf(t, fpos, full):
    i = fpos * t["B"] // full
    val = fpos * 1.0 / full * t["B"]
    return t["r_cdf"][i] + (val - i) * t["r_pdf"][i + 1]


def ref_code(t, sid, pos, d):
    s = t["seq"][sid]
    if d == 0:
        return BASE.get(s[pos].upper(), 4)
    c = BASE.get(s[t["tot"][sid] - pos - 1].upper(), 4)
    return 4 if c == 4 else 3 - c


def draw_mate(t, src, sid, n, pos, d):
    """-> (letters, qualities or None)"""
    if t["type"] in (1, 3):
        qv = []
        for i in range(n):
            qv.append(sample_list(src, t["qc_init"]) if i == 0 else sample_list(src, t["qc_trans"][qv[-1]]))
            if qv[-1] > 93:  # the reference ends at the assertion of c2q (QProfile.h:40)
                raise Undefined("a quality of %d" % qv[-1])
        letters = []
        for i in range(n):
            row = t["npc"][qv[i]] if sid == 0 else t["pc"][qv[i]][ref_code(t, sid, i + pos, d)]
            letters.append(LETTER[sample_list(src, row)])
        return "".join(letters), "".join(chr(v + 33) for v in qv)
    if sid != 0 and n > len(t["pc"]):
        raise Undefined("a read of %d bases, a profile of %d positions" % (n, len(t["pc"])))
    letters = []
    for i in range(n):
        row = t["npc"] if sid == 0 else t["pc"][i][ref_code(t, sid, i + pos, d)]
        letters.append(LETTER[sample_list(src, row)])
    return "".join(letters), None


def attempt(t, src):
    """-> None (the attempt failed) or dict(sid, dir, pos, insertL, mates=[(letters, qualities)])"""
    paired = t["type"] >= 2
    gld, mld = t["gld"], t["mld"]
    sid = sample_list(src, t["theta_cdf"])
    d = pos = insert = 0
    if sid == 0:
        mates = []
        for _ in range(2 if paired else 1):
            n = draw_length(src, mld if mld is not None else gld, -1)
            mates.append(draw_mate(t, src, 0, n, 0, 0))
        return {"sid": 0, "dir": 0, "pos": 0, "insertL": 0, "mates": mates}
    tot, full = t["tot"][sid], t["full"][sid]
    d = 0 if src.next() < t["probF"] else 1
    frag = draw_length(src, gld, tot)
    if frag < 0:
        return None
    eff = min(full, tot - frag + 1)
    if t["est"]:
        if not eval_cdf(t, eff, full) > 0.0:
            return None
        pos = sample(src, lambda j: eval_cdf(t, j + 1, full), eff)
    else:
        pos = int(src.next() * eff)
    if d > 0:
        pos = tot - pos - frag
    if paired:
        n1 = draw_length(src, mld, frag)
        if n1 < 0:
            raise Undefined("an insert of %d, shorter than every mate length" % frag)
        m1 = draw_mate(t, src, sid, n1, pos, d)
        n2 = draw_length(src, mld, frag)
        m2 = draw_mate(t, src, sid, n2, tot - pos - frag, 1 - d)
        return {"sid": sid, "dir": d, "pos": pos, "insertL": frag, "mates": [m1, m2]}
    n = frag
    if mld is not None:
        n = draw_length(src, mld, frag)
        if n < 0:
            return None
    return {"sid": sid, "dir": d, "pos": pos, "insertL": 0, "mates": [draw_mate(t, src, sid, n, pos, d)]}


def simulate(t, src, N, first_read=0, cap=ATTEMPT_CAP):
    """simulation.cpp:121-126 -> (reads, counts[M + 1], resimulations); reads[i]["attempts"]: the failed attempts before it"""
    reads, counts, resim = [], [0] * (t["M"] + 1), 0
    for i in range(first_read, first_read + N):
        failed = 0
        while True:
            src.begin(i, failed)
            r = attempt(t, src)
            if r is not None:
                break
            failed += 1
            if failed >= cap:
                raise RuntimeError("read %d failed %d attempts" % (i, failed))
        r["rid"], r["attempts"] = i, failed
        resim += failed
        counts[r["sid"]] += 1
        reads.append(r)
    return reads, counts, resim


# ---- the files ---------------------------------------------------------------------------------------------------------------------

def read_files(model_type, reads):
    """{suffix: text} of the read files (simulation.cpp:60-84; the write() members of the four read classes)"""
    fastq, paired = model_type in (1, 3), model_type >= 2
    ext = ".fq" if fastq else ".fa"
    out = {("_%d%s" % (k + 1, ext) if paired else ext): [] for k in range(2 if paired else 1)}
    for r in reads:
        name = "%d_%d_%d_%d" % (r["rid"], r["dir"], r["sid"], r["pos"]) + ("_%d" % r["insertL"] if paired else "")
        for k, (letters, quals) in enumerate(r["mates"]):
            nm = name + ("/%d" % (k + 1) if paired else "")
            key = "_%d%s" % (k + 1, ext) if paired else ext
            out[key].append("@%s\n%s\n+\n%s\n" % (nm, letters, quals) if fastq else ">%s\n%s\n" % (nm, letters))
    return {k: "".join(v) for k, v in out.items()}


def calc_eel(gld, full, tot):
    """calcExpectedEffectiveLengths (WriteResults.h:24-53)"""
    clen = [0.0] * (gld.span + 1)
    for i in range(1, gld.span + 1):
        clen[i] = clen[i - 1] + gld.pdf[i] * (gld.lb + i)
    eel = [0.0] * len(full)
    for i in range(1, len(full)):
        pos1 = max(min(tot[i] - full[i] + 1, gld.ub) - gld.lb, 0)
        pos2 = max(min(tot[i], gld.ub) - gld.lb, 0)
        if pos2 == 0:
            continue
        eel[i] = full[i] * gld.cdf[pos1] + ((gld.cdf[pos2] - gld.cdf[pos1]) * (tot[i] + 1) - (clen[pos2] - clen[pos1]))
        if eel[i] < MINEEL:
            eel[i] = 0.0
    return eel


def theta_from_results(path, M, eel, theta0, allele):
    """simulation.cpp:97-115: the TPM column (atof) times eel, scaled to 1 - theta0"""
    col = 6 if allele else 5
    theta = [0.0] * (M + 1)
    theta[0] = theta0
    with open(path) as f:
        lines = f.read().split("\n")
    denom = 0.0
    for i in range(1, M + 1):
        theta[i] = float(lines[i].split("\t")[col]) * eel[i]
        denom += theta[i]
    assert denom > EPS
    for i in range(1, M + 1):
        theta[i] = theta[i] / denom * (1.0 - theta[0])
    return theta


def calc_expression(M, theta, eel):
    """calcExpressionValues (WriteResults.h:77-104)"""
    frac = [0.0] * (M + 1)
    denom = 0.0
    for i in range(1, M + 1):
        if eel[i] >= EPS:
            frac[i] = theta[i]
            denom += frac[i]
    if denom < EPS:
        denom = 1.0
    fpkm, tpm = [0.0] * (M + 1), [0.0] * (M + 1)
    for i in range(1, M + 1):
        frac[i] /= denom
        if eel[i] >= EPS:
            fpkm[i] = frac[i] * 1e9 / eel[i]
    denom = 0.0
    for i in range(1, M + 1):
        denom += fpkm[i]
    if denom < EPS:
        denom = 1.0
    for i in range(1, M + 1):
        tpm[i] = fpkm[i] / denom * 1e6
    return tpm, fpkm


def _roll_up(starts, counts, tpm, fpkm, lens, eel):
    n = len(starts) - 1
    out = {k: [0.0] * n for k in ("counts", "tpm", "fpkm", "len", "eel")}
    pct = [0.0] * len(counts)
    for i in range(n):
        b, e = starts[i], starts[i + 1]
        for j in range(b, e):
            out["counts"][i] += counts[j]
            out["tpm"][i] += tpm[j]
            out["fpkm"][i] += fpkm[j]
        if out["tpm"][i] < EPS:
            frac = 1.0 / (e - b)
            for j in range(b, e):
                out["len"][i] += lens[j] * frac
                out["eel"][i] += eel[j] * frac
        else:
            for j in range(b, e):
                pct[j] = tpm[j] / out["tpm"][i]
                out["len"][i] += lens[j] * pct[j]
                out["eel"][i] += eel[j] * pct[j]
    return out, pct


def result_files(ref_name, transcripts, eel, counts):
    """writeResultsSimulation (WriteResults.h:481-635) -> {suffix: text}"""
    M = len(transcripts) - 1
    gi = load_groups(ref_name + ".grp")
    allele = os.path.exists(ref_name + ".gt") and os.path.exists(ref_name + ".ta")
    counts = [float(c) for c in counts]
    tpm, fpkm = calc_expression(M, counts, eel)
    tlens = [0] + [transcripts[i][3] for i in range(1, M + 1)]
    G, isopct = _roll_up(gi, counts, tpm, fpkm, tlens, eel)
    out = {}
    if allele:
        gt, ta = load_groups(ref_name + ".gt"), load_groups(ref_name + ".ta")
        A, ta_pct = _roll_up(ta, counts, tpm, fpkm, tlens, eel)
        gt_pct = [0.0] * (len(ta) - 1)
        for i in range(len(gi) - 1):
            if G["tpm"][i] >= EPS:
                for j in range(gt[i], gt[i + 1]):
                    gt_pct[j] = A["tpm"][j] / G["tpm"][i]
        rows = ["allele_id\ttranscript_id\tgene_id\tlength\teffective_length\tcount\tTPM\tFPKM\tAlleleIsoPct\tAlleleGenePct\n"]
        for i in range(1, M + 1):
            tid, gid, seqname, _ = transcripts[i]
            rows.append("%s\t%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n" % (seqname, tid, gid, tlens[i], eel[i], counts[i], tpm[i], fpkm[i], ta_pct[i] * 1e2,
                                                                                isopct[i] * 1e2))
        out[".sim.alleles.results"] = "".join(rows)
    rows = ["transcript_id\tgene_id\tlength\teffective_length\tcount\tTPM\tFPKM\tIsoPct\n"]
    if not allele:
        for i in range(1, M + 1):
            rows.append("%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n" % (transcripts[i][0], transcripts[i][1], tlens[i], eel[i], counts[i], tpm[i], fpkm[i], isopct[i] * 1e2))
    else:
        for i in range(len(ta) - 1):
            tr = transcripts[ta[i]]
            rows.append("%s\t%s\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n" % (tr[0], tr[1], A["len"][i], A["eel"][i], A["counts"][i], A["tpm"][i], A["fpkm"][i], gt_pct[i] * 1e2))
    out[".sim.isoforms.results"] = "".join(rows)
    rows = ["gene_id\ttranscript_id(s)\tlength\teffective_length\tcount\tTPM\tFPKM\n"]
    for i in range(len(gi) - 1):
        b, e = gi[i], gi[i + 1]
        tids = []
        for j in range(b, e):
            if not tids or tids[-1] != transcripts[j][0]:
                tids.append(transcripts[j][0])
        rows.append("%s\t%s\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n" % (transcripts[b][1], ",".join(tids), G["len"][i], G["eel"][i], G["counts"][i], G["tpm"][i], G["fpkm"][i]))
    out[".sim.genes.results"] = "".join(rows)
    return out


def run_program(ref_name, model_path, results_path, theta0, N, src, quiet=True):
    """the whole program -> ({suffix: text} of every file it writes, stdout text, tables)"""
    full, tot, seq = load_refs(ref_name + ".seq")
    M = len(full) - 1
    transcripts = load_transcripts(ref_name + ".ti")
    model = load_model(model_path)
    allele = os.path.exists(ref_name + ".gt") and os.path.exists(ref_name + ".ta")
    eel = calc_eel(model["gld"], full, tot)
    theta = theta_from_results(results_path, M, eel, theta0, allele)
    t = build_tables(model, full, tot, seq, theta)
    reads, counts, resim = simulate(t, src, N)
    files = read_files(model["type"], reads)
    files.update(result_files(ref_name, transcripts, eel, counts))
    # (Refs.h's loadRefs reports, simulation.cpp:125 counts the millions: both only without -q)
    stdout = "" if quiet else "Refs.loadRefs finished!\n" + "".join("GEN %d\n" % n for n in range(1000000, N + 1, 1000000))
    stdout += "Total number of resimulation is %d\n" % resim
    return files, stdout, {"tables": t, "reads": reads, "counts": counts, "resim": resim, "theta": theta, "eel": eel}


def dump(reads, counts, resim):
    """the text tests/simulate_emu.cpp writes: a line per read, the counts, the failed attempts"""
    out = []
    for i, r in enumerate(reads):
        m = r["mates"] + [("", None)] * (2 - len(r["mates"]))
        cells = [m[0][0] or "-", m[0][1] or "-", m[1][0] or "-", m[1][1] or "-"]
        out.append("%d %d %d %d %d %d %s\n" % (i, r["dir"], r["sid"], r["pos"], r["insertL"], r["attempts"], " ".join(cells)))
    out.append("counts " + " ".join(str(c) for c in counts) + "\n")
    out.append("resim %d\n" % resim)
    return "".join(out)
