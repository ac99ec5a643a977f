"""The table of generated inputs that put the model-round kernel (k_model_group, rsem_amd/csrc/model_block.hpp) on each of its
paths, and the conditions that prove it from the files themselves.  Shared by tests/test_model_paths_gpu.py (reference binary
against the drop-in on the GPU) and tests/test_model_paths_cpu.py (every case generates, meets its conditions and is accepted
by the reference binary).

Paths (model_block.hpp):
  1  reads with more than 16 alignments: several 16-alignment chunks, runs of equal windows carried across a chunk boundary;
  2  reads (mates) longer than 128 positions: a lane's second 8-position share (wi = g + 16);
  3  models without qualities and positions >= 204 (profile counts beyond kProfLds go to global atomics), fragment-length
     table indices >= kGldLds = 1024 (likewise);
  4  plane output for reads of 17..256 alignments, CSR only for reads with more than 256;
  5  reads of different lengths side by side, N bases, low-quality reads (shorter than the seed length 25), probF 0 / 1, RSPD
     estimation, a mate-length distribution, omitted transcripts;
  6  reads as an aligner reports them (the repeat_ cases; gen_temp --near-repeat / --shuffle-alignments): a transcript hit at two
     positions by one read, on equal bases or on bases that differ in a few places, alignments in any order -- runs of equal
     windows (same_prev) between two alignments of ONE transcript, runs that are interrupted and resume, a second hit as the
     first alignment of a chunk.

Every case: positional arguments of tools/gen_temp.cpp (reads, M, read type, read_len, isoforms per gene) + named options.
20 000 reads each (19 000 alignable): the reference binary finishes a case in 5-20 s with -p 4 (over_256, 271 alignments per
read and an EM that runs into the limit of 10 000 rounds: -p 16).
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_temp")
REF_EM = os.path.join(ROOT, "oracle", "_ref", "rsem-run-em")
REF_IDX = os.path.join(ROOT, "oracle", "_ref", "rsem-build-read-index")
SEED_LEN = 25      # s.mparams line 7
THREADS = 4        # -p of both programs, as test_generated_dataset_vs_reference_binary
K_GRP, K_POS, K_NOQ_POS, K_GLD_LDS, K_PLANE_MAX = 16, 128, 204, 1024, 256  # kGrp, 16 lanes x 8 positions, kProfLds / 25, kGldLds, sell_layout

CASES = {
    # path 1 (+ 4): chunks of 16 alignments, both a quality paired-end model and the model without qualities
    "chunks_pe_q": dict(rt=3, n=20000, M=2000, L=75, iso="17-40", opts=[], planes0=True),
    "chunks_se_noq": dict(rt=0, n=20000, M=2000, L=75, iso="17-40", opts=[], planes0=True),
    # path 2: the second positional pass (paired-end mates <= 150: 0.25^(len1 + len2) stays a normal double)
    "two_pass_se_q": dict(rt=1, n=20000, M=2000, L=250, iso="2-9", opts=["--len", "130-250"], planes0=False),
    "two_pass_pe_q": dict(rt=3, n=20000, M=2000, L=150, iso="2-9", opts=["--len", "120-150", "--pe-frag", "300,50,600"], planes0=False),
    # path 3 (+ 2): positions >= 204 of the models without qualities
    "noq_long_se": dict(rt=0, n=20000, M=2000, L=250, iso="2-9", opts=["--len", "150-250"], planes0=False),
    "noq_long_pe": dict(rt=2, n=20000, M=2000, L=230, iso="2-9", opts=["--len", "150-230", "--pe-frag", "400,60,800"], planes0=False),
    # paths 1 + 2 + 5 at once: chunks, second pass, variable lengths in one wave, N bases, low-quality reads
    "chunks_two_pass_se_q": dict(rt=1, n=20000, M=2000, L=250, iso="17-40", opts=["--len", "20-250", "--n-rate", "0.01"], planes0=True),
    "chunks_two_pass_pe_noq": dict(rt=2, n=20000, M=2000, L=150, iso="17-40",
                                   opts=["--len", "20-150", "--n-rate", "0.01", "--pe-frag", "300,60,600"], planes0=True),
    # path 3: fragment-length counts beyond the LDS table, with a lower bound of the table that is not 0
    "wide_gld": dict(rt=3, n=20000, M=1000, L=75, iso="2-9",
                     opts=["--gene-len", "3000-5000", "--frag-range", "50-1500", "--pe-frag", "900,250,1500"], planes0=False),
    # path 4: reads that stay in the CSR
    # (271 alignments per read and an EM that runs to the round limit: -p 16 keeps the reference under a minute)
    "over_256": dict(rt=1, n=20000, M=840, L=75, iso="260-300", opts=[], planes0=True, threads=16),
    # path 5 with path 1: one strand only, RSPD estimation, omitted transcripts
    "stranded_rev_rspd_omit": dict(rt=0, n=20000, M=2000, L=75, iso="17-40", opts=["--probF", "0", "--est-rspd", "1", "--omit", "60"], planes0=True),
    "stranded_fwd_rspd_omit": dict(rt=3, n=20000, M=2000, L=75, iso="17-40", opts=["--probF", "1", "--est-rspd", "1", "--omit", "60"], planes0=True),
    # single-end reads with a fragment length distribution (the loop over fragment lengths and a mate-length table), with path 1
    "se_mld": dict(rt=1, n=20000, M=2000, L=100, iso="17-40", opts=["--len", "50-100", "--se-frag", "180,40", "--frag-range", "1-300"], planes0=True),
    # path 6.  Short genes and reads of 50 bases: one fragment in five lies inside one copy of its gene's 200-base repeat.
    # expect: the least share of the reads with each feature (assert_path / assert_path_ofg); at_chunk: a second hit at entry 16 or 32
    "repeat_se_q": dict(rt=1, n=20000, M=2000, L=50, iso="2-9", opts=["--gene-len", "1500-2000", "--near-repeat", "200:0.02", "--shuffle-alignments"],
                        planes0=False, expect=dict(repeat=0.05, not_ascending=0.05, resumed=0.01)),
    "repeat_pe": dict(rt=3, n=20000, M=2000, L=50, iso="2-9", opts=["--gene-len", "1500-2000", "--pe-frag", "120,20,200", "--near-repeat", "200:0"],
                      planes0=False, expect=dict(repeat=0.05)),
    "repeat_long": dict(rt=1, n=20000, M=2000, L=50, iso="17-40", opts=["--gene-len", "1500-2000", "--near-repeat", "200:0.02", "--shuffle-alignments"],
                        planes0=True, expect=dict(repeat=0.05, not_ascending=0.05, resumed=0.01, at_chunk=True)),
}


def have_tools(need_ref=True):
    return os.path.exists(GEN) and (not need_ref or (os.path.exists(REF_EM) and os.path.exists(REF_IDX)))


def run(cmd, timeout, env=None):
    """One subprocess under its own time limit -> its stdout (stderr apart: a warning written there -- the round limit's -- would land
    in the middle of a buffered ROUND line)."""
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def opt(case, name, default=None):
    o = case["opts"]
    return o[o.index(name) + 1] if name in o else default


def read_files(case):
    rt = case["rt"]
    ext = ".fq" if rt in (1, 3) else ".fa"
    return ["s_alignable" + ext] if rt < 2 else ["s_alignable_1" + ext, "s_alignable_2" + ext]


def generate(case, d, threads=None):
    cmd = [GEN, d, str(case["n"]), str(case["M"]), str(case["rt"]), "7", str(case["L"]), "nosam", case["iso"]] + case["opts"]
    if threads:
        cmd += ["--threads", str(threads)]
    return run(cmd, 120)


def em_args(case, d):
    return [os.path.join(d, "ref"), str(case["rt"]), os.path.join(d, "s"), os.path.join(d, "temp", "s"), os.path.join(d, "stat", "s"),
            "-p", str(case.get("threads", THREADS)), "--gibbs-out"]


def run_reference(case, d):
    """rsem-build-read-index gap hasQ quiet files (buildReadIndex.cpp:72-84), then the reference's rsem-run-em -> its log."""
    run([REF_IDX, "32", "1" if case["rt"] in (1, 3) else "0", "1"] + [os.path.join(d, "temp", r) for r in read_files(case)], 120)
    return run([REF_EM] + em_args(case, d), 300)


def _read_lengths(path, fastq):
    """-> (length, holds an N) per read of a FASTA / FASTQ file with one line per sequence."""
    with open(path) as f:
        lines = f.read().split("\n")
    per = 4 if fastq else 2
    assert lines[-1] == "" and len(lines) % per == 1
    seqs = lines[1:-1:per]
    return np.array([len(s) for s in seqs], np.int64), np.array(["N" in s for s in seqs], bool)


def parse_inputs(case, d):
    """What the kernel will see, from s.dat (parseIt.cpp:195-199: 'N1 nHits read_type', then per read 'k (sid pos [insertL])*k')
    and the read files: alignments per read, the mates' lengths, N bases, the fragment lengths, the transcripts aligned to."""
    pe = case["rt"] >= 2
    w = 3 if pe else 2
    with open(os.path.join(d, "temp", "s.dat")) as f:
        N1, nHits, rt = [int(x) for x in f.readline().split()]
        assert rt == case["rt"]
        nal = np.zeros(N1, np.int64)
        frag = np.zeros(N1, np.int64)
        strands, sids = set(), set()
        alns = [] if "expect" in case else None   # per read: (transcript ids, positions) in file order
        for i, line in enumerate(f):
            t = line.split()
            k = int(t[0])
            assert len(t) == 1 + w * k and k >= 1
            nal[i] = k
            ids = [int(x) for x in t[1::w]]
            strands.update(x < 0 for x in ids)
            sids.update(abs(x) for x in ids)
            if pe:
                frag[i] = int(t[3])
            if alns is not None:
                alns.append((np.array(ids, np.int64), np.array(t[2::w], np.int64)))
    assert i + 1 == N1 and int(nal.sum()) == nHits
    mates = [_read_lengths(os.path.join(d, "temp", r), case["rt"] in (1, 3)) for r in read_files(case)]
    assert all(len(m[0]) == N1 for m in mates)
    lens = np.stack([m[0] for m in mates])          # [mates, N1]
    has_n = np.logical_or.reduce([m[1] for m in mates])
    with open(os.path.join(d, "temp", "s.omit")) as f:
        omit = [int(x) for x in f.read().split()]
    with open(os.path.join(d, "temp", "s.mparams")) as f:
        mparams = f.read().split()
    P = dict(N1=N1, nal=nal, lens=lens, maxlen=lens.max(0), minlen=lens.min(0), has_n=has_n, frag=frag, strands=strands, sids=sids, omit=omit,
             mparams=mparams)
    if alns is not None:
        P["aligner_like"] = _aligner_like_counts(case, d, alns, lens[0])
    return P


def _aligner_like_counts(case, d, alns, len1):
    """Reads with: a transcript hit twice (repeat); ids not ascending; a run of equal windows that is interrupted and resumes -- an
    alignment whose window holds other bases than its predecessor's and the same as the one before that (single-end: the window
    is the read's length of the transcript's strand at the position); a second hit of a transcript as entry 16 or 32 (at_chunk)."""
    with open(os.path.join(d, "ref.seq")) as f:
        lines = f.read().split("\n")
    seqs = [""] + lines[2::4][:case["M"]]            # per transcript: 'len len', name, bases, mask words
    assert len(seqs) == case["M"] + 1 and all(set(s) <= set("ACGTN") for s in seqs[1:20])
    c = dict(repeat=0, not_ascending=0, resumed=0, at_chunk=0)
    for i, (ids, pos) in enumerate(alns):
        t = np.abs(ids)
        if len(np.unique(t)) == len(t) and not np.any(t[1:] < t[:-1]):
            continue
        c["repeat"] += len(np.unique(t)) < len(t)
        c["not_ascending"] += bool(np.any(t[1:] < t[:-1]))
        c["at_chunk"] += any(len(t) > e and t[e] in t[:e] for e in (K_GRP, 2 * K_GRP))
        if case["rt"] < 2:
            n = int(len1[i])
            win = [seqs[a][p:p + n] if s > 0 else seqs[a][len(seqs[a]) - p - n:len(seqs[a]) - p] for s, a, p in zip(ids.tolist(), t.tolist(), pos.tolist())]
            assert all(len(x) == n for x in win)
            c["resumed"] += any(win[j] != win[j - 1] and win[j] == win[j - 2] for j in range(2, len(win)))
    return c


def assert_path(name, P):
    """The conditions under which a case tests what its name says.  A read is 'longer than x' when one of its mates is."""
    case = CASES[name]
    nal, maxlen, N1 = P["nal"], P["maxlen"], P["N1"]
    frac = lambda m: float(np.count_nonzero(m)) / N1
    assert N1 == case["n"] - case["n"] // 20
    assert P["mparams"][9] == str(SEED_LEN)  # minL maxL probF estRSPD B mate_minL mate_maxL mean sd seedLen
    if name.startswith("chunks_") or name.startswith("stranded_") or name == "se_mld":
        assert frac(nal > K_GRP) >= 0.20 and (nal > 2 * K_GRP).any(), (name, frac(nal > K_GRP), int(nal.max()))
        assert nal.max() <= K_PLANE_MAX  # every read has a place in the planes
    if name.startswith("two_pass_"):
        assert frac(maxlen > K_POS) >= 0.50, (name, frac(maxlen > K_POS))
    if name == "two_pass_pe_q":
        assert P["lens"].max() <= 150
    if name.startswith("noq_long_"):
        assert case["rt"] in (0, 2) and frac(maxlen > K_NOQ_POS) >= 0.05, (name, frac(maxlen > K_NOQ_POS))
    if name.startswith("chunks_two_pass_"):
        assert (P["minlen"] < SEED_LEN).any() and P["has_n"].any() and ((nal > K_GRP) & (maxlen > K_POS)).any(), name
        assert ((nal > K_GRP) & (P["minlen"] < SEED_LEN)).any() and ((nal > K_GRP) & P["has_n"]).any(), name
        # reads of different lengths side by side in one wave: 4 consecutive reads
        assert len(set(maxlen[:4].tolist())) > 1
    if name == "wide_gld":
        lb = int(P["mparams"][0]) - 1                     # LenDist(minL, maxL): lb = minL - 1, table index = len - lb
        assert lb > 0 and frac(P["frag"] - lb > K_GLD_LDS) >= 0.05, (name, frac(P["frag"] - lb > K_GLD_LDS))
        assert (P["frag"] - lb < K_GLD_LDS).any()
    if name == "over_256":
        assert frac(nal > K_PLANE_MAX) >= 0.20 and (nal <= K_PLANE_MAX).any(), (name, frac(nal > K_PLANE_MAX))
    if name.startswith("stranded_"):
        want_rev = opt(case, "--probF") == "0"
        assert P["strands"] == {want_rev}, (name, P["strands"])
        assert P["mparams"][2] == opt(case, "--probF") and P["mparams"][3] == "1"
        assert len(P["omit"]) == int(opt(case, "--omit")) and not (set(P["omit"]) & P["sids"])
    else:
        assert P["omit"] == [] and P["strands"] == {False, True}
    if name == "se_mld":
        assert float(P["mparams"][7]) > 0 and len(set(maxlen.tolist())) > 1
    else:
        assert P["mparams"][7] == "-1"
    if name.startswith("repeat_"):
        c = P["aligner_like"]
        print("aligner_like %s: of %d reads %s" % (name, N1, " ".join("%s=%d" % kv for kv in c.items())))
        for k, least in case["expect"].items():
            assert c[k] >= (1 if least is True else least * N1), (name, k, c[k], least)
        if name == "repeat_long":
            assert frac(nal > K_GRP) >= 0.20 and nal.max() <= K_PLANE_MAX, (name, frac(nal > K_GRP), int(nal.max()))


def assert_path_ofg(name, ofg):
    """... and from the reference's .ofg (M, N0, row_ptr, ids, values): among the reads with two entries of one transcript at least
    half have the two within a factor of 100 of each other -- the second hit then takes a share of the read that the model's
    statistics depend on, and a kernel that lost or doubled it would show in every table."""
    if not name.startswith("repeat_"):
        return
    _, _, rp, sid, val = ofg
    rp = rp.astype(np.int64)
    both = close = 0
    for i in range(len(rp) - 1):
        s, v = sid[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
        if len(np.unique(s)) == len(s):
            continue
        both += 1
        o = np.argsort(s, kind="stable")
        s, v = s[o], v[o]
        pair = np.flatnonzero(s[1:] == s[:-1])
        ratio = np.maximum(v[pair], v[pair + 1]) / np.minimum(v[pair], v[pair + 1])
        close += bool(np.any(ratio <= 100.0))
    print("aligner_like %s: .ofg rows with two entries of one transcript %d, of them within a factor of 100 %d" % (name, both, close))
    assert both >= 0.05 * (len(rp) - 1) and 2 * close >= both, (name, both, close)
