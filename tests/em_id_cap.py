"""Reads whose ids lie at and above the anchor cap of the sliced layout (rsem_amd/csrc/sell_layout.hpp: kKeyMinSidCap = 2^23 - 1, the
largest anchor id a read's sort key holds), for tests/test_em_id_cap_gpu.py, tests/test_gibbs_id_cap_gpu.py and the emulator tests.

row_key_of clamps an anchor above the cap to it and splits no read whose anchor lies above it; the kernels that read the anchor back
out of the key get the cap; sell_build_units gives a unit whose every id lies above cap + 2048 a window of one id at the cap, so all
its entries take the out-of-window path.  The reads come in three populations -- anchors below the cap, across it, above it -- of the
kinds of tests/test_em_units_gpu.py (compact, apart, stray, outside), a few single-alignment reads, one of 300 alignments, and reads
of 12 alignments that all lie above cap + 2048."""
import numpy as np

CAP = 2 ** 23 - 1   # kKeyMinSidCap
WINDOW = 2048       # kLayoutWindow
M = CAP + 12000

OFFS = {"compact": np.arange(16), "apart": np.concatenate([np.arange(15), [3000]]), "stray": np.concatenate([np.arange(15), [2000]]),
        "outside": np.array([0, 1, 3000, 3001]), "single": np.array([0]), "long": np.arange(300), "compact12": np.arange(12)}
# (kind, first id of the first read, id step from read to read, reads): the anchor of an `outside` read is its first id + 3000
GROUPS = [
    # below: every anchor under the cap, the control
    ("compact", CAP - 9000, 10, 128), ("apart", CAP - 7700, 10, 128), ("stray", CAP - 6400, 10, 128), ("outside", CAP - 8000, 5, 100),
    # across: anchors from cap - 1500 up to the cap itself, ids and windows over it
    ("compact", CAP - 1500, 10, 151), ("apart", CAP - 1500, 10, 151), ("stray", CAP - 1500, 10, 151), ("outside", CAP - 3100, 2, 101),
    # above: anchors inside [cap, cap + 2048), whose ids the clamped window still holds, and beyond it, where no id is inside
    ("compact", CAP + 1, 10, 300), ("apart", CAP + 1, 10, 150), ("apart", CAP + 4000, 10, 150), ("stray", CAP + 1, 10, 150), ("stray", CAP + 4000, 10, 150),
    ("outside", CAP - 2999, 5, 80), ("outside", CAP + 2000, 5, 80),
    # a shape of its own (12 alignments) with no read below cap + 4000: its units' windows start at the cap and hold none of their ids
    ("compact12", CAP + 4000, 10, 200),
    ("single", CAP - 1, 1, 3), ("single", CAP + 2047, 1, 3), ("single", CAP + 5000, 1, 1),
]
LONG = ("long", CAP - 150, 1, 1)  # ids cap - 150 .. cap + 149


def reads(with_long=True, seed=23):
    """-> dict(M, N0, row_ptr, sid, conprb, ncp, theta0, anchor, kind); values as tests/test_em_units_gpu.py makes them (every read
    takes Q32 planes with value_bits 32); the reads shuffled, so that the layout and not the input brings a kind's reads together"""
    rng = np.random.default_rng(seed)
    rows = []
    for kind, a0, step, n in GROUPS + ([LONG] if with_long else []):
        for i in range(n):
            ids = a0 + step * i + OFFS[kind]
            rows.append((kind, ids, int(ids[0]) + (3000 if kind == "outside" else 0)))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    lens = np.array([len(r[1]) for r in rows], np.int64)
    sid = np.concatenate([r[1] for r in rows])
    assert sid.min() >= 1 and sid.max() <= M
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    cp = rng.uniform(0.05, 0.2, len(sid))
    cp[rp[:-1].astype(np.int64) + rng.integers(0, 1 << 30, len(lens)) % lens] = rng.uniform(0.5, 1.0, len(lens))
    ncp = rng.uniform(0.01, 1.0, len(lens)) * 1e-5
    theta0 = np.full(M + 1, 0.95 / M)
    theta0[0] = 0.05
    return dict(M=M, N0=100, row_ptr=rp, sid=sid.astype(np.int32), conprb=cp, ncp=ncp, theta0=theta0,
                anchor=np.array([r[2] for r in rows], np.int64), kind=[r[0] for r in rows])


def expected_split_rows(d, policy):
    """the rule of row_key_of: a read splits where at least half of its ids (policy 2: any id) lie outside [anchor, anchor + 2048) AND
    its anchor is at most the cap; reads of more than 256 alignments never split.  -> (split rows, reads the cap alone keeps whole)"""
    rp = d["row_ptr"].astype(np.int64)
    split = kept_by_cap = 0
    for i, a in enumerate(d["anchor"]):
        ids = d["sid"][rp[i]:rp[i + 1]].astype(np.int64)
        if len(ids) < 2 or len(ids) > 256:
            continue
        inside = int(((ids >= a) & (ids < a + WINDOW)).sum())
        if inside < len(ids) and (policy == 2 or 2 * inside <= len(ids)):
            split += a <= CAP
            kept_by_cap += a > CAP
    return split, kept_by_cap
