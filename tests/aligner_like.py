"""Inputs as an aligner writes them: a read may hit one transcript at several positions, and its alignments come in the aligner's
own order.  Every generator of this suite gives a read distinct, ascending transcript ids; aligner_like() takes such a CSR and
moves ids only (row_ptr, lengths and values stay): per read one of

  repeat     some entries take the id of another entry of the same read -- half of the time an entry of the same value plane
             (another lane of the read) or of the same lane (another plane), as the sliced layout places entry c of a read of
             G = 2^lg lanes in plane c >> lg, lane c & (G - 1) (rsem_amd/csrc/sell_shape.hpp);
  all_same   every entry takes the id of one of them (the first read of every shape 1..256, L = 2 and 3 among them, and one
             read in ten after that);
  order      the read's ids reversed or permuted.  The values of these inputs are drawn independently of the ids, so permuting
             the ids under the values is the CSR of the permuted alignments; the oracle is given the same arrays;

or repeat followed by order, or nothing.  `keep`: entry indices that are never overwritten (they may still move within an
order step: the read's set of ids is what the layout's groupings depend on); all_same on a read with kept entries gives the
others the smallest kept id.  `first_fixed`: entry 0 of every read stays where
and what it is, and is never copied (the noise item of the Gibbs items, id 0).

describe() counts, from the arrays alone, how many reads carry each feature; the tests assert on these counts before a kernel
runs.  No project imports: the few layout rules needed are restated here."""
import numpy as np

WINDOW = 2048          # ids per LDS window (sell_layout.hpp kLayoutWindow)
ANCHOR_REACH = 1024
MEDIAN_EXACT_MAX = 64


def lg_of_len(L):
    """log2(lanes per read) of a read of L alignments (sell_layout.hpp shape_id_of); 7: longer than any shape (stays in the CSR)."""
    if L <= 4:
        return 0
    lg, cap = 1, 8
    while L > cap:
        cap, lg = cap * 2, lg + 1
    return lg


def shape_of_len(L):
    lg = lg_of_len(L)
    return (lg, L if lg == 0 else -(-L // (1 << lg)))


def anchor_of(ids):
    """The id a read's LDS window starts at (sell_layout.hpp row_key_of): the smallest id within ANCHOR_REACH below the median."""
    L = len(ids)
    if L == 1:
        return int(ids[0])
    med = int(np.sort(ids)[L // 2]) if L <= MEDIAN_EXACT_MAX else int(ids[L // 2])
    near = ids[(ids >= med - ANCHOR_REACH) & (ids <= med)]
    return int(near.min())


def aligner_like(row_ptr, sid, seed, keep=None, first_fixed=False):
    rp = np.asarray(row_ptr).astype(np.int64)
    out = np.array(sid, copy=True)
    kept = np.zeros(len(out), bool)
    if keep is not None:
        kept[np.asarray(keep, np.int64)] = True
    rng = np.random.default_rng(seed)
    lo = 1 if first_fixed else 0
    shapes_done = set()
    for i in range(len(rp) - 1):
        fr, L = int(rp[i]), int(rp[i + 1] - rp[i])
        if L - lo < 2:
            continue
        ids = out[fr:fr + L]                       # (a view)
        free = np.flatnonzero(~kept[fr + lo:fr + L]) + lo
        u = rng.random()
        shape = shape_of_len(L)
        if shape not in shapes_done and len(free) == L - lo:
            shapes_done.add(shape)
            u = 0.35                               # all_same
        if u < 0.30 or 0.70 <= u < 0.85:           # repeat
            lg = min(lg_of_len(L), 6)
            G = 1 << lg
            orig = ids.copy()
            n = int(rng.integers(1, max(1, L // 4) + 1))
            for t in rng.permutation(free)[:n]:
                cand = np.arange(lo, L)
                v = rng.random()
                if v < 0.3:
                    c = cand[(cand >> lg) == (t >> lg)]
                elif v < 0.6:
                    c = cand[(cand & (G - 1)) == (t & (G - 1))]
                else:
                    c = cand
                c = c[c != t]
                if len(c) == 0:
                    c = cand[cand != t]
                ids[t] = orig[rng.choice(c)]
        elif u < 0.40:                             # all_same
            src = lo + int(rng.integers(0, L - lo))
            if len(free) < L - lo:                 # (the kept entry of the smallest id gives it: the read's median and anchor stay)
                k = np.setdiff1d(np.arange(lo, L), free)
                src = int(k[np.argmin(ids[k])])
            ids[free] = ids[src]
        if 0.40 <= u < 0.55:                       # order: reversed
            ids[lo:] = ids[lo:][::-1].copy()
        elif 0.55 <= u < 0.85:                     # order: permuted
            ids[lo:] = ids[lo:][rng.permutation(L - lo)]
    return out


def describe(row_ptr, sid, lg_of_len=lg_of_len, first_fixed=False, window=WINDOW):
    """-> counts of reads: reads, multi (two alignments or more), repeat, all_same, not_ascending, same_plane (a repeated id in two
    lanes of one value plane), same_lane (in two planes of one lane), far_repeat (a repeated id outside [anchor, anchor + window))."""
    rp = np.asarray(row_ptr).astype(np.int64)
    sid = np.asarray(sid).astype(np.int64)
    lo = 1 if first_fixed else 0
    d = dict(reads=len(rp) - 1, multi=0, repeat=0, all_same=0, not_ascending=0, same_plane=0, same_lane=0, far_repeat=0)
    for i in range(len(rp) - 1):
        ids = sid[rp[i] + lo:rp[i + 1]]
        L = len(ids)
        if L < 2:
            continue
        d["multi"] += 1
        d["not_ascending"] += bool(np.any(ids[1:] < ids[:-1]))
        vals, cnt = np.unique(ids, return_counts=True)
        if len(vals) == L:
            continue
        d["repeat"] += 1
        d["all_same"] += len(vals) == 1
        lg = min(lg_of_len(L + lo), 6)
        c = np.arange(lo, L + lo)
        d["same_plane"] += len(np.unique(ids * 4096 + (c >> lg))) < L
        d["same_lane"] += len(np.unique(ids * 4096 + (c & ((1 << lg) - 1)))) < L
        a = anchor_of(ids)
        rep = vals[cnt > 1]
        d["far_repeat"] += bool(np.any((rep < a) | (rep >= a + window)))
    return d


def assert_on_path(d, of="multi", **shares):
    """Prints the counts; every named count is at least its share (0.05 = 5 %) of the reads counted under `of`."""
    print("aligner_like:", " ".join("%s=%d" % kv for kv in d.items()))
    for k, share in shares.items():
        assert d[k] >= share * d[of], (k, d[k], share, d[of])
