"""A FASTA file of a given size whose entries share segments, for rsem-for-ebseq-calculate-clustering-info.

    python tools/gen_shared_fasta.py out.fa --entries 100000 --bases 200000000 [--seed 1] [--shared 0.5] [--width 70]

Entry lengths are log-normal around bases / entries (at least 30).  A fraction --shared of the entries is built as an "isoform":
it takes up to three segments of 150 .. 900 bases from a pool that many entries draw from, so that their k-mers occur elsewhere;
the rest of every entry is random A C G T.  Seven entries in ten end in a poly(A) tail of 30 .. 80 bases, one in fifty holds a run of
N, one in a hundred has a part in lower case.  The same arguments give the same file.
"""
import argparse

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--bases", type=int, default=30000000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shared", type=float, default=0.5)
    ap.add_argument("--width", type=int, default=70)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    mean = max(a.bases / a.entries, 30.0)
    lens = np.maximum(rng.lognormal(np.log(mean) - 0.32, 0.8, a.entries), 30).astype(np.int64)
    pool = letters[rng.integers(0, 4, max(int(a.bases * 0.05), 2000))]
    total = 0
    with open(a.out, "wb") as f:
        for t in range(a.entries):
            n = int(lens[t])
            s = letters[rng.integers(0, 4, n)]
            if rng.random() < a.shared:
                for _ in range(int(rng.integers(1, 4))):
                    m = int(min(rng.integers(150, 900), n, len(pool)))
                    src = int(rng.integers(0, len(pool) - m + 1))
                    src -= src % 50  # segments start on a grid: entries that draw from the same region share whole stretches
                    dst = int(rng.integers(0, n - m + 1))
                    s[dst:dst + m] = pool[src:src + m]
            if rng.random() < 0.7:
                s[-int(min(rng.integers(30, 80), n)):] = ord("A")
            if rng.random() < 0.02:
                m = int(min(rng.integers(10, 200), n))
                dst = int(rng.integers(0, n - m + 1))
                s[dst:dst + m] = ord("N")
            if rng.random() < 0.01:
                s[: n // 2] |= 32
            b = s.tobytes()
            f.write(b">tr%07d len=%d\n" % (t + 1, n))
            f.write(b"\n".join(b[i:i + a.width] for i in range(0, n, a.width)) + b"\n")
            total += n
    print("%s: %d entries, %d bases" % (a.out, a.entries, total))


if __name__ == "__main__":
    main()
