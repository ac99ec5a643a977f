#!/usr/bin/env python3
"""A seeded genome and GTF of a given size, for the reference-preparation programs (tests/test_refseq_gpu.py, tools/time_refprep.py).
Nothing is downloaded.

    python tools/gen_genome.py <out_dir> [--seed S] [--chromosomes N] [--bases B] [--transcripts T] [--absent F]

writes <out_dir>/genome.fa (lines of 60, upper case with lower-case runs and a few N / other IUPAC letters) and <out_dir>/genes.gtf
(genes of one to four transcripts on either strand, 1 to 12 exons each, some exons touching or overlapping, a fraction F of the
genes on a chromosome the genome does not have)."""
import argparse
import os

import numpy as np

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def write(out_dir, seed=1, n_chromosomes=3, chromosome_bases=40000, n_transcripts=200, absent_fraction=0.05):
    rng = np.random.default_rng(seed)
    os.makedirs(out_dir, exist_ok=True)
    lengths = [int(chromosome_bases * f) for f in rng.uniform(0.8, 1.2, n_chromosomes)]
    with open(os.path.join(out_dir, "genome.fa"), "wb") as f:
        for c, n in enumerate(lengths):
            seq = LETTERS[rng.integers(0, 4, n, dtype=np.uint8)]
            for _ in range(max(1, n // 5000)):  # soft-masked runs, N runs, the odd IUPAC letter
                a = int(rng.integers(0, n))
                seq[a:a + int(rng.integers(10, 400))] |= 0x20
            for _ in range(max(1, n // 20000)):
                a = int(rng.integers(0, n))
                seq[a:a + int(rng.integers(1, 200))] = ord("N")
            seq[rng.integers(0, n, max(1, n // 10000))] = ord("R")
            f.write(b">chr%d generated\n" % (c + 1))
            pad = (-n) % 60
            body = np.concatenate([seq, np.zeros(pad, np.uint8)]).reshape(-1, 60)
            rows = np.concatenate([body, np.full((len(body), 1), 10, np.uint8)], axis=1).reshape(-1)
            out = rows.tobytes()
            if pad:
                out = out[:-(pad + 1)] + b"\n"
            f.write(out)
    with open(os.path.join(out_dir, "genes.gtf"), "w") as f:
        f.write("# generated, seed %d\n" % seed)
        t, g = 0, 0
        while t < n_transcripts:
            g += 1
            absent = rng.random() < absent_fraction
            c = int(rng.integers(0, n_chromosomes))
            chrom, clen = ("chrAbsent", 10 ** 6) if absent else ("chr%d" % (c + 1), lengths[c])
            strand = "+-"[int(rng.integers(0, 2))]
            for _ in range(int(rng.integers(1, 5))):
                if t >= n_transcripts:
                    break
                t += 1
                n_ex = int(rng.integers(1, 13))
                pos = int(rng.integers(1, max(2, clen - 13 * 700)))
                exons = []
                for _ in range(n_ex):
                    ln = int(rng.integers(1, 400))
                    exons.append((pos, pos + ln - 1))
                    pos += max(1, ln + int(rng.integers(-20, 300)))  # touching and overlapping exons among them; the starts ascend strictly
                for k in rng.permutation(n_ex):
                    s, e = exons[int(k)]
                    name = ' gene_name "G%d";' % g if k % 3 == 0 else ""
                    f.write('%s\tgen\texon\t%d\t%d\t.\t%s\t.\tgene_id "gene%05d"; transcript_id "tx%06d";%s\n' % (chrom, s, min(e, clen), strand, g, t, name))
    return lengths


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--chromosomes", type=int, default=3)
    ap.add_argument("--bases", type=int, default=40000, help="bases a chromosome, about")
    ap.add_argument("--transcripts", type=int, default=200)
    ap.add_argument("--absent", type=float, default=0.05)
    a = ap.parse_args()
    print(write(a.out_dir, a.seed, a.chromosomes, a.bases, a.transcripts, a.absent))
