"""An RSEM-shaped transcript.bam with its reference, for timing rsem-tbam2gbam (tools/time_tbam2gbam.py): P read pairs, each aligned
to about A isoforms of one gene (the alignments of a read next to each other, mate 1 before mate 2, ZW weights that add up to 1),
over G genes on 24 chromosomes; from a fixed seed, so that two hosts write the same files.

    python tools/gen_transcript_bam.py out_dir --pairs 1000000 [--per-read 10] [--genes 4000] [--seed 1]

Writes out_dir/ref.ti (type 0), out_dir/ref.chrlist and out_dir/transcript.bam.  A gene has 4 to 40 exons; an isoform keeps the first
and last exon and three quarters of the others, so that a read's alignments often land on one genomic locus and collapse, and often
do not.  Reads are 2 x 100 bases; names, bases and qualities are there (inflate, record walk and deflate cost what they cost on real
files).  BGZF blocks of up to 0xff00 bytes through zlib level 1; every 20 000 pairs come from a seed of their own and are made side by side
on up to 16 processes.
"""
import argparse
import io
import multiprocessing
import os
import struct
import zlib

import numpy as np


class Bgzf:
    def __init__(self, f):
        self.f, self.buf = f, bytearray()

    def write(self, data):
        self.buf += data
        while len(self.buf) >= 0xff00:
            self.block(bytes(self.buf[:0xff00]))
            del self.buf[:0xff00]

    def block(self, chunk):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        self.f.write(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp +
                     struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))

    def close_stream(self):  # (without the empty block that ends a file)
        if self.buf:
            self.block(bytes(self.buf))
        self.buf = bytearray()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--per-read", type=int, default=10)
    ap.add_argument("--genes", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    os.makedirs(a.out_dir, exist_ok=True)
    n_chr, chr_len = 24, 120000000
    # genes -> isoforms
    trs, gene_trs = [], []  # (chromosome, strand, exons), per gene the indices of its isoforms
    for g in range(a.genes):
        c, strand = int(rng.integers(0, n_chr)), "+-"[int(rng.integers(0, 2))]
        n_ex = int(rng.integers(4, 41))
        ex_len = rng.integers(60, 400, n_ex)
        ex_len[0] += 300
        ex_len[-1] += 300
        gaps = rng.integers(80, 5000, n_ex)
        start = int(rng.integers(1000, chr_len - 400000))
        exons = []
        for k in range(n_ex):
            start += int(gaps[k])
            exons.append((start, start + int(ex_len[k]) - 1))
            start += int(ex_len[k])
        mine = []
        for _ in range(a.per_read + int(rng.integers(-2, 3))):
            keep = rng.random(n_ex) < 0.75
            keep[0] = keep[-1] = True
            mine.append(len(trs))
            trs.append((c, strand, [e for e, k in zip(exons, keep) if k]))
        gene_trs.append(mine)
    lens = [sum(e - s + 1 for s, e in t[2]) for t in trs]
    with open(os.path.join(a.out_dir, "ref.ti"), "w") as f:
        f.write("%d 0\n" % len(trs))
        for i, (c, strand, exons) in enumerate(trs):
            f.write("T%d\nG%d\nchr%d\n%s %d\n%d %s\n\n" % (i, i, c + 1, strand, lens[i], len(exons), " ".join("%d %d" % e for e in exons)))
    with open(os.path.join(a.out_dir, "ref.chrlist"), "w") as f:
        for c in range(n_chr):
            f.write("chr%d\t%d\n" % (c + 1, chr_len))
    global G
    G = dict(gene_trs=gene_trs, lens=lens, genes=a.genes, seed=a.seed, pairs=a.pairs)
    chunk = 20000
    with open(os.path.join(a.out_dir, "transcript.bam"), "wb") as f:
        z = Bgzf(f)
        text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:T%d\tLN:%d\n" % (i, l + 125) for i, l in enumerate(lens)) + "@PG\tID:RSEM\n"
        head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(trs))
        for i, l in enumerate(lens):
            nm = b"T%d\0" % i
            head += struct.pack("<i", len(nm)) + nm + struct.pack("<i", l + 125)
        z.write(head)
        z.close_stream()
        # the records: chunks of pairs, each from its own seed and in its own run of BGZF blocks, made side by side and written in order
        with multiprocessing.Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
            for blocks in pool.imap(records_of, range(0, a.pairs, chunk)):
                f.write(blocks)
        z.block(b"")


G = None


def records_of(p0):
    """the BGZF blocks of the pairs p0 .. p0 + 20000"""
    gene_trs, lens = G["gene_trs"], G["lens"]
    rng = np.random.default_rng([G["seed"], p0])
    n = min(20000, G["pairs"] - p0)
    pool_seq = bytes(((1, 2, 4, 8)[x >> 6] << 4) | (1, 2, 4, 8)[(x >> 4) & 3] for x in rng.integers(0, 256, 1 << 16, dtype=np.uint8).tolist())
    pool_qual = rng.integers(2, 41, 1 << 16, dtype=np.uint8).tobytes()
    cig = struct.pack("<I", 100 << 4)
    genes = rng.integers(0, G["genes"], n)
    frac = rng.random((n, 2))
    at = rng.integers(0, (1 << 16) - 200, (n, 2))
    out = bytearray()
    for i in range(n):
        mine = gene_trs[int(genes[i])]
        name = b"read%d\0" % (p0 + i)
        w = rng.dirichlet(np.full(len(mine), 0.3)).astype(np.float32)
        s1, q1 = pool_seq[at[i, 0]:at[i, 0] + 50], pool_qual[at[i, 0]:at[i, 0] + 100]
        s2, q2 = pool_seq[at[i, 1]:at[i, 1] + 50], pool_qual[at[i, 1]:at[i, 1] + 100]
        for k, t in enumerate(mine):
            L = lens[t]
            p1 = int(frac[i, 0] * (L - 300))
            p2 = p1 + 100 + int(frac[i, 1] * 100)
            tag = b"ZWf" + struct.pack("<f", w[k])
            b1 = struct.pack("<iiBBHHHiiii", t, p1, len(name), 0, 4681, 1, 99, 100, t, p2, p2 + 100 - p1) + name + cig + s1 + q1 + tag
            b2 = struct.pack("<iiBBHHHiiii", t, p2, len(name), 0, 4681, 1, 147, 100, t, p1, p1 - p2 - 100) + name + cig + s2 + q2 + tag
            out += struct.pack("<i", len(b1)) + b1 + struct.pack("<i", len(b2)) + b2
    mem = io.BytesIO()
    z = Bgzf(mem)
    z.write(out)
    z.close_stream()
    return mem.getvalue()


if __name__ == "__main__":
    main()
