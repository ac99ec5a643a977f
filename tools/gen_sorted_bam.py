"""A coordinate-sorted BAM with ZW weights for timing rsem-bam2wig / rsem-bam2readdepth (tools/time_bam2wig.py): R records over M
reference sequences, from a fixed seed, so that two hosts write the same file.

    python tools/gen_sorted_bam.py out.bam --records 1000000 --targets 10000 [--seed 1]

Records are 100 bases long with names, bases and qualities (the inflate and the record walk cost what they cost on real files);
one in ten has an insertion, one in ten a gap of 150 (N); the weights are floats in (0, 1], a quarter of them exactly 1.
BGZF blocks of 0xff00 bytes through zlib level 1.
"""
import argparse
import struct
import zlib

import numpy as np


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


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

    def close(self):
        if self.buf:
            self.block(bytes(self.buf))
        self.block(b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    lens = rng.integers(400, 6000, a.targets)
    share = rng.gamma(0.5, 1.0, a.targets) * lens
    counts = rng.multinomial(a.records, share / share.sum())
    pool_seq = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    pool_qual = rng.integers(2, 41, 1 << 20, dtype=np.uint8).tobytes()
    cigs = [struct.pack("<I", 100 << 4), struct.pack("<III", 40 << 4, 1 << 4 | 1, 59 << 4), struct.pack("<III", 50 << 4, 150 << 4 | 3, 50 << 4)]
    span = [100, 99, 250]
    with open(a.out, "wb") as f:
        z = Bgzf(f)
        text = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:t%d\tLN:%d\n" % (i, l) for i, l in enumerate(lens))
        head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", a.targets)
        for i, l in enumerate(lens):
            nm = b"t%d\0" % i
            head += struct.pack("<i", len(nm)) + nm + struct.pack("<i", int(l))
        z.write(head)
        serial = 0
        for tid in range(a.targets):
            n = int(counts[tid])
            if not n:
                continue
            kind = rng.choice(3, n, p=[0.8, 0.1, 0.1])
            room = np.array([lens[tid] - span[k] for k in kind])
            pos = np.sort((rng.random(n) * (room + 1)).astype(np.int64))
            pos = np.minimum(pos, room)
            w = np.where(rng.random(n) < 0.25, 1.0, rng.random(n) * 0.999 + 0.001).astype(np.float32)
            at = rng.integers(0, (1 << 20) - 200, n)
            out = bytearray()
            for i in range(n):
                k = int(kind[i])
                p = int(pos[i])
                name = b"read%d\0" % serial
                serial += 1
                cig = cigs[k]
                body = struct.pack("<iiBBHHHiiii", tid, p, len(name), 100, reg2bin(p, p + span[k]), len(cig) // 4, 0, 100, -1, -1, 0) + name + cig + \
                    pool_seq[at[i]:at[i] + 50] + pool_qual[at[i]:at[i] + 100] + b"NHC\x01ZWf" + struct.pack("<f", w[i])
                out += struct.pack("<i", len(body)) + body
            z.write(out)
        z.close()


if __name__ == "__main__":
    main()
