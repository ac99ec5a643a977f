"""Writes tests/golden/clustering/: small FASTA files and, for every k in use, the .ump file that the UNMODIFIED reference program
(EBSeq/calcClusteringInfo.cpp, g++ -O3) wrote for them.

    python tests/golden/make_clustering_golden.py /path/to/rsem-for-ebseq-calculate-clustering-info

The FASTA files are generated from fixed seeds; the expected outputs are recorded, not computed here.
"""
import os
import random
import subprocess
import sys

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clustering")
KS = {"mixed.fa": (1, 5, 25, 28, 60), "crlf.fa": (5, 25), "tails.fa": (25, 27, 54, 55)}


def rnd(r, n, letters="ACGT"):
    return "".join(r.choice(letters) for _ in range(n))


def wrap(r, s, lo=17, hi=71):
    """lines of uneven width"""
    out = []
    while s:
        w = r.randint(lo, hi)
        out.append(s[:w])
        s = s[w:]
    return out


def mixed():
    r = random.Random(20240611)
    tail = "A" * 40
    seg = rnd(r, 90)          # present in several entries
    rep = rnd(r, 33)          # repeated inside one entry only
    both = rnd(r, 35)         # repeated inside one entry and present in another
    nrun = "N" * 70
    e = []
    e.append(("t1 plain gene=G1", rnd(r, 210) + seg + rnd(r, 50) + tail))
    e.append(("t2\twith a tab  and  blanks ", rnd(r, 120) + seg.lower() + rnd(r, 80).lower() + tail))
    e.append(("t3_iupac", rnd(r, 60) + "RYKMSWBDHVN" + rnd(r, 40) + "ryk" + seg[:50] + "acgu" + rnd(r, 30) + tail))
    e.append(("t4_self_repeat", rnd(r, 40) + rep + rnd(r, 25) + rep + rnd(r, 40) + tail))
    e.append(("t5_repeat_and_elsewhere", rnd(r, 30) + both + rnd(r, 20) + both + rnd(r, 30) + tail))
    e.append(("t6_has_it_once", rnd(r, 70) + both + rnd(r, 70)))
    e.append(("t7_short", rnd(r, 10)))
    e.append(("t8_exactly_25", rnd(r, 25)))
    e.append(("t9_empty", ""))
    dup = rnd(r, 150) + tail
    e.append(("t10_twin", dup))
    e.append(("t11_twin", dup))
    e.append(("t12_n_run", rnd(r, 50) + nrun + rnd(r, 50) + tail))
    e.append(("t13_n_run", rnd(r, 35) + nrun.lower() + "NNNNN" + rnd(r, 45) + tail))
    e.append(("t14_exactly_5", "ACGTA"))
    e.append(("t15_three", "AAA"))
    e.append(("t16 other digits 0123 and a dash", rnd(r, 40) + "-*." + rnd(r, 40) + "0123" + seg[40:] + tail))
    e.append(("t17_all_a", "A" * 95))
    lines = []
    for name, s in e:
        lines.append(">" + name)
        lines += wrap(r, s)
    return "\n".join(lines) + "\n"


def crlf():
    r = random.Random(7)
    seg = rnd(r, 80)
    e = [("c1 first", rnd(r, 100) + seg + "A" * 30), ("c2", seg + rnd(r, 60) + "a" * 30), ("c3_empty", ""),
         ("c4", rnd(r, 45) + "A" * 30), ("c5_short", "ACG")]
    lines = []
    for name, s in e:
        lines.append(">" + name)
        lines += wrap(r, s, 20, 40)
    return "\r\n".join(lines) + "\r\n"


def tails():
    """entries around the chunk seams (27 | 28, 54 | 55) that share a head, a middle or a tail; the last line has no newline"""
    r = random.Random(99)
    head, mid, tail = rnd(r, 56), rnd(r, 58, "AC"), "A" * 60
    e = []
    for i in range(14):
        s = (head if i % 3 == 0 else rnd(r, r.randint(20, 60))) + (mid if i % 2 else rnd(r, r.randint(10, 70), "ACGTN")) + (tail if i % 5 else "")
        e.append(("s%d" % i, s))
    e += [("s_27", head[:27]), ("s_28", head[:28]), ("s_54", head[:54]), ("s_55", head[:55])]
    lines = []
    for name, s in e:
        lines.append(">" + name)
        lines += wrap(r, s, 30, 90)
    return "\n".join(lines)


def main():
    ref = sys.argv[1]
    os.makedirs(HERE, exist_ok=True)
    for name, text in (("mixed.fa", mixed()), ("crlf.fa", crlf()), ("tails.fa", tails())):
        path = os.path.join(HERE, name)
        with open(path, "wb") as f:
            f.write(text.encode())
        for k in KS[name]:
            subprocess.check_call([ref, str(k), path, os.path.join(HERE, "%s.k%d.ump" % (name[:-3], k))], stdout=subprocess.DEVNULL)


if __name__ == "__main__":
    main()
