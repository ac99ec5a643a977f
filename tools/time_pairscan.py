"""Times rsem-scan-for-paired-end-reads on a generated transcript.bam (tools/gen_transcript_bam.py) whose mates have been pulled apart, and
records the result in profiles/pairscan_<size>.json: wall time, where it goes (inflate and cut, fields, device call, gather and deflate,
write), upload and kernel times by HIP events, the device bytes held, and two hashes of the DECOMPRESSED output (the compressed bytes
differ between two deflate implementations by design).

    python tools/time_pairscan.py --size 20m --pairs 1000000 [--out profiles/pairscan_20m.json] [-p 16]
    python tools/time_pairscan.py --size 20m ... --reference /path/to/rsem-scan-for-paired-end-reads

The generated file holds a read's alignments next to each other, mate 1 before mate 2 -- what this program produces.  It is rewritten
first (apart.bam) so that each read's first mates precede its second mates, the shape a name-sorted aligner output has.

Without --reference the drop-in of rsem_amd/bin runs (a GPU is needed); with it the given reference binary runs on the same rewritten
file, on whatever host this is; each is timed on its second run.  Both kinds of run merge into the same JSON, each under its own key
with its host's name: the two wall times usually come from two different hosts.

With 10 alignments a read most groups hold more than 16 properly paired records, where the reference's std::sort leaves the order
inside a run of tied records to its library and the drop-in keeps file order.  So two hashes are taken on either side:
`canonical_sha256` over the whole decompressed output with every maximal run of records that tie under less_than inside a group sorted
by the records' bytes, and `small_groups_sha256` over the untouched records of the groups with at most 16 properly paired records
(`small_groups` of them), which must be byte-equal as they are.  Where both sides are present both pairs must be equal, and the script
fails if they are not.
"""
import argparse
import hashlib
import json
import os
import platform
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_transcript_bam import Bgzf  # noqa: E402

TIMING = re.compile(r"^\[timing\] (\{.*\})\n", re.M)


def inflated(path):
    """the decompressed bytes of a BGZF file, block by block"""
    with open(path, "rb") as f:
        while True:
            head = f.read(18)
            if len(head) < 18:
                return
            xlen, bsize = struct.unpack_from("<H", head, 10)[0], struct.unpack_from("<H", head, 16)[0]
            rest = f.read(bsize + 1 - 18)
            yield zlib.decompress(rest[xlen - 6:-8], -15)


def groups(path):
    """(header bytes, iterator over the file's groups: lists of records with their block_size, a group being a run of equal names)"""
    stream = inflated(path)
    buf = bytearray()

    def need(n):
        while len(buf) < n:
            try:
                buf.extend(next(stream))
            except StopIteration:
                return False
        return True

    need(12)
    l_text = struct.unpack_from("<i", buf, 4)[0]
    need(12 + l_text)
    n_ref, p = struct.unpack_from("<i", buf, 8 + l_text)[0], 12 + l_text
    for _ in range(n_ref):
        need(p + 4)
        p += 8 + struct.unpack_from("<i", buf, p)[0]
    need(p)
    header = bytes(buf[:p])
    del buf[:p]

    def walk():
        nonlocal buf
        group, name, p = [], None, 0
        while True:
            if len(buf) - p < 4 and not need(p + 4):
                break
            size = struct.unpack_from("<i", buf, p)[0]
            if len(buf) - p < 4 + size:
                del buf[:p]
                p = 0
                need(4 + size)
            r = bytes(buf[p:p + 4 + size])
            p += 4 + size
            nm = r[36:36 + r[12] - 1]
            if nm != name and group:
                yield group
                group = []
            name = nm
            group.append(r)
        if group:
            yield group

    return header, walk()


def pull_apart(src, dst):
    """each read's first mates before its second mates"""
    header, gs = groups(src)
    with open(dst, "wb") as f:
        z = Bgzf(f)
        z.write(header)
        for g in gs:
            z.write(b"".join([r for r in g if r[18] & 0x40] + [r for r in g if not r[18] & 0x40]))
        z.close_stream()
        z.block(b"")


def key(r):
    """less_than of scanForPairedEndReads.cpp:39-51 on a record with its block_size"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    flag, mpos = struct.unpack_from("<H", r, 18)[0], struct.unpack_from("<i", r, 28)[0]
    rev = flag >> 4 & 1
    return (tid, min(pos, mpos), max(pos, mpos), rev if flag & 0x40 else 1 - rev)


def output_hashes(path):
    """(canonical_sha256, small_groups_sha256, groups, small_groups, bytes) of an output whose reads are all paired-end"""
    header, gs = groups(path)
    canon, small = hashlib.sha256(header), hashlib.sha256()
    n_groups = n_small = n_bytes = 0
    for g in gs:
        n_groups += 1
        both = sum(1 for r in g if not r[18] & 4 and r[18] & 2)
        if both <= 16:
            n_small += 1
            small.update(b"".join(g))
        out, i = [], 0
        while i < len(g):
            j = i + 1
            if i < both:  # (the properly paired records come first)
                k = key(g[i])
                while j < both and key(g[j]) == k:
                    j += 1
            out += sorted(g[i:j])
            i = j
        blob = b"".join(out)
        n_bytes += len(blob)
        canon.update(blob)
    return canon.hexdigest(), small.hexdigest(), n_groups, n_small, n_bytes + len(header)


def timed(cmd, exe, cwd, env=None):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, executable=exe, cwd=cwd, stdout=subprocess.PIPE, text=True, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s failed with %d" % (exe, r.returncode))
    return wall, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", required=True)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--per-read", type=int, default=10)
    ap.add_argument("--genes", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-p", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--reference", metavar="SCAN_FOR_PAIRED_END_READS")
    ap.add_argument("--workdir")
    ap.add_argument("--host-label", default="", help="what to call this host in the record, e.g. 'CPU-only host' or 'MI355X host'")
    a = ap.parse_args()
    out_json = a.out or os.path.join(ROOT, "profiles", "pairscan_%s.json" % a.size)
    work = a.workdir or tempfile.mkdtemp(prefix="pairscan_")
    bam, apart = os.path.join(work, "transcript.bam"), os.path.join(work, "apart.bam")
    if not os.path.exists(bam):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_transcript_bam.py"), work, "--pairs", str(a.pairs), "--per-read", str(a.per_read),
                               "--genes", str(a.genes), "--seed", str(a.seed)])
    if not os.path.exists(apart):
        pull_apart(bam, apart)
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    doc["input"] = {"pairs": a.pairs, "per_read": a.per_read, "genes": a.genes, "seed": a.seed, "bytes": os.path.getsize(apart),
                    "generated_sha256": hashlib.sha256(open(bam, "rb").read()).hexdigest(), "shape": "each read's first mates before its second mates"}
    out = os.path.join(work, "adjacent.bam")
    cmd = ["rsem-scan-for-paired-end-reads", str(a.p), "apart.bam", "adjacent.bam"]
    if a.reference:
        exe = os.path.abspath(a.reference)
        timed(cmd, exe, work)  # once to warm the file cache
        wall, stdout = timed(cmd, exe, work)
        side = {"host": a.host_label or "CPU host", "cpu": platform.processor(), "wall_s": round(wall, 3), "threads": a.p, "stdout": stdout}
        doc["reference"] = side
    else:
        env = dict(os.environ, RSEM_HIP_TIMING="1")
        exe = os.path.join(ROOT, "rsem_amd", "bin", "rsem-scan-for-paired-end-reads")
        timed(cmd, exe, work, env)  # once to warm the file cache and the device
        wall, stdout = timed(cmd, exe, work, env)
        side = json.loads(TIMING.search(stdout).group(1))
        side["host"] = a.host_label or "GPU host"
        side["wall_s_outside"] = round(wall, 4)
        parts = {"inflate and cut": side["inflate_cut_s"], "fields": side["fields_s"], "device call": side["device_call_s"], "gather and deflate": side["gather_deflate_s"],
                 "write": side["write_s"]}
        side["dominant_stage"] = max(parts, key=parts.get)
        side["stdout"] = TIMING.sub("", stdout)
        doc["drop_in"] = side
    side["canonical_sha256"], side["small_groups_sha256"], side["groups"], side["small_groups"], side["inflated_bytes"] = output_hashes(out)
    side["bytes"] = os.path.getsize(out)
    if "reference" in doc and "drop_in" in doc:
        r, d = doc["reference"], doc["drop_in"]
        doc["outputs_equal_up_to_tie_runs"] = r["canonical_sha256"] == d["canonical_sha256"]
        doc["small_groups_byte_equal"] = (r["small_groups_sha256"], r["small_groups"]) == (d["small_groups_sha256"], d["small_groups"])
        doc["stdout_equal"] = r["stdout"] == d["stdout"]
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))
    if doc.get("outputs_equal_up_to_tie_runs") is False or doc.get("small_groups_byte_equal") is False or doc.get("stdout_equal") is False:
        sys.exit("the outputs differ from the reference's")


if __name__ == "__main__":
    main()
