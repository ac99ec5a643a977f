"""Times rsem-tbam2gbam on a generated transcript.bam (tools/gen_transcript_bam.py) and records the result in
profiles/tbam2gbam_<size>.json: wall time, where it goes (inflate and cut, fields, upload, device, assemble, deflate, write), the
sha256 of the DECOMPRESSED output (the compressed bytes differ between two deflate implementations by design).

    python tools/time_tbam2gbam.py --size 1m --pairs 1000000 [--out profiles/tbam2gbam_1m.json] [-p 16]
    python tools/time_tbam2gbam.py --size 1m ... --reference /path/to/rsem-tbam2gbam

Without --reference the drop-in of rsem_amd/bin runs (a GPU is needed); with it the given reference binary runs on the same generated
file, on whatever host this is.  Both kinds of run merge into the same JSON, each under its own key with its host's name: the two
wall times usually come from two different hosts.  Both are run in the work directory as `rsem-tbam2gbam ref transcript.bam genome.bam
-p N` (argv[0] the bare name), so that the @PG line is the same.  Where both are present the hashes must be equal -- the full-size
parity check -- and the script fails if they are not.
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


def sha256_inflated(path):
    h, n = hashlib.sha256(), 0
    data = open(path, "rb").read()
    o = 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = -1
        x = o + 12
        while x < o + 12 + xlen:
            slen = struct.unpack_from("<H", data, x + 2)[0]
            if data[x:x + 2] == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        raw = zlib.decompress(data[o + 12 + xlen: o + bsize + 1 - 8], -15)
        h.update(raw)
        n += len(raw)
        o += bsize + 1
    return h.hexdigest(), n


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
    ap.add_argument("--reference", metavar="TBAM2GBAM")
    ap.add_argument("--workdir")
    ap.add_argument("--host-label", default="", help="what to call this host in the record, e.g. 'CPU-only host' or 'MI355X host'")
    a = ap.parse_args()
    out_json = a.out or os.path.join(ROOT, "profiles", "tbam2gbam_%s.json" % a.size)
    work = a.workdir or tempfile.mkdtemp(prefix="tbam2gbam_")
    bam = os.path.join(work, "transcript.bam")
    if not os.path.exists(bam):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_transcript_bam.py"), work, "--pairs", str(a.pairs), "--per-read", str(a.per_read),
                               "--genes", str(a.genes), "--seed", str(a.seed)])
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    h = hashlib.sha256(open(bam, "rb").read()).hexdigest()
    doc["input"] = {"pairs": a.pairs, "per_read": a.per_read, "genes": a.genes, "seed": a.seed, "bytes": os.path.getsize(bam), "sha256": h}
    cmd = ["rsem-tbam2gbam", "ref", "transcript.bam", "genome.bam", "-p", str(a.p)]
    out = os.path.join(work, "genome.bam")
    if a.reference:
        wall, _ = timed(cmd, os.path.abspath(a.reference), work)
        sha, n = sha256_inflated(out)
        doc["reference"] = {"host": a.host_label or "CPU host", "cpu": platform.processor(), "threads": a.p, "wall_s": round(wall, 3), "inflated_sha256": sha,
                            "inflated_bytes": n, "bytes": os.path.getsize(out)}
    else:
        env = dict(os.environ, RSEM_HIP_TIMING="1")
        exe = os.path.join(ROOT, "rsem_amd", "bin", "rsem-tbam2gbam")
        timed(cmd, exe, work, env)  # once to warm the file cache and the device
        wall, stdout = timed(cmd, exe, work, env)
        t = json.loads(re.search(r"^\[timing\] (\{.*\})$", stdout, re.M).group(1))
        t["wall_s_outside"] = round(wall, 4)
        parts = {"inflate and cut": t["inflate_cut_s"], "fields": t["fields_s"], "device call": t["device_call_s"], "assemble": t["assemble_s"],
                 "deflate": t["deflate_s"], "write": t["write_s"]}
        t["dominant_stage"] = max(parts, key=parts.get)
        t["inflated_sha256"], t["inflated_bytes"] = sha256_inflated(out)
        t["bytes"] = os.path.getsize(out)
        t["host"] = a.host_label or "GPU host"
        doc["drop_in"] = t
    if "reference" in doc and "drop_in" in doc:
        doc["outputs_equal"] = doc["reference"]["inflated_sha256"] == doc["drop_in"]["inflated_sha256"]
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))
    if doc.get("outputs_equal") is False:
        sys.exit("the outputs differ from the reference's")


if __name__ == "__main__":
    main()
