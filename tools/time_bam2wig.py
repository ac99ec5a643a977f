"""Times rsem-bam2wig and rsem-bam2readdepth on a generated, coordinate-sorted BAM (tools/gen_sorted_bam.py) and records the result in
profiles/bam2wig_<size>.json: wall time, where it goes (inflate + blocks, stitch, upload, kernels, formatting, writing), entries and
lane-iterations per second of the device stage, the sha256 of both outputs.

    python tools/time_bam2wig.py --size 1m --records 1000000 --targets 10000 [--out profiles/bam2wig_1m.json] [-p 16]
    python tools/time_bam2wig.py --size 1m ... --reference /path/to/rsem-bam2wig /path/to/rsem-bam2readdepth

Without --reference the drop-ins of rsem_amd/bin run (a GPU is needed); with it the two given reference binaries run on the same
generated file, on whatever host this is.  Both kinds of run merge into the same JSON, each under its own key with its host's name:
the two wall times usually come from two different hosts.  Where both are present the hashes must be equal -- the full-size parity
check -- and the script fails if they are not.
"""
import argparse
import hashlib
import json
import os
import platform
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 512  # rsem_amd/csrc/depth_block.hpp


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def timed(cmd, env=None):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s failed with %d" % (cmd[0], r.returncode))
    return wall, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", required=True)
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-p", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--reference", nargs=2, metavar=("BAM2WIG", "BAM2READDEPTH"))
    ap.add_argument("--workdir")
    ap.add_argument("--host-label", default="", help="what to call this host in the record, e.g. 'CPU-only host' or 'MI355X host'")
    a = ap.parse_args()
    out_json = a.out or os.path.join(ROOT, "profiles", "bam2wig_%s.json" % a.size)
    work = a.workdir or tempfile.mkdtemp(prefix="bam2wig_")
    bam = os.path.join(work, "sorted_%s.bam" % a.size)
    if not os.path.exists(bam):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_sorted_bam.py"), bam, "--records", str(a.records), "--targets", str(a.targets),
                               "--seed", str(a.seed)])
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    doc["input"] = {"records": a.records, "targets": a.targets, "seed": a.seed, "bytes": os.path.getsize(bam), "sha256": sha256(bam)}
    wig, rd = os.path.join(work, "out.wig"), os.path.join(work, "out.readdepth")
    if a.reference:
        w1, _ = timed([a.reference[0], bam, wig, "track"])
        w2, _ = timed([a.reference[1], bam, rd])
        doc["reference"] = {"host": a.host_label or "CPU host", "cpu": platform.processor(), "bam2wig_wall_s": round(w1, 3), "bam2readdepth_wall_s": round(w2, 3),
                            "wig_sha256": sha256(wig), "readdepth_sha256": sha256(rd), "wig_bytes": os.path.getsize(wig), "readdepth_bytes": os.path.getsize(rd)}
    else:
        env = dict(os.environ, RSEM_HIP_TIMING="1")
        res = {"host": a.host_label or "GPU host", "threads": a.p}
        for key, cmd, path in (("bam2wig", [os.path.join(ROOT, "rsem_amd", "bin", "rsem-bam2wig"), bam, wig, "track", "-p", str(a.p)], wig),
                               ("bam2readdepth", [os.path.join(ROOT, "rsem_amd", "bin", "rsem-bam2readdepth"), bam, rd, "-p", str(a.p)], rd)):
            timed(cmd, env)  # once to warm the file cache and the device
            wall, stdout = timed(cmd, env)
            m = re.search(r"^\[timing\] (\{.*\})$", stdout, re.M)
            t = json.loads(m.group(1))
            t["wall_s_outside"] = round(wall, 4)
            k_s = t["kernel_ms"] / 1e3
            t["entries_per_s"] = t["entries"] / k_s if k_s else None
            t["lane_iterations_per_s"] = t["entries"] * TILE / k_s if k_s else None  # every entry is looked at by the 512 bases of its tile
            parts = {"inflate + blocks": t["read_blocks_s"], "stitch": t["stitch_s"], "device call": t["device_call_s"], "format": t["format_s"], "write": t["write_s"]}
            t["dominant_stage"] = max(parts, key=parts.get)
            t["sha256"] = sha256(path)
            t["bytes"] = os.path.getsize(path)
            res[key] = t
        doc["drop_in"] = res
    if "reference" in doc and "drop_in" in doc:
        same = doc["reference"]["wig_sha256"] == doc["drop_in"]["bam2wig"]["sha256"] and doc["reference"]["readdepth_sha256"] == doc["drop_in"]["bam2readdepth"]["sha256"]
        doc["outputs_equal"] = same
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))
    if doc.get("outputs_equal") is False:
        sys.exit("the outputs differ from the reference's")


if __name__ == "__main__":
    main()
