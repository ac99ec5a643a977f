"""Times rsem-sam-validator and rsem-get-unique on a generated transcript.bam (tools/gen_transcript_bam.py) and records the result in
profiles/alncheck_<size>.json: wall time, where it goes (inflate and cut, fields, device call, deflate, write), upload and kernel times,
the device bytes held, the validator's stdout and the sha256 of get-unique's DECOMPRESSED output (the compressed bytes differ between two
deflate implementations by design).

    python tools/time_alncheck.py --size 20m --pairs 1000000 [--out profiles/alncheck_20m.json] [-p 16] [--kernel-stats]
    python tools/time_alncheck.py --size 20m ... --reference-validator /path/to/rsem-sam-validator --reference-get-unique /path/to/rsem-get-unique

Without the --reference options the drop-ins of rsem_amd/bin run (a GPU is needed); with them the given reference binaries run on the
same generated file, on whatever host this is.  Both kinds of run merge into the same JSON, each under its own key with its host's
name: the two wall times usually come from two different hosts.  Where both are present the validator's stdout and the hash of
get-unique's output must be equal -- the full-size parity check -- and the script fails if they are not.  --kernel-stats runs each
drop-in once more under `rocprofv3 --kernel-trace --stats` and keeps every kernel's calls and total time.
"""
import argparse
import csv
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_tbam2gbam import sha256_inflated  # noqa: E402

TIMING = re.compile(r"^\[timing\] (\{.*\})\n", re.M)


def timed(cmd, exe, cwd, env=None):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, executable=exe, cwd=cwd, stdout=subprocess.PIPE, text=True, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("%s failed with %d" % (exe, r.returncode))
    return wall, r.stdout


def kernel_stats(cmd, exe, work, tag):
    """every kernel's calls and total time from one run under rocprofv3"""
    d = os.path.join(work, "trace_" + tag)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", tag, "--output-format", "csv", "--", exe] + cmd[1:], cwd=work,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("rocprofv3 failed with %d: %s" % (r.returncode, r.stderr[-500:]))
    out = {}
    for dp, _, fns in os.walk(d):
        for fn in fns:
            if fn.endswith("kernel_stats.csv"):
                for row in csv.DictReader(open(os.path.join(dp, fn))):
                    k = out.setdefault(row["Name"][:160], {"calls": 0, "total_ms": 0.0})  # (the library's kernels are told apart by their first template arguments)
                    k["calls"] += int(row["Calls"])
                    k["total_ms"] = round(k["total_ms"] + float(row["TotalDurationNs"]) / 1e6, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", required=True)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--per-read", type=int, default=10)
    ap.add_argument("--genes", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-p", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--reference-validator", metavar="SAM_VALIDATOR")
    ap.add_argument("--reference-get-unique", metavar="GET_UNIQUE")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--workdir")
    ap.add_argument("--host-label", default="", help="what to call this host in the record, e.g. 'CPU-only host' or 'MI355X host'")
    a = ap.parse_args()
    out_json = a.out or os.path.join(ROOT, "profiles", "alncheck_%s.json" % a.size)
    work = a.workdir or tempfile.mkdtemp(prefix="alncheck_")
    bam = os.path.join(work, "transcript.bam")
    if not os.path.exists(bam):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_transcript_bam.py"), work, "--pairs", str(a.pairs), "--per-read", str(a.per_read),
                               "--genes", str(a.genes), "--seed", str(a.seed)])
    doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
    h = hashlib.sha256(open(bam, "rb").read()).hexdigest()
    doc["input"] = {"pairs": a.pairs, "per_read": a.per_read, "genes": a.genes, "seed": a.seed, "bytes": os.path.getsize(bam), "sha256": h}
    out = os.path.join(work, "unique.bam")
    v_cmd = ["rsem-sam-validator", "transcript.bam"]
    u_cmd = ["rsem-get-unique", str(a.p), "transcript.bam", "unique.bam"]
    if a.reference_validator or a.reference_get_unique:
        ref = doc.setdefault("reference", {})
        ref.update({"host": a.host_label or "CPU host", "cpu": platform.processor()})
        if a.reference_validator:
            wall, stdout = timed(v_cmd, os.path.abspath(a.reference_validator), work)
            ref["sam_validator"] = {"wall_s": round(wall, 3), "threads": 1, "stdout": stdout}
        if a.reference_get_unique:
            wall, _ = timed(u_cmd, os.path.abspath(a.reference_get_unique), work)
            sha, n = sha256_inflated(out)
            ref["get_unique"] = {"wall_s": round(wall, 3), "threads": a.p, "inflated_sha256": sha, "inflated_bytes": n, "bytes": os.path.getsize(out)}
    else:
        env = dict(os.environ, RSEM_HIP_TIMING="1")
        drop = doc.setdefault("drop_in", {})
        drop["host"] = a.host_label or "GPU host"
        exe = os.path.join(ROOT, "rsem_amd", "bin", "rsem-sam-validator")
        cmd = v_cmd + ["-p", str(a.p)]
        timed(cmd, exe, work, env)  # once to warm the file cache and the device
        wall, stdout = timed(cmd, exe, work, env)
        t = json.loads(TIMING.search(stdout).group(1))
        t["wall_s_outside"] = round(wall, 4)
        parts = {"inflate and cut": t["inflate_cut_s"], "fields": t["fields_s"], "device call": t["device_call_s"]}
        t["dominant_stage"] = max(parts, key=parts.get)
        t["stdout"] = TIMING.sub("", stdout)
        if a.kernel_stats:
            t["kernels"] = kernel_stats(cmd, exe, work, "validator")
        drop["sam_validator"] = t
        exe = os.path.join(ROOT, "rsem_amd", "bin", "rsem-get-unique")
        timed(u_cmd, exe, work, env)
        wall, stdout = timed(u_cmd, exe, work, env)
        t = json.loads(TIMING.search(stdout).group(1))
        t["wall_s_outside"] = round(wall, 4)
        parts = {"inflate and cut": t["inflate_cut_s"], "fields": t["fields_s"], "device call": t["device_call_s"], "deflate": t["deflate_s"], "write": t["write_s"]}
        t["dominant_stage"] = max(parts, key=parts.get)
        t["inflated_sha256"], t["inflated_bytes"] = sha256_inflated(out)
        t["bytes"] = os.path.getsize(out)
        if a.kernel_stats:
            t["kernels"] = kernel_stats(u_cmd, exe, work, "unique")
        drop["get_unique"] = t
    if "reference" in doc and "drop_in" in doc:
        r, d = doc["reference"], doc["drop_in"]
        if "sam_validator" in r:
            doc["validator_stdout_equal"] = r["sam_validator"]["stdout"] == d["sam_validator"]["stdout"]
        if "get_unique" in r:
            doc["unique_outputs_equal"] = r["get_unique"]["inflated_sha256"] == d["get_unique"]["inflated_sha256"]
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))
    if doc.get("validator_stdout_equal") is False or doc.get("unique_outputs_equal") is False:
        sys.exit("the outputs differ from the reference's")


if __name__ == "__main__":
    main()
