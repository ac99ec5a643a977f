#!/usr/bin/env python3
"""Wall clocks of the three reference-preparation programs on one host, the reference's (oracle/_ref/) and then the drop-ins
(rsem_amd/bin/), one after the other on a generated genome (tools/gen_genome.py), every step under its own `timeout -k 10`; the
outputs are compared by SHA-256 and the result goes to profiles/refprep_<size>.json.

    python tools/time_refprep.py [--chromosomes 6] [--bases 100000000] [--transcripts 100000] [--seed 1] [--limit 600] [--keep DIR]

The JSON holds the wall clock of each program from both sides; for the drop-ins the stages (read and frame, upload, kernels by HIP
events, download, write: RSEM_REFPREP_STAGES) and the bytes the two kernels read and write, by construction (the load kernels read a
batch's raw bytes twice and write its bases; the gather reads and writes every segment's bytes, fills are written only); and the
kernels' rate beside the device's streaming rate (rsem_hip_stream_probe, the probe bench.py --full reports)."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROGRAMS = ("rsem-extract-reference-transcripts", "rsem-preref", "rsem-synthesis-reference-transcripts")


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def timed(argv, cwd, limit, env=None):
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=cwd, env=e, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s: status %d after %.1f s\n%s" % (argv[0], r.returncode, dt, r.stderr.decode(errors="replace")[-2000:]))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chromosomes", type=int, default=6)
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--transcripts", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--limit", type=int, default=600, help="seconds a step may take")
    ap.add_argument("--keep", default=None, help="work here and keep the files")
    ap.add_argument("--no-probe", action="store_true")
    a = ap.parse_args()
    import gen_genome
    work = a.keep or tempfile.mkdtemp(prefix="refprep_")
    os.makedirs(work, exist_ok=True)
    t0 = time.perf_counter()
    lengths = gen_genome.write(work, a.seed, a.chromosomes, a.bases, a.transcripts, 0.02)
    gen_s = time.perf_counter() - t0
    sides = {"reference": os.path.join(ROOT, "oracle", "_ref"), "dropin": os.path.join(ROOT, "rsem_amd", "bin")}
    out = {"genome_bases": int(sum(lengths)), "chromosomes": a.chromosomes, "transcripts_in_gtf": a.transcripts, "seed": a.seed, "generate_s": gen_s,
           "genome_file_bytes": os.path.getsize(os.path.join(work, "genome.fa")), "wall_s": {}, "stages": {}, "sha256_equal": {}}
    for side, bindir in sides.items():
        d = os.path.join(work, side)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        steps = (("rsem-extract-reference-transcripts", ["out", "1", "../genes.gtf", "None", "0", "../genome.fa"]),
                 ("rsem-preref", ["out.transcripts.fa", "0", "out", "-l", "125", "-q"]),
                 ("rsem-synthesis-reference-transcripts", ["syn", "1", "0", "out.transcripts.fa"]))
        out["wall_s"][side] = {}
        for prog, args in steps:
            stages = os.path.join(d, prog + ".stages.json")
            out["wall_s"][side][prog] = timed([os.path.join(bindir, prog)] + args, d, a.limit, {"RSEM_REFPREP_STAGES": stages} if side == "dropin" else None)
            if side == "dropin":
                with open(stages) as f:
                    s = json.load(f)
                os.remove(stages)
                s["note"] = "upload_ms, kernel_ms, download_ms are spans between HIP events on the stream, not transfer rates: the host's part of a copy from pageable memory is in device_calls_ms"
                s["load_kernels_bytes"] = 2 * s["raw_bytes"] + s["n_bases"]
                s["gather_kernel_bytes_at_most"] = 2 * s["gathered_bytes"]
                s["kernel_GBps"] = (s["load_kernels_bytes"] + s["gather_kernel_bytes_at_most"]) / max(s["kernel_ms"], 1e-9) / 1e6
                out["stages"][prog] = s
            print("%-9s %-40s %8.2f s" % (side, prog, out["wall_s"][side][prog]), flush=True)
    names = sorted(os.listdir(os.path.join(work, "reference")))
    assert names == sorted(os.listdir(os.path.join(work, "dropin"))), "the two sides wrote different files"
    for fn in names:
        out["sha256_equal"][fn] = sha256(os.path.join(work, "reference", fn)) == sha256(os.path.join(work, "dropin", fn))
    out["all_equal"] = all(out["sha256_equal"].values())
    out["speedup"] = {p: out["wall_s"]["reference"][p] / out["wall_s"]["dropin"][p] for p in PROGRAMS}
    if not a.no_probe:
        from rsem_amd import capi
        r, c = capi.stream_probe(0, 2 << 30, 3)
        out["stream_probe_GBps"] = {"read": r, "copy": c}
    size = "%dmbases" % round(sum(lengths) / 1e6)
    path = os.path.join(ROOT, "profiles", "refprep_%s.json" % size)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("genome_bases", "all_equal", "speedup")}))
    print("wrote", path)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 0 if out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
