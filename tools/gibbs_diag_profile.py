"""Time rsem_gibbs_diagnose at the shape of BASELINE configs[3]'s Gibbs stage: M = 200 000 transcripts, 8 chains x 125 kept samples
of generated counts (0.8 GB of count vectors), for several values of RSEM_GIBBS_DIAG_L0.

    python tools/gibbs_diag_profile.py [--M 200000] [--chains 8] [--samples 125] [--L0 7,15,31] [--reps 3] [--out file.json]

Prints one JSON line per L0: upload_ms, kernel_ms (best of --reps), the time of ONE streaming read of the uploaded blocks at the
device's measured read rate (rsem_hip_stream_probe) and kernel_ms as a multiple of it, and the share of transcripts that went to
the long path.  The counts are AR(1) series per transcript, rounded: 70 % with phi = 0.2, 20 % 0.7, 8 % 0.9, 2 % 0.98 -- how fast
real chains mix is the data's business; the mix is there so that every L0 has a long path to pay for.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def generate(M, chains, samples, seed=3):
    rng = np.random.default_rng(seed)
    phi = rng.choice([0.2, 0.7, 0.9, 0.98], size=M + 1, p=[0.7, 0.2, 0.08, 0.02])
    centre = 10.0 ** rng.uniform(0.5, 4.0, M + 1)
    sd = np.sqrt(centre)
    a = np.sqrt(1.0 - phi * phi)
    cvs = []
    for _ in range(chains):
        z = rng.standard_normal(M + 1)
        out = np.empty((samples, M + 1), np.int32)
        for s in range(samples):
            z = phi * z + a * rng.standard_normal(M + 1)
            out[s] = np.maximum(np.rint(centre + sd * z), 0.0)
        cvs.append(out)
    return cvs, phi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=200000)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--samples", type=int, default=125)
    ap.add_argument("--L0", default="7,15,31")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rsem_amd import capi
    assert capi.device_count() >= 1, "needs a GPU"
    cvs, _ = generate(args.M, args.chains, args.samples)
    nbytes = sum(a.nbytes for a in cvs)
    read_gbps, _ = capi.stream_probe(0, 1 << 30, 5)
    n_used = 2 * (args.samples // 2)
    stream_ms = args.chains * n_used * (args.M + 1) * 4 / (read_gbps * 1e9) * 1e3
    results = []
    for L0 in [int(x) for x in args.L0.split(",")]:
        os.environ["RSEM_GIBBS_DIAG_L0"] = str(L0)
        capi.gibbs_diagnose(cvs)  # warm-up: code object, first touch
        best = None
        for _ in range(args.reps):
            sm = capi.gibbs_diagnose(cvs)[5]
            if best is None or sm["kernel_ms"] < best["kernel_ms"]:
                best = sm
        r = dict(M=args.M, chains=args.chains, samples=args.samples, count_vector_bytes=nbytes, L0=L0, upload_ms=best["upload_ms"],
                 kernel_ms=best["kernel_ms"], stream_read_GBps=read_gbps, one_streaming_read_ms=stream_ms,
                 kernel_over_streaming_read=best["kernel_ms"] / stream_ms, n_long=best["n_long"], long_share=best["n_long"] / args.M,
                 max_rhat=best["max_rhat"], min_ess=best["min_ess"])
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
