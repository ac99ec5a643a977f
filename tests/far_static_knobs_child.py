"""Child process of tests/test_em_far_seams_gpu.py::test_static_knobs_in_a_child_process: RSEM_HIP_ROWSUM_BATCHED and
RSEM_HIP_COLSUM_XCD are read once per process, so the instantiations they choose need a process of their own.  Runs the seam input
and three sizes of the colsum family (tests/far_cases.py) against the oracle and prints its verdict as one JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import far_cases as fc  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402
from rsem_amd import capi  # noqa: E402


def case(d):
    oc = orc.em_estep(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"], d["theta0"])
    oc[0] += d["N0"]
    ctx = capi.EmContext(d["M"], d["row_ptr"], d["sid"], d["conprb"], d["ncp"])
    F = ctx.debug_far()
    fp, nxs = F["far_ptr"].astype(np.int64), F["n_x_slots"]
    w = np.arange((nxs + 63) // 64)
    nw = fp[np.minimum(64 * (w + 1), nxs)] - fp[64 * w]
    counts, theta_new, _, _, _ = ctx.step(d["theta0"], d["N0"])
    ok = bool(np.allclose(counts, oc, rtol=1e-9, atol=1e-9) and np.allclose(theta_new, oc / oc.sum(), rtol=1e-9, atol=1e-12))
    ctx.close()
    return dict(ok=ok, split_rows=int(fc.expected_layout(d)["split"].sum()), far_entries=F["n_far"], grid=max(1, -(-F["n_far"] // fc.COLSUM_WG)),
                waves_over_cap=int((nw > fc.ROWSUM_CAP).sum()), waves_staged=int(((nw > 0) & (nw <= fc.ROWSUM_CAP)).sum()),
                max_abs_diff=float(np.abs(counts - oc).max()))


def main():
    knobs = {k: os.environ.get(k) for k in ("RSEM_HIP_ROWSUM_BATCHED", "RSEM_HIP_COLSUM_XCD")}
    cases = {"seams": case(fc.seams())}
    for n in (1, 8 * 1024 + 1, 16 * 1024 + 1):
        cases["colsum %d" % n] = case(fc.colsum_family(n, "runs"))
    print(json.dumps(dict(knobs=knobs, cases=cases)))


if __name__ == "__main__":
    main()
