"""The process a profiler wraps for the start-list measurements: a fresh EM context at C3 (the library named by RSEM_HIP_LIB),
10 + N rounds of rsem_em_run.   usage: start_list_profile_run.py N"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rsem_amd import capi  # noqa: E402
from tools.synth_data import make_em_workload  # noqa: E402

n = int(sys.argv[1])
wl = make_em_workload("C3")
ctx = capi.EmContext(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
ctx.run(wl["theta0"], wl["N0"], min_round=10, max_round=10)
out = ctx.run(wl["theta0"], wl["N0"], min_round=n, max_round=n)
print("rounds", out["rounds"], "physical_bytes_per_launch", ctx.info("physical_bytes_per_launch"))
ctx.close()
