"""One sample of the start-list measurements (profiles/r11_start_list_ab.json): a fresh process and EM context, the library named by
RSEM_HIP_LIB (unset: the tree's), the workload from RSEM_WL_CACHE where set.  The headline region of bench.py (bench.headline_steps:
10 untimed rounds, then 100 timed rounds in one rsem_em_run call) REGIONS times -- the first region is the sample's figure --, then
the average E-step launch time by HIP events (bench.launch_ms) and the info keys of the byte accounting.

usage: start_list_sample.py TAG OPT OUT.json [CONFIG] [DUMPDIR]
  OPT       -1: leave option sid_start_list alone (a library without it), 0 / 1: set it
  CONFIG    a workload of tools/synth_data.py (default C3)
  DUMPDIR   theta.npy / counts.npy of the last region go there
environment: START_LIST_VALUE_BITS=32 (Q32 planes), START_LIST_REGIONS (default 5)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from rsem_amd import capi  # noqa: E402
from tools.synth_data import make_em_workload  # noqa: E402

INFO_KEYS = ("physical_bytes_per_launch", "sid_plane_bytes_loaded", "sid_plane_bytes", "value_plane_bytes", "slices", "slots", "units", "units_compact",
             "units_main", "start_list_entries", "start_list_bytes", "sid_first_slice_planes", "start_list_entries_loaded", "start_list_slices",
             "sid_marked_planes_far_queue")


def main():
    tag, opt, outp = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    config = sys.argv[4] if len(sys.argv) > 4 else "C3"
    dump = sys.argv[5] if len(sys.argv) > 5 else None
    t0 = time.time()
    wl = make_em_workload(config)
    t1 = time.time()
    ctx = capi.EmContext(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
    if os.environ.get("START_LIST_VALUE_BITS") == "32":
        ctx.set_option("value_bits", 32)
    if opt >= 0:
        ctx.set_option("sid_start_list", opt)
    t2 = time.time()

    def none():   # (rsem_em_run hands theta back to the host: the call itself ends in a device synchronise)
        return None
    regions, out = [], None
    for r in range(int(os.environ.get("START_LIST_REGIONS", "5"))):
        el, out = bench.headline_steps(ctx, wl, wl["N0"], 100, 10 if r == 0 else 0, none, none)
        regions.append(el / 100 * 1e3)
    launch = bench.launch_ms(ctx, wl, wl["N0"], 100)
    info = {}
    for k in INFO_KEYS:
        try:
            info[k] = ctx.info(k)
        except Exception:   # (a library from before the key existed)
            info[k] = None
    if dump:
        bench.dump_outputs(dump, out)
    rec = dict(tag=tag, opt=opt, config=config, ms_per_step_first_region=regions[0], ms_regions=regions, estep_avg_launch_ms=launch,
               rounds=out["rounds"], info=info, load_s=t1 - t0, ctx_s=t2 - t1)
    with open(outp, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
