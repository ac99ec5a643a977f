"""Option sid_start_list switched on / off / on ... inside ONE EM context (same layout, same tuned unit order: the kernels are handed the
list or a null pointer), a 100-round headline region and an event-timed 64-round region each, eight of each
(profiles/r11_start_list_ab.json, "in_one_context").

usage: start_list_in_context.py OUT.json CONFIG [VALUE_BITS]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rsem_amd import capi  # noqa: E402
from tools.synth_data import make_em_workload  # noqa: E402


def main():
    outp, config = sys.argv[1], sys.argv[2]
    bits = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    wl = make_em_workload(config)
    ctx = capi.EmContext(wl["M"], wl["row_ptr"], wl["sid"], wl["conprb"], wl["ncp"])
    if bits == 32:
        ctx.set_option("value_bits", 32)

    def none():
        return None
    bench.headline_steps(ctx, wl, wl["N0"], 100, 10, none, none)
    ms = {1: [], 0: []}
    launch = {1: [], 0: []}
    for r in range(8):
        for on in (1, 0):
            ctx.set_option("sid_start_list", on)
            ms[on].append(bench.headline_steps(ctx, wl, wl["N0"], 100, 0, none, none)[0] * 10)
            launch[on].append(bench.launch_ms(ctx, wl, wl["N0"], 64))
    phys = {}
    for on in (1, 0):
        ctx.set_option("sid_start_list", on)
        phys[on] = ctx.info("physical_bytes_per_launch")
    rec = dict(config=config, value_bits=bits, ms_per_round_on=ms[1], ms_per_round_off=ms[0], estep_launch_ms_on=launch[1], estep_launch_ms_off=launch[0],
               physical_bytes_on=phys[1], physical_bytes_off=phys[0], units=ctx.info("units"), units_compact=ctx.info("units_compact"),
               units_main=ctx.info("units_main"))
    with open(outp, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
