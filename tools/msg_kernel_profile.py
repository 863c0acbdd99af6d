"""The DHGN message kernels (k_msgw*, k_msg_ones_sorted_*, k_msg_agg_bwd_reduce) of a rocprofv3 run, one line per (kernel, grid): the
rollout's launches and the update's differ by their grid, so the two are kept apart.
  python tools/msg_kernel_profile.py <..._kernel_trace.csv | ..._counter_collection.csv> [out.csv]
kernel trace (rocprofv3 --kernel-trace): calls, mean / min / max us per call.
counter pass (rocprofv3 --pmc, a run of its own): mean of every counter per call, and from SQ_WAVES / SQ_WAVE_CYCLES / SQ_BUSY_CYCLES (the
SQ cycle counters are in quad-cycles) the instructions and wave-cycles per wave."""
import csv, re, sys
from collections import defaultdict


def short(name):
    m = re.search(r"(k_msg\w+)(<[^>]*>)?", name)
    return (m.group(1) + (m.group(2) or "")).replace(" ", "") if m else None


rows = list(csv.DictReader(open(sys.argv[1])))
out = []
if "Counter_Name" in rows[0]:
    acc = defaultdict(lambda: defaultdict(list))
    for r in rows:
        k = short(r["Kernel_Name"])
        if k:
            acc[(k, int(r["Grid_Size"]) // int(r["Workgroup_Size"]), int(r["Workgroup_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    names = sorted({c for v in acc.values() for c in v})
    hdr = ["kernel", "workgroups", "workgroup_size", "calls"] + names + ["wave_cycles_per_wave", "valu_per_wave", "salu_per_wave", "smem_per_wave", "branch_per_wave"]
    for (k, g, wg), v in sorted(acc.items()):
        mean = {c: sum(x) / len(x) for c, x in v.items()}
        w = mean.get("SQ_WAVES", 0) or float("nan")
        out.append([k, g, wg, len(next(iter(v.values())))] + [round(mean.get(c, float("nan")), 1) for c in names] +
                   [round(4 * mean.get("SQ_WAVE_CYCLES", float("nan")) / w, 1)] +
                   [round(mean.get(c, float("nan")) / w, 1) for c in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_BRANCH")])
else:
    acc = defaultdict(list)
    for r in rows:
        k = short(r["Kernel_Name"])
        if k:
            acc[(k, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]), int(r["Workgroup_Size_X"]), r["VGPR_Count"], r["SGPR_Count"])].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    hdr = ["kernel", "workgroups_x", "grid_y", "workgroup_size", "vgprs", "sgprs", "calls", "mean_us", "min_us", "max_us", "total_ms"]
    for key, v in sorted(acc.items()):
        out.append(list(key) + [len(v), round(sum(v) / len(v), 1), round(min(v), 1), round(max(v), 1), round(sum(v) / 1e3, 2)])
w = csv.writer(open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout)
w.writerow(hdr)
w.writerows(out)
if len(sys.argv) > 2:
    for r in [hdr] + out:
        print(",".join(str(x) for x in r))
