#!/usr/bin/env python3
"""One summary of two profile runs of the plain bench command (each a run of its own): the fused k_knn launch's average from
`rocprofv3 --kernel-trace --stats`, and its instruction counters per launch from one `rocprofv3 --pmc` pass without tracing.
usage: tools/knn_profile_summary.py <trace dir> <pmc dir> <label> > profiles/<name>.json"""
import csv, glob, json, os, sys
from collections import defaultdict

trace_dir, pmc_dir, label = sys.argv[1:4]
KERNEL = "k_knn<16,true,0,false,false,1>"
same = lambda name: KERNEL in name.replace(" ", "")
out = {"label": label, "workload": "uniform_10m_k15", "kernel": KERNEL,
       "trace_command": "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --steps 10 --warmup 2",
       "pmc_command": "rocprofv3 --pmc SQ_INSTS SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD "
                      "GRBM_GUI_ACTIVE --output-format csv -- python bench.py --steps 3 --warmup 1   (no tracing in this run)"}
for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        if same(row["Name"]):
            out["k_knn_launches"] = int(row["Calls"])
            out["k_knn_avg_ms"] = float(row["AverageNs"]) * 1e-6
            out["k_knn_min_ms"], out["k_knn_max_ms"] = float(row["MinNs"]) * 1e-6, float(row["MaxNs"]) * 1e-6
acc = defaultdict(list)
for f in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        if same(row.get("Kernel_Name", "")):
            acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
out["counters_per_launch"] = {c: sum(v) / len(v) for c, v in sorted(acc.items())}
out["counter_launches"] = max((len(v) for v in acc.values()), default=0)
c = out["counters_per_launch"]
if "SQ_INSTS" in c:
    named = sum(c.get(n, 0.0) for n in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_LDS", "SQ_INSTS_BRANCH"))
    out["other_instructions_per_launch (s_waitcnt, s_nop, s_setprio, vector memory)"] = c["SQ_INSTS"] - named
if "GRBM_GUI_ACTIVE" in c and "k_knn_avg_ms" in out:
    # (GRBM_GUI_ACTIVE counts every XCD's busy cycles: / 8.  The counter run serialises launches, so its own launch time is not the
    #  traced one; the clock is the busy cycles of a counted launch over the traced average -- an estimate good to the few per cent
    #  the two runs' launch times differ by)
    out["shader_clock_hz"] = c["GRBM_GUI_ACTIVE"] / 8.0 / (out["k_knn_avg_ms"] * 1e-3)
    out["shader_clock_source"] = "GRBM_GUI_ACTIVE / 8 per counted launch over the traced launch's average duration"
json.dump(out, sys.stdout, indent=1)
print()
