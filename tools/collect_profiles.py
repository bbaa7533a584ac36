#!/usr/bin/env python3
"""Copies the evidence of the last tools/gpu_check.sh + tools/gpu_pmc.sh runs from $OUT (default out/) into profiles/ under a tag:

    python tools/collect_profiles.py r01_e [kernel-name-substring]

Writes <tag>_bench.json, <tag>_kernel_stats.csv, <tag>_pmc_summary.csv, <tag>_pmc_traffic.json."""
import collections
import csv
import glob
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1]
key = sys.argv[2] if len(sys.argv) > 2 else "step_kernel"
out = os.environ.get("PROFILES_OUT", os.path.join(ROOT, "profiles"))     # or a directory under $OUT (the raw counter csvs are then deleted there)
go = os.path.join(ROOT, os.environ.get("OUT", "out"))
os.makedirs(out, exist_ok=True)

shutil.copy(os.path.join(go, "bench.json"), os.path.join(out, f"{tag}_bench.json"))
stats = sorted(glob.glob(os.path.join(go, "prof", "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
shutil.copy(stats[-1], os.path.join(out, f"{tag}_kernel_stats.csv"))

rows, means = [], {}
for name in ("sq1", "sq2", "fetch", "write", "grbm"):
    acc = collections.defaultdict(list)
    for f in glob.glob(os.path.join(go, "pmc", name, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if key in row["Kernel_Name"]:
                acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
    for k in sorted(acc):
        v = acc[k]
        rows.append((name, k, len(v), sum(v) / len(v)))
        means[k] = sum(v) / len(v)
with open(os.path.join(out, f"{tag}_pmc_summary.csv"), "w") as f:
    f.write("pass,counter,dispatches,mean_per_dispatch\n")
    for r in rows:
        f.write("%s,%s,%d,%.1f\n" % r)
bench = json.load(open(os.path.join(go, "bench.json")))
traffic = {
    "num_envs": bench["config"]["num_envs_per_gpu"],
    "kernel": bench["roofline"]["kernel"],
    "FETCH_SIZE_KB": means["FETCH_SIZE"],
    "WRITE_SIZE_KB": means["WRITE_SIZE"],
    "correction": "FETCH_SIZE doubled (gfx950 reports 1/2 of streamed read bytes, MI355X_MICROARCH.md HBM section); WRITE_SIZE as is; "
                  "separate --pmc passes with --kernel-trace only",
    "hbm_bytes_per_launch": int(round((2 * means["FETCH_SIZE"] + means["WRITE_SIZE"]) * 1024)),
}
json.dump(traffic, open(os.path.join(out, f"{tag}_pmc_traffic.json"), "w"), indent=1)
print(json.dumps(traffic))
