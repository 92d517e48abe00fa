#!/usr/bin/env python3
"""Means per launch of one counter from a rocprofv3 --pmc counter_collection.csv, per kernel, and for the 7 resize launches of a step per level
(dispatch order).   usage: pmc_per_launch.py <counter_collection.csv> <COUNTER>   (FETCH_SIZE / WRITE_SIZE are in KiB; printed in MB)"""
import collections, csv, re, sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if r["Counter_Name"] == sys.argv[2]]
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
per = collections.defaultdict(list)
lev = collections.defaultdict(list)
i = 0
for r in rows:
    name = re.split(r"[(<]", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", ""))[0].strip()
    if name.startswith("at::") or "rocclr" in name:
        continue
    per[name].append(float(r["Counter_Value"]))
    if name == "resize_kernel":
        lev[i % 7 + 1].append(float(r["Counter_Value"]))
        i += 1
for k in sorted(per):
    print("%-28s %s %9.1f MB per launch (%d launches)" % (k, sys.argv[2], sum(per[k]) / len(per[k]) * 1024 / 1e6, len(per[k])))
for l in sorted(lev):
    print("resize level %d                %s %9.1f MB" % (l, sys.argv[2], sum(lev[l]) / len(lev[l]) * 1024 / 1e6))
