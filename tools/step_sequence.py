"""Every launch of one training step in launch order, from a rocprofv3 --kernel-trace CSV: position, start
offset, duration averaged over the last K steps (a replayed graph launches the same kernels every step; launches are
matched by name, grid and occurrence; when the steps differ only the last one is printed), grid and name.  What a
per-launch table of one stack (e.g. the vote aggregation's layers between group_first_fwd_k<64> and pool_select_k) is read from.
usage: python tools/step_sequence.py <kernel_trace.csv> [K=5] [steps to drop at the end=0]
ONLY=<regex>: print only the launches whose kernel name matches (positions and offsets stay those of the whole step)."""
import csv
import os
import re
import sys

path = sys.argv[1]
K = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SKIP = int(sys.argv[3]) if len(sys.argv) > 3 else 0
rows = list(csv.DictReader(open(path)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "fps_reg_kernel<1024, 20>" in r["Kernel_Name"]
         or "fps_prune_kernel<20" in r["Kernel_Name"] or "fps_pair_kernel<20" in r["Kernel_Name"]]
steps = [rows[marks[-2 - SKIP - j]:marks[-1 - SKIP - j]] for j in range(K)]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
def keyed(step):
    """launch -> (name, grid, occurrence index inside the step): launches of concurrent streams interleave
    differently from step to step, their j-th occurrence is the same launch of the graph"""
    seen, out = {}, []
    for r in step:
        k = (r["Kernel_Name"], r.get("Grid_Size_X", r.get("Grid_Size", "?")))
        j = seen.get(k, 0)
        seen[k] = j + 1
        out.append(k + (j,))
    return out


keys = [keyed(s) for s in steps]
if any(sorted(k) != sorted(keys[0]) for k in keys):
    steps, keys = steps[:1], keys[:1]
durs = [{k: dur(r) for k, r in zip(ks, s)} for ks, s in zip(keys, steps)]
one = steps[0]
t0 = int(one[0]["Start_Timestamp"])
print("# %d launches per step, durations averaged over %d step(s)" % (len(one), len(steps)))
only = re.compile(os.environ["ONLY"]) if os.environ.get("ONLY") else None
for i, r in enumerate(one):
    if only is not None and not only.search(r["Kernel_Name"]):
        continue
    d = [m[keys[0][i]] for m in durs]
    print("%4d @%8.1f %8.1f us (min %7.1f max %7.1f)  grid %-8s wg %-5s %s" % (
        i, (int(r["Start_Timestamp"]) - t0) / 1e3, sum(d) / len(d), min(d), max(d),
        r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")),
        r["Kernel_Name"][:150]))
