"""fam_summary.py LABEL DIR: a rocprofv3 output directory (kernel trace, optionally one --pmc counter) -> per family of the
finish / fine-level convolution kernels: launches per scene, mean duration per launch, counter sum per scene.
Scenes = head_joint launches of the whole run (warm-up included: same launch policy)."""
import collections
import csv
import glob
import sys

label, d = sys.argv[1:3]


def find(pat):
    f = glob.glob("%s/**/*%s" % (d, pat), recursive=True)
    return sorted(f)[-1] if f else None


def fam(r):
    n = r["Kernel_Name"]
    if "conv_finish_small" in n:
        return "conv_finish_small"
    if "conv_finish" in n:
        return "conv_finish (other)"
    if "conv_hd" in n:
        return "conv_hd"
    if "conv_hl" in n:
        try:
            gz = int(r["Grid_Size_Z"]) // max(1, int(r["Workgroup_Size_Z"]))
            gx = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
        except (KeyError, ValueError):
            return "conv_hl"
        return "conv_hl mask-sorted" if gz == 3 and gx >= 64 else "conv_hl (other)"
    if "head_" in n:
        return "head"
    return None


t = find("kernel_trace.csv")
rows = list(csv.DictReader(open(t)))
scenes = sum(1 for r in rows if "head_joint" in r["Kernel_Name"] or "head_" in r["Kernel_Name"])
dur = collections.defaultdict(float)
cnt = collections.Counter()
tot = 0.0
for r in rows:
    dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    tot += dt
    f = fam(r)
    if f:
        dur[f] += dt
        cnt[f] += 1
print("%s: %d kernels, %d scenes, %.1f us of kernel time per scene" % (label, len(rows), scenes, tot / max(scenes, 1)))
ctr = collections.defaultdict(lambda: collections.defaultdict(float))
c = find("counter_collection.csv")
names = []
if c:
    crow = list(csv.DictReader(open(c)))
    by_id = {}
    for r in rows:
        by_id[r.get("Dispatch_Id")] = r
    for r in crow:
        base = by_id.get(r.get("Dispatch_Id"), r)
        f = fam(base if "Grid_Size_Z" in base else r) or "(all other)"
        ctr[f][r["Counter_Name"]] += float(r["Counter_Value"])
        ctr["(every kernel)"][r["Counter_Name"]] += float(r["Counter_Value"])
    names = sorted({k for v in ctr.values() for k in v})
print("%-22s %10s %14s %14s " % ("family", "launches", "us / launch", "us / scene") + " ".join("%18s" % (n + " MB/scene") for n in names))
for f in sorted(set(cnt) | set(ctr)):
    if f == "head":
        continue
    n = cnt.get(f, 0)
    # FETCH_SIZE / WRITE_SIZE count kilobytes
    print("%-22s %10.1f %14.2f %14.1f " % (f, n / max(scenes, 1), dur[f] / max(n, 1), dur[f] / max(scenes, 1)) +
          " ".join("%18.2f" % (ctr[f].get(k, 0.0) / 1024.0 / max(scenes, 1)) for k in names))
