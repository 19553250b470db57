"""Per-launch durations of the coordinate plan from a kernel trace of `bench.py --full` (profiles/in_flight_trace.sh /
in_flight_counters.sh pass T): median duration of every plan launch, seven in flight (the timed region's steady state) and alone
(the one-scene-in-flight side pass at the end of the run).  Launches are told apart by kernel name and grid (workgroups, y).
    python profiles/plan_launches.py <trace dir or kernel_trace.csv[.gz]> <bench json of the trace run> [<label>]"""
import collections
import csv
import gzip
import json
import statistics
import sys

from in_flight_summary import family, find


def main():
    tdir, bench_json = sys.argv[1:3]
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    bench = json.loads(open(bench_json).read().strip().splitlines()[-1])
    steps = bench["steps"]
    tfile = tdir if tdir.endswith((".gz", ".csv")) else find(tdir, "kernel_trace.csv")
    rows = list(csv.DictReader(gzip.open(tfile, "rt") if tfile.endswith(".gz") else open(tfile)))

    def grid(r):
        g = [int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")]
        w = [max(1, int(r[k])) for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")]
        return g[0] // w[0], max(1, g[1] // w[1])

    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid(r)) for r in rows)
    heads = [e for e in ev if family(e[2]) == "head"]
    iso = 2 * 4 + max(min(steps, 48), 24)              # the side pass: 8 warm scenes + the measured ones (in_flight_summary.py)
    assert len(heads) >= steps + iso, (len(heads), steps, iso)
    t_lo, t_hi = heads[-(steps + iso) + 20][0], heads[-(iso + 20) - 1][1]
    t_iso = heads[-(iso - 8) - 1][1]
    dur = {"in flight": collections.defaultdict(list), "alone": collections.defaultdict(list)}
    for s, e, n, g in ev:
        if family(n) != "plan":
            continue
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        where = "in flight" if t_lo < s < t_hi else "alone" if s > t_iso else None
        if where:
            dur[where][(short, g)].append((e - s) * 1e-3)
    scenes = {"in flight": len([h for h in heads if t_lo < h[1] <= t_hi]), "alone": iso - 8}
    print("%s: plan launches, median us (launches per scene) - %.1f scenes/s under the tracer" % (label, bench["value"]))
    print("%-26s %6s %3s %18s %18s" % ("kernel", "wgs", "y", "in flight", "alone"))
    keys = sorted(set(dur["in flight"]) | set(dur["alone"]), key=lambda k: (k[0], -k[1][0], k[1][1]))
    tot = {"in flight": 0.0, "alone": 0.0}
    for k in keys:
        cells = []
        for w in ("in flight", "alone"):
            v = dur[w].get(k)
            if v:
                per = len(v) / scenes[w]
                tot[w] += sum(v) / scenes[w]
                cells.append("%8.1f (%4.2f)" % (statistics.median(v), per))
            else:
                cells.append("%15s" % "-")
        print("%-26s %6d %3d %18s %18s" % (k[0][:26], k[1][0], k[1][1], cells[0], cells[1]))
    print("%-26s %10s %18.1f %18.1f   (sum of plan kernel time per scene, us)" % ("all plan launches", "", tot["in flight"], tot["alone"]))


if __name__ == "__main__":
    main()
