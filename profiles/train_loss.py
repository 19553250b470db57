"""What the training losses cost as torch ops and on the row-loss kernels (csrc/row_loss.hip), on one fixed batch of
3 x 80 000 voxels of synthetic scenes.

    python profiles/train_loss.py [--out profiles/train/row_loss.txt] [--points 80000] [--repeats 3] [--no-trace]

(a) the loss alone, forward plus backward on a fixed network output [240 000, 64] / [240 000, 8]: train.joint_loss against
    train.joint_loss_device, train.separate_loss_packed against device_rows=True; HIP events around 50 iterations after a
    warm-up of 10, the two variants of a pair alternating
(b) train.train_step and train.train_step_separate with and without device_loss on the same batches: events around 12 steps
    after a warm-up of 4, alternating (each variant its own model and optimizer from one seed)
(c) launches per iteration of each loss: rocprofv3 --kernel-trace --stats runs of their own (two per loss, 10 and 30
    iterations: the difference over 20 leaves the start-up out)
(d) from the same traces, the medians of the three row-loss kernels against their algorithmic bytes over the HBM peak
    (n ld 4 read forward; the same plus n grad_ld 4 written backward; labels n (8 + 24)), 8.0 TB/s
Every repeat of (a) and (b) is a child process of its own under a time limit; the first child that fails ends the run.  The
text file holds every repeat's figures, the medians over the repeats and their spread (min .. max)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
LOSSES = ("joint_torch", "joint_device", "separate_torch", "separate_device")


def _batches(points, dev):
    import torch

    from canonicalvoting_amd.data import SyntheticScanDataset, SyntheticSymDataset, collate_fn, collate_sym, sym_to_device
    joint = collate_fn([SyntheticScanDataset(3, points, seed0=7000)[i] for i in range(3)])
    _, coords, feats, xyz, scale, cls = joint
    joint = (coords.to(dev), feats.to(dev) * 2 - 1, xyz.to(dev), scale.to(dev), cls.to(dev))
    _, coords, feats, sym, scale, obj, _ = collate_sym([SyntheticSymDataset(3, points, seed0=7000)[i] for i in range(3)])
    sep = (coords.to(dev), feats.to(dev) * 2 - 1, sym_to_device(sym, dev), scale.to(dev), obj.to(dev))
    torch.cuda.synchronize()
    return joint, sep


def _loss_fns(joint, sep, dev):
    """name -> a closure running forward and backward of one loss on a fixed output"""
    import torch

    from canonicalvoting_amd import train
    n = joint[0].shape[0]
    g = torch.Generator(device="cpu").manual_seed(5)
    out64 = (torch.randn(n, 64, generator=g) * 0.5).to(dev).requires_grad_(True)
    out8 = (torch.randn(sep[0].shape[0], 8, generator=g) * 0.5).to(dev).requires_grad_(True)

    def run(fn, out, *args, **kw):
        def go():
            out.grad = None
            fn(out, *args, **kw)[0].backward()
        return go

    return {"joint_torch": run(train.joint_loss, out64, joint[2], joint[3], joint[4]),
            "joint_device": run(train.joint_loss_device, out64, joint[2], joint[3], joint[4]),
            "separate_torch": run(train.separate_loss_packed, out8, sep[2], sep[3], sep[4]),
            "separate_device": run(train.separate_loss_packed, out8, sep[2], sep[3], sep[4], device_rows=True)}


def _events_ms(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def child_measure(points):
    import torch

    from canonicalvoting_amd import train
    from canonicalvoting_amd.minkunet import MinkUNet34C
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    joint, sep = _batches(points, dev)
    fns = _loss_fns(joint, sep, dev)
    res = {"rows": int(joint[0].shape[0])}
    for pair in (("joint_torch", "joint_device"), ("separate_torch", "separate_device")):
        acc = {k: [] for k in pair}
        for _ in range(3):                                              # alternate inside the process too
            for k in pair:
                acc[k].append(_events_ms(fns[k], 10, 50))
        res.update({"loss_" + k: statistics.median(v) for k, v in acc.items()})
    steps = {}
    for name, cout, step, batch in (("joint", 64, train.train_step, joint), ("separate", 8, train.train_step_separate, sep)):
        for device_loss in (False, True):
            torch.manual_seed(0)
            model = MinkUNet34C(3, cout).to(dev).train()
            opt = train.make_optimizer(model, lr=1e-3)
            steps["step_%s_%s" % (name, "device" if device_loss else "torch")] = \
                (lambda m=model, o=opt, s=step, b=batch, d=device_loss: s(m, o, *b, device_loss=d))
    acc = {k: [] for k in steps}
    for _ in range(2):
        for k, fn in steps.items():
            acc[k].append(_events_ms(fn, 4, 12))
    res.update({k: statistics.median(v) for k, v in acc.items()})
    print("RESULT " + json.dumps(res), flush=True)


def child_trace(which, iters, points):
    """`iters` iterations of one loss, for a kernel trace"""
    import torch
    dev = torch.device("cuda:0")
    joint, sep = _batches(points, dev)
    fn = _loss_fns(joint, sep, dev)[which]
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()


def _trace_rows(which, iters, points, limit):
    """kernel-trace rows [(name, ns)] of a rocprofv3 run of child_trace"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--child-trace", which, "--iters", str(iters), "--points", str(points)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel trace under %s" % d)
        rows = []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                rows.append((row["Kernel_Name"], int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
        return rows


def algorithmic_bytes(n, ld, grad_ld):
    fwd = n * ld * 4 + n * (8 + 24)
    return {"fwd": fwd, "bwd": fwd + n * grad_ld * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "row_loss.txt"))
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip (c) and (d), the rocprofv3 runs")
    ap.add_argument("--child-measure", action="store_true")
    ap.add_argument("--child-trace", default=None)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if a.child_measure:
        return child_measure(a.points)
    if a.child_trace:
        return child_trace(a.child_trace, a.iters, a.points)
    lines = ["training losses: torch ops against the row-loss kernels, 3 x %d voxels" % a.points, ""]
    reps = []
    for i in range(a.repeats):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-measure", "--points", str(a.points)],
                           capture_output=True, text=True, timeout=420)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            raise RuntimeError("repeat %d failed (%d):\n%s" % (i, r.returncode, r.stderr[-2000:]))
        reps.append(json.loads(got[-1][7:]))
        print("repeat %d: %s" % (i, reps[-1]), flush=True)
    n = reps[0]["rows"]
    lines.append("rows %d; HIP events; ms per iteration; median over %d child processes (min .. max); every repeat listed" % (n, a.repeats))
    for key in [k for k in reps[0] if k != "rows"]:
        v = [r[key] for r in reps]
        lines.append("  %-22s %8.3f  (%.3f .. %.3f)   %s" % (key, statistics.median(v), min(v), max(v), "  ".join("%.3f" % x for x in v)))
    for name in ("joint", "separate"):
        for kind in ("loss", "step"):
            t = [r["%s_%s_torch" % (kind, name)] for r in reps]
            d = [r["%s_%s_device" % (kind, name)] for r in reps]
            gain = statistics.median(t) - statistics.median(d)
            spread = max(max(t) - min(t), max(d) - min(d))
            lines.append("  %s %s: torch - device = %.3f ms, largest spread of either %.3f ms" % (name, kind, gain, spread))
    if not a.no_trace:
        lines += ["", "launches per iteration (rocprofv3 --kernel-trace --stats, runs of 10 and 30 iterations, difference / 20):"]
        kernels = {}
        for which in LOSSES:
            few, many = _trace_rows(which, 10, a.points, 300), _trace_rows(which, 30, a.points, 300)
            lines.append("  %-18s %.1f" % (which, (len(many) - len(few)) / 20.0))
            for name, ns in many:
                m = re.search(r"row_loss_\w+(<\d+>)?", name)
                if m:
                    kernels.setdefault((which, m.group(0)), []).append(ns)
        lines += ["", "row-loss kernels: median time, algorithmic bytes, share of the %.1f TB/s HBM peak:" % (HBM_PEAK / 1e12)]
        for (which, name), ns in sorted(kernels.items()):
            ld = 64 if which.startswith("joint") else 8
            b = algorithmic_bytes(n, ld, ld)
            nbytes = b["bwd"] if "backward" in name else (b["fwd"] if "partials" in name else 0)
            us = statistics.median(ns) / 1e3
            share = ("%5.1f %%" % (100.0 * nbytes / HBM_PEAK / (us * 1e-6))) if nbytes else "   -   "
            lines.append("  %-16s %-24s %8.2f us  %10d bytes  %s" % (which, name, us, nbytes, share))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
