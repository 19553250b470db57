"""What a training step of the per-category model costs with list labels and with packed symmetry labels.

    python profiles/train_separate.py [--out profiles/train/separate_step.txt] [--parent DIR] [--points 80000] [--steps 20]

Data: data.SyntheticSymDataset, 3 scenes of --points rows.  Fused Adam, MinkUNet34C(3, 8), one thread per process.  Rows:
  step, list labels    train.train_step_separate with data.collate_fn_separate's nested lists.  With --parent DIR (a checkout of
                       the parent commit with its library built) that tree's code runs it, otherwise this tree's list path, which
                       is the parent's code unchanged
  step, packed labels  train.train_step_separate with data.collate_sym's SymBatch, its copies from pinned memory included
  loss, list / packed  train.separate_loss / train.separate_loss_packed alone, forward + backward, on a fixed network output
Every row is measured in a child process of its own (time between two HIP events around all timed iterations, and wall time,
per iteration), the two step rows alternating over three repeats.  A child that fails ends the run.
Launch counts come from a separate run (no counters collected in it):
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/train_separate.py --worker loss-packed --items FILE --root .
"""
import os

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_k] = "1"

import argparse  # noqa: E402
import json  # noqa: E402
import pickle  # noqa: E402
import statistics  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402
import time  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(a):
    """one row in this process, with the package of --root"""
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    torch.set_num_threads(1)
    from canonicalvoting_amd import data, train
    from canonicalvoting_amd.minkunet import MinkUNet34C
    with open(a.items, "rb") as f:
        items = pickle.load(f)
    dev = torch.device("cuda:0")
    packed = a.worker.endswith("packed")
    batch = (data.collate_sym if packed else data.collate_fn_separate)(items)
    coords, feats = batch[1].to(dev), batch[2].to(dev) * 2 - 1
    labels, scale, obj = batch[3], batch[4], batch[5]
    if packed:
        labels = labels._replace(**{k: v.pin_memory() for k, v in labels._asdict().items() if torch.is_tensor(v)})
        scale, obj = scale.pin_memory(), obj.pin_memory()
    if a.worker.startswith("step"):
        torch.manual_seed(0)
        model = MinkUNet34C(3, 8).to(dev).train()
        opt = train.make_optimizer(model, lr=1e-3)
        run = lambda: train.train_step_separate(model, opt, coords, feats, labels, scale, obj)
    else:
        torch.manual_seed(0)
        out = torch.randn(coords.shape[0], 8, device=dev).requires_grad_(True)

        def run():
            out.grad = None
            if packed:
                loss, _ = train.separate_loss_packed(out, data.sym_to_device(labels, dev), scale.to(dev, non_blocking=True),
                                                     obj.to(dev, non_blocking=True))
            else:
                loss, _ = train.separate_loss(out, labels, scale.to(dev), obj.to(dev))
            loss.backward()
            return loss
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        res = run()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / a.steps
    last = res[0] if isinstance(res, tuple) else res
    if packed:
        segments, jobs = labels.n_segments, labels.n_jobs
    else:
        segments, jobs = sum(len(p) for p in labels), sum(len(x) for p in labels for _, x in p)
    print("RESULT " + json.dumps({"row": a.worker, "root": os.path.abspath(a.root), "event_ms": e0.elapsed_time(e1) / a.steps,
                                  "wall_ms": wall, "rows": int(coords.shape[0]), "last_loss": float(last),
                                  "segments": segments, "jobs": jobs}), flush=True)


def child(row, root, items, steps, warmup, limit=600):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", row, "--root", root, "--items", items, "--steps", str(steps),
           "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("%s in %s failed (%d):\n%s\n%s" % (row, root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "separate_step.txt"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--worker", default=None, choices=["step-list", "step-packed", "loss-list", "loss-packed"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--items", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    sys.path.insert(0, ROOT)
    from canonicalvoting_amd import data
    ds = data.SyntheticSymDataset(3, a.points, seed0=0)
    items = [ds[i] for i in range(3)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "items.pkl")
        with open(path, "wb") as f:
            pickle.dump(items, f)
        parent = a.parent or ROOT
        rows = {"step-list": [], "step-packed": [], "loss-list": [], "loss-packed": []}
        for _ in range(a.repeats):
            rows["step-list"].append(child("step-list", parent, path, a.steps, a.warmup))
            rows["step-packed"].append(child("step-packed", ROOT, path, a.steps, a.warmup))
        for _ in range(a.repeats):
            rows["loss-list"].append(child("loss-list", ROOT, path, max(a.steps // 2, 1), 2))
            rows["loss-packed"].append(child("loss-packed", ROOT, path, a.steps, a.warmup))
    first = rows["step-packed"][0]
    text = ["separate-model training step, %d rows (3 synthetic scenes), %d segments, %d (segment, pose) jobs" %
            (first["rows"], first["segments"], first["jobs"]),
            "ms per iteration over %d timed iterations, %d repeats in alternating child processes: [event] / [wall]" % (a.steps, a.repeats),
            "step, list labels runs the code of: %s" % ("the parent checkout" if a.parent else "this tree (list path = the parent's code)"), ""]
    names = {"step-list": "step, list labels", "step-packed": "step, packed labels", "loss-list": "loss fwd+bwd, list",
             "loss-packed": "loss fwd+bwd, packed"}
    for k, rs in rows.items():
        ev, wl = [r["event_ms"] for r in rs], [r["wall_ms"] for r in rs]
        text.append("%-22s event %s (median %.3f, spread %.3f)   wall %s (median %.3f)   last loss %.6f" %
                    (names[k], " ".join("%.3f" % v for v in ev), statistics.median(ev), max(ev) - min(ev),
                     " ".join("%.3f" % v for v in wl), statistics.median(wl), rs[-1]["last_loss"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
