"""What feeding the per-category trainer from real files costs, on the host and on the device.

    python profiles/train_loader_sym.py [--out profiles/train/sym_loader_rate.txt] [--host-only] [--scans 6] [--vertices 150000]

Shaped like profiles/train_loader.py (whose room-shaped scans and helpers it uses): a ScanNet / Scan2CAD-format dataset of
150 000-vertex scans with 15 aligned models each, symmetry classes cycling through none / 2 / 4 / INF, colour augmentation
and rotation on, written to a temporary directory.  It records
  (a) host ms per ``ds[i]`` (the default path) and per ``ds.raw_item(i)``, one thread, median over the scans - no GPU needed
  (b) device ms per batch of 3: ``data.device_batch_sym`` between two HIP events (its one host wait inside), and the launches
      of a batch
  (c) wall ms per ``data.device_batch_sym`` of 3 scans, from a pinned RawSymBatch, synchronised before and after
  (d) steps/s of the loop of scripts/train_separate.py both ways (``collate_sym`` batches copied up - the default path, which
      this change leaves as it was - and --device-loader) with 0 / 4 / 12 DataLoader workers, train.train_step_separate included
Every process computes on ONE thread (the BLAS / OpenMP pools are set to 1 before numpy loads): the per-item figures are per
core and the workers are the parallelism.  The GPU part runs in one child process under a time limit.  Part (e) of the
recorded file - bench.py's headline and --mode train against the parent commit, alternated, three runs each - is not run by
this script: it needs a checkout of the parent beside this one, and its lines were appended to the output."""
import os

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_k] = "1"

import argparse  # noqa: E402
import importlib.util  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_loader as joint  # noqa: E402

RES, BATCH, MODELS = joint.RES, joint.BATCH, 15
SYMS = ["__SYM_NONE", "__SYM_ROTATE_UP_2", "__SYM_ROTATE_UP_4", "__SYM_ROTATE_UP_INF"]
# per batch: the voxeliser's clear / insert / flag / emit / inverse, then cv_sp_sym_rows_f32's ten kernels (csrc/train_rows.hip)
LAUNCHES = (5, 10)


def write_dataset(root, n_scans, n_vertices):
    """train_loader's scans with 15 models whose symmetry classes cycle"""
    joint.write_dataset(root, n_scans, n_vertices, n_models=MODELS)
    path = os.path.join(root, "full_annotations.json")
    with open(path) as f:
        annotations = json.load(f)
    for ann in annotations:
        for mi, m in enumerate(ann["aligned_models"]):
            m["sym"] = SYMS[mi % len(SYMS)]
    with open(path, "w") as f:
        json.dump(annotations, f)


def dataset(root):
    from canonicalvoting_amd import data
    return data.ScanNetXYZProbSymDataset(joint.config(root), training=True, augment=True)


def host_part(root):
    ds = dataset(root)
    item_ms, raw_ms, voxels, cand, targets = [], [], [], [], []
    np.random.seed(0)
    for i in range(len(ds)):
        t0 = time.perf_counter()
        item = ds[i]
        item_ms.append((time.perf_counter() - t0) * 1e3)
        voxels.append(item[1].shape[0])
        t0 = time.perf_counter()
        raw = ds.raw_item(i)
        raw_ms.append((time.perf_counter() - t0) * 1e3)
        cand.append(raw.seg_vertex.shape[0])
        targets.append(int((np.diff(raw.seg_vptr) * np.diff(raw.pose_ptr)).sum()))
    med = statistics.median
    return dict(item_ms=med(item_ms), item_min=min(item_ms), item_max=max(item_ms), raw_ms=med(raw_ms), raw_min=min(raw_ms),
                raw_max=max(raw_ms), voxels=int(med(voxels)), scans=len(ds), cand=int(med(cand)), targets=int(med(targets)))


def gpu_child(root, steps, warm):
    import torch

    from canonicalvoting_amd import data, train
    from canonicalvoting_amd.minkunet import MinkUNet34C
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    spec = importlib.util.spec_from_file_location("cv_train_separate", os.path.join(ROOT, "scripts", "train_separate.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    ds = dataset(root)
    cfg = ds.cfg
    np.random.seed(0)
    raw = data.collate_raw_sym([ds.raw_item(i) for i in range(BATCH)])
    raw = type(raw)(*[t.pin_memory() if torch.is_tensor(t) else t for t in raw])
    out = {}
    for _ in range(5):
        batch = data.device_batch_sym(raw, dev, RES)
    sync()
    ev_ms, wall_ms = [], []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        t0 = time.perf_counter()
        e0.record()
        batch = data.device_batch_sym(raw, dev, RES)
        e1.record()
        sync()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(e0.elapsed_time(e1))
    sym = batch[3]
    out.update(rows=int(batch[1].shape[0]), points=int(raw.points.shape[0]), cand=raw.n_cand, kept=int(sym.rows.shape[0]),
               segments=sym.n_segments, jobs=sym.n_jobs, targets=int(sym.targets.shape[0]), urows=int(sym.urow.shape[0]),
               batch_ev_ms=statistics.median(ev_ms), batch_ev_min=min(ev_ms), batch_ev_max=max(ev_ms),
               batch_wall_ms=statistics.median(wall_ms), batch_wall_min=min(wall_ms), batch_wall_max=max(wall_ms))

    torch.manual_seed(0)
    model = MinkUNet34C(3, 8).to(dev).train()
    opt = train.make_optimizer(model, lr=1e-3)
    out["loops"] = []
    for workers in (0, 4, 12):
        for device_loader in (False, True):
            items = joint.Cycle(ds, BATCH * (warm + steps), device_loader)
            loader = torch.utils.data.DataLoader(items, batch_size=BATCH, shuffle=True,
                                                 collate_fn=data.collate_raw_sym if device_loader else data.collate_sym,
                                                 drop_last=True, num_workers=workers, pin_memory=True)
            done, t0 = 0, None
            for b in (script.device_loader_batches(loader, dev, cfg, True) if device_loader else script.device_batches(loader, dev)):
                res = train.train_step_separate(model, opt, *b)
                float(res[0])
                done += 1
                if done == warm:
                    sync()
                    t0 = time.perf_counter()
            assert done == warm + steps
            sync()
            out["loops"].append(dict(workers=workers, device_loader=device_loader, steps_per_s=steps / (time.perf_counter() - t0)))
            del loader
    b = data.device_batch_sym(raw, dev, RES)
    b = (b[1], b[2], b[3], b[4], b[5])
    for _ in range(3):
        train.train_step_separate(model, opt, *b)
    sync()
    t0 = time.perf_counter()
    for _ in range(10):
        float(train.train_step_separate(model, opt, *b)[0])
    sync()
    out["step_ms"] = (time.perf_counter() - t0) * 100.0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "sym_loader_rate.txt"))
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--vertices", type=int, default=150000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--gpu-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.gpu_child:
        return gpu_child(a.gpu_child, a.steps, a.warm)
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, a.scans, a.vertices)
        h = host_part(root)
        lines = ["separate-model training input from real files: %d scans of %d vertices (room surfaces, %d models, symmetry none / 2 / 4 / INF,"
                 % (h["scans"], a.vertices, MODELS),
                 "colour + rotation), res %.2f, %d voxels, %d segment vertices and %d target rows (upper bound) per scan"
                 % (RES, h["voxels"], h["cand"], h["targets"]),
                 "host CPU: %s; one thread per process" % joint.cpu_model(), "",
                 "(a) host ms per scan, median (min .. max) over the scans",
                 "    ds[i]        (default path)  %8.1f  (%.1f .. %.1f)" % (h["item_ms"], h["item_min"], h["item_max"]),
                 "    raw_item(i)  (device path)   %8.1f  (%.1f .. %.1f)" % (h["raw_ms"], h["raw_min"], h["raw_max"]),
                 "    raw_item < ds[i]: %s   ratio %.1f" % ("yes" if h["raw_ms"] < h["item_ms"] else "NO", h["item_ms"] / h["raw_ms"]), ""]
        if a.host_only:
            lines.append("(b) (c) (d): not measured (--host-only)")
        else:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-child", root, "--steps", str(a.steps), "--warm", str(a.warm)],
                               capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit("train_loader_sym: the GPU part ended with status %d" % r.returncode)
            g = json.loads(r.stdout.strip().splitlines()[-1])
            lines += ["batch of %d scans: %d vertices -> %d rows; %d segment vertices -> %d labelled points on %d distinct rows,"
                      % (BATCH, g["points"], g["rows"], g["cand"], g["kept"], g["urows"]),
                      "    %d segments, %d poses, %d target rows" % (g["segments"], g["jobs"], g["targets"]),
                      "(b) device ms per batch, HIP events, median of 30 (min .. max)",
                      "    device_batch_sym (copies, voxelisation, sym_rows, its one wait)  %8.3f  (%.3f .. %.3f)"
                      % (g["batch_ev_ms"], g["batch_ev_min"], g["batch_ev_max"]),
                      "    launches per batch: %d of the voxeliser + %d of cv_sp_sym_rows_f32 + one copy of the eight counts" % LAUNCHES,
                      "(c) wall ms per device_batch_sym, median of 30 (min .. max)         %8.3f  (%.3f .. %.3f)"
                      % (g["batch_wall_ms"], g["batch_wall_min"], g["batch_wall_max"]),
                      "    train.train_step_separate alone on that batch, wall ms          %8.1f" % g["step_ms"], "",
                      "(d) steps/s of the loop of scripts/train_separate.py (%d steps after %d), train_step_separate included" % (a.steps, a.warm),
                      "    workers   collate_sym + copies   --device-loader"]
            for w in (0, 4, 12):
                row = {l["device_loader"]: l["steps_per_s"] for l in g["loops"] if l["workers"] == w}
                lines.append("    %7d   %20.2f   %15.2f" % (w, row[False], row[True]))
        text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
