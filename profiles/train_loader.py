"""What feeding the training step from real files costs, on the host and on the device.

    python profiles/train_loader.py [--out profiles/train/loader_rate.txt] [--host-only] [--scans 6] [--vertices 150000]

Writes a ScanNet / Scan2CAD-format dataset of room-shaped scans (150 000 vertices on the surfaces of a 5.2 x 2.6 x 5.2 m room,
20 aligned models each, colour augmentation and rotation on) to a temporary directory and records
  (a) host ms per ``ds[i]`` (the parent path) and per ``ds.raw_item(i)``, one thread, median over the scans - no GPU needed
  (b) device ms per batch of 3: ``data.device_batch`` between two HIP events (its host wait for N inside), and the
      cv_sp_scan_rows_f32 launch alone
  (c) wall ms per ``data.device_batch`` of 3 scans, from a pinned RawBatch, synchronised before and after
  (d) steps/s of the loop of scripts/train_joint.py both ways (``collate_fn`` batches copied up, and --device-loader) with
      0 / 4 / 12 DataLoader workers, train.train_step included
Every process computes on ONE thread (the BLAS / OpenMP pools are set to 1 before numpy loads): the per-item figures are per
core and the workers are the parallelism.  The GPU part runs in one child process under a time limit."""
import os

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_k] = "1"

import argparse  # noqa: E402
import importlib.util  # noqa: E402
import json  # noqa: E402
import pickle  # noqa: E402
import statistics  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402
import time  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, BATCH = 0.03, 3
ROOM = np.array([5.2, 2.6, 5.2])
CATS = ["03001627", "04379243", "02933112", "02871439", "04256520", "03211117", "02808440", "02747177", "99999999", "03001627"]


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def write_ply(path, xyz, rgb):
    """binary little-endian, float xyz + uchar rgba vertices: the layout of ScanNet's *_vh_clean_2.ply"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    v = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("a", "u1")])
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["r"], v["g"], v["b"], v["a"] = rgb[:, 0], rgb[:, 1], rgb[:, 2], 255
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n" % len(xyz)).encode())
        f.write(v.tobytes())


def write_dataset(root, n_scans, n_vertices, n_models=20):
    """room-shaped scans: points on the six faces with 5 mm jitter; a model's segment is the vertices within 0.5 m of it"""
    annotations, segments, ids = [], {}, []
    for si in range(n_scans):
        rng = np.random.default_rng(si)
        p = rng.random((n_vertices, 3)) * ROOM
        face = rng.integers(0, 3, n_vertices)
        p[np.arange(n_vertices), face] = np.where(rng.random(n_vertices) < 0.5, 0.0, ROOM[face])
        p += rng.normal(0, 0.005, p.shape)
        sid = "scene%04d_00" % si
        ids.append(sid)
        models, segs = [], []
        for mi in range(n_models):
            t = p[rng.integers(0, n_vertices)]
            a = rng.uniform(0, 2 * np.pi)
            models.append({"catid_cad": CATS[mi % len(CATS)], "id_cad": "generated", "sym": "__SYM_NONE",
                           "trs": {"translation": [float(v) for v in t], "rotation": [float(np.cos(a / 2)), 0.0, float(np.sin(a / 2)), 0.0],
                                   "scale": [float(v) for v in rng.uniform(0.7, 1.4, 3)]},
                           "bbox": [float(v) for v in rng.uniform(0.2, 0.6, 3)], "center": [0.0, 0.0, 0.0]})
            segs.append(np.flatnonzero(np.abs(p - t).max(1) < 0.5))
        write_ply(os.path.join(root, "scans", sid, sid + "_vh_clean_2.ply"), p.astype(np.float32), rng.integers(0, 256, (n_vertices, 3)))
        annotations.append({"id_scan": sid, "trs": {"translation": [0.0, 0.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.0], "scale": [1.0, 1.0, 1.0]},
                            "aligned_models": models, "n_aligned_models": n_models})
        segments[sid] = segs
    with open(os.path.join(root, "full_annotations.json"), "w") as f:
        json.dump(annotations, f)
    for name in ("train", "val"):
        with open(os.path.join(root, "segments_%s.pkl" % name), "wb") as f:
            pickle.dump(segments, f, protocol=2)
        with open(os.path.join(root, "%s_split.txt" % name), "w") as f:
            f.write("".join(s + "\n" for s in ids))


def config(root):
    d = types.SimpleNamespace(scan2cad=os.path.join(root, "full_annotations.json"), scannet=root,
                              train_split=os.path.join(root, "train_split.txt"), val_split=os.path.join(root, "val_split.txt"),
                              train_segments=os.path.join(root, "segments_train.pkl"), val_segments=os.path.join(root, "segments_val.pkl"))
    return types.SimpleNamespace(data=d, category="all", augment_color=True, use_xyz=False, scannet_res=RES)


def dataset(root):
    from canonicalvoting_amd import data
    return data.ScanNetXYZProbMultiDataset(config(root), training=True, augment=True)


class Cycle:
    """``n`` items that walk round a dataset's scans (a map-style dataset): one DataLoader epoch spans a whole measurement, so
    the workers start once"""

    def __init__(self, ds, n, raw):
        self.ds, self.n, self.raw = ds, n, raw

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.ds.raw_item(i % len(self.ds)) if self.raw else self.ds[i % len(self.ds)]


def host_part(root):
    ds = dataset(root)
    item_ms, raw_ms, voxels = [], [], []
    np.random.seed(0)
    for i in range(len(ds)):
        t0 = time.perf_counter()
        item = ds[i]
        item_ms.append((time.perf_counter() - t0) * 1e3)
        voxels.append(item[1].shape[0])
        t0 = time.perf_counter()
        ds.raw_item(i)
        raw_ms.append((time.perf_counter() - t0) * 1e3)
    return dict(item_ms=statistics.median(item_ms), item_min=min(item_ms), item_max=max(item_ms), raw_ms=statistics.median(raw_ms),
                raw_min=min(raw_ms), raw_max=max(raw_ms), voxels=int(statistics.median(voxels)), scans=len(ds))


def gpu_child(root, steps, warm):
    import torch

    from canonicalvoting_amd import data, train
    from canonicalvoting_amd.me import utils as me_utils
    from canonicalvoting_amd.minkunet import MinkUNet34C
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    spec = importlib.util.spec_from_file_location("cv_train_joint", os.path.join(ROOT, "scripts", "train_joint.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    ds = dataset(root)
    cfg = ds.cfg
    np.random.seed(0)
    raw = data.collate_raw([ds.raw_item(i) for i in range(BATCH)])
    raw = type(raw)(*[t.pin_memory() if torch.is_tensor(t) else t for t in raw])
    out = {}

    # (b) + (c)
    for _ in range(5):
        batch = data.device_batch(raw, dev, RES)
    sync()
    ev_ms, wall_ms = [], []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        t0 = time.perf_counter()
        e0.record()
        batch = data.device_batch(raw, dev, RES)
        e1.record()
        sync()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(e0.elapsed_time(e1))
    out.update(rows=int(batch[1].shape[0]), points=int(raw.points.shape[0]), batch_ev_ms=statistics.median(ev_ms), batch_ev_min=min(ev_ms),
               batch_ev_max=max(ev_ms), batch_wall_ms=statistics.median(wall_ms), batch_wall_min=min(wall_ms), batch_wall_max=max(wall_ms))
    up = [t.to(dev) if torch.is_tensor(t) else t for t in raw]
    _, points, rgb, owner, minv, scale, cls, colour, jitter, _ = up
    coords4, index = me_utils.quantize_batch(points, RES, offsets=raw.offsets)
    kern_ms = []
    for i in range(35):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        me_utils.scan_rows(coords4, index, points, rgb, owner, minv, scale, cls, colour, jitter, recentre=True)
        e1.record()
        e1.synchronize()
        if i >= 5:
            kern_ms.append(e0.elapsed_time(e1))
    out.update(kernel_ms=statistics.median(kern_ms), kernel_min=min(kern_ms), kernel_max=max(kern_ms))

    # (d) the script's loop both ways
    torch.manual_seed(0)
    model = MinkUNet34C(3, 6 * 9 + 9 + 1).to(dev).train()
    opt = train.make_optimizer(model, lr=1e-3)
    out["loops"] = []
    for workers in (0, 4, 12):
        for device_loader in (False, True):
            loader = torch.utils.data.DataLoader(Cycle(ds, BATCH * (warm + steps), device_loader), batch_size=BATCH, shuffle=True,
                                                 collate_fn=data.collate_raw if device_loader else data.collate_fn, drop_last=True,
                                                 num_workers=workers, pin_memory=device_loader)
            done, t0 = 0, None
            for b in (script.device_batches(loader, dev, cfg) if device_loader else script.host_batches(loader, dev)):
                loss, _ = train.train_step(model, opt, *b)
                float(loss)
                done += 1
                if done == warm:
                    sync()
                    t0 = time.perf_counter()
            assert done == warm + steps
            sync()
            out["loops"].append(dict(workers=workers, device_loader=device_loader, steps_per_s=steps / (time.perf_counter() - t0)))
            del loader
    # the step alone, on a resident batch
    b = data.device_batch(raw, dev, RES)[1:]
    for _ in range(3):
        train.train_step(model, opt, *b)
    sync()
    t0 = time.perf_counter()
    for _ in range(10):
        float(train.train_step(model, opt, *b)[0])
    sync()
    out["step_ms"] = (time.perf_counter() - t0) * 100.0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "loader_rate.txt"))
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--vertices", type=int, default=150000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--gpu-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.gpu_child:
        return gpu_child(a.gpu_child, a.steps, a.warm)
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, a.scans, a.vertices)
        h = host_part(root)
        lines = ["training input from real files: %d scans of %d vertices (room surfaces, 20 models, colour + rotation), res %.2f, %d voxels per scan"
                 % (h["scans"], a.vertices, RES, h["voxels"]),
                 "host CPU: %s; one thread per process" % cpu_model(), "",
                 "(a) host ms per scan, median (min .. max) over the scans",
                 "    ds[i]        (parent path)   %8.1f  (%.1f .. %.1f)" % (h["item_ms"], h["item_min"], h["item_max"]),
                 "    raw_item(i)  (device path)   %8.1f  (%.1f .. %.1f)" % (h["raw_ms"], h["raw_min"], h["raw_max"]),
                 "    raw_item < ds[i]: %s   ratio %.1f" % ("yes" if h["raw_ms"] < h["item_ms"] else "NO", h["item_ms"] / h["raw_ms"]), ""]
        if a.host_only:
            lines.append("(b) (c) (d): not measured (--host-only)")
        else:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-child", root, "--steps", str(a.steps), "--warm", str(a.warm)],
                               capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit("train_loader: the GPU part ended with status %d" % r.returncode)
            g = json.loads(r.stdout.strip().splitlines()[-1])
            lines += ["batch of %d scans: %d vertices -> %d rows" % (BATCH, g["points"], g["rows"]),
                      "(b) device ms per batch, HIP events, median of 30 (min .. max)",
                      "    device_batch (copies, voxelisation with its wait, scan_rows)  %8.3f  (%.3f .. %.3f)"
                      % (g["batch_ev_ms"], g["batch_ev_min"], g["batch_ev_max"]),
                      "    cv_sp_scan_rows_f32 alone                                    %8.3f  (%.3f .. %.3f)"
                      % (g["kernel_ms"], g["kernel_min"], g["kernel_max"]),
                      "(c) wall ms per device_batch, median of 30 (min .. max)          %8.3f  (%.3f .. %.3f)"
                      % (g["batch_wall_ms"], g["batch_wall_min"], g["batch_wall_max"]),
                      "    train.train_step alone on that batch, wall ms                %8.1f" % g["step_ms"], "",
                      "(d) steps/s of the loop of scripts/train_joint.py (%d steps after %d), train_step included" % (a.steps, a.warm),
                      "    workers   collate_fn + copies   --device-loader"]
            for w in (0, 4, 12):
                row = {l["device_loader"]: l["steps_per_s"] for l in g["loops"] if l["workers"] == w}
                lines.append("    %7d   %19.2f   %15.2f" % (w, row[False], row[True]))
        text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
