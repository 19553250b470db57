"""What voxelising a raw cloud costs next to running the scene it makes (fp32 clouds of synth.make_raw_scene, 3 cm voxels).

    python profiles/quantize_rate.py [--out profiles/quantize/quantize_rate.txt] [--sizes 300000 1000000]

Per size, after a warm-up of that shape:
  (a) device time of the quantise (cv_sp_quantize_f32 without its host wait) between two HIP events, median of 50 calls
  (b) wall time of ME.utils.sparse_quantize(device cloud, return_index=True), its host wait for N included, median of 50
  (c) the route without the kernels, same host, same process: the numpy sparse_quantize plus the host-to-device copy of its
      result, median of 3
  (d) wall time of pipeline.detect_scene_c on the resulting scene (teacher predictions), median of 20
No profiler.  Every size runs in a child process of its own under a time limit; the first child that fails ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = 0.03


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def child(m):
    import numpy as np
    import torch

    from canonicalvoting_amd import _lib, pipeline
    from canonicalvoting_amd.hough import HoughVoting
    from canonicalvoting_amd.me import utils as me_utils
    from canonicalvoting_amd.minkunet import MinkUNet34C
    from canonicalvoting_amd.synth import make_raw_scene, synth_predictions
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    raw = make_raw_scene(0, m)
    p_host = raw.points.astype(np.float32)
    p_dev = torch.from_numpy(p_host).to(dev)
    sync = torch.cuda.synchronize

    # (a) the four launches between two events, no host wait
    vp = ctypes.c_void_p
    coords4 = torch.empty((m, 4), dtype=torch.int32, device=dev)
    index = torch.empty(m, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.cv_sp_quantize_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        _lib.check(L.cv_sp_quantize_f32(vp(p_dev.data_ptr()), m, 3, float(np.float32(RES)), 0, None, 0, vp(coords4.data_ptr()),
                                        vp(index.data_ptr()), None, vp(counts.data_ptr()), None, vp(ws.data_ptr()), ws.numel(),
                                        stream), "cv_sp_quantize_f32")
    for _ in range(5):
        launch()
    sync()
    dev_ms = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    n_vox, rejected = counts.tolist()
    assert rejected == 0

    # (b) the Python call with its host wait
    def wall(fn, reps):
        out = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    call = lambda: me_utils.sparse_quantize(p_dev, quantization_size=RES, return_index=True)
    for _ in range(5):
        call()
    call_ms = wall(call, 50)

    # (c) numpy + upload
    def host_route():
        c, idx = me_utils.sparse_quantize(p_host, quantization_size=RES, return_index=True)
        return torch.from_numpy(c).to(dev), torch.from_numpy(idx).to(dev)
    host_ms = wall(host_route, 3)
    c_host, idx_host = me_utils.sparse_quantize(p_host, quantization_size=RES, return_index=True)
    c_dev, i_dev = call()
    assert np.array_equal(c_dev.cpu().numpy(), c_host) and np.array_equal(i_dev.cpu().numpy(), idx_host)     # the same scene
    assert n_vox == idx_host.size

    # (d) the scene
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(dev).eval()
    hv = HoughVoting(RES, 120)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c4 = torch.cat([torch.zeros((n_vox, 1), dtype=torch.int32, device=dev), c_dev], 1).contiguous()
    feats = t((raw.feats * 2 - 1).astype(np.float32)[idx_host])
    pred = tuple(t(a[idx_host]) for a in synth_predictions(raw))
    scene = lambda: pipeline.detect_scene_c(model, hv, c4, feats, RES, predictions=pred, thresh_high=60)
    for _ in range(5):
        dets, _, _ = scene()
    scene_ms = wall(scene, 20)
    med = statistics.median
    print(json.dumps(dict(points=m, voxels=n_vox, detections=len(dets), a_device_ms=med(dev_ms), a_min=min(dev_ms), a_max=max(dev_ms),
                          b_call_ms=med(call_ms), b_min=min(call_ms), b_max=max(call_ms), c_host_ms=med(host_ms),
                          c_min=min(host_ms), c_max=max(host_ms), d_scene_ms=med(scene_ms), d_min=min(scene_ms),
                          d_max=max(scene_ms))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantize", "quantize_rate.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[300000, 1000000])
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    rows = []
    for m in a.sizes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(m)], capture_output=True, text=True,
                           timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("quantize_rate: the run for %d points ended with status %d; nothing more is started" % (m, r.returncode))
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = ["voxelisation next to the scene it makes: fp32 clouds of synth.make_raw_scene(0, M), quantization_size %.2f" % RES,
             "host CPU: %s" % cpu_model(),
             "medians in ms (min .. max): (a) 50 calls, HIP events; (b) 50 calls, wall; (c) 3 calls, wall; (d) 20 calls, wall", ""]
    for r in rows:
        lines += ["%d points -> %d voxels (%d detections)" % (r["points"], r["voxels"], r["detections"]),
                  "  (a) quantise, device time (no host wait)          %9.3f  (%.3f .. %.3f)" % (r["a_device_ms"], r["a_min"], r["a_max"]),
                  "  (b) sparse_quantize(device cloud), with its wait  %9.3f  (%.3f .. %.3f)" % (r["b_call_ms"], r["b_min"], r["b_max"]),
                  "  (c) numpy sparse_quantize + host-to-device copy   %9.3f  (%.3f .. %.3f)" % (r["c_host_ms"], r["c_min"], r["c_max"]),
                  "  (d) detect_scene_c on the resulting scene         %9.3f  (%.3f .. %.3f)" % (r["d_scene_ms"], r["d_min"], r["d_max"]),
                  "  (b) < (d): %s      (c) / (b) = %.0f" % ("yes" if r["b_call_ms"] < r["d_scene_ms"] else "NO",
                                                           r["c_host_ms"] / r["b_call_ms"]), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
