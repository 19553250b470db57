"""What the instance labels of a scene's detections cost, alone and behind the scene call that produced them.

    python profiles/instances_rate.py [--out profiles/instances/instances_rate.txt] [--points 80000]

One synthetic teacher scene (synth.make_scene(1, N), 3 cm voxels, the scene's own detections), after a warm-up:
  (a) device time of the two launches (inst_boxes, inst_assign: decode.instance_labels on the cells of the detections)
      between two HIP events, median of 50 calls; per support mode, with and without the count outputs
  (b) wall time of pipeline.scene_instances (box matching on the host, the two launches, the wait), median of 50
  (c) wall time of pipeline.detect_scene_c + wait, and of detect_scene_c + scene_instances + wait, median of 30 each: the
      difference is what the labels add to a scene, its share is of the scene alone
No profiler.  Nothing here is a pass / fail criterion: the numbers are recorded, not asserted."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return "%8.3f  (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances", "instances_rate.txt"))
    ap.add_argument("--points", type=int, default=80000)
    a = ap.parse_args()
    import numpy as np
    import torch

    from canonicalvoting_amd import decode, pipeline
    from canonicalvoting_amd.hough import HoughVoting
    from canonicalvoting_amd.minkunet import MinkUNet34C
    from canonicalvoting_amd.synth import make_scene, synth_predictions
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    n = a.points
    sc = make_scene(1, n_points=n)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    c4 = torch.cat([torch.zeros((n, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(dev)
    feats = (t(sc.feats) * 2 - 1).contiguous()
    pts = (c4[:, 1:] * sc.res).float().contiguous()
    xyz, scale, prob, cls = [t(x) for x in synth_predictions(sc)]
    teacher = (xyz, scale, prob, cls.int())
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(dev).eval()
    hv = HoughVoting(sc.res, 120)

    def scene(keep):
        return pipeline.detect_scene_c(model, hv, c4, feats, sc.res, scan_points=pts, predictions=teacher, keep=keep)[0]

    for _ in range(3):
        keep = {}
        dets = scene(keep)
        pipeline.scene_instances(keep, dets, pts, counts=True)
    sync()
    raw = keep["raw"]
    accepted = raw["cand_idx"][raw["verdict"] == 0]
    order = sorted(range(len(dets)), key=lambda p: (-dets[p][2], p))
    cells = [int(accepted[next(i for i in range(len(accepted)) if np.array_equal(raw["boxes"][i], dets[p][1]))]) for p in order]
    lines = ["instance labels of a scene's detections: synth.make_scene(1, %d) with teacher predictions, %d scan points, "
             "%d detections (%d accepted boxes, %d candidates)" % (n, n, len(dets), len(accepted), len(raw["cand_idx"])),
             "device: %s" % torch.cuda.get_device_name(0),
             "medians in ms (min .. max): (a) 50 calls, HIP events; (b) 50 calls, wall; (c) 30 calls, wall", ""]
    _, g_rot, g_scale = keep["grids"]
    for support in ("confident", "inside"):
        for counts in (False, True):
            ev, wall = [], []
            for _ in range(50):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                decode.instance_labels(g_rot, g_scale, keep["corner"], keep["res"], pts, prob, cells, order, support=support,
                                       counts=counts)
                e1.record()
                sync()
                ev.append(e0.elapsed_time(e1))
            for _ in range(50):
                sync()
                t0 = time.perf_counter()
                out = pipeline.scene_instances(keep, dets, pts, support=support, counts=counts)
                sync()
                wall.append((time.perf_counter() - t0) * 1e3)
            tag = "support=%-9s counts=%-5s" % (support, counts)
            lines.append("  (a) %s two launches, device time        %s" % (tag, med(ev)))
            lines.append("  (b) %s scene_instances, wall with wait   %s" % (tag, med(wall)))
        owned = int((out["owner"] >= 0).sum())
        lines.append("      support=%s: %d of %d scan points owned" % (support, owned, n))
    lines.append("")
    alone, both = [], []
    for _ in range(30):
        sync()
        t0 = time.perf_counter()
        scene({})
        sync()
        alone.append((time.perf_counter() - t0) * 1e3)
    for _ in range(30):
        sync()
        t0 = time.perf_counter()
        keep = {}
        d = scene(keep)
        pipeline.scene_instances(keep, d, pts, counts=True)
        sync()
        both.append((time.perf_counter() - t0) * 1e3)
    ma, mb = statistics.median(alone), statistics.median(both)
    lines.append("  (c) detect_scene_c(keep=...) + wait                         %s" % med(alone))
    lines.append("  (c) detect_scene_c(keep=...) + scene_instances + wait       %s" % med(both))
    lines.append("      the labels add %.3f ms to the scene: %.1f %% of the scene alone" % (mb - ma, 100.0 * (mb - ma) / ma))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
