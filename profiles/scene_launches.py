"""Kernel launches of ONE one-call scene, for comparing two trees launch by launch.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/scene_launches.py run joint|separate [ROOT]
    python profiles/scene_launches.py count DIR

`run` issues one 80k-point scene through pipeline.detect_scene_c (joint) or pipeline.detect_scene_separate_c (nine
8-channel models) of the tree at ROOT (default: this one), teacher predictions, after the model set-up and nothing else: no
warm-up scene, so every dispatch of the trace belongs to the set-up or to that scene and two trees that launch the same
work give the same counts.  `count` prints "count  kernel name" per kernel of the trace under DIR, sorted by name."""
import collections
import csv
import glob
import os
import sys


def run(mode, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from canonicalvoting_amd import pipeline
    from canonicalvoting_amd.hough import HoughVoting
    from canonicalvoting_amd.minkunet import MinkUNet34C
    from canonicalvoting_amd.synth import make_scene, synth_predictions
    dev = torch.device("cuda:0")
    n = 80000
    sc = make_scene(12, n_points=n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c4 = torch.cat([torch.zeros((n, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(dev)
    feats = (t(sc.feats) * 2 - 1).float().contiguous()
    xyz, scale, prob, cls = [t(a) for a in synth_predictions(sc)]
    hv = HoughVoting(sc.res, 120)
    if mode == "joint":
        torch.manual_seed(0)
        model = MinkUNet34C(3, 64).to(dev).eval()
        dets = pipeline.detect_scene_c(model, hv, c4, feats, sc.res, predictions=(xyz, scale, prob, cls.int()))[0]
    else:
        models = {}
        for c in range(9):
            torch.manual_seed(100 + c)
            models[c] = MinkUNet34C(3, 8).to(dev).eval()
        pred = (torch.stack([xyz] * 9), torch.stack([scale] * 9), torch.stack([prob * (cls == c) + 0.01 for c in range(9)]))
        dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, predictions=pred)
    torch.cuda.synchronize()
    print("%s scene from %s: %d detections" % (mode, pipeline.__file__, len(dets)))


def count(trace_dir):
    counts = collections.Counter()
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                counts[row["Kernel_Name"]] += 1
    for name in sorted(counts):
        print("%6d  %s" % (counts[name], name))
    print("%6d  TOTAL (%d kernel names)" % (sum(counts.values()), len(counts)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    else:
        count(sys.argv[2])
