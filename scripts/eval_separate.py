#!/usr/bin/env python
"""eval_separate.py counterpart (reference eval_separate.py:136-312) on synthetic scans: nine per-category 8-channel
models on one scan -> ONE scene call (plan once, nine networks, nine heads, one vote and one decode over the category
axis, NMS per category) per scene, then mAP @0.25 / @0.5.  argparse instead of hydra (absent here).

    python scripts/eval_separate.py [--scenes 4] [--points 80000] [--weights-dir DIR] [--teacher] [--config config.yaml]

--weights-dir holds one state dict per category, DIR/<category>.pth (reference checkpoints are loaded through
minkunet.load_reference_checkpoint).  --teacher feeds the vote/decode stage with per-category predictions synthesised from
the labels (there is no trained checkpoint offline); the networks still run.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd import calc_map, pipeline  # noqa: E402
from canonicalvoting_amd.data import (ScanNetXYZProbMultiDataset, SyntheticScanDataset, collate_fn,  # noqa: E402
                                     load_config)
from canonicalvoting_amd.hough import HoughVoting  # noqa: E402
from canonicalvoting_amd.minkunet import MinkUNet34C, load_reference_checkpoint  # noqa: E402
from canonicalvoting_amd.synth import synth_predictions  # noqa: E402


def teacher_predictions(scene, categories, device):
    """category c's points keep the teacher's probability, the others a background-level non-zero one"""
    xyz, scale, prob, cls = synth_predictions(scene)
    rng = np.random.default_rng(scene.seed)
    P = np.stack([np.where(cls == c, prob, rng.uniform(1e-3, 0.1, prob.shape[0])) for c in categories]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    return t(np.stack([xyz] * len(categories))), t(np.stack([scale] * len(categories))), t(P)


def evaluate(models, dataset, res=0.03, teacher=False, device="cuda", models_per_pass=None):
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=1, shuffle=False)
    for index, (ids, coords, feats, _, _, _) in enumerate(loader):
        id_scan = ids[0]
        feats = feats.to(device)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                             # eval_separate.py: colour columns only
        coords = coords.to(device)
        pred = teacher_predictions(dataset.scene(index), list(models), device) if teacher else None
        pred_map_cls[id_scan] = pipeline.detect_scene_separate_c(models, hv, coords, feats, res, predictions=pred,
                                                                 models_per_pass=models_per_pass)
        gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in dataset.gt(index)]
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--weights-dir", default=None, help="one state dict per category: DIR/<category>.pth")
    ap.add_argument("--categories", type=int, nargs="+", default=list(range(9)))
    ap.add_argument("--teacher", action="store_true")
    ap.add_argument("--config", default=None, help="the reference's config.yaml: evaluate on real ScanNet/Scan2CAD files")
    ap.add_argument("--models-per-pass", type=int, default=0,
                    help="G >= 1: the networks run batched over a model axis, G per pass (same bits, fewer launches, G arenas of "
                         "scratch); 0: one network after another")
    a = ap.parse_args()
    cfg = load_config(a.config, category="all") if a.config else None
    models = {}
    for c in a.categories:
        m = MinkUNet34C(6 if (cfg and cfg.use_xyz) else 3, 8)
        if a.weights_dir:
            load_reference_checkpoint(m, os.path.join(a.weights_dir, "%s.pth" % c))
        models[c] = m.cuda().eval()
    if cfg:
        res = evaluate(models, ScanNetXYZProbMultiDataset(cfg, training=False, augment=False), res=cfg.scannet_res,
                       models_per_pass=a.models_per_pass)
    else:
        res = evaluate(models, SyntheticScanDataset(a.scenes, a.points, seed0=100), teacher=a.teacher, models_per_pass=a.models_per_pass)
    for thr, r in res.items():
        print("IoU %.2f: mAP %.4f  AR %.4f" % (thr, r["mAP"], r["AR"]))


if __name__ == "__main__":
    main()
