#!/usr/bin/env python
"""eval_separate.py counterpart (reference eval_separate.py:136-312) on synthetic scans: nine per-category 8-channel
models on one scan -> ONE scene call (plan once, nine networks, nine heads, one vote and one decode over the category
axis, NMS per category) per scene, then mAP @0.25 / @0.5.  argparse instead of hydra (absent here).

    python scripts/eval_separate.py [--scenes 4] [--points 80000] [--weights-dir DIR] [--teacher] [--config config.yaml]
                                    [--raw-points [M]] [--instances]

--weights-dir holds one state dict per category, DIR/<category>.pth (reference checkpoints are loaded through
minkunet.load_reference_checkpoint).  --teacher feeds the vote/decode stage with per-category predictions synthesised from
the labels (there is no trained checkpoint offline); the networks still run.
--raw-points (synthetic scenes only): every scene is a RAW cloud of M surface samples (default 300000) that goes through
pipeline.detect_points_separate_c: voxelised on the device, gathered and detected in one C call.
--instances (synthetic scenes only): after each scene, the scan points every detection owns within its category and the
ones inside its box (pipeline.scene_instances; with --raw-points also the raw points it owns over all categories).
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
from canonicalvoting_amd.data import parse_gt_lines  # noqa: E402
from canonicalvoting_amd.synth import make_raw_scene, synth_predictions  # noqa: E402


def teacher_predictions(scene, categories, device):
    """category c's points keep the teacher's probability, the others a background-level non-zero one"""
    xyz, scale, prob, cls = synth_predictions(scene)
    rng = np.random.default_rng(scene.seed)
    P = np.stack([np.where(cls == c, prob, rng.uniform(1e-3, 0.1, prob.shape[0])) for c in categories]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    return t(np.stack([xyz] * len(categories))), t(np.stack([scale] * len(categories))), t(P)


def report_instances(id_scan, keep, dets, scan_points=None, inverse=None):
    print("%s: %d detections" % (id_scan, len(dets)))
    out = pipeline.scene_instances(keep, dets, scan_points, counts=True, inverse=inverse)
    print("\n".join(pipeline.instances_report(dets, out)))


def evaluate(models, dataset, res=0.03, teacher=False, device="cuda", models_per_pass=None, instances=False):
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=1, shuffle=False)
    for index, (ids, coords, feats, _, _, _) in enumerate(loader):
        id_scan = ids[0]
        feats = feats.to(device)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                             # eval_separate.py: colour columns only
        coords = coords.to(device)
        pred = teacher_predictions(dataset.scene(index), list(models), device) if teacher else None
        keep = {} if instances else None
        pts = (coords[:, 1:] * res).float().contiguous()
        pred_map_cls[id_scan] = pipeline.detect_scene_separate_c(models, hv, coords, feats, res, predictions=pred, keep=keep,
                                                                 scan_points=pts, models_per_pass=models_per_pass)
        if instances:
            report_instances(id_scan, keep, pred_map_cls[id_scan], pts)
        gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in dataset.gt(index)]
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def evaluate_raw(models, n_scenes, n_samples, seed0=100, res=0.03, teacher=False, device="cuda", models_per_pass=None,
                 instances=False):
    """the synthetic evaluation from raw clouds: one C call per scene (pipeline.detect_points_separate_c)"""
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    for index in range(n_scenes):
        raw = make_raw_scene(seed0 + index, n_samples)
        id_scan = "synth%04d" % (seed0 + index)
        pred = teacher_predictions(raw, list(models), device) if teacher else None
        keep = {} if instances else None
        out = pipeline.detect_points_separate_c(models, hv, t(raw.points), t(raw.feats), res, predictions=pred, keep=keep,
                                                recentre_from=0, models_per_pass=models_per_pass, return_inverse=instances)
        pred_map_cls[id_scan] = out[0]
        if instances:
            report_instances(id_scan, keep, out[0], inverse=out[-1])
        lines = ["%f %f %f %f %f %f %f %d" % tuple(list(b[:7]) + [int(b[7])]) for b in raw.boxes]
        gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in parse_gt_lines(lines)]
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def build_parser():
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
    ap.add_argument("--raw-points", type=int, nargs="?", const=300000, default=0, metavar="M",
                    help="synthetic scenes as raw clouds of M samples: voxelise, gather and detect in one C call "
                         "(pipeline.detect_points_separate_c)")
    ap.add_argument("--instances", action="store_true",
                    help="print the scan points each detection owns and has inside its box (pipeline.scene_instances)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if (a.raw_points or a.instances) and a.config:
        ap.error("--raw-points and --instances run on the synthetic scenes only")
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
    elif a.raw_points:
        res = evaluate_raw(models, a.scenes, a.raw_points, seed0=100, teacher=a.teacher, models_per_pass=a.models_per_pass,
                           instances=a.instances)
    else:
        res = evaluate(models, SyntheticScanDataset(a.scenes, a.points, seed0=100), teacher=a.teacher, models_per_pass=a.models_per_pass,
                       instances=a.instances)
    for thr, r in res.items():
        print("IoU %.2f: mAP %.4f  AR %.4f" % (thr, r["mAP"], r["AR"]))


if __name__ == "__main__":
    main()
