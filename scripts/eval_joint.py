#!/usr/bin/env python
"""eval_joint.py counterpart (reference eval_joint.py:137-312) on synthetic scans: network -> head -> vote ->
decode -> NMS per scene, then mAP @0.25 / @0.5.  argparse instead of hydra (absent here).

    python scripts/eval_joint.py [--scenes 4] [--points 80000] [--weights joint.pth] [--teacher] [--raw-points [M]] [--instances]
                                 [--scenes-per-call B]

--teacher feeds the vote/decode stage with predictions synthesised from the labels (there is no trained
checkpoint offline); the network forward still runs.
--raw-points (synthetic scenes only): every scene is a RAW cloud of M surface samples (default 300000) that goes through
pipeline.detect_points_c: voxelised on the device, gathered (with the colour recentre) and detected in one C call.
--instances (synthetic scenes only): after each scene, the scan points every detection owns and the ones inside its box
(pipeline.scene_instances on the one-call scene's keep; with --raw-points also the raw points it owns).
--scenes-per-call B (synthetic voxel scenes only): B scans per C call (pipeline.detect_scenes_c: one plan, one network program,
one decode over the scene axis; two host waits per call instead of two per scan).  The default 1 is the one-scan path.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd import calc_map, decode, pipeline  # noqa: E402
from canonicalvoting_amd import me as ME  # noqa: E402
from canonicalvoting_amd.data import (ScanNetXYZProbMultiDataset, SyntheticScanDataset, collate_fn,  # noqa: E402
                                     load_config)
from canonicalvoting_amd.hough import HoughVoting  # noqa: E402
from canonicalvoting_amd.minkunet import MinkUNet34C  # noqa: E402
from canonicalvoting_amd.data import parse_gt_lines  # noqa: E402
from canonicalvoting_amd.synth import make_raw_scene, synth_predictions  # noqa: E402


def evaluate(model, dataset, res=0.03, teacher=False, nclasses=9, device="cuda", instances=False):
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=1, shuffle=False)
    for index, (ids, coords, feats, _, _, _) in enumerate(loader):
        id_scan = ids[0]
        feats = feats.to(device)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                             # eval_joint.py:167-168: colour columns only
        coords = coords.to(device)
        with torch.no_grad():
            out = model(ME.SparseTensor(feats, coords, device=device))
            xyz, scale, prob, cls = pipeline.head_joint(out.F, nclasses)
        if teacher:
            t = lambda a: torch.from_numpy(a).to(device)
            xyz, scale, prob, cls = [t(a) for a in synth_predictions(dataset.scene(index))]
        if instances:
            # the one-call scene (the same detections, bit for bit) hands out the grids the labels are formed from
            keep = {}
            pts = (coords[:, 1:] * res).float().contiguous()
            dets = pipeline.detect_scene_c(model, hv, coords, feats, res, nclasses, scan_points=pts, keep=keep,
                                           predictions=(xyz, scale, prob, cls) if teacher else None)[0]
            print("%s: %d detections" % (id_scan, len(dets)))
            print("\n".join(pipeline.instances_report(dets, pipeline.scene_instances(keep, dets, pts, counts=True))))
        else:
            dets, _ = decode.detect(hv, coords[:, 1:], xyz, scale, prob, cls, res, nclasses)
        pred_map_cls[id_scan] = dets
        gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in dataset.gt(index)]     # eval_joint.py:285-301
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def evaluate_batched(model, dataset, scenes_per_call, res=0.03, teacher=False, nclasses=9, device="cuda", instances=False):
    """evaluate() with B = scenes_per_call scans per C call (pipeline.detect_scenes_c): the scans are collated with batch
    indices 0..B-1, the last call of a pass may be short.  Vote, decode and NMS of a scan are those of the one-scan path."""
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=scenes_per_call, shuffle=False)
    index = 0
    for ids, coords, feats, _, _, _ in loader:
        B = len(ids)
        feats = feats.to(device)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                             # eval_joint.py:167-168: colour columns only
        coords = coords.to(device)
        pts = (coords[:, 1:] * res).float().contiguous()
        pred = None
        if teacher:
            per = [synth_predictions(dataset.scene(index + b)) for b in range(B)]
            pred = tuple(torch.from_numpy(np.concatenate([p[i] for p in per])).to(device) for i in range(4))
        keep = [] if instances else None
        out, _ = pipeline.detect_scenes_c(model, hv, coords, feats, res, B, scan_points=pts, predictions=pred, keep=keep,
                                          nclasses=nclasses)
        for b, id_scan in enumerate(ids):
            dets = out[b][0]
            if instances:
                lo, hi = keep[b]["rows"]
                print("%s: %d detections" % (id_scan, len(dets)))
                print("\n".join(pipeline.instances_report(dets, pipeline.scene_instances(keep[b], dets, pts[lo:hi], counts=True))))
            pred_map_cls[id_scan] = dets
            gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in dataset.gt(index + b)]
        index += B
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def evaluate_raw(model, n_scenes, n_samples, seed0=100, res=0.03, teacher=False, nclasses=9, device="cuda", detections=None,
                 instances=False, **scene_kw):
    """the synthetic evaluation from raw clouds: one C call per scene (pipeline.detect_points_c voxelises, gathers - the
    colour recentre of eval_joint.py:167-168 in the gather - and detects).  ``detections`` (a dict) receives every scene's
    detection list; ``scene_kw`` goes to make_raw_scene / detect_points_c (room=..., thresh_high=...)."""
    hv = HoughVoting(res)
    pred_map_cls, gt_map_cls = {}, {}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    raw_kw = {k: scene_kw.pop(k) for k in ("room", "n_boxes", "margin", "box_scale") if k in scene_kw}
    for index in range(n_scenes):
        raw = make_raw_scene(seed0 + index, n_samples, **raw_kw)
        id_scan = "synth%04d" % (seed0 + index)
        pred = tuple(t(a) for a in synth_predictions(raw)) if teacher else None
        keep = {} if instances else None
        out = pipeline.detect_points_c(model, hv, t(raw.points), t(raw.feats), res, predictions=pred, recentre_from=0,
                                       nclasses=nclasses, return_inverse=instances, keep=keep, **scene_kw)
        dets = out[0]
        if instances:
            print("%s: %d detections" % (id_scan, len(dets)))
            print("\n".join(pipeline.instances_report(dets, pipeline.scene_instances(keep, dets, counts=True, inverse=out[-1]))))
        pred_map_cls[id_scan] = dets
        lines = ["%f %f %f %f %f %f %f %d" % tuple(list(b[:7]) + [int(b[7])]) for b in raw.boxes]
        gt_map_cls[id_scan] = [(c, calc_map.gt_box(*p)) for c, p in parse_gt_lines(lines)]
    if detections is not None:
        detections.update(pred_map_cls)
    return {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--teacher", action="store_true")
    ap.add_argument("--config", default=None, help="the reference's config.yaml: evaluate on real ScanNet/Scan2CAD files")
    ap.add_argument("--raw-points", type=int, nargs="?", const=300000, default=0, metavar="M",
                    help="synthetic scenes as raw clouds of M samples: voxelise, gather and detect in one C call (pipeline.detect_points_c)")
    ap.add_argument("--instances", action="store_true",
                    help="print the scan points each detection owns and has inside its box (pipeline.scene_instances)")
    ap.add_argument("--scenes-per-call", type=int, default=1, metavar="B",
                    help="B scans per C call (pipeline.detect_scenes_c, 1..16); 1: one scan at a time, as before")
    a = ap.parse_args()
    if (a.raw_points or a.instances) and a.config:
        ap.error("--raw-points and --instances run on the synthetic scenes only")
    if not 1 <= a.scenes_per_call <= 16 or (a.scenes_per_call > 1 and (a.raw_points or a.config)):
        ap.error("--scenes-per-call takes 1..16 and runs on the synthetic voxel scenes only")
    cfg = load_config(a.config, category="all") if a.config else None
    model = MinkUNet34C(6 if (cfg and cfg.use_xyz) else 3, 6 * 9 + 9 + 1)
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location="cpu"))
    model = model.cuda().eval()
    if cfg:
        res = evaluate(model, ScanNetXYZProbMultiDataset(cfg, training=False, augment=False), res=cfg.scannet_res)
    elif a.raw_points:
        res = evaluate_raw(model, a.scenes, a.raw_points, seed0=100, teacher=a.teacher, instances=a.instances)
    elif a.scenes_per_call > 1:
        res = evaluate_batched(model, SyntheticScanDataset(a.scenes, a.points, seed0=100), a.scenes_per_call, teacher=a.teacher,
                               instances=a.instances)
    else:
        res = evaluate(model, SyntheticScanDataset(a.scenes, a.points, seed0=100), teacher=a.teacher, instances=a.instances)
    for thr, r in res.items():
        print("IoU %.2f: mAP %.4f  AR %.4f" % (thr, r["mAP"], r["AR"]))


if __name__ == "__main__":
    main()
