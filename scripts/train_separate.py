#!/usr/bin/env python
"""train_separate.py counterpart (reference train_separate.py:201-299): one 8-channel model for ONE category - Adam
(lr 1e-3, the config's weight decay), step LR decay and BatchNorm-momentum schedule, objectness CE + MSE(log scale) + the
coordinate loss with the minimum over symmetry-equivalent poses on the device (data.collate_sym -> train.train_step_separate);
one process per GPU with DDP when launched through torch.distributed.run (the reference is single-GPU).

    python scripts/train_separate.py [--epochs 2] [--scenes 6] [--points 20000] [--batch 3]        # synthetic scenes
    python scripts/train_separate.py --config config.yaml --category 03001627                       # ScanNet / Scan2CAD files
    python scripts/train_separate.py --config config.yaml --category 03001627 --device-loader       # batches built on the device

--device-loader: the DataLoader workers stop at the raw scan (ScanNetXYZProbSymDataset.raw_item / collate_raw_sym) and
data.device_batch_sym voxelises, filters the models' points, evaluates the targets of every pose and packs the labels on the
device - the same bits as the default path, one host wait per batch.

--val-every K: every K epochs and on the last one, next to the checkpoint and on rank 0, the reference's validation pass
(train_separate.py:301-458, ``train.validate_separate``): the three validation losses, detections of the category and its AP
and recall at 0.25 / 0.5 over the validation scans (the config's validation split with the ground truth under
``cfg.data.gt_path``; without --config, ``--val-scenes`` further synthetic scenes whose boxes all count as class 0).  0 = off.
Every rank calls ``train.finish_pending`` at the end of every epoch, in front of the checkpoint and the validation: a
fp16-range flag of the epoch's last steps is acted on before anything reads the BatchNorm statistics.
"""
import argparse
import functools
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd import dist as cvd  # noqa: E402
from canonicalvoting_amd import train  # noqa: E402
from canonicalvoting_amd.data import (TOP8_CLASSES, RawItems, ScanNetXYZProbSymDataset, SyntheticSymDataset,  # noqa: E402
                                      collate_raw_sym, collate_sym, device_batch_sym, load_config, sym_to_device)
from canonicalvoting_amd.minkunet import MinkUNet34C  # noqa: E402


def device_batches(loader, dev):
    """train_separate.py:237-243: the collated batch on the device (non-blocking copies), colour columns recentred"""
    for _, coords, feats, sym, scale, obj, _ in loader:
        feats = feats.to(dev, non_blocking=True)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                         # train_separate.py:242-243: colour columns only
        yield (coords.to(dev, non_blocking=True), feats, sym_to_device(sym, dev), scale.to(dev, non_blocking=True),
               obj.to(dev, non_blocking=True))


def device_loader_batches(loader, dev, cfg, reference_indexing):
    """--device-loader: RawSymBatches -> the tuples of device_batches, built on the device (colour columns recentred there)"""
    for raw in loader:
        _, coords, feats, sym, scale, obj, _ = device_batch_sym(raw, dev, cfg.scannet_res, use_xyz=bool(cfg.use_xyz), recentre=True,
                                                                reference_indexing=reference_indexing)
        yield coords, feats, sym, scale, obj


def validation_scans(val_ds, dev, cfg, device_loader):
    """train_separate.py:309-317: one scan per batch, in the form train.validate_separate reads; with --device-loader the scan
    is built on the device from its raw form, the same bits (one scan: both row indexings are the same rows)"""
    if device_loader:
        loader = torch.utils.data.DataLoader(RawItems(val_ds), collate_fn=collate_raw_sym, batch_size=1, shuffle=False)
        for raw in loader:
            ids, coords, feats, sym, scale, obj, _ = device_batch_sym(raw, dev, cfg.scannet_res, use_xyz=bool(cfg.use_xyz),
                                                                      recentre=True)
            yield ids[0], coords, feats, sym, scale, obj
        return
    loader = torch.utils.data.DataLoader(val_ds, collate_fn=collate_sym, batch_size=1, shuffle=False)
    for ids, coords, feats, sym, scale, obj, _ in loader:
        feats = feats.to(dev)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0
        yield ids[0], coords.to(dev), feats, sym, scale, obj


def synthetic_gt_lines(val_ds):
    """{id_scan: ground-truth lines} of a SyntheticSymDataset: the scenes' own boxes, every one as class 0 - synthetic scenes
    have no categories, and the one model under training predicts category 0"""
    gt = {}
    for i in range(len(val_ds)):
        lines = val_ds.scenes.gt_lines(i)
        gt[val_ds.scenes[i][0]] = [" ".join(line.split(" ")[:-1] + ["0"]) for line in lines]
    return gt


def config_gt_lines(val_ds, cfg):
    """{id_scan: ground-truth lines} from the files under cfg.data.gt_path (train_separate.py:436)"""
    gt = {}
    for ann in val_ds.annotations:
        with open(os.path.join(cfg.data.gt_path, ann["id_scan"] + ".txt")) as f:
            gt[ann["id_scan"]] = f.read().splitlines()
    return gt


def validation_line(epoch, v, category):
    """the one line of a validation: scan count, the four mean losses, AP and recall of the category at 0.25 and 0.5"""
    # (calc_map.compute_map has no entry for a class with neither a detection nor a ground-truth box)
    return "epoch %d  validation over %d scans  %s%s" % (
        epoch, v["n_scans"], "  ".join("%s %.4f" % kv for kv in v["losses"].items()),
        "".join("  AP@%.2f %.4f  recall@%.2f %.4f" % (t, m.get("%d Average Precision" % category, 0.0), t,
                                                      m.get("%d Recall" % category, 0.0))
                for t, m in v.get("map", {}).items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--save", default=None, help="prefix of the saved models: <prefix>_epoch<N>.pth every 10 epochs and at the end")
    ap.add_argument("--config", default=None, help="the reference's config.yaml: train on real ScanNet/Scan2CAD files")
    ap.add_argument("--category", default=None, help="with --config: the category of this model (a catid or 'others'; default: the config's)")
    ap.add_argument("--repaired-indexing", action="store_true",
                    help="offset the label rows of scan j by the rows of the scans in front (the reference indexes the batch "
                         "output with each scan's own row numbers, train_separate.py:270)")
    ap.add_argument("--device-loader", action="store_true",
                    help="with --config: workers read raw scans, the batch is built on the device (data.device_batch_sym)")
    ap.add_argument("--device-loss", action="store_true",
                    help="scale term and cross entropy on the row-loss kernels (train_step_separate(device_loss=True)) instead of torch ops")
    ap.add_argument("--val-every", type=int, default=0,
                    help="run the validation pass (train.validate_separate: losses, AP and recall of the category at 0.25 / 0.5) "
                         "every K epochs and on the last one, on rank 0; 0 = off")
    ap.add_argument("--val-scenes", type=int, default=2, help="without --config: synthetic validation scenes")
    a = ap.parse_args()
    if a.val_every < 0:
        ap.error("--val-every counts epochs: 0 (off) or more")
    if a.val_every > 0 and not a.config and a.val_scenes < 1:
        ap.error("--val-every without --config validates on synthetic scenes: --val-scenes must be 1 or more")
    if a.device_loader and not a.config:
        ap.error("--device-loader needs --config: the synthetic scenes (SyntheticSymDataset) are generated as finished items "
                 "and have no raw-scan form")
    if a.category and not a.config:
        ap.error("--category needs --config (synthetic scenes have no categories)")
    cfg = None
    if a.config:
        cfg = load_config(a.config, **({"category": a.category} if a.category else {}))
    world, rank, local = cvd.world()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    cvd.init("nccl", dev)
    torch.manual_seed(0)
    model = MinkUNet34C(6 if (cfg and cfg.use_xyz) else 3, 8).to(dev)
    net = train.make_ddp(model, dev) if world > 1 else model
    base_lr, wd, steps, rates = 1e-3, 0.0, (80, 120, 160), (0.1, 0.1, 0.1)      # train_separate.py:213: lr is 1e-3, not the config's
    bn_step, bn_rate = 20.0, 0.5
    first_epoch, last_epoch = 0, a.epochs - 1
    loss_kw = {}
    if cfg:
        wd = float(cfg.weight_decay)
        steps = [int(x) for x in str(cfg.opt.lr_decay_steps).split(",")]
        rates = [float(x) for x in str(cfg.opt.lr_decay_rates).split(",")]
        first_epoch, last_epoch = int(cfg.start_epoch), int(cfg.max_epoch)      # range(start_epoch, max_epoch + 1)
        bn_step, bn_rate = float(cfg.opt.bn_decay_step), float(cfg.opt.bn_decay_rate)
        loss_kw = dict(log_scale=bool(cfg.log_scale), xyz_factor=float(cfg.xyz_factor), scale_factor=float(cfg.scale_factor),
                       xyz_component_weights=tuple(float(x) for x in str(cfg.xyz_component_weights).split(",")))
    opt = train.make_optimizer(model, lr=base_lr, weight_decay=wd)
    collate = functools.partial(collate_sym, reference_indexing=not a.repaired_indexing)
    if cfg:
        ds = ScanNetXYZProbSymDataset(cfg, training=True, augment=cfg.augment)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=True) if world > 1 else None
        loader = torch.utils.data.DataLoader(RawItems(ds) if a.device_loader else ds, batch_size=cfg.batch_size,
                                             shuffle=sampler is None, sampler=sampler,
                                             collate_fn=collate_raw_sym if a.device_loader else collate, drop_last=True,
                                             num_workers=cfg.num_workers, pin_memory=True)
    else:
        ds = SyntheticSymDataset(a.scenes, a.points, seed0=1000 * rank)       # every rank owns its scenes
        loader = torch.utils.data.DataLoader(ds, batch_size=a.batch, shuffle=True, collate_fn=collate, drop_last=True)
    val_ds, hv = None, None
    if a.val_every > 0 and rank == 0:
        from canonicalvoting_amd.hough import HoughVoting
        val_res = float(cfg.scannet_res) if cfg else ds.scenes.res
        hv = HoughVoting(val_res)
        if cfg:
            val_ds = ScanNetXYZProbSymDataset(cfg, training=False, augment=False)
            val_gt, category = config_gt_lines(val_ds, cfg), TOP8_CLASSES.get(str(cfg.category), 0)
        else:
            val_ds = SyntheticSymDataset(a.val_scenes, a.points, seed0=500000)
            val_gt, category = synthetic_gt_lines(val_ds), 0
    for epoch in range(first_epoch, last_epoch + 1):
        train.adjust_learning_rate(opt, epoch, base_lr, steps, rates)
        train.set_bn_momentum(model, train.bn_momentum(epoch, bn_step, bn_rate))   # train_separate.py:216-217,230
        net.train()
        t0, losses = time.perf_counter(), []
        batches = device_loader_batches(loader, dev, cfg, not a.repaired_indexing) if a.device_loader else device_batches(loader, dev)
        for batch in batches:
            res = train.train_step_separate(net, opt, *batch, device_loss=a.device_loss, **loss_kw)
            if res is not None:                                             # train_separate.py:238-240: no object, no step
                losses.append(res[0])
        # every rank, in front of everything that reads the model between two steps: a range flag of the epoch's last steps
        # would otherwise be noticed only in the next epoch, behind a checkpoint and a validation over non-finite statistics
        train.finish_pending(net)
        if rank == 0:
            mean = float(torch.stack(losses).mean()) if losses else float("nan")          # one host wait per epoch
            print("epoch %d  loss %.4f  %d steps  %.1f s" % (epoch, mean, len(losses), time.perf_counter() - t0), flush=True)
        if a.save and rank == 0 and (epoch % 10 == 0 or epoch == last_epoch):
            # train_separate.py:298-299: one file per saved epoch, 'epoch{N}.pth' (here under the --save prefix)
            stem, ext = os.path.splitext(a.save)
            torch.save(model.state_dict(), "%s_epoch%d%s" % (stem, epoch, ext or ".pth"))
        if val_ds is not None and (epoch % a.val_every == 0 or epoch == last_epoch):
            # train_separate.py:301-458; the other ranks go on to their next epoch and meet this one at its first all-reduce
            v = train.validate_separate(model, hv, validation_scans(val_ds, dev, cfg, a.device_loader), val_res, category=category,
                                        gt_boxes=val_gt, device_loss=a.device_loss, **loss_kw)
            print(validation_line(epoch, v, category), flush=True)
    cvd.finalize()


if __name__ == "__main__":
    main()
