#!/usr/bin/env python
"""train_joint.py counterpart (reference train_joint.py:191-291) on synthetic scans: Adam, step LR decay,
batch of 3 scenes, masked MSE(xyz) + MSE(log scale) + CE(class); one process per GPU with DDP when launched
through torch.distributed.run (the reference is single-GPU).

    python scripts/train_joint.py [--epochs 2] [--scenes 6] [--points 20000] [--batch 3]
    python scripts/train_joint.py --config config.yaml [--device-loader]
    python scripts/train_joint.py --device-loss --val-every 10

--device-loader (with --config): the workers stop at the raw scan (``raw_item``) and the batch - colours, labels,
voxelisation, gathers - is built on the device (``data.device_batch``); the same batches bit for bit.
--device-loss: the loss and its backward on the row-loss kernels (``train.joint_loss_device``).
--val-every K: every K epochs, next to the checkpoint and on rank 0, the reference's validation pass
(train_joint.py:293-430, ``train.validate_joint``): validation losses, detections and mAP at 0.25 / 0.5 over the validation
scans (the config's validation split; without --config, ``--val-scenes`` further synthetic scenes).  0 = off.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd import dist as cvd  # noqa: E402
from canonicalvoting_amd import train  # noqa: E402
from canonicalvoting_amd.data import (RawItems, ScanNetXYZProbMultiDataset, SyntheticScanDataset, collate_fn,  # noqa: E402
                                     collate_raw, device_batch, load_config)
from canonicalvoting_amd.minkunet import MinkUNet34C  # noqa: E402


def host_batches(loader, dev):
    """train_joint.py:245-249: the collated host batch, copied to the device, colour columns recentred"""
    for _, coords, feats, xyz, scale, cls in loader:
        feats = feats.to(dev)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0                         # train_joint.py:248-249: colour columns only
        yield coords.to(dev), feats, xyz.to(dev), scale.to(dev), cls.to(dev)


def validation_scans(val_ds, dev):
    """train_joint.py:301-306: one scan per batch, in the form train.validate_joint reads"""
    loader = torch.utils.data.DataLoader(val_ds, collate_fn=collate_fn, batch_size=1, shuffle=False)
    for ids, coords, feats, xyz, scale, cls in loader:
        feats = feats.to(dev)
        feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0
        yield ids[0], coords.to(dev), feats, xyz.to(dev), scale.to(dev), cls.to(dev)


def validation_gt_lines(val_ds, cfg):
    """{id_scan: ground-truth lines}: the files under cfg.data.gt_path, or the synthetic scenes' own boxes"""
    if cfg is None:
        return {val_ds[i][0]: val_ds.gt_lines(i) for i in range(len(val_ds))}
    gt = {}
    for ann in val_ds.annotations:
        with open(os.path.join(cfg.data.gt_path, ann["id_scan"] + ".txt")) as f:
            gt[ann["id_scan"]] = f.read().splitlines()
    return gt


def device_batches(loader, dev, cfg):
    """the same batches from raw scans (--device-loader)"""
    for raw in loader:
        yield device_batch(raw, dev, cfg.scannet_res, use_xyz=cfg.use_xyz, recentre=True)[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--save", default=None)
    ap.add_argument("--config", default=None, help="the reference's config.yaml: train on real ScanNet/Scan2CAD files")
    ap.add_argument("--device-loader", action="store_true",
                    help="with --config: build every batch on the device from raw scans (data.device_batch)")
    ap.add_argument("--device-loss", action="store_true",
                    help="loss and its backward on the row-loss kernels (train.joint_loss_device) instead of torch ops")
    ap.add_argument("--val-every", type=int, default=0,
                    help="run the validation pass (train.validate_joint: losses, mAP@0.25/0.5) every K epochs on rank 0; 0 = off")
    ap.add_argument("--val-scenes", type=int, default=2, help="without --config: synthetic validation scenes")
    a = ap.parse_args()
    if a.device_loader and not a.config:
        ap.error("--device-loader needs --config (synthetic items are already voxel-level)")
    cfg = load_config(a.config, category="all") if a.config else None
    world, rank, local = cvd.world()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    cvd.init("nccl", dev)
    torch.manual_seed(0)
    model = MinkUNet34C(6 if (cfg and cfg.use_xyz) else 3, 6 * 9 + 9 + 1).to(dev)
    net = train.make_ddp(model, dev) if world > 1 else model
    base_lr, wd, steps, rates = a.lr, 0.0, (80, 120, 160), (0.1, 0.1, 0.1)
    bn_step, bn_rate = 20.0, 0.5                                               # config/config.yaml opt.bn_decay_*
    first_epoch, last_epoch = 0, a.epochs - 1
    if cfg:
        # train_joint.py:204-206,219-223,235: the optimizer and the schedule come from the config
        base_lr, wd = float(cfg.opt.learning_rate), float(cfg.weight_decay)
        steps = [int(x) for x in str(cfg.opt.lr_decay_steps).split(",")]
        rates = [float(x) for x in str(cfg.opt.lr_decay_rates).split(",")]
        first_epoch, last_epoch = int(cfg.start_epoch), int(cfg.max_epoch)      # range(start_epoch, max_epoch + 1)
        bn_step, bn_rate = float(cfg.opt.bn_decay_step), float(cfg.opt.bn_decay_rate)
    opt = train.make_optimizer(model, lr=base_lr, weight_decay=wd)
    if cfg:
        # train_joint.py:205-211; every rank reads its own slice of the scans (DistributedSampler)
        ds = ScanNetXYZProbMultiDataset(cfg, training=True, augment=cfg.augment)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, world, rank, shuffle=True) if world > 1 else None
        loader = torch.utils.data.DataLoader(RawItems(ds) if a.device_loader else ds, batch_size=cfg.batch_size,
                                             shuffle=sampler is None, sampler=sampler,
                                             collate_fn=collate_raw if a.device_loader else collate_fn, drop_last=True,
                                             num_workers=cfg.num_workers, pin_memory=a.device_loader)
    else:
        ds = SyntheticScanDataset(a.scenes, a.points, seed0=1000 * rank)      # every rank owns its scenes
        loader = torch.utils.data.DataLoader(ds, batch_size=a.batch, shuffle=True, collate_fn=collate_fn, drop_last=True)
    val_ds, hv = None, None
    if a.val_every > 0 and rank == 0:
        from canonicalvoting_amd.hough import HoughVoting
        res = float(cfg.scannet_res) if cfg else ds.res
        hv = HoughVoting(res)
        val_ds = (ScanNetXYZProbMultiDataset(cfg, training=False, augment=False) if cfg
                  else SyntheticScanDataset(a.val_scenes, a.points, seed0=500000))
        val_gt = validation_gt_lines(val_ds, cfg)
    for epoch in range(first_epoch, last_epoch + 1):
        train.adjust_learning_rate(opt, epoch, base_lr, steps, rates)
        train.set_bn_momentum(model, train.bn_momentum(epoch, bn_step, bn_rate))   # train_joint.py:224-225,239
        net.train()
        t0, tot, n = time.perf_counter(), 0.0, 0
        for batch in (device_batches(loader, dev, cfg) if a.device_loader else host_batches(loader, dev)):
            loss, _ = train.train_step(net, opt, *batch, device_loss=a.device_loss)
            tot += float(loss)
            n += 1
        # every rank, in front of the checkpoint and the validation: act on a range flag of the epoch's last steps now
        train.finish_pending(net)
        if rank == 0:
            print("epoch %d  loss %.4f  %.1f s" % (epoch, tot / max(n, 1), time.perf_counter() - t0), flush=True)
        if a.save and rank == 0 and (epoch % 10 == 0 or epoch == last_epoch):
            # train_joint.py:290-291: one file per saved epoch, 'epoch{N}.pth' (here under the --save prefix)
            stem, ext = os.path.splitext(a.save)
            torch.save(model.state_dict(), "%s_epoch%d%s" % (stem, epoch, ext or ".pth"))
        if val_ds is not None and (epoch % a.val_every == 0 or epoch == last_epoch):
            # train_joint.py:293-430; the other ranks go on to their next epoch and meet this one at its first all-reduce
            v = train.validate_joint(model, hv, validation_scans(val_ds, dev), res, gt_boxes=val_gt)      # the training loss's settings
            print("epoch %d  validation over %d scans  %s%s" % (
                epoch, v["n_scans"], "  ".join("%s %.4f" % kv for kv in v["losses"].items()),
                "".join("  mAP@%.2f %.4f" % (t, m["mAP"]) for t, m in v.get("map", {}).items())), flush=True)
    cvd.finalize()


if __name__ == "__main__":
    main()
