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

The reference's validation every 10 epochs is not repeated here: scripts/eval_separate.py evaluates the saved models.
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
from canonicalvoting_amd.data import (RawItems, ScanNetXYZProbSymDataset, SyntheticSymDataset, collate_raw_sym,  # noqa: E402
                                      collate_sym, device_batch_sym, load_config, sym_to_device)
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


def main():
    ap = argparse.ArgumentParser(epilog="There is no validation pass in this trainer (scripts/train_joint.py has --val-every): "
                                        "the reference's validation every 10 epochs stays with scripts/eval_separate.py, which "
                                        "evaluates the saved models.")
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
    a = ap.parse_args()
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
        if rank == 0:
            mean = float(torch.stack(losses).mean()) if losses else float("nan")          # one host wait per epoch
            print("epoch %d  loss %.4f  %d steps  %.1f s" % (epoch, mean, len(losses), time.perf_counter() - t0), flush=True)
        if a.save and rank == 0 and (epoch % 10 == 0 or epoch == last_epoch):
            # train_separate.py:298-299: one file per saved epoch, 'epoch{N}.pth' (here under the --save prefix)
            stem, ext = os.path.splitext(a.save)
            torch.save(model.state_dict(), "%s_epoch%d%s" % (stem, epoch, ext or ".pth"))
    cvd.finalize()


if __name__ == "__main__":
    main()
