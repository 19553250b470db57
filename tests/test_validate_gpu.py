"""train.validate_joint (train_joint.py:293-430) on the GPU: its losses are joint_loss_val on the eval-mode forward, its
detections pipeline.detect_scene's on the same model and scan, and it leaves the model in train mode with untouched BatchNorm
statistics."""
import numpy as np
import pytest
import torch

from canonicalvoting_amd import pipeline, train
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_scene

pytestmark = pytest.mark.gpu
RES = 0.06
# a seeded, untrained network votes weakly: thresholds under which its grids still yield candidates and boxes
DECODE = dict(thresh_high=3.0, thresh_low=1, valid_ratio=0.0, prob_thresh=0.0, err_thresh=1e9)


def _scans(cuda):
    out = []
    for seed in (61, 62):
        s = make_scene(seed, n_points=3000, res=RES, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
        coords4 = torch.cat([torch.zeros((3000, 1), dtype=torch.int32), torch.from_numpy(s.coords)], 1).to(cuda)
        t = lambda a: torch.from_numpy(a).to(cuda)
        lines = ["%f %f %f %f %f %f %f %d" % tuple(list(b[:7]) + [int(b[7])]) for b in s.boxes]
        out.append((("scan%d" % seed, coords4, t(s.feats) * 2 - 1, t(s.xyz_labels), t(s.scale_labels), t(s.class_labels)), lines))
    return out


def test_validate_joint_is_the_eval_forward_its_val_loss_and_detect_scene(cuda, built_lib):
    scans = _scans(cuda)
    torch.manual_seed(3)
    model = MinkUNet34C(3, 64).cuda()
    hv = HoughVoting(RES)
    model.eval()
    want_losses, want_dets = [], {}
    for (sid, coords4, feats, xyz, scale, cls), _ in scans:
        dets, raw, y = pipeline.detect_scene(model, hv, coords4, feats, RES, **DECODE)
        total, parts = train.joint_loss_val(y.F, xyz, scale, cls)
        want_losses.append(torch.stack([total, parts["loss_xyz"], parts["loss_scale"], parts["loss_class"]]))
        want_dets[sid] = dets
    want = torch.stack(want_losses).mean(0).tolist()
    model.train()
    torch.cuda.synchronize()
    stats = {k: b.detach().clone() for k, b in model.named_buffers()}
    res = train.validate_joint(model, hv, [b for b, _ in scans], RES, gt_boxes={b[0]: lines for b, lines in scans}, **DECODE)
    torch.cuda.synchronize()
    assert model.training and all(m.training for m in model.modules())
    assert len(stats) > 0 and all(torch.equal(stats[k].reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
                                  for k, b in model.named_buffers())
    assert res["n_scans"] == 2 and sorted(res["pred_map_cls"]) == sorted(want_dets)
    got = [res["losses"][k] for k in ("loss", "loss_xyz", "loss_scale", "loss_class")]
    print("validation losses", got, "detections", {k: len(v) for k, v in want_dets.items()})
    assert np.isfinite(got).all() and np.array_equal(np.array(got), np.array(want))
    for sid, dets in want_dets.items():
        have = res["pred_map_cls"][sid]
        assert len(have) == len(dets)
        for (c0, b0, s0), (c1, b1, s1) in zip(have, dets):
            assert c0 == c1 and s0 == s1 and np.array_equal(np.asarray(b0), np.asarray(b1))
    assert sorted(res["map"]) == [0.25, 0.5] and all("mAP" in res["map"][t] for t in (0.25, 0.5))
    # without ground truth there is no mAP, and a model in eval mode stays in eval mode
    model.eval()
    res = train.validate_joint(model, hv, [scans[0][0]], RES, **DECODE)
    assert "map" not in res and res["n_scans"] == 1 and not model.training
