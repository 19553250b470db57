"""train.validate_separate (train_separate.py:301-458) and train.finish_pending on the GPU: the pass is separate_loss_packed on
the eval-mode forward plus pipeline.detect_scene_separate's detections of the one category, it skips a scan without objects and
leaves the model as it found it; its losses reproduce the reference's validation lines (tests/golden/sep_val_loss_ref.npz) at
the kernels' derived bounds; finish_pending acts on a range flag the lagged read has not reached; the script prints a
validation line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from canonicalvoting_amd import calc_map, data, pipeline, train
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests import row_loss_ref, sym_loss_ref
from tests.golden import make_sep_val_loss_golden as golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.06
CATEGORY = 6
# a seeded, untrained network votes weakly: thresholds under which its grids still yield candidates and boxes
DECODE = dict(thresh_high=3.0, thresh_low=1, valid_ratio=0.0, prob_thresh=0.0, err_thresh=1e9)
LOSS_KEYS = ("loss", "loss_obj", "loss_scale", "loss_xyz")


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _scans(cuda):
    """[(the scan as validate_separate reads it, labels on the host), ground-truth lines as the category]: two synthetic
    scans with objects, then the first one again under another name with its labels blanked"""
    ds = data.SyntheticSymDataset(2, 3000, res=RES, seed0=61, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
    out = []
    for i in range(2):
        ids, coords4, feats, sym, scale, obj, _ = data.collate_sym([ds[i]])
        assert sym.n_segments > 0
        lines = [" ".join(line.split(" ")[:-1] + [str(CATEGORY)]) for line in ds.scenes.gt_lines(i)]
        out.append(((ids[0], coords4.to(cuda), feats.to(cuda) * 2 - 1, sym, scale, obj), lines))
    (_, coords4, feats, _, scale, obj), lines = out[0]
    blank = data.pack_sym([[]], [coords4.shape[0]])
    assert blank.n_segments == 0
    out.append((("blank", coords4, feats, blank, scale, torch.zeros_like(obj)), lines))
    return out


def _loss_row(total, parts):
    return torch.stack([total, parts["loss_obj"], parts["loss_scale"], parts["loss_xyz"]])


def test_validate_separate_is_the_eval_forward_its_packed_loss_and_detect_scene_separate(cuda, built_lib):
    scans = _scans(cuda)
    torch.manual_seed(3)
    model = MinkUNet34C(3, 8).cuda()
    hv = HoughVoting(RES)
    model.eval()
    want_rows, want_dets = {False: [], True: []}, {}
    for (sid, coords4, feats, sym, scale, obj), _ in scans[:2]:
        with torch.no_grad():
            y = model(ME.SparseTensor(feats, coords4, device=cuda))
            for device_rows in (False, True):
                want_rows[device_rows].append(_loss_row(*train.separate_loss_packed(
                    y.F, data.sym_to_device(sym, cuda), scale.to(cuda), obj.to(cuda), device_rows=device_rows)))
        want_dets[sid] = pipeline.detect_scene_separate({CATEGORY: model}, hv, coords4, feats, RES, **DECODE)
    print("detections of the call-by-call path", {k: len(v) for k, v in want_dets.items()})
    assert any(len(v) > 0 for v in want_dets.values())                  # the comparison below is not one of empty lists
    model.train()
    torch.cuda.synchronize()
    stats = {k: b.detach().clone() for k, b in model.named_buffers()}
    gt = {b[0]: lines for b, lines in scans}
    res = train.validate_separate(model, hv, [b for b, _ in scans], RES, category=CATEGORY, gt_boxes=gt, **DECODE)
    torch.cuda.synchronize()
    assert model.training and all(m.training for m in model.modules())
    assert len(stats) > 0 and all(torch.equal(_bits(stats[k]), _bits(b)) for k, b in model.named_buffers())
    assert res["n_scans"] == 2 and sorted(res["pred_map_cls"]) == sorted(want_dets) and "blank" not in res["pred_map_cls"]
    assert tuple(res["losses"]) == LOSS_KEYS
    got = [res["losses"][k] for k in LOSS_KEYS]
    want = torch.stack(want_rows[False]).mean(0).tolist()
    print("validation losses", got)
    assert np.isfinite(got).all() and np.array_equal(np.array(got), np.array(want))
    for sid, dets in want_dets.items():
        have = res["pred_map_cls"][sid]
        assert len(have) == len(dets)
        for (c0, b0, s0), (c1, b1, s1) in zip(have, dets):
            assert c0 == c1 == CATEGORY and s0 == s1 and np.array_equal(np.asarray(b0), np.asarray(b1))
    # the mAP dicts: compute_map over the returned detections and the ground truth of the scans that ran
    gt_map_cls = {i: [(c, calc_map.gt_box(*p)) for c, p in data.parse_gt_lines(gt[i])] for i in res["pred_map_cls"]}
    assert all(c == CATEGORY for boxes in gt_map_cls.values() for c, _ in boxes)
    assert sorted(res["map"]) == [0.25, 0.5]
    for thr in (0.25, 0.5):
        again = calc_map.compute_map(res["pred_map_cls"], gt_map_cls, thr)
        assert sorted(again) == sorted(res["map"][thr]) and "%d Average Precision" % CATEGORY in again
        assert all(np.array_equal(np.asarray(again[k]), np.asarray(res["map"][thr][k]), equal_nan=True) for k in again)
    # the row terms on row_loss.hip
    res_dev = train.validate_separate(model, hv, [b for b, _ in scans], RES, category=CATEGORY, device_loss=True, **DECODE)
    got_dev = [res_dev["losses"][k] for k in LOSS_KEYS]
    assert np.isfinite(got_dev).all() and np.array_equal(np.array(got_dev), np.array(torch.stack(want_rows[True]).mean(0).tolist()))
    assert "map" not in res_dev and res_dev["n_scans"] == 2 and model.training
    # a model in eval mode stays in eval mode; no scan with objects: NaN means, nothing else
    model.eval()
    res = train.validate_separate(model, hv, [scans[0][0]], RES, category=CATEGORY, **DECODE)
    assert "map" not in res and res["n_scans"] == 1 and not model.training
    res = train.validate_separate(model, hv, [scans[2][0]], RES, category=CATEGORY, gt_boxes=gt, **DECODE)
    assert res["n_scans"] == 0 and res["pred_map_cls"] == {} and all(np.isnan(res["losses"][k]) for k in LOSS_KEYS)
    assert not model.training


class _FixedOutput(torch.nn.Module):
    """a 'network' whose output is a fixed [n, 8] array on the input's coordinate set"""

    def __init__(self, F):
        super().__init__()
        self.register_buffer("out", F)

    def forward(self, x):
        return ME.SparseTensor(self.out, coordinate_manager=x.coordinate_manager)


def test_validate_separate_reproduces_the_references_validation_losses(cuda, built_lib):
    """train_separate.py:322-357 executed on the golden's inputs (tests/golden/make_sep_val_loss_golden.py) against the pass over
    that one scan, every term at the bound its kernel was specified with (tests/sym_loss_ref.py, tests/row_loss_ref.py: the
    bounds come from the fp64 oracle on the same inputs; tests/test_validate_separate.py shows the golden values themselves
    inside them).  Both forms of the row terms: the torch ops and row_loss.hip."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "sep_val_loss_ref.npz"))
    out, labels, scale, obj = golden.make_inputs()
    n = out.shape[0]
    sym = data.pack_sym([labels], [n])
    r_xyz = sym_loss_ref.oracle(out, sym, golden.WEIGHTS, golden.XYZ_FACTOR)
    c = row_loss_ref.config("separate", w=golden.WEIGHTS, xyz_factor=golden.XYZ_FACTOR, scale_factor=golden.SCALE_FACTOR)
    r_row = row_loss_ref.oracle(out, obj, None, scale, c)
    bounds = {"loss_xyz": sym_loss_ref.LOSS_BOUND * sym_loss_ref.U * r_xyz["loss"], "loss_scale": r_row["loss_bounds"][1],
              "loss_obj": r_row["loss_bounds"][2]}
    oracle = {"loss_xyz": r_xyz["loss"], "loss_scale": r_row["losses"][1], "loss_obj": r_row["losses"][2]}
    grid = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    coords4 = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.int64), grid], 1).astype(np.int32)).to(cuda)
    feats = torch.zeros((n, 3), device=cuda)
    model = _FixedOutput(torch.from_numpy(out).to(cuda))
    hv = HoughVoting(RES)
    scan = ("golden", coords4, feats, sym, torch.from_numpy(scale), torch.from_numpy(obj))
    kw = dict(xyz_factor=golden.XYZ_FACTOR, scale_factor=golden.SCALE_FACTOR, xyz_component_weights=golden.WEIGHTS)
    for device_loss in (False, True):
        res = train.validate_separate(model, hv, [scan], RES, device_loss=device_loss, **kw)
        assert res["n_scans"] == 1 and list(res["pred_map_cls"]) == ["golden"]
        for k in ("loss_obj", "loss_scale", "loss_xyz"):
            have, want = res["losses"][k], float(z[k])
            print("device_loss=%s %s: %.9g  golden %.9g  |have - golden| / bound %.3f  |have - oracle| / bound %.3f"
                  % (device_loss, k, have, want, abs(have - want) / bounds[k], abs(have - oracle[k]) / bounds[k]))
        for k in ("loss_obj", "loss_scale", "loss_xyz"):
            assert abs(res["losses"][k] - float(z[k])) <= bounds[k], (device_loss, k)
            assert abs(res["losses"][k] - oracle[k]) <= bounds[k], (device_loss, k)
        total = float(z["loss_obj"]) + float(z["loss_scale"]) + float(z["loss_xyz"])
        assert abs(res["losses"]["loss"] - total) <= sum(bounds.values()) + 2 * row_loss_ref.U * total


def test_finish_pending_acts_on_a_flag_nobody_has_read(cuda, built_lib, monkeypatch):
    """The recipe of tests/test_train_gpu.py (a BatchNorm gain of 1e7 under the fused Adam), stopped ONE step after the flag
    was raised - where an epoch may end: the lagged read has not looked, the running statistics are non-finite.
    finish_pending restores them from the snapshot, clears the flag, counts the fallback and leaves the model on the triples;
    without a raised flag it changes no bit."""
    monkeypatch.setattr(ME, "TRAIN_FWD_HL", 1)
    (sid, coords4, feats, sym, scale, obj), _ = _scans(cuda)[0]
    args = (coords4, feats, data.sym_to_device(sym, cuda), scale.to(cuda), obj.to(cuda))
    dev = torch.device(cuda)
    torch.manual_seed(0)
    model = MinkUNet34C(3, 8).cuda().train()
    opt = train.make_optimizer(model, lr=1e-3)
    assert train.finish_pending(model) is False                        # never stepped
    train.train_step_separate(model, opt, *args)                       # healthy
    torch.cuda.synchronize()
    st = train._step_state(model)
    ring = st.ring
    assert ring is not None and not st.pairs_off
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ring_k, snapshot = ring.k, [s.clone() for s in st.snapshot]
    assert train.finish_pending(model) is False
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(state[k]), _bits(v)) for k, v in model.state_dict().items())
    assert st.ring is ring and ring.k == ring_k and not st.pairs_off and getattr(model, "train_range_fallbacks", 0) == 0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(snapshot, st.snapshot))
    assert int(ME.range_flag(dev)[0]) == 0
    gain = model.bn0.bn.weight.detach().clone()
    with torch.no_grad():
        model.bn0.bn.weight.fill_(1e7)
    torch.cuda.synchronize()
    params_before = {k: p.detach().clone() for k, p in model.named_parameters()}
    stats_before = {k: b.detach().clone() for k, b in model.named_buffers()}
    nbt = int(model.bn0.bn.num_batches_tracked)
    train.train_step_separate(model, opt, *args)                       # ONE flagged step
    torch.cuda.synchronize()
    assert getattr(model, "train_range_fallbacks", 0) == 0 and not ring.noticed()             # nobody has looked yet
    assert not all(bool(torch.isfinite(b).all()) for b in model.buffers() if b.is_floating_point())
    assert int(ME.range_flag(dev)[0]) != 0
    assert train.finish_pending(model) is True
    assert all(torch.equal(_bits(stats_before[k]), _bits(b)) for k, b in model.named_buffers())
    assert all(torch.equal(params_before[k], p.detach()) for k, p in model.named_parameters())    # the update was skipped
    assert int(ME.range_flag(dev)[0]) == 0 and model.train_range_fallbacks == 1
    assert st.pairs_off and st.ring is None
    assert train.finish_pending(model) is False and model.train_range_fallbacks == 1
    with torch.no_grad():
        model.bn0.bn.weight.copy_(gain)
    scan = (sid, coords4, feats, sym, scale, obj)
    res = train.validate_separate(model, HoughVoting(RES), [scan], RES, **DECODE)
    assert res["n_scans"] == 1 and np.isfinite([res["losses"][k] for k in LOSS_KEYS]).all(), res["losses"]
    assert model.training and int(model.bn0.bn.num_batches_tracked) == nbt
    loss, _ = train.train_step_separate(model, opt, *args)             # an ordinary step on the triples
    assert np.isfinite(float(loss)) and model.train_range_fallbacks == 1 and st.ring is None
    assert all(int(m.bn.num_batches_tracked) == nbt + 1 for m in model.modules() if isinstance(m, ME.MinkowskiBatchNorm))
    assert all(bool(torch.isfinite(b).all()) for b in model.buffers())
    assert any(not torch.equal(params_before[k], p.detach()) for k, p in model.named_parameters() if k != "bn0.bn.weight")


def test_the_script_prints_a_validation_line(cuda, built_lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_separate.py"), "--epochs", "1", "--scenes", "3",
                        "--points", "3000", "--batch", "3", "--val-every", "1", "--val-scenes", "2"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    lines = [line for line in r.stdout.splitlines() if "validation over" in line]
    assert len(lines) == 1 and lines[0].startswith("epoch 0  validation over ")
    m = re.search(r"validation over (\d+) scans  loss (\S+)  loss_obj (\S+)  loss_scale (\S+)  loss_xyz (\S+)", lines[0])
    assert m and 1 <= int(m.group(1)) <= 2
    assert np.isfinite([float(m.group(i)) for i in range(2, 6)]).all()
    assert all(("%s@%s" % (what, thr)) in lines[0] for what in ("AP", "recall") for thr in ("0.25", "0.50"))
