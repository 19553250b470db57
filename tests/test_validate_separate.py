"""The per-category trainer's validation pass without a GPU: the script's new arguments, the synthetic ground truth as class 0,
train.finish_pending on a model that has no flag ring, and the golden values of the reference's validation lines
(train_separate.py:322-357, tests/golden/sep_val_loss_ref.npz) against train.separate_loss - the validation lines are the
training lines' arithmetic - and against the fp64 oracles whose bounds the GPU test uses."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

from canonicalvoting_amd import data, train
from tests import row_loss_ref, sym_loss_ref
from tests.golden import make_sep_val_loss_golden as golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "train_separate.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sep_val_loss_ref.npz")


def _script():
    spec = importlib.util.spec_from_file_location("cv_train_separate", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_script_has_the_validation_flags_and_refuses_bad_ones():
    r = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--val-every" in r.stdout and "--val-scenes" in r.stdout
    assert "no validation pass" not in r.stdout
    r = subprocess.run([sys.executable, SCRIPT, "--val-every", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--val-every counts epochs" in r.stderr
    r = subprocess.run([sys.executable, SCRIPT, "--val-every", "1", "--val-scenes", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--val-scenes must be 1 or more" in r.stderr
    # the earlier refusals still come first
    r = subprocess.run([sys.executable, SCRIPT, "--val-every", "1", "--device-loader"], capture_output=True, text=True)
    assert r.returncode == 2 and "--device-loader needs --config" in r.stderr


def test_synthetic_ground_truth_counts_as_class_0():
    mod = _script()
    ds = data.SyntheticSymDataset(2, 2000, res=0.06, seed0=500000, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
    gt = mod.synthetic_gt_lines(ds)
    assert sorted(gt) == sorted(ds[i][0] for i in range(2))
    seen = set()
    for i in range(2):
        own = ds.scenes.gt_lines(i)
        lines = gt[ds[i][0]]
        assert len(lines) == len(own) > 0
        for line, was in zip(lines, own):
            assert line.split(" ")[:7] == was.split(" ")[:7] and line.split(" ")[-1] == "0"
            seen.add(was.split(" ")[-1])
        assert [c for c, _ in data.parse_gt_lines(lines)] == [0] * len(own)
        assert [p for _, p in data.parse_gt_lines(lines)] == [p for _, p in data.parse_gt_lines(own)]
    assert seen - {"0"}                                # the scenes' own classes were not all 0: the rewrite did something


def test_validation_line_names_the_losses_and_the_category():
    mod = _script()
    v = {"n_scans": 2, "losses": {"loss": 1.5, "loss_obj": 0.5, "loss_scale": 0.75, "loss_xyz": 0.25},
         "map": {0.25: {"6 Average Precision": 0.5, "6 Recall": 1.0, "mAP": 0.5}, 0.5: {"mAP": 0.0}}}
    line = mod.validation_line(3, v, 6)
    assert line.startswith("epoch 3  validation over 2 scans  loss 1.5000  loss_obj 0.5000  loss_scale 0.7500  loss_xyz 0.2500")
    assert "AP@0.25 0.5000  recall@0.25 1.0000" in line and "AP@0.50 0.0000  recall@0.50 0.0000" in line
    assert "\n" not in line


def test_finish_pending_without_a_ring_is_false():
    model = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.BatchNorm1d(3))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert train.finish_pending(model) is False                      # never stepped: no state at all
    assert "_cv_step_state" not in model.__dict__
    st = train._step_state(model)                                    # stepped, but without a ring (non-fused optimizer)
    assert train.finish_pending(model) is False
    st.pairs_off = True                                              # on the triples already
    assert train.finish_pending(model) is False
    assert st.pairs_off and st.ring is None and st.snapshot is None and not hasattr(model, "train_range_fallbacks")
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())


def test_finish_pending_reads_every_slot_of_a_host_ring():
    """the ring on the host (no events): a flag in the YOUNGEST slot, which the lagged read would not look at yet"""
    ring = train._FlagRing(torch.device("cpu"))
    assert not ring.pending()
    ring.push(torch.zeros(()))
    assert not ring.pending() and not ring.noticed()
    ring.push(torch.ones(()))
    assert not ring.noticed() and ring.pending()
    ring.push(None)                                                  # a step without fp16 pairs invalidates its slot
    assert ring.pending()
    ring.push(None)
    assert not ring.pending()


def test_golden_validation_losses_are_the_training_arithmetic():
    z = np.load(GOLDEN)
    assert sorted(z.files) == ["loss_obj", "loss_scale", "loss_xyz"]
    assert all(isinstance(z[k], np.ndarray) and z[k].dtype == np.float32 and z[k].shape == () for k in z.files)
    out, labels, scale, obj = golden.make_inputs()
    assert out.shape == (1000, 8) and len(labels) == 3 and sorted(len(x) for _, x in labels) == [1, 4, 36]
    kw = dict(xyz_factor=golden.XYZ_FACTOR, scale_factor=golden.SCALE_FACTOR, xyz_component_weights=golden.WEIGHTS)
    total, parts = train.separate_loss(torch.from_numpy(out), golden.nested_torch(labels), torch.from_numpy(scale),
                                       torch.from_numpy(obj), **kw)
    # the same lines on the same CPU: the same bits
    for k in ("loss_obj", "loss_scale", "loss_xyz"):
        assert np.array_equal(parts[k].numpy(), z[k]), (k, float(parts[k]), float(z[k]))
    assert float(total) == float(parts["loss_obj"] + parts["loss_scale"] + parts["loss_xyz"])
    # the factors and weights are in the values: unit settings give other ones
    _, unit = train.separate_loss(torch.from_numpy(out), golden.nested_torch(labels), torch.from_numpy(scale), torch.from_numpy(obj))
    assert abs(float(unit["loss_xyz"]) - float(z["loss_xyz"])) > 1e-4 and abs(float(unit["loss_scale"]) - float(z["loss_scale"])) > 1e-2


def test_golden_validation_losses_lie_inside_the_oracles_bounds():
    """what lets the GPU test hold validate_separate to the kernels' bounds AT the golden values: the reference's fp32 results
    are themselves within those bounds of the fp64 oracles, and the minimum over the poses is decidable"""
    z = np.load(GOLDEN)
    out, labels, scale, obj = golden.make_inputs()
    sym = data.pack_sym([labels], [out.shape[0]])
    r = sym_loss_ref.oracle(out, sym, golden.WEIGHTS, golden.XYZ_FACTOR)
    assert sym_loss_ref.decidable(r) > 1.0 and list(r["best"]) == [3, 0, 0]
    assert abs(float(z["loss_xyz"]) - r["loss"]) <= sym_loss_ref.LOSS_BOUND * sym_loss_ref.U * r["loss"]
    c = row_loss_ref.config("separate", w=golden.WEIGHTS, xyz_factor=golden.XYZ_FACTOR, scale_factor=golden.SCALE_FACTOR)
    rr = row_loss_ref.oracle(out, obj, None, scale, c)
    assert abs(float(z["loss_scale"]) - rr["losses"][1]) <= rr["loss_bounds"][1]
    assert abs(float(z["loss_obj"]) - rr["losses"][2]) <= rr["loss_bounds"][2]
