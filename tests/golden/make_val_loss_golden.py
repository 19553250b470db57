"""Golden vectors for the joint trainer's VALIDATION losses, produced by executing the reference's own lines
(train_joint.py:311-340: head gather by the predicted class, mean squared errors over the object rows, CE(class)) on CPU torch
tensors in the build container; `.cuda()` patched to a plain copy.  Two cases of 1 000 seeded rows: labels -1 .. 9, and labels
that are all background, where both means are the mean over nothing (NaN).  Stores the three losses of each case, arrays only
(tests/golden/val_loss_ref.npz); tests/test_row_loss.py compares the fp64 oracle's argmax / nan form with them,
tests/test_row_loss_gpu.py the kernels.

    python tests/golden/make_val_loss_golden.py            # needs /root/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_loss_golden import REF, ref_lines  # noqa: E402

WEIGHTS, XYZ_FACTOR, SCALE_FACTOR = (0.5, 2.0, 1.0), 0.7, 1.3


def make_inputs(case, seed=11, n=1000, nclasses=9):
    """case 'mixed': labels -1 .. 9; 'background': 9 and -1 only (no object row)"""
    rng = np.random.default_rng(seed + (0 if case == "mixed" else 1))
    F = rng.normal(0, 1.5, (n, 7 * nclasses + 1)).astype(np.float32)
    labels = (rng.integers(-1, nclasses + 1, n) if case == "mixed" else rng.choice([-1, nclasses], n)).astype(np.int64)
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    scale = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    return F, labels, xyz, scale


def run_reference(case):
    F, labels, xyz, scale = make_inputs(case)
    cfg = types.SimpleNamespace(log_scale=True, xyz_factor=XYZ_FACTOR, scale_factor=SCALE_FACTOR)
    # the reference's dataloader has mapped -1 to 9 before the labels reach these lines (utils/dataloader.py:172)
    ns = {"torch": torch, "nclasses": 9, "cfg": cfg, "scan_output": types.SimpleNamespace(F=torch.from_numpy(F.copy())),
          "scan_class_labels": torch.from_numpy(np.where(labels < 0, 9, labels)), "scan_xyz_labels": torch.from_numpy(xyz),
          "scan_scale_labels": torch.from_numpy(scale), "xyz_weights": torch.tensor(WEIGHTS),
          "obj_criterion": torch.nn.CrossEntropyLoss(), "losses": {}}
    exec(ref_lines(311, 340), ns)
    return {k: np.asarray(ns["losses"][k].numpy(), np.float32) for k in ("loss_xyz", "loss_scale", "loss_class")}


if __name__ == "__main__":
    assert os.path.exists(REF), "run where /root/reference is mounted"
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self.clone()      # a host-to-device transfer is a copy
    try:
        store = {}
        for case in ("mixed", "background"):
            r = run_reference(case)
            print(case, {k: float(v) for k, v in r.items()})
            store.update({"%s_%s" % (case, k): v for k, v in r.items()})
        np.savez_compressed(os.path.join(HERE, "val_loss_ref.npz"), **store)
    finally:
        torch.Tensor.cuda = orig_cuda
