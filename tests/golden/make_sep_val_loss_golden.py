"""Golden vectors for the per-category trainer's VALIDATION losses, produced by executing the reference's own lines
(train_separate.py:322-357: head split, CE(objectness), mean squared log-scale error over the object rows, the coordinate loss
as the minimum over the symmetry-equivalent poses per model and the mean over the models, the two factors) on CPU torch
tensors in the build container; `.cuda()` patched to a plain copy.  One case: 1 000 seeded rows of an [n, 8] output, one scan
with 3 segments of 300 / 257 / 120 points and 4 / 1 / 36 poses (tests/sym_loss_ref.make_case: the predictions lie 0.05 from
the targets of one pose, so the minimum is decidable), non-unit component weights and factors.  Stores the three losses,
arrays only (tests/golden/sep_val_loss_ref.npz); tests/test_validate_separate.py compares train.separate_loss and the fp64
oracles with them, tests/test_validate_separate_gpu.py train.validate_separate.

    python tests/golden/make_sep_val_loss_golden.py            # needs /root/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_loss_golden import REF_SEP, ref_lines  # noqa: E402

WEIGHTS, XYZ_FACTOR, SCALE_FACTOR = (0.5, 2.0, 1.25), 0.7, 1.3
N_ROWS, LENS, POSES, BEST_AT = 1000, (300, 257, 120), (4, 1, 36), ("last", "first", "first")


def make_inputs(seed=17):
    """(out [1000, 8] float32, one scan's nested labels [[rows int64, [xyz float32 per pose]] x 3], scale_labels [1000, 3],
    obj_labels int64 [1000]: 1 on the rows of a segment)"""
    from tests.sym_loss_ref import make_case
    out, labels = make_case(seed, list(LENS), list(POSES), list(BEST_AT), n_rows=N_ROWS, ld=8)
    rng = np.random.default_rng(seed + 1)
    scale = rng.uniform(0.2, 0.9, (N_ROWS, 3)).astype(np.float32)
    obj = np.zeros(N_ROWS, np.int64)
    for rows, _ in labels:
        obj[rows] = 1
    return out, labels, scale, obj


def nested_torch(labels):
    """the scan's labels as data.collate_fn_separate hands them to the loss: a batch of one scan"""
    return [[[torch.from_numpy(rows).long(), [torch.from_numpy(x).float() for x in xyzs]] for rows, xyzs in labels]]


def run_reference():
    out, labels, scale, obj = make_inputs()
    cfg = types.SimpleNamespace(log_scale=True, xyz_factor=XYZ_FACTOR, scale_factor=SCALE_FACTOR)
    obj_t = torch.from_numpy(obj)
    ns = {"torch": torch, "cfg": cfg, "scan_output": types.SimpleNamespace(F=torch.from_numpy(out.copy())),
          "scan_obj_labels": obj_t, "mask": obj_t == 1,                   # :310, in front of the executed lines
          "scan_scale_labels": torch.from_numpy(scale), "scan_xyz_labels": nested_torch(labels),
          "scan_points": torch.zeros((N_ROWS, 4), dtype=torch.int32), "xyz_weights": torch.tensor(WEIGHTS),
          "obj_criterion": torch.nn.CrossEntropyLoss(), "losses": {}}
    exec(ref_lines(322, 357, REF_SEP), ns)
    return {k: np.asarray(ns["losses"][k].numpy(), np.float32) for k in ("loss_obj", "loss_scale", "loss_xyz")}


if __name__ == "__main__":
    assert os.path.exists(REF_SEP), "run where /root/reference is mounted"
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self.clone()      # a host-to-device transfer is a copy
    try:
        r = run_reference()
        print({k: float(v) for k, v in r.items()})
        np.savez_compressed(os.path.join(HERE, "sep_val_loss_ref.npz"), **r)
    finally:
        torch.Tensor.cuda = orig_cuda
