"""The Python facade above the kernels (ME.conv_forward, the three eval forwards of MinkUNet, train.train_step in every
tested mode) against recorded bits: tests/golden/facade_parent_bits.json holds, for every case, the sha256 of raw bytes as
the facade produced them before its weight packing and its training-step state were folded into one path each.  An eval
case hashes the network output [N, 64]; a training case hashes, after each step, the loss followed by every p.grad in
named_parameters() order.  Every case was recorded twice, in two processes, and is pinned because both agreed.

That refactor moved no arithmetic, so the hashes are expected to be EQUAL: there is no tolerance.

The second test needs no recorded bits: the eval-time cache of packed weights may never hand out the packing of another
tensor, or of the same tensor before it was changed."""
import hashlib
import json
import os

import pytest
import torch

from canonicalvoting_amd import me as ME
from canonicalvoting_amd import train
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests.test_conv_paths_gpu import _manager
from tests.test_train_gpu import _small_batch

pytestmark = pytest.mark.gpu
BITS = os.path.join(os.path.dirname(__file__), "golden", "facade_parent_bits.json")
LOWERED = 512           # the smallest threshold that sends the two finest levels of the 4500-row scene to the mask-sorted route


@pytest.fixture(autouse=True)
def _clean_flag(cuda, built_lib):
    ME.range_flag(cuda).zero_()
    yield
    torch.cuda.synchronize()
    ME.range_flag(cuda).zero_()


def _hash(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _model(cuda):
    torch.manual_seed(0)
    return MinkUNet34C(3, 64).to(cuda)


def _eval(call, **attrs):
    def run(cuda, monkeypatch):
        coords, feats = _small_batch(cuda, seed0=50, n=1500)[:2]
        model = _model(cuda).eval()
        for k, v in attrs.items():
            setattr(model, k, v)
        with torch.no_grad():
            return _hash(call(model, ME.SparseTensor(feats, coords, device=cuda)).F)
    return run


def _train(steps=3, sgd_overflow=False, dtype=None, model_attrs=(), **knobs):
    def run(cuda, monkeypatch):
        batch = _small_batch(cuda, seed0=50, n=1500)
        for k, v in knobs.items():
            monkeypatch.setattr(ME, k, v)
        prev = ME.set_compute_dtype(dtype) if dtype else None
        try:
            model = _model(cuda).train()
            for k, v in model_attrs:
                setattr(model, k, v)
            if sgd_overflow:
                with torch.no_grad():
                    model.bn0.bn.weight.fill_(1e7)        # activations beyond the fp16 range: the step is redone on the triples
                opt = torch.optim.SGD(model.parameters(), lr=1e-6)
            else:
                opt = train.make_optimizer(model, lr=1e-3)
            out = []
            for _ in range(steps):
                loss, _ = train.train_step(model, opt, *batch)
                out.append(_hash(loss, *[p.grad for _, p in model.named_parameters()]))
            if sgd_overflow:
                assert model.train_range_fallbacks == 1
            return out
        finally:
            if prev is not None:
                ME.set_compute_dtype(prev)
    return run


CASES = {
    "eval_program_p1": _eval(lambda m, x: m.program_forward(x, pieces=1)),
    "eval_program_p2": _eval(lambda m, x: m.program_forward(x, pieces=2)),
    "eval_program_p3": _eval(lambda m, x: m.program_forward(x, pieces=3)),
    "eval_fused": _eval(lambda m, x: m.fused_forward(x)),
    "eval_program_p2_masked": _eval(lambda m, x: m.program_forward(x, pieces=2), MASKED_MIN_ROWS=LOWERED),
    "eval_program_p3_unfused_ds": _eval(lambda m, x: m.program_forward(x, pieces=3), FUSE_DOWNSAMPLE=False),
    "train_defaults": _train(),
    "train_bwd_hl_0": _train(TRAIN_BWD_HL=0),
    "train_prepack_0": _train(TRAIN_PREPACK=0),
    "train_fwd_hl_0": _train(TRAIN_FWD_HL=0),
    "train_bf16": _train(dtype="bf16"),
    "train_auto_mask": _train(AUTO_MASK_MIN_ROWS=LOWERED),
    "train_unsorted": _train(model_attrs=(("SORTED_TRAINING", False),)),
    "train_sgd_redo_on_triples": _train(steps=1, sgd_overflow=True),
}


def _recorded():
    with open(BITS) as f:
        return json.load(f)


def test_every_case_has_recorded_bits():
    assert set(_recorded()) == set(CASES)            # (every case reproduced between the two recording processes)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_recorded_bits(name, cuda, monkeypatch):
    assert CASES[name](cuda, monkeypatch) == _recorded()[name], name + ": not the bits the parent's facade produced"


@pytest.mark.parametrize("pieces", [2, 3])
def test_weight_cache_never_returns_a_stale_packing(pieces, cuda):
    """one 3x3x3 convolution, 300 rows, 32 -> 64 channels, through the cache of packed weights: the same weight, the weight
    changed in place, and a NEW tensor of the same shape in its place (the allocator may hand it the freed block, CPython the
    freed id) each give what the uncached call gives"""
    nbr = _manager(300, "mixed").kernel_map(3, 1)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(300, 32, generator=g).to(cuda)
    run = lambda w, cache: ME.conv_forward(x, w, nbr, 300, pieces=pieces, cache_weights=cache)
    w = (torch.randn(27, 32, 64, generator=g) * 0.1).to(cuda)
    assert torch.equal(run(w, True), run(w, False))
    assert torch.equal(run(w, True), run(w, False))               # (a hit)
    w.mul_(1.5)
    assert torch.equal(run(w, True), run(w, False))
    first = run(w, False)
    del w
    w = (torch.randn(27, 32, 64, generator=g) * 0.3).to(cuda)
    out = run(w, True)
    assert torch.equal(out, run(w, False)) and not torch.equal(out, first)
