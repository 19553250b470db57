"""The packed symmetry loss on the GPU: cv_sym_loss_fwd_f32 / cv_sym_loss_bwd_f32 per element against the fp64 oracle at the
derived bounds (tests/sym_loss_ref.py), their reproducibility, the autograd Function and train.separate_loss_packed against
torch and the golden values of the reference's lines, and train.train_step_separate over a SymBatch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data, train
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests import sym_loss_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_ref.npz")
SENTINEL = 123.0
GRAD_LOSS = 0.75


@pytest.fixture(scope="module")
def cases(built_lib):
    chunk = _lib.lib().cv_sym_loss_chunk_rows()
    named = ref.named_cases(chunk)
    golden, batch = ref.golden_cases()
    return {**named, **golden}, batch


@pytest.fixture(scope="module")
def oracles(cases):
    """the fp64 reference of every case, computed once and shared"""
    return {k: ref.oracle(out, sym, w, xf, grad_loss=GRAD_LOSS) for k, (out, sym, w, xf) in cases[0].items()}


def run_abi(dev, out, sym, w, xf, grad_loss=GRAD_LOSS):
    """forward and backward through the C ABI on torch's current stream, every output in a NaN / sentinel-filled buffer;
    returns the device tensors (loss, pose_loss, best, seg_loss, grad [N, ld] with the foreign columns at SENTINEL)"""
    L = _lib.lib()
    vp = ctypes.c_void_p
    o = torch.from_numpy(np.ascontiguousarray(out)).to(dev)
    s = data.sym_to_device(sym, dev)
    n, ld = o.shape
    assert sym.max_row < n                                                  # the precondition the kernels rely on
    S, J = sym.n_segments, sym.n_jobs
    loss = torch.full((1,), float("nan"), device=dev)
    pose_loss = torch.full((J + 1,), float("nan"), device=dev)
    seg_loss = torch.full((S + 1,), float("nan"), device=dev)
    best = torch.full((S + 1,), -7, dtype=torch.int32, device=dev)
    grad = torch.full((n, ld), SENTINEL, device=dev)
    grad[:, :3] = 0.0
    gl = torch.tensor([grad_loss], dtype=torch.float32, device=dev)
    need = int(L.cv_sym_loss_workspace_bytes(sym.targets.shape[0], J))
    ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    p = lambda t: vp(t.data_ptr()) if t.numel() else None
    d = _lib.SymLossDesc()
    d.d_out, d.n_rows, d.ld = p(o), n, ld
    d.d_rows, d.d_pseg, d.n_points = p(s.rows), p(s.pseg), s.rows.shape[0]
    d.d_seg_ptr, d.d_pose_ptr, d.d_tgt_ptr, d.n_segments, d.n_jobs = p(s.seg_ptr), p(s.pose_ptr), p(s.tgt_ptr), S, J
    d.d_targets, d.n_targets = p(s.targets), s.targets.shape[0]
    d.d_urow, d.d_uptr, d.d_upoint, d.n_urows = p(s.urow), p(s.uptr), p(s.upoint), s.urow.shape[0]
    d.w = (ctypes.c_float * 3)(*w)
    d.xyz_factor = xf
    d.d_loss, d.d_pose_loss, d.d_best, d.d_seg_loss = p(loss), p(pose_loss), p(best), p(seg_loss)
    d.d_grad_loss, d.d_grad, d.grad_ld = p(gl), p(grad), ld
    d.d_ws, d.ws_bytes = p(ws), need
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.cv_sym_loss_fwd_f32(ctypes.byref(d), stream), "cv_sym_loss_fwd_f32")
    _lib.check(L.cv_sym_loss_bwd_f32(ctypes.byref(d), stream), "cv_sym_loss_bwd_f32")
    torch.cuda.current_stream(dev).synchronize()
    return {"loss": loss, "pose_loss": pose_loss, "best": best, "seg_loss": seg_loss, "grad": grad, "keep": (o, s, gl, ws)}


def to_host(r, sym):
    """the outputs without their guard elements, which must still hold their sentinels"""
    S, J = sym.n_segments, sym.n_jobs
    assert np.isnan(float(r["pose_loss"][J])) and np.isnan(float(r["seg_loss"][S])) and int(r["best"][S]) == -7
    g = r["grad"].cpu().numpy()
    assert (g[:, 3:] == SENTINEL).all()                                     # the foreign columns are left alone
    return {"loss": float(r["loss"][0]), "pose_loss": r["pose_loss"][:J].cpu().numpy(), "best": r["best"][:S].cpu().numpy(),
            "seg_loss": r["seg_loss"][:S].cpu().numpy(), "grad": g[:, :3]}


CASE_NAMES = ["lengths_0", "lengths_1", "lengths_2", "lengths_3", "one_segment_1", "one_segment_4", "one_segment_36",
              "segments_300", "shared_rows", "two_scans_reference", "two_scans_offset", "golden_reference", "golden_offset"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_c_abi_matches_the_fp64_oracle_per_element(cuda, built_lib, cases, oracles, name):
    """segment lengths 1 / 63 / 64 / 65 / 255 / 256 / 257 / CHUNK-1 / CHUNK / CHUNK+1 / 2 CHUNK+1 with 1 / 2 / 4 / 36 poses and the
    best pose first and last, S = 1 and S = 300, ld = 8 and 11, both weight sets, rows shared by two and three segments,
    colliding rows under the reference's indexing, the mini batch: pose losses, segment losses, loss and every gradient
    element inside their bounds, best exact, unlabelled rows exactly zero, foreign columns untouched."""
    out, sym, w, xf = cases[0][name]
    assert sorted(cases[0]) == sorted(CASE_NAMES)
    assert ref.decidable(oracles[name]) > 1.0
    got = to_host(run_abi(cuda, out, sym, w, xf), sym)
    ref.assert_within(got, oracles[name], name)
    assert not got["grad"][oracles[name]["grad_m"] == 0].any()


def test_nan_predictions_and_no_segments(cuda, built_lib, cases):
    out, sym, w, xf = cases[0]["shared_rows"]
    plain = run_abi(cuda, out, sym, w, xf)
    labelled = np.zeros(out.shape[0], bool)
    labelled[sym.urow.numpy()] = True
    free = int(np.nonzero(~labelled)[0][0])
    poisoned = out.copy()
    poisoned[free, :3] = np.nan
    again = run_abi(cuda, poisoned, sym, w, xf)
    for k in ("loss", "pose_loss", "best", "seg_loss", "grad"):             # an unlabelled row is never read
        assert torch.equal(plain[k].view(torch.int32), again[k].view(torch.int32)), k
    poisoned = out.copy()
    row = int(sym.rows[int(sym.seg_ptr[3])])                                # a row of segment 3 (one pose), which segment 4 shares
    poisoned[row, 1] = np.nan
    bad = run_abi(cuda, poisoned, sym, w, xf)
    assert np.isnan(float(bad["loss"][0])) and np.isnan(float(bad["seg_loss"][3]))          # as torch.min / mean give
    assert np.isfinite(bad["seg_loss"][:3].cpu().numpy()).all()
    t = torch.from_numpy(poisoned)
    want, _ = train.separate_loss(torch.cat([t[:, :3], torch.zeros(len(t), 5)], 1), [[[r, x] for r, x in data.unpack_sym(sym)]],
                                  torch.ones(len(t), 3), torch.ones(len(t), dtype=torch.long))
    assert np.isnan(float(want))
    empty = data.pack_sym([[]], [out.shape[0]])
    r = run_abi(cuda, out, empty, w, xf)
    assert float(r["loss"][0]) == 0.0 and not r["grad"][:, :3].any()


def test_outputs_are_the_same_bytes_on_every_run_and_stream(cuda, built_lib, cases):
    for name in ("segments_300", "golden_reference", "lengths_1"):
        out, sym, w, xf = cases[0][name]
        first = run_abi(cuda, out, sym, w, xf)
        second = run_abi(cuda, out, sym, w, xf)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(side):
            third = run_abi(cuda, out, sym, w, xf)
        torch.cuda.synchronize()
        for other in (second, third):
            for k in ("loss", "pose_loss", "best", "seg_loss", "grad"):
                assert torch.equal(first[k].view(torch.int32), other[k].view(torch.int32)), (name, k)


def _torch_reference(cuda, F, batch, **kw):
    out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
    loss, parts = train.separate_loss(out, batch[3], batch[4].to(cuda), batch[5].to(cuda), coords4=batch[1].to(cuda), **kw)
    loss.backward()
    return loss, parts, out.grad


def test_function_and_packed_loss_match_torch_and_the_golden(cuda, built_lib, cases):
    """ME.utils.sym_loss and train.separate_loss_packed against train.separate_loss (list form, torch on the GPU) and the golden
    values of train_separate.py:247-286 on the mini batch, at the golden test's tolerances; the gradient is [N, C], zero
    outside columns 0..2 of labelled rows for the coordinate term."""
    z = np.load(GOLDEN)
    (F, sym, w, xf), batch = cases[0]["golden_reference"], cases[1]
    sym_d = data.sym_to_device(sym, cuda)
    out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
    loss_xyz, pose_loss, best = ME.utils.sym_loss(out, sym_d, return_poses=True)
    assert loss_xyz.shape == () and pose_loss.shape == (sym.n_jobs,) and best.shape == (sym.n_segments,)
    (loss_xyz * 1.0).backward()
    g = out.grad.cpu().numpy()
    assert g.shape == F.shape and not g[:, 3:].any()
    labelled = np.zeros(len(F), bool)
    labelled[sym.urow.numpy()] = True
    assert not g[~labelled].any() and g[labelled].any()
    assert abs(float(loss_xyz.detach()) - float(z["sep_loss_xyz"])) < 1e-6 * max(1.0, abs(float(z["sep_loss_xyz"])))
    np.testing.assert_allclose(g[:, :3], z["sep_grad"][:, :3], rtol=1e-5, atol=1e-8)
    t_loss, t_parts, t_grad = _torch_reference(cuda, F, batch)
    out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
    loss, parts = train.separate_loss_packed(out, sym_d, batch[4].to(cuda), batch[5].to(cuda))
    loss.backward()
    assert sorted(parts) == sorted(t_parts) == ["loss_obj", "loss_scale", "loss_xyz"]
    for k in parts:
        assert abs(float(parts[k].detach()) - float(t_parts[k].detach())) < 1e-6 * max(1.0, abs(float(t_parts[k].detach()))), k
        assert abs(float(parts[k].detach()) - float(z["sep_" + k])) < 1e-6 * max(1.0, abs(float(z["sep_" + k]))), k
    assert abs(float(loss.detach()) - float(z["sep_loss"])) < 1e-6
    np.testing.assert_allclose(out.grad.cpu().numpy(), z["sep_grad"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(out.grad.cpu().numpy(), t_grad.cpu().numpy(), rtol=1e-5, atol=1e-8)
    # the repaired indexing, weights and factors
    F2, sym2, w2, _ = cases[0]["golden_offset"]
    kw = dict(xyz_component_weights=w2, xyz_factor=0.5, scale_factor=2.0)
    t_loss, t_parts, t_grad = _torch_reference(cuda, F2, batch, reference_indexing=False, **kw)
    out = torch.from_numpy(F2.copy()).to(cuda).requires_grad_(True)
    loss, parts = train.separate_loss_packed(out, data.sym_to_device(sym2, cuda), batch[4].to(cuda), batch[5].to(cuda), **kw)
    loss.backward()
    for k in parts:
        assert abs(float(parts[k].detach()) - float(t_parts[k].detach())) < 1e-6 * max(1.0, abs(float(t_parts[k].detach()))), k
    np.testing.assert_allclose(out.grad.cpu().numpy(), t_grad.cpu().numpy(), rtol=1e-5, atol=1e-8)
    with pytest.raises(ValueError, match="outside"):
        train.separate_loss_packed(out[:sym2.max_row], data.sym_to_device(sym2, cuda), batch[4].to(cuda), batch[5].to(cuda))


def test_non_finite_background_scale_predictions_reach_nothing(cuda, built_lib, cases):
    (F, sym, w, xf), batch = cases[0]["golden_reference"], cases[1]
    sym_d, scale, obj = data.sym_to_device(sym, cuda), batch[4].to(cuda), batch[5].to(cuda)
    res = []
    for poison in (False, True):
        Fp = F.copy()
        if poison:
            bg = np.nonzero(batch[5].numpy() == 0)[0]
            Fp[bg[0], 3:6] = np.inf
            Fp[bg[1], 3:6] = np.nan
            Fp[bg[2], 4] = -np.inf
        out = torch.from_numpy(Fp).to(cuda).requires_grad_(True)
        loss, parts = train.separate_loss_packed(out, sym_d, scale, obj)
        loss.backward()
        res.append((loss.detach(), out.grad))
    (l0, g0), (l1, g1) = res
    assert bool(torch.isfinite(l1)) and bool(torch.isfinite(g1).all())
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def _mini_step_inputs(cuda, batch, sym):
    return (batch[1].to(cuda), batch[2].to(cuda) * 2 - 1, data.sym_to_device(sym, cuda), batch[4].to(cuda), batch[5].to(cuda))


def test_train_step_separate_over_a_sym_batch(cuda, built_lib, cases, monkeypatch):
    """the packed step runs through train_step's core: the loss falls, the weights come from the batched pack and the input
    gradients run on the fp16 pairs from the second step on (neither exists for the list form), two fresh models from one seed
    end with the same parameter bytes, and a batch without segments is skipped without a host wait."""
    monkeypatch.setattr(ME, "TRAIN_FWD_HL", 1)
    monkeypatch.setattr(ME, "TRAIN_BWD_HL", 1)
    monkeypatch.setattr(ME, "TRAIN_PREPACK", 1)
    (F, sym, w, xf), batch = cases[0]["golden_reference"], cases[1]
    args = _mini_step_inputs(cuda, batch, sym)
    finals = []
    for rep in range(2):
        torch.manual_seed(1)
        model = MinkUNet34C(3, 8).cuda().train()
        opt = train.make_optimizer(model, lr=1e-3)
        ME.TRAIN_COUNTERS["prepacked"] = ME.TRAIN_COUNTERS["hl_dgrad"] = 0
        hist = []
        for step in range(6 if rep == 0 else 3):
            loss, parts = train.train_step_separate(model, opt, *args)
            hist.append(float(loss))
            if step == 1:
                assert ME.TRAIN_COUNTERS["prepacked"] > 100 and ME.TRAIN_COUNTERS["hl_dgrad"] > 0, ME.TRAIN_COUNTERS
            if step == 2:
                finals.append([p.detach().clone() for p in model.parameters()])
        assert sorted(parts) == ["loss_obj", "loss_scale", "loss_xyz"]
        if rep == 0:
            print("packed separate step, loss over 6 steps:", hist)
            assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*finals))
    assert getattr(model, "train_range_fallbacks", 0) == 0
    # the host copy of the labels is accepted too, and gives the same first step
    torch.manual_seed(1)
    other = MinkUNet34C(3, 8).cuda().train()
    first = train.train_step_separate(other, train.make_optimizer(other, lr=1e-3), args[0], args[1], sym, batch[4], batch[5])
    torch.manual_seed(1)
    again = MinkUNet34C(3, 8).cuda().train()
    want = train.train_step_separate(again, train.make_optimizer(again, lr=1e-3), *args)
    assert torch.equal(first[0], want[0])
    empty = data.pack_sym([[], []], [10, 10])
    assert train.train_step_separate(model, opt, args[0], args[1], empty, args[3], torch.zeros_like(args[4])) is None


def test_separate_step_beyond_the_fp16_range_skips_its_update_on_the_device(cuda, built_lib, cases, monkeypatch):
    """test_a_forward_beyond_the_fp16_range_skips_its_update_on_the_device (tests/test_train_gpu.py) for the separate step: a
    BatchNorm gain of 1e7 raises the range flag; the fused Adam leaves the parameters alone for FLAG_LAG calls, then the step
    notices, restores the BatchNorm statistics, counts ONE fallback and goes through on the bf16 triples."""
    monkeypatch.setattr(ME, "TRAIN_FWD_HL", 1)
    (F, sym, w, xf), batch = cases[0]["golden_reference"], cases[1]
    args = _mini_step_inputs(cuda, batch, sym)
    torch.manual_seed(0)
    model = MinkUNet34C(3, 8).cuda().train()
    opt = train.make_optimizer(model, lr=1e-3)
    train.train_step_separate(model, opt, *args)                        # healthy
    assert getattr(model, "train_range_fallbacks", 0) == 0
    with torch.no_grad():
        model.bn0.bn.weight.fill_(1e7)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    torch.cuda.synchronize()
    stats_before = {k: b.detach().clone() for k, b in model.named_buffers()}
    nbt = int(model.bn0.bn.num_batches_tracked)
    for _ in range(train.FLAG_LAG):
        train.train_step_separate(model, opt, *args)
        torch.cuda.synchronize()
        assert all(torch.equal(before[k], p.detach()) for k, p in model.named_parameters())   # skipped on the device
        assert getattr(model, "train_range_fallbacks", 0) == 0
    bufs, saved = train._bn_state(model)
    names = [k for k, _ in model.named_buffers()]
    assert len(names) == len(saved) and all(torch.equal(stats_before[k], s) for k, s in zip(names, saved))
    loss, _ = train.train_step_separate(model, opt, *args)
    torch.cuda.synchronize()
    assert model.train_range_fallbacks == 1 and np.isfinite(float(loss))
    assert any(not torch.equal(before[k], p.detach()) for k, p in model.named_parameters())   # the triples step went through
    assert all(int(m.bn.num_batches_tracked) == nbt + 1 for m in model.modules() if isinstance(m, ME.MinkowskiBatchNorm))
    assert all(bool(torch.isfinite(b).all()) for b in model.buffers())
    assert int(ME.range_flag(torch.device(cuda))[0]) == 0
    loss, _ = train.train_step_separate(model, opt, *args)
    assert model.train_range_fallbacks == 1 and np.isfinite(float(loss)) and int(model.bn0.bn.num_batches_tracked) == nbt + 2
