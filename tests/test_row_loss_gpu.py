"""The per-row losses on the GPU: cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32 through the C ABI, every loss and every gradient
element against the fp64 oracle at the derived bounds (tests/row_loss_ref.py) on sentinel-filled buffers, their
reproducibility, train.joint_loss_device / separate_loss_packed(device_rows=True) against the torch-op losses and the golden
values of the reference's lines, and the two training steps with device_loss."""
import ctypes
import os

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data, train
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests import row_loss_ref as ref
from tests import sym_loss_ref
from tests.golden import make_val_loss_golden as val_golden
from tests.golden.make_loss_golden import make_inputs

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 123.0
W, XF, SF, GL = (0.5, 2.0, 1.0), 0.7, 1.3, 0.37
PAD_ROWS = 3


def _cfg(layout="joint", **kw):
    return ref.config(layout, **dict(dict(w=W, xyz_factor=XF, scale_factor=SF, grad_loss=GL), **kw))


def _case_table(chunk):
    """name -> (make_case arguments, config, grad_ld, n_cols)"""
    big = chunk * 256 + 1                       # more partials than the finish workgroup has lanes
    t = {}
    for i, n in enumerate((1, 255, 256, 257)):
        ld = (64, 72)[i % 2]
        t["joint_%d" % n] = (dict(seed=n, n=n, layout="joint", ld=ld, poison=True), _cfg(), ld + 4, ld)
        ld = (8, 11)[i % 2]
        t["separate_%d" % n] = (dict(seed=n, n=n, layout="separate", ld=ld, poison=True), _cfg("separate"), ld + 1, ld)
    t["joint_big"] = (dict(seed=3, n=big, layout="joint", ld=64), _cfg(), 68, 64)
    t["separate_big"] = (dict(seed=4, n=big, layout="separate", ld=8), _cfg("separate"), 12, 8)
    t["joint_odd_strides"] = (dict(seed=5, n=600, layout="joint", ld=67, poison=True), _cfg(), 65, 65)
    t["joint_cols_inside"] = (dict(seed=6, n=600, layout="joint", ld=72), _cfg(), 72, 66)
    t["joint_plain_scale"] = (dict(seed=7, n=600, layout="joint", ld=72), _cfg(log_scale=False), 64, 64)
    t["separate_plain_scale"] = (dict(seed=8, n=600, layout="separate", ld=8), _cfg("separate", log_scale=False), 8, 8)
    t["joint_background_zero"] = (dict(seed=9, n=600, layout="joint", labels="background", poison=True), _cfg(), 64, 64)
    t["joint_background_nan"] = (dict(seed=9, n=600, layout="joint", labels="background", poison=True), _cfg(empty="nan"), 64, 64)
    t["separate_background_zero"] = (dict(seed=10, n=600, layout="separate", labels="background"), _cfg("separate"), 8, 8)
    t["separate_background_nan"] = (dict(seed=10, n=600, layout="separate", labels="background"), _cfg("separate", empty="nan"), 8, 8)
    t["joint_objects"] = (dict(seed=11, n=600, layout="joint", labels="objects"), _cfg(empty="nan"), 64, 64)
    t["separate_objects"] = (dict(seed=12, n=600, layout="separate", labels="objects"), _cfg("separate"), 8, 8)
    t["joint_pm90"] = (dict(seed=13, n=600, layout="joint", logits="pm90", poison=True), _cfg(), 64, 64)
    t["separate_pm90"] = (dict(seed=14, n=600, layout="separate", logits="pm90"), _cfg("separate"), 8, 8)
    t["joint_label_10"] = (dict(seed=15, n=600, layout="joint", bad_label=True), _cfg(), 64, 64)
    t["val_mixed"] = (dict(seed=16, n=600, layout="joint", ld=72, poison=True), _cfg(gather="argmax", empty="nan"), 72, 72)
    t["val_background"] = (dict(seed=17, n=600, layout="joint", labels="background"), _cfg(gather="argmax", empty="nan"), 64, 64)
    return t


CASE_NAMES = ["joint_1", "separate_1", "joint_255", "separate_255", "joint_256", "separate_256", "joint_257", "separate_257",
              "joint_big", "separate_big", "joint_odd_strides", "joint_cols_inside", "joint_plain_scale", "separate_plain_scale",
              "joint_background_zero", "joint_background_nan", "separate_background_zero", "separate_background_nan",
              "joint_objects", "separate_objects", "joint_pm90", "separate_pm90", "joint_label_10", "val_mixed", "val_background"]


@pytest.fixture(scope="module")
def table(built_lib):
    return _case_table(_lib.lib().cv_row_loss_chunk_rows())


@pytest.fixture(scope="module")
def oracles():
    """name -> (inputs, fp64 reference), computed once per case and shared"""
    return {}


def _case(table, oracles, name):
    if name not in oracles:
        args, c, grad_ld, n_cols = table[name]
        arrays = ref.make_case(**args)
        oracles[name] = (arrays, ref.oracle(*arrays, c))
    return oracles[name] + table[name][1:]


def run_abi(dev, arrays, c, grad_ld, n_cols, backward=True):
    """forward and backward through the C ABI on torch's current stream, every output in a NaN / sentinel-filled buffer with
    guard elements, PAD_ROWS guard rows behind the gradient; returns the device tensors"""
    L = _lib.lib()
    vp = ctypes.c_void_p
    out, y, xyz, scale = arrays
    n, ld = out.shape
    o = torch.from_numpy(np.ascontiguousarray(out)).to(dev)
    lab, xl, sl = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (y, xyz, scale))
    losses = torch.full((5,), float("nan"), device=dev)
    losses[4] = SENTINEL
    info = torch.full((3,), -7, dtype=torch.int32, device=dev)
    grad = torch.full((n + PAD_ROWS, grad_ld), SENTINEL, device=dev)
    gl = torch.tensor([c["grad_loss"]], dtype=torch.float32, device=dev)
    need = int(L.cv_row_loss_workspace_bytes(n))
    ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)
    p = lambda t: vp(t.data_ptr()) if t.numel() else None
    d = _lib.RowLossDesc()
    d.d_out, d.n_rows, d.ld = p(o), n, ld
    d.d_labels, d.d_xyz_labels, d.d_scale_labels = p(lab), p(xl) if c["with_xyz"] else None, p(sl)
    for k in ("heads", "n_logits", "xyz_col", "scale_col", "logit_col", "obj_lo", "obj_hi", "with_xyz"):
        setattr(d, k, c[k])
    d.log_scale, d.gather, d.empty = int(c["log_scale"]), _lib.ROW_LOSS_GATHER[c["gather"]], _lib.ROW_LOSS_EMPTY[c["empty"]]
    d.w = (ctypes.c_float * 3)(*c["w"])
    d.xyz_factor, d.scale_factor = c["xyz_factor"], c["scale_factor"]
    d.d_losses, d.d_info = p(losses), p(info)
    d.d_grad_loss, d.d_grad, d.grad_ld, d.n_cols = p(gl), p(grad), grad_ld, n_cols
    d.d_ws, d.ws_bytes = p(ws), need
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.cv_row_loss_fwd_f32(ctypes.byref(d), stream), "cv_row_loss_fwd_f32")
    if backward and c["gather"] == "label":
        _lib.check(L.cv_row_loss_bwd_f32(ctypes.byref(d), stream), "cv_row_loss_bwd_f32")
    elif backward:
        assert L.cv_row_loss_bwd_f32(ctypes.byref(d), stream) == -22              # no backward of the validation form
    torch.cuda.current_stream(dev).synchronize()
    return {"losses": losses, "info": info, "grad": grad, "keep": (o, lab, xl, sl, gl, ws)}


def to_host(r, n, n_cols, wrote_grad=True):
    """the outputs without their guards, which must still hold their sentinels"""
    assert float(r["losses"][4]) == SENTINEL and int(r["info"][2]) == -7
    g = r["grad"].cpu().numpy()
    assert (g[n:] == SENTINEL).all() and (g[:, n_cols:] == SENTINEL).all()    # rows beyond n_rows, columns beyond n_cols
    if not wrote_grad:
        assert (g == SENTINEL).all()
    return r["losses"][:4].cpu().numpy(), r["info"][:2].cpu().numpy(), g[:n, :n_cols]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_c_abi_matches_the_fp64_oracle_per_element(cuda, built_lib, table, oracles, name):
    """n_rows 1 / 255 / 256 / 257 / CHUNK * 256 + 1, both layouts, ld 64 / 72 / 67 and 8 / 11 with another gradient stride and
    gradient columns that end inside the row, log scale on and off, w = (0.5, 2, 1), factors 0.7 and 1.3, grad_loss 0.37, labels
    all background (both empty modes), all objects, mixed with -1 and 9, NaN and Inf planted in background rows, logits +-90,
    one label of 10, the validation form: every loss and every gradient element inside its bound, exact zeros exact, guards
    untouched."""
    assert sorted(table) == sorted(CASE_NAMES)
    arrays, r, c, grad_ld, n_cols = _case(table, oracles, name)
    n = arrays[0].shape[0]
    losses, info, grad = to_host(run_abi(cuda, arrays, c, grad_ld, n_cols), n, n_cols, wrote_grad=c["gather"] == "label")
    assert int(info[0]) == r["cnt"] and int(info[1]) == r["n_bad"]
    want_grad = c["gather"] == "label"
    ref.assert_within(losses, grad if want_grad else None, {**r, "grad": r["grad"][:, :n_cols], "grad_bounds": r["grad_bounds"][:, :n_cols],
                                                            "grad_zero": r["grad_zero"][:, :n_cols]}, name)
    if "background" in name:
        assert r["cnt"] == 0
        if c["empty"] == "nan":
            assert np.isnan(losses[[0, 1, 3]]).all() and np.isfinite(losses[2])
        else:
            assert losses[0] == 0.0 and losses[1] == 0.0 and np.isfinite(losses).all()
    if name == "joint_label_10":
        assert np.isnan(losses[2]) and np.isnan(losses[3]) and int(info[1]) == 1 and np.isfinite(losses[:2]).all()
    elif "background_nan" not in name and name != "val_background":
        assert np.isfinite(losses).all()                                    # planted NaN / Inf reached no loss ...
        if want_grad:
            assert np.isfinite(grad).all()                                  # ... and no gradient (their entries are exact 0 above)
    if table[name][0].get("poison"):
        out, y = arrays[0], arrays[1]
        bg = ~((y >= c["obj_lo"]) & (y <= c["obj_hi"]))
        assert (bg.any() or n == 1) and not np.isfinite(out[bg][:, :c["logit_col"]]).any()
        if want_grad:
            assert not grad[bg][:, :c["logit_col"]].any()


def test_no_rows(cuda, built_lib):
    for empty, check in (("zero", lambda v: (v == 0).all()), ("nan", lambda v: np.isnan(v).all())):
        c = _cfg(empty=empty)
        arrays = ref.make_case(1, 0, "joint")
        losses, info, grad = to_host(run_abi(cuda, arrays, c, 64, 64), 0, 64)
        assert check(losses) and (info == 0).all()


def test_outputs_are_the_same_bytes_on_every_run_and_stream(cuda, built_lib, table, oracles):
    for name in ("joint_big", "separate_257", "joint_odd_strides"):
        arrays, r, c, grad_ld, n_cols = _case(table, oracles, name)
        first = run_abi(cuda, arrays, c, grad_ld, n_cols)
        second = run_abi(cuda, arrays, c, grad_ld, n_cols)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(side):
            third = run_abi(cuda, arrays, c, grad_ld, n_cols)
        torch.cuda.synchronize()
        for other in (second, third):
            for k in ("losses", "info", "grad"):
                assert torch.equal(first[k].view(torch.int32), other[k].view(torch.int32)), (name, k)


def _dev(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def test_joint_loss_device_against_torch_and_the_goldens(cuda, built_lib):
    """3 x 20 000 rows: |joint_loss_device - joint_loss| is at most the device bound plus torch's own distance from the fp64
    oracle, measured here, per loss and per gradient element - no fixed tolerance.  Then the golden values of the reference's
    lines, training and validation form, at the oracle's bounds around the oracle (which the CPU test ties to the goldens)."""
    arrays = ref.make_case(31, 60000, "joint")
    c = _cfg()
    r = ref.oracle(*arrays, c)
    F, y, xyz, scale = _dev(arrays, cuda)
    kw = dict(xyz_factor=XF, scale_factor=SF, xyz_component_weights=W)
    res = {}
    for name, fn in (("torch", train.joint_loss), ("device", train.joint_loss_device)):
        out = F.clone().requires_grad_(True)
        total, parts = fn(out, xyz, scale, y, **kw)
        assert sorted(parts) == ["loss_class", "loss_scale", "loss_xyz"]
        (total * GL).backward()
        res[name] = (np.array([float(parts["loss_xyz"]), float(parts["loss_scale"]), float(parts["loss_class"]), float(total.detach())]),
                     out.grad.cpu().numpy())
    (tl, tg), (dl, dg) = res["torch"], res["device"]
    torch_off, torch_off_g = np.abs(tl - r["losses"]), np.abs(tg - r["grad"])
    print("torch's distance from the oracle / device bound: losses %s, gradient max %.2f"
          % (np.round(torch_off / r["loss_bounds"], 2), float((torch_off_g / np.maximum(r["grad_bounds"], 1e-300))[~r["grad_zero"]].max())))
    assert (np.abs(dl - tl) <= r["loss_bounds"] + torch_off).all()
    assert (np.abs(dg - tg) <= r["grad_bounds"] + torch_off_g).all()
    ref.assert_within(dl, dg, r, "3 x 20 000 rows")
    # goldens: the training form ...
    z = np.load(os.path.join(GOLDEN_DIR, "loss_ref.npz"))
    arrays = make_inputs()
    F, y, xyz, scale = _dev(arrays, cuda)
    out = F.clone().requires_grad_(True)
    total, parts = train.joint_loss_device(out, xyz, scale, y)
    total.backward()
    rg = ref.oracle(*arrays, ref.config("joint"))
    got = np.array([float(parts["loss_xyz"]), float(parts["loss_scale"]), float(parts["loss_class"]), float(total.detach())])
    ref.assert_within(got, out.grad.cpu().numpy(), rg, "golden training form")
    for k, key in enumerate(("loss_xyz", "loss_scale", "loss_class", "loss")):
        assert abs(got[k] - float(z[key])) < 1e-6 * max(1.0, abs(float(z[key]))), key
    np.testing.assert_allclose(out.grad.cpu().numpy(), z["grad"], rtol=1e-5, atol=1e-8)
    # ... and the validation form, with and without object rows
    zv = np.load(os.path.join(GOLDEN_DIR, "val_loss_ref.npz"))
    kwv = dict(xyz_factor=val_golden.XYZ_FACTOR, scale_factor=val_golden.SCALE_FACTOR, xyz_component_weights=val_golden.WEIGHTS)
    for case in ("mixed", "background"):
        F, y, xyz, scale = _dev(val_golden.make_inputs(case), cuda)
        total, parts = train.joint_loss_val(F.requires_grad_(True), xyz, scale, y, **kwv)
        assert not total.requires_grad
        for key in ("loss_xyz", "loss_scale", "loss_class"):
            want, have = float(zv["%s_%s" % (case, key)]), float(parts[key])
            assert (np.isnan(want) and np.isnan(have)) or abs(have - want) < 1e-6 * max(1.0, abs(want)), (case, key)
        assert np.isnan(float(total)) == (case == "background")


@pytest.fixture(scope="module")
def mini(built_lib):
    cases, batch = sym_loss_ref.golden_cases()
    return cases["golden_reference"], batch


def test_separate_loss_packed_device_rows_against_torch(cuda, built_lib, mini):
    """the same comparison for the per-category loss: the row terms from row_loss.hip against the torch ops, each within the
    device bound plus torch's own distance from the oracle; the coordinate term is sym_loss's in both, so columns 0..2 of the
    two gradients are the same bytes"""
    (F, sym, _, _), batch = mini
    sym_d, scale, obj = data.sym_to_device(sym, cuda), batch[4].to(cuda), batch[5].to(cuda)
    c = _cfg("separate")
    r = ref.oracle(F, batch[5].numpy(), None, batch[4].numpy(), c)
    kw = dict(xyz_factor=XF, scale_factor=SF, xyz_component_weights=W)
    res = {}
    for device_rows in (False, True):
        out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
        total, parts = train.separate_loss_packed(out, sym_d, scale, obj, device_rows=device_rows, **kw)
        assert sorted(parts) == ["loss_obj", "loss_scale", "loss_xyz"]
        (total * GL).backward()
        res[device_rows] = (np.array([float(parts["loss_scale"].detach()), float(parts["loss_obj"].detach())]),
                            float(parts["loss_xyz"].detach()), float(total.detach()),
                            out.grad.cpu().numpy())
    (tl, txyz, ttot, tg), (dl, dxyz, dtot, dg) = res[False], res[True]
    assert txyz == dxyz and np.array_equal(tg[:, :3], dg[:, :3])
    torch_off = np.abs(tl - r["losses"][1:3])
    assert (np.abs(dl - tl) <= r["loss_bounds"][1:3] + torch_off).all()
    assert (np.abs(dl - r["losses"][1:3]) <= r["loss_bounds"][1:3]).all()
    torch_off_g = np.abs(tg[:, 3:] - r["grad"][:, 3:])
    assert (np.abs(dg[:, 3:] - tg[:, 3:]) <= r["grad_bounds"][:, 3:] + torch_off_g).all()
    assert (np.abs(dg[:, 3:] - r["grad"][:, 3:]) <= r["grad_bounds"][:, 3:]).all()
    # the total: the rows' fp32 total plus the coordinate term, one more rounding
    want = r["losses"][3] + dxyz
    assert abs(dtot - want) <= r["loss_bounds"][3] + 2 * ref.U * abs(want) + abs(ttot - want)
    z = np.load(os.path.join(GOLDEN_DIR, "loss_ref.npz"))
    out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
    total, parts = train.separate_loss_packed(out, sym_d, scale, obj, device_rows=True)
    total.backward()
    for k in parts:
        assert abs(float(parts[k].detach()) - float(z["sep_" + k])) < 1e-6 * max(1.0, abs(float(z["sep_" + k]))), k
    assert abs(float(total.detach()) - float(z["sep_loss"])) < 1e-6
    np.testing.assert_allclose(out.grad.cpu().numpy(), z["sep_grad"], rtol=1e-5, atol=1e-8)


def _no_host_wait(fn):
    """fn() under torch's synchronisation guard: a host wait inside raises"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _small_batch(cuda, seed0=30, n=900):
    from canonicalvoting_amd.synth import make_scene
    scenes = [make_scene(seed0 + b, n_points=n, res=0.06, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4) for b in range(3)]
    coords = torch.cat([torch.cat([torch.full((n, 1), b, dtype=torch.int32), torch.from_numpy(s.coords)], 1)
                        for b, s in enumerate(scenes)]).to(cuda)
    feats = torch.cat([torch.from_numpy(s.feats) for s in scenes]).to(cuda) * 2 - 1
    xyz = torch.cat([torch.from_numpy(s.xyz_labels) for s in scenes]).to(cuda)
    scale = torch.cat([torch.from_numpy(s.scale_labels) for s in scenes]).to(cuda)
    cls = torch.cat([torch.from_numpy(s.class_labels) for s in scenes]).to(cuda)
    return coords, feats, xyz, scale, cls


def test_train_step_with_the_device_loss(cuda, built_lib):
    coords, feats, xyz, scale, cls = _small_batch(cuda)
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).cuda().train()
    opt = train.make_optimizer(model, lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    hist = []
    for _ in range(2):
        loss, parts = train.train_step(model, opt, coords, feats, xyz, scale, cls, device_loss=True)
        hist.append(float(loss))
    assert sorted(parts) == ["loss_class", "loss_scale", "loss_xyz"]
    assert np.isfinite(hist).all(), hist
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    # the first step's loss is the torch-op step's, to the two losses' distance
    torch.manual_seed(0)
    other = MinkUNet34C(3, 64).cuda().train()
    want = float(train.train_step(other, train.make_optimizer(other, lr=1e-3), coords, feats, xyz, scale, cls)[0])
    assert abs(hist[0] - want) <= 1e-5 * abs(want)
    # no host wait in the loss, forward or backward
    out = torch.randn(len(cls), 64, device=cuda, requires_grad=True)
    cls64 = cls.long()

    def loss_and_backward():
        total, _ = train.joint_loss_device(out, xyz, scale, cls64)
        total.backward()
        return total

    assert bool(torch.isfinite(_no_host_wait(loss_and_backward))) and bool(torch.isfinite(out.grad).all())


def test_train_step_separate_with_the_device_loss(cuda, built_lib, mini):
    (F, sym, _, _), batch = mini
    args = (batch[1].to(cuda), batch[2].to(cuda) * 2 - 1, data.sym_to_device(sym, cuda), batch[4].to(cuda), batch[5].to(cuda))
    torch.manual_seed(1)
    model = MinkUNet34C(3, 8).cuda().train()
    opt = train.make_optimizer(model, lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    hist = []
    for _ in range(2):
        loss, parts = train.train_step_separate(model, opt, *args, device_loss=True)
        hist.append(float(loss))
    assert sorted(parts) == ["loss_obj", "loss_scale", "loss_xyz"]
    assert np.isfinite(hist).all(), hist
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    torch.manual_seed(1)
    other = MinkUNet34C(3, 8).cuda().train()
    want = float(train.train_step_separate(other, train.make_optimizer(other, lr=1e-3), *args)[0])
    assert abs(hist[0] - want) <= 1e-5 * abs(want)
    with pytest.raises(ValueError, match="packed"):
        train.train_step_separate(model, opt, args[0], args[1], batch[3], batch[4], batch[5], device_loss=True)
    out = torch.from_numpy(F.copy()).to(cuda).requires_grad_(True)
    obj64 = args[4].long()

    def loss_and_backward():
        total, _ = train.separate_loss_packed(out, args[2], args[3], obj64, device_rows=True)
        total.backward()
        return total

    assert bool(torch.isfinite(_no_host_wait(loss_and_backward))) and bool(torch.isfinite(out.grad).all())
