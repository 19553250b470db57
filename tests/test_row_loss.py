"""The per-row losses (cv_row_loss_*, canonicalvoting_amd/csrc/row_loss.hip) without a GPU: the exported ABI and its host-side
argument checks, the fp64 oracle against the golden values of the reference's own lines (training and validation form, both
layouts), the restatement of the kernels' sequence inside the derived bounds, and named wrong results far outside them."""
import ctypes
import os

import numpy as np
import pytest

from canonicalvoting_amd import _lib
from tests import row_loss_ref as ref
from tests.golden import make_val_loss_golden as val_golden
from tests.golden.make_loss_golden import make_inputs, make_separate_inputs

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, XF, SF, GL = (0.5, 2.0, 1.0), 0.7, 1.3, 0.37


def _configs():
    return {"joint": ref.config("joint", w=W, xyz_factor=XF, scale_factor=SF, grad_loss=GL),
            "joint_plain": ref.config("joint", log_scale=False, w=W, xyz_factor=XF, scale_factor=SF, grad_loss=GL),
            "separate": ref.config("separate", w=W, xyz_factor=XF, scale_factor=SF, grad_loss=GL),
            "val": ref.config("joint", gather="argmax", empty="nan", w=W, xyz_factor=XF, scale_factor=SF)}


def test_the_library_exports_the_row_loss_abi_and_checks_its_arguments(built_lib):
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, "include", "cv_hip.h")).read()
    assert L.cv_abi_version() == _lib.ABI_VERSION == 6 and "#define CV_ABI_VERSION 6" in header
    assert L.cv_sizeof_row_loss_desc() == ctypes.sizeof(_lib.RowLossDesc)
    chunk = L.cv_row_loss_chunk_rows()
    assert chunk == 256
    assert L.cv_row_loss_workspace_bytes(10 * chunk + 5) >= 11 * 4 * 8 and L.cv_row_loss_workspace_bytes(-1) == 0
    FAKE = 0x1000                                                            # never dereferenced: every call below is refused first
    for fn in (L.cv_row_loss_fwd_f32, L.cv_row_loss_bwd_f32):
        assert fn(None, None) == -22 and b"null" in L.cv_last_error()

    def desc(layout="joint", **kw):
        d = _lib.RowLossDesc()
        for f in ("d_out", "d_labels", "d_xyz_labels", "d_scale_labels", "d_losses", "d_info", "d_grad_loss", "d_grad", "d_ws"):
            setattr(d, f, FAKE)
        d.heads, d.n_logits, d.xyz_col, d.scale_col, d.logit_col, d.obj_lo, d.obj_hi, d.with_xyz = _lib.ROW_LOSS_LAYOUTS[layout]
        width = d.logit_col + d.n_logits
        d.n_rows, d.ld, d.grad_ld, d.n_cols, d.ws_bytes = 1000, width, width, width, 1 << 20
        d.w = (ctypes.c_float * 3)(1, 1, 1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn in (L.cv_row_loss_fwd_f32, L.cv_row_loss_bwd_f32):
        for layout in ("joint", "separate"):
            for f in ("d_out", "d_labels", "d_scale_labels", "d_info"):
                assert fn(ctypes.byref(desc(layout, **{f: None})), None) == -22 and b"null pointer" in L.cv_last_error(), f
            width = 64 if layout == "joint" else 8
            assert fn(ctypes.byref(desc(layout, ld=width - 1)), None) == -22 and b"stride" in L.cv_last_error()
            assert fn(ctypes.byref(desc(layout, n_rows=-1)), None) == -22 and b"row count" in L.cv_last_error()
            assert fn(ctypes.byref(desc(layout, n_rows=1 << 31)), None) == -22
            assert fn(ctypes.byref(desc(layout, heads=0)), None) == -22 and b"heads" in L.cv_last_error()
            assert fn(ctypes.byref(desc(layout, n_logits=1)), None) == -22 and b"logits" in L.cv_last_error()
            assert fn(ctypes.byref(desc(layout, n_logits=17, ld=128)), None) == -22
            assert fn(ctypes.byref(desc(layout, gather=2)), None) == -22 and fn(ctypes.byref(desc(layout, empty=2)), None) == -22
            assert fn(ctypes.byref(desc(layout, scale_col=-1)), None) == -22
            clash = desc(layout, scale_col=desc(layout).logit_col - 1, ld=128, n_cols=128, grad_ld=128)
            assert fn(ctypes.byref(clash), None) == -22 and b"overlapping" in L.cv_last_error()
        assert fn(ctypes.byref(desc(d_xyz_labels=None)), None) == -22
        assert fn(ctypes.byref(desc(obj_hi=9)), None) == -22 and b"outside the 9 heads" in L.cv_last_error()
        assert fn(ctypes.byref(desc(obj_lo=-1)), None) == -22
    # without a coordinate term the coordinate labels may be missing; whatever remains is refused for its own reason
    assert L.cv_row_loss_fwd_f32(ctypes.byref(desc("separate", d_xyz_labels=None, d_ws=None)), None) == -12
    assert L.cv_row_loss_fwd_f32(ctypes.byref(desc(d_losses=None)), None) == -22
    assert L.cv_row_loss_fwd_f32(ctypes.byref(desc(gather=1, heads=8, obj_hi=7, n_logits=10)), None) == -22      # argmax 8 -> no head 8
    need = L.cv_row_loss_workspace_bytes(1000)
    assert L.cv_row_loss_fwd_f32(ctypes.byref(desc(ws_bytes=need - 1)), None) == -12
    assert (b"needs %d bytes" % need) in L.cv_last_error()
    assert L.cv_row_loss_fwd_f32(ctypes.byref(desc(d_ws=None)), None) == -12
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(gather=1)), None) == -22 and b"label gather" in L.cv_last_error()
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(n_cols=63)), None) == -22
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(ld=72, n_cols=72, grad_ld=70)), None) == -22
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(d_grad=None)), None) == -22
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(d_grad_loss=None)), None) == -22
    assert L.cv_row_loss_bwd_f32(ctypes.byref(desc(n_rows=0, d_out=None, d_grad=None)), None) == 0     # nothing to do, nothing launched


def test_the_python_layer_names_its_layouts_like_the_oracle():
    from canonicalvoting_amd.me import utils
    keys = ("heads", "n_logits", "xyz_col", "scale_col", "logit_col", "obj_lo", "obj_hi", "with_xyz")
    for layout in ("joint", "separate"):
        assert utils.row_loss_layout(layout) == tuple(ref.LAYOUTS[layout][k] for k in keys) == _lib.ROW_LOSS_LAYOUTS[layout]
    assert utils.row_loss_layout("joint", 4) == (4, 5, 0, 12, 24, 0, 3, 1)
    with pytest.raises(ValueError):
        utils.row_loss_layout("both")


def test_oracle_reproduces_the_golden_training_loss_and_gradient():
    z = np.load(os.path.join(GOLDEN_DIR, "loss_ref.npz"))
    F, labels, xyz, scale = make_inputs()
    r = ref.oracle(F, labels, xyz, scale, ref.config("joint"))
    for k, name in enumerate(("loss_xyz", "loss_scale", "loss_class", "loss")):
        assert abs(r["losses"][k] - float(z[name])) < 1e-6 * max(1.0, abs(float(z[name]))), name
    np.testing.assert_allclose(r["grad"], z["grad"], rtol=1e-5, atol=1e-8)
    assert r["cnt"] == int(((labels >= 0) & (labels < 9)).sum()) and r["n_bad"] == 0
    # the per-category layout: objectness and scale terms of train_separate.py:247-262 on the mini batch
    batch, F8 = make_separate_inputs()
    r = ref.oracle(F8, batch[5].numpy(), None, batch[4].numpy(), ref.config("separate"))
    assert r["losses"][0] == 0.0 and not r["grad"][:, :3].any()
    assert abs(r["losses"][1] - float(z["sep_loss_scale"])) < 1e-6 * max(1.0, abs(float(z["sep_loss_scale"])))
    assert abs(r["losses"][2] - float(z["sep_loss_obj"])) < 1e-6 * max(1.0, abs(float(z["sep_loss_obj"])))
    np.testing.assert_allclose(r["grad"][:, 3:], z["sep_grad"][:, 3:], rtol=1e-5, atol=1e-8)


def test_oracle_reproduces_the_golden_validation_losses():
    z = np.load(os.path.join(GOLDEN_DIR, "val_loss_ref.npz"))
    assert all(isinstance(z[k], np.ndarray) and z[k].dtype == np.float32 for k in z.files)
    c = ref.config("joint", gather="argmax", empty="nan", w=val_golden.WEIGHTS, xyz_factor=val_golden.XYZ_FACTOR,
                   scale_factor=val_golden.SCALE_FACTOR)
    for case in ("mixed", "background"):
        F, labels, xyz, scale = val_golden.make_inputs(case)
        r = ref.oracle(F, labels, xyz, scale, c)
        for k, name in enumerate(("loss_xyz", "loss_scale", "loss_class")):
            want = float(z["%s_%s" % (case, name)])
            if np.isnan(want):
                assert case == "background" and name != "loss_class" and np.isnan(r["losses"][k])
            else:
                assert abs(r["losses"][k] - want) < 1e-6 * max(1.0, abs(want)), (case, name)
        assert np.isnan(r["losses"][3]) == (case == "background")
        # the label form picks other heads: the validation form is not the training form
        other = ref.oracle(F, labels, xyz, scale, dict(c, gather="label"))
        assert case == "background" or abs(other["losses"][0] - r["losses"][0]) > 1e-3


def _restatement_cases():
    cfg = _configs()
    cases = []
    for n in (1, 255, 256, 257, 256 * 256 + 1):
        for name in ("joint", "separate"):
            cases.append(("%s_%d" % (name, n), ref.make_case(n, n, cfg[name]["layout"], ld=72 if name == "joint" else 11), cfg[name]))
    cases.append(("joint_plain", ref.make_case(5, 700, "joint"), cfg["joint_plain"]))
    cases.append(("val", ref.make_case(6, 700, "joint"), cfg["val"]))
    cases.append(("pm90", ref.make_case(7, 700, "joint", logits="pm90", poison=True), cfg["joint"]))
    cases.append(("background_zero", ref.make_case(8, 300, "joint", labels="background"), cfg["joint"]))
    cases.append(("background_nan", ref.make_case(8, 300, "joint", labels="background"), cfg["val"]))
    cases.append(("objects", ref.make_case(9, 300, "separate", labels="objects"), cfg["separate"]))
    cases.append(("bad_label", ref.make_case(10, 300, "joint", bad_label=True), cfg["joint"]))
    return cases


def test_restatement_stays_inside_the_bounds():
    """The kernels' sequence in numpy (chunk order, lane stretches, trees) against the oracle at every shape the GPU test runs:
    the worst error / bound over all cases measured here is 0.194 for the losses and 0.250 for the gradient elements (the one
    rounding to fp32, at most u of a 4 u bound); the assertion holds both to 0.3, under a third of the bound."""
    worst_l, worst_g = 0.0, 0.0
    for name, (out, y, xyz, scale), c in _restatement_cases():
        r = ref.oracle(out, y, xyz, scale, c)
        losses, info, grad = ref.restate(out, y, xyz, scale, c)
        assert info[0] == r["cnt"] and info[1] == r["n_bad"], name
        lr, gr = ref.worst_ratios(losses, grad, r)
        ref.assert_within(losses, grad, r, name)
        worst_l, worst_g = max(worst_l, float(lr.max())), max(worst_g, gr)
        if name in ("background_nan", "bad_label"):
            assert np.isnan(losses[3])
        if name == "background_zero":
            assert losses[0] == 0.0 and losses[1] == 0.0 and np.isfinite(losses[2])
        if name == "pm90":
            assert np.isfinite(losses).all() and np.isfinite(grad).all()
    print("restatement: worst error / bound  losses %.3f  gradient %.3f" % (worst_l, worst_g))
    assert worst_l <= 0.3 and worst_g <= 0.3


def test_named_wrong_results_land_far_outside_the_bounds():
    """each mistake an implementation could make moves a loss or a gradient element by at least 10 x its bound"""
    cfg = _configs()

    def outside(case, c, mutant):
        r = ref.oracle(*case, c)
        m = ref.oracle(*case, c, mutate=mutant)
        lr, gr = ref.worst_ratios(m["losses"], m["grad"], r)
        return max(float(lr.max()), gr)

    plain = ref.make_case(21, 700, "joint")
    assert outside(plain, cfg["joint"], "argmax_head") > 10.0                # head taken from argmax in the label form
    assert outside(plain, cfg["joint"], "denom_cnt") > 10.0                  # denominator cnt instead of 3 cnt
    assert outside(ref.make_case(22, 700, "separate"), cfg["separate"], "denom_cnt") > 10.0
    assert outside(plain, cfg["joint"], "neg_index") > 10.0                  # negative label used as an index
    poisoned = ref.make_case(23, 700, "joint", poison=True)                   # background row times 0 instead of selected away
    assert np.isfinite(ref.oracle(*poisoned, cfg["joint"])["losses"]).all()
    assert outside(poisoned, cfg["joint"], "times_zero") > 10.0
    hot = ref.make_case(24, 700, "joint", logits="pm90")                      # softmax without the max subtraction at +-90
    assert np.isfinite(ref.oracle(*hot, cfg["joint"])["losses"]).all()
    assert outside(hot, cfg["joint"], "no_max_fp32") > 10.0
    for case, c in ((plain, cfg["joint"]), (poisoned, cfg["joint"]), (hot, cfg["joint"])):        # (and the right one is inside)
        losses, _, grad = ref.restate(*case, c)
        lr, gr = ref.worst_ratios(losses, grad, ref.oracle(*case, c))
        assert max(float(lr.max()), gr) <= 1.0
