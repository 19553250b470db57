"""Category-axis entry points of the C ABI (cv_hv_forward_cat_f32, cv_decode_cat_f32) without a GPU: exported, workspace
sizes that reduce to the single-category ones at K = 1 and grow with K, and bad input refused with CV_EINVAL by the
host-side checks, before anything reaches the device."""
import ctypes
import os
import subprocess
import sys

import pytest

from canonicalvoting_amd import _lib

EINVAL = -22
NEW = ("cv_hv_forward_cat_workspace_bytes", "cv_hv_forward_cat_f32", "cv_decode_cat_workspace_bytes", "cv_decode_cat_f32",
       "cv_detect_scene_separate_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_category_symbols_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _lib.SIGNATURES, s


@pytest.mark.parametrize("n,dims", [(80000, (174, 88, 174)), (300000, (301, 101, 301)), (3000, (40, 30, 40))])
def test_workspace_sizes(built_lib, n, dims):
    L = _lib.lib()
    d = (ctypes.c_int * 3)(*dims)
    for algo in (0, 1, 2):
        one = L.cv_hv_forward_workspace_bytes(n, 120, d, algo)
        assert L.cv_hv_forward_cat_workspace_bytes(n, 120, d, algo, 1) == one
        sizes = [L.cv_hv_forward_cat_workspace_bytes(n, 120, d, algo, k) for k in (1, 2, 9, 16)]
        assert sizes == sorted(sizes) and sizes[2] >= 9 * one - 8 * 256 and len(set(sizes)) == 4
        assert L.cv_hv_forward_cat_workspace_bytes(n, 120, d, algo, 0) == 0
        assert L.cv_hv_forward_cat_workspace_bytes(n, 120, d, algo, 17) == 0
    for m in (8, 512):
        one = L.cv_decode_workspace_bytes(d, n, m)
        assert L.cv_decode_cat_workspace_bytes(d, n, m, 1) == one
        assert L.cv_decode_cat_workspace_bytes(d, n, m, 9) == 9 * one
        assert L.cv_decode_cat_workspace_bytes(d, n, m, 0) == 0
        assert L.cv_decode_cat_workspace_bytes(d, n, m, 17) == 0


def test_category_calls_refuse_bad_input_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every refusal below comes from a host-side check
    dims = (ctypes.c_int * 3)(40, 30, 40)
    corner = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def vote(k, pts=fake, obj=fake, g=fake):
        return L.cv_hv_forward_cat_f32(pts, fake, fake, obj, 3000, ctypes.c_float(0.03), 120, corner, dims, k, g, fake, fake,
                                       fake, 1 << 30, 0, None)

    for k in (0, -1, 17, 1000):
        assert vote(k) == EINVAL and b"num_cats" in L.cv_last_error()
    assert vote(9, pts=None) == EINVAL and b"null" in L.cv_last_error()
    assert vote(9, obj=None) == EINVAL and b"null" in L.cv_last_error()
    assert vote(9, g=None) == EINVAL and b"null" in L.cv_last_error()

    p = _lib.DecodeParams(60.0, 10.0, 0.2, 2, 0.3, 0, 8, 0.3)
    ni = (ctypes.c_int * 16)()
    i64 = (ctypes.c_int64 * 256)()
    i32 = (ctypes.c_int32 * 256)()
    f32 = (ctypes.c_float * 4096)()

    def dec(k, g=fake, xyz=fake, prm=ctypes.byref(p), out=ni):
        return L.cv_decode_cat_f32(g, fake, fake, dims, corner, ctypes.c_float(0.03), fake, xyz, fake, None, 3000, k, prm, 0, fake,
                                   1 << 30, out, i64, i32, ni, f32, f32, i32, ni, None)

    for k in (0, 17, -3):
        assert dec(k) == EINVAL and b"num_cats" in L.cv_last_error()
    assert dec(9, g=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(9, xyz=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(9, prm=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(9, out=None) == EINVAL and b"null" in L.cv_last_error()
    p.max_iters = 0
    assert dec(9) == EINVAL and b"max_iters" in L.cv_last_error()
    p.max_iters, p.thresh_high = 8, 0.0
    assert dec(9) == EINVAL and b"thresh_high" in L.cv_last_error()


def test_separate_scene_call_refuses_bad_descriptors_before_touching_the_gpu(built_lib):
    """cv_detect_scene_separate_f32: K out of range, null pointers and a model table shorter than K come back as CV_EINVAL
    with a message (host-side checks only: the fake pointers are never dereferenced); the result is zeroed first"""
    L = _lib.lib()
    d, r = _lib.SceneSeparateDesc(), _lib.SceneSeparateResult()
    assert L.cv_detect_scene_separate_f32(None, ctypes.byref(r), None) == EINVAL
    fake = ctypes.c_void_p(4096)
    vp = ctypes.c_void_p
    K = 3
    ops, bufs, outs = (vp * K)(4096, 4096, 4096), (vp * K)(4096, 4096, 4096), (vp * K)(4096, 4096, 4096)
    n_ops, n_bufs = (ctypes.c_int * K)(10, 10, 10), (ctypes.c_int * K)(5, 5, 5)
    for f in ("d_coords4", "d_feats", "d_points", "h_pinned", "d_ws", "h_boxes", "h_scores", "h_cand_idx", "h_verdict",
              "h_det_cat", "h_det_box"):
        setattr(d, f, fake)
    d.ops, d.bufs, d.d_out_feats = ctypes.cast(ops, vp), ctypes.cast(bufs, vp), ctypes.cast(outs, vp)
    d.n_ops, d.n_bufs = ctypes.cast(n_ops, vp), ctypes.cast(n_bufs, vp)
    d.n, d.out_ld, d.out_channels, d.pinned_bytes, d.max_candidates, d.num_models = 100, 8, 8, 4096, 8, K
    d.conv_split_target = -1          # valid otherwise: the last check refuses it, before any device call
    r.host_us[0] = 7.0
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
    assert b"negative launch sizing" in L.cv_last_error() and r.host_us[0] == 0.0
    d.conv_split_target = 0
    for k in (0, -1, 17):
        d.num_models = k
        assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
        assert b"num_models" in L.cv_last_error()
    d.num_models = K
    ops[2] = None                     # the tables hold fewer models than num_models
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL and b"model 2" in L.cv_last_error()
    ops[2] = 4096
    outs[1] = None
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL and b"model 1" in L.cv_last_error()
    outs[1] = 4096
    d.pinned_bytes = 64 + 64 * K - 1
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL and b"pinned" in L.cv_last_error()
    d.pinned_bytes = 4096
    d.d_xyz_in = fake                 # predictions: all three or none
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL and b"predictions" in L.cv_last_error()
    assert L.cv_hv_set_part_records_thread(0) == 0 and L.cv_sp_set_split_target_thread(0) == 0      # nothing left behind


def test_detect_scene_separate_c_refuses_a_model_count_out_of_range(built_lib):
    import torch
    from canonicalvoting_amd import pipeline
    c4 = torch.zeros((4, 4), dtype=torch.int32)
    for models in ({}, {c: None for c in range(17)}):
        with pytest.raises(ValueError, match="models"):
            pipeline.detect_scene_separate_c(models, None, c4, torch.zeros((4, 3)), 0.03)


def test_eval_separate_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_separate.py"), "--help"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "--weights-dir" in r.stdout and "--teacher" in r.stdout and "--config" in r.stdout
