"""The raw-cloud calls (cv_sp_voxel_rows_f32, cv_detect_points_f32, cv_detect_points_separate_f32), the parts that need no
GPU: exported symbols and ABI version, the ctypes mirrors of the new structures, the host-side argument checks (fake
pointers, never dereferenced: every refusal comes before the first device call) and the eval script's new flag."""
import ctypes
import importlib.util
import os
import re

import pytest

from canonicalvoting_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096
EINVAL, ENOMEM = -22, -12


def test_new_symbols_are_exported_and_the_abi_version_is_6(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ("cv_sp_voxel_rows_f32", "cv_detect_points_f32", "cv_detect_points_separate_f32"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "cv_hip.h")).read()
    header_version = int(re.search(r"#define\s+CV_ABI_VERSION\s+(\d+)", header).group(1))
    assert _lib.lib().cv_abi_version() == header_version == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define\s+CV_GATHER_MAX_JOBS\s+(\d+)", header).group(1)) == _lib.GATHER_MAX_JOBS == 8


def test_ctypes_structures_have_the_sizes_the_library_was_compiled_with(built_lib):
    L = _lib.lib()
    for helper, mirror in (("cv_sizeof_gather_job", _lib.GatherJob), ("cv_sizeof_points_desc", _lib.PointsDesc),
                           ("cv_sizeof_points_separate_desc", _lib.PointsSeparateDesc),
                           ("cv_sizeof_points_result", _lib.PointsResult),
                           ("cv_sizeof_points_separate_result", _lib.PointsSeparateResult)):
        assert getattr(L, helper)() == ctypes.sizeof(mirror), helper
    # the embedded scene descriptors / results are the existing ones, unchanged, behind the front / in front of the tail
    assert _lib.PointsDesc.scene.offset == _lib.PointsSeparateDesc.scene.offset == ctypes.sizeof(_lib.PointsFront)
    assert _lib.PointsDesc.scene.size == ctypes.sizeof(_lib.SceneDesc)
    assert _lib.PointsSeparateDesc.scene.size == ctypes.sizeof(_lib.SceneSeparateDesc)
    assert _lib.PointsResult.scene.offset == _lib.PointsSeparateResult.scene.offset == 0


def fill_front(f):
    f.d_raw_points = f.d_raw_feats = f.d_coords4 = f.d_index = FAKE
    f.m, f.points_ld, f.points_f64, f.quantization_size = 100, 3, 0, 0.03
    f.raw_feats_ld, f.in_channels, f.recentre_from = 3, 3, -1


def joint_desc():
    d, r = _lib.PointsDesc(), _lib.PointsResult()
    fill_front(d.front)
    s = d.scene
    for name in ("ops", "bufs", "d_out_feats", "h_pinned", "d_ws", "h_boxes", "h_scores", "h_classes", "h_cand_idx", "h_verdict",
                 "h_pick"):
        setattr(s, name, FAKE)
    s.n_ops, s.n_bufs, s.out_ld, s.out_channels, s.pinned_bytes, s.max_candidates = 1, 1, 64, 64, 256, 8
    s.stem_k, s.mask_groups, s.masked_min_rows, s.max_channels, s.num_rots, s.nclasses = 5, 4, 16384, 256, 120, 9
    s.ws_bytes = 0
    return d, r, (_lib.lib().cv_detect_points_f32,)


def separate_desc(K=3):
    d, r = _lib.PointsSeparateDesc(), _lib.PointsSeparateResult()
    fill_front(d.front)
    s = d.scene
    vp = ctypes.c_void_p
    tables = [(vp * K)(*[FAKE] * K), (ctypes.c_int * K)(*[1] * K), (vp * K)(*[FAKE] * K), (ctypes.c_int * K)(*[1] * K),
              (vp * K)(*[FAKE] * K)]
    s.ops, s.n_ops, s.bufs, s.n_bufs, s.d_out_feats = [ctypes.cast(t, vp) for t in tables]
    for name in ("h_pinned", "d_ws", "h_boxes", "h_scores", "h_cand_idx", "h_verdict", "h_det_cat", "h_det_box"):
        setattr(s, name, FAKE)
    s.num_models, s.out_ld, s.out_channels, s.pinned_bytes, s.max_candidates = K, 8, 8, 64 + 64 * K, 8
    s.stem_k, s.mask_groups, s.masked_min_rows, s.max_channels, s.num_rots = 5, 4, 16384, 256, 120
    s.ws_bytes = 0
    return d, r, (_lib.lib().cv_detect_points_separate_f32, tables)


def refused(make, message, **edits):
    """the call on a descriptor that is valid but for ``edits`` (front__m=..., scene__n=...) returns CV_EINVAL with ``message``"""
    L = _lib.lib()
    d, r, (fn, *alive) = make()
    for path, value in edits.items():
        part, field = path.split("__")
        setattr(getattr(d, part), field, value)
    rc = fn(ctypes.byref(d), ctypes.byref(r), None)
    err = L.cv_last_error()
    assert rc == EINVAL and message in err, (edits, rc, err)
    return r


@pytest.mark.parametrize("make", [joint_desc, separate_desc])
def test_points_calls_refuse_bad_arguments_before_touching_the_gpu(built_lib, make):
    L = _lib.lib()
    d, r, (fn, *alive) = make()
    assert fn(None, ctypes.byref(r), None) == EINVAL and b"null raw-cloud descriptor" in L.cv_last_error()
    assert fn(ctypes.byref(d), None, None) == EINVAL and b"null raw-cloud descriptor" in L.cv_last_error()
    for null in ("d_raw_points", "d_raw_feats", "d_coords4", "d_index"):
        refused(make, b"null pointer", **{"front__" + null: None})
    for m in (0, -5):
        refused(make, b"point count", front__m=m)
    refused(make, b"row stride", front__points_ld=2)
    for q in (0.0, -0.03, float("nan"), float("inf"), 1e-60, 1e60):       # (the last two: zero / infinite as the scene's fp32 res)
        refused(make, b"quantization_size", front__quantization_size=q)
    for c in (0, -1, 4):
        refused(make, b"feature width", front__in_channels=c)
    refused(make, b"recentre_from", front__recentre_from=4)
    refused(make, b"must be NULL / 0", scene__d_coords4=FAKE)
    refused(make, b"must be NULL / 0", scene__n=100)
    for f in ("d_feats", "d_points", "d_xyz_in", "d_scale_in", "d_prob_in"):
        refused(make, b"must be NULL / 0", **{"scene__" + f: FAKE})
    refused(make, b"must be NULL / 0", scene__feats_ld=3)
    for f in ("ops", "bufs", "d_out_feats", "d_ws", "h_pinned"):
        refused(make, b"bad scene descriptor", **{"scene__" + f: None})
    r = refused(make, b"bad scene descriptor", scene__max_candidates=0)
    assert r.n == 0 and r.rejected == 0 and r.front_ws_bytes == 0


def test_predictions_come_all_or_none(built_lib):
    for some in (("d_raw_xyz",), ("d_raw_xyz", "d_raw_scale", "d_raw_prob"), ("d_raw_class",), ("d_raw_scale", "d_raw_class")):
        refused(joint_desc, b"predictions: all 4 arrays or none", **{"front__" + f: FAKE for f in some})
    for some in (("d_raw_xyz",), ("d_raw_scale", "d_raw_prob")):
        refused(separate_desc, b"predictions: all 3 arrays or none", **{"front__" + f: FAKE for f in some})
    refused(separate_desc, b"no class array", front__d_raw_class=FAKE)
    refused(separate_desc, b"num_models out of range", scene__num_models=0)
    refused(separate_desc, b"num_models out of range", scene__num_models=17)


@pytest.mark.parametrize("make", [joint_desc, separate_desc])
@pytest.mark.parametrize("with_predictions", [False, True])
def test_a_workspace_without_room_for_the_front_reports_front_plus_scene(built_lib, make, with_predictions):
    """ws_bytes = 0: nothing is launched; needed_ws_bytes is the front's carve plus what the scene call asks for when every
    point is a voxel (its fixed-part estimate for n = m)"""
    L = _lib.lib()
    d, r, (fn, *alive) = make()
    if with_predictions:
        d.front.d_raw_xyz = d.front.d_raw_scale = d.front.d_raw_prob = FAKE
        if make is joint_desc:
            d.front.d_raw_class = FAKE
    m, K = d.front.m, (1 if make is joint_desc else d.scene.num_models)
    assert fn(ctypes.byref(d), ctypes.byref(r), None) == ENOMEM and b"workspace too small" in L.cv_last_error()
    up = lambda v: (v + 255) // 256 * 256
    front = up(L.cv_sp_quantize_workspace_bytes(m)) + up(8) + up(m * 3 * 4) + up(m * 3 * 4)
    if with_predictions:
        front += 2 * up(K * m * 3 * 4) + up(K * m * 4) + (up(m * 4) if make is joint_desc else 0)
    assert r.front_ws_bytes == front
    assert r.scene.needed_ws_bytes > front + (256 << 20) and str(r.scene.needed_ws_bytes).encode() in L.cv_last_error()
    assert r.n == 0 and r.rejected == 0


def test_voxel_rows_refuses_bad_arguments_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    vp = ctypes.c_void_p

    def call(n=100, res=0.03, coords4=FAKE, index=FAKE, points=FAKE, jobs=((FAKE, 6, FAKE, 6, 3, -1),), n_jobs=None, no_jobs=False):
        arr = (_lib.GatherJob * max(len(jobs), 1))(*[_lib.GatherJob(*j) for j in jobs])
        p = lambda v: None if v is None else vp(v)
        return L.cv_sp_voxel_rows_f32(p(coords4), p(index), n, res, p(points), None if no_jobs else arr,
                                      len(jobs) if n_jobs is None else n_jobs, None)

    for n in (0, -3):
        assert call(n=n) == EINVAL and b"row count" in L.cv_last_error()
    job = (FAKE, 6, FAKE, 6, 3, -1)
    assert call(jobs=(job,) * 9) == EINVAL and b"job count" in L.cv_last_error()
    assert call(n_jobs=-1) == EINVAL and b"job count" in L.cv_last_error()
    assert call(coords4=None) == EINVAL and b"null pointer" in L.cv_last_error()
    assert call(index=None) == EINVAL and b"null pointer" in L.cv_last_error()
    assert call(no_jobs=True) == EINVAL and b"null pointer" in L.cv_last_error()
    assert call(jobs=((None, 6, FAKE, 6, 3, -1),)) == EINVAL and b"job 0: null pointer" in L.cv_last_error()
    assert call(jobs=(job, (FAKE, 6, None, 6, 3, -1))) == EINVAL and b"job 1: null pointer" in L.cv_last_error()
    for bad in ((FAKE, 2, FAKE, 6, 3, -1), (FAKE, 6, FAKE, 2, 3, -1), (FAKE, 6, FAKE, 6, 0, -1), (FAKE, 6, FAKE, 6, -2, -1)):
        assert call(jobs=(job, job, bad)) == EINVAL and b"job 2: bad width" in L.cv_last_error()
    assert call(jobs=((FAKE, 6, FAKE, 6, 3, 4),)) == EINVAL and b"recentre_from" in L.cv_last_error()
    for res in (0.0, -0.03, float("nan"), float("inf")):
        assert call(res=res) == EINVAL and b"res must be" in L.cv_last_error()
    # nothing asked for: no launch, no error (no device is touched)
    assert call(points=None, jobs=(), coords4=None, index=None, res=0.0) == 0


def test_eval_separate_parses_with_the_raw_points_flag():
    spec = importlib.util.spec_from_file_location("cv_eval_separate", os.path.join(ROOT, "scripts", "eval_separate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(["--help"])
    assert e.value.code == 0 and "--raw-points" in ap.format_help()
    assert ap.parse_args([]).raw_points == 0 and ap.parse_args(["--raw-points"]).raw_points == 300000
    assert ap.parse_args(["--raw-points", "5000", "--teacher"]).raw_points == 5000
    assert callable(mod.evaluate_raw)
