"""The scene axis of the C ABI (cv_decode_scenes_f32, cv_detect_scenes_f32) without a GPU: exported, struct sizes equal to
the ctypes mirrors, workspace sizes that reduce to the single-scene ones at B = 1 and grow with B, every pre-device refusal,
the per-scene result layout restated in numpy, and what tests/decode_ref.py says about the hand-made decode jobs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from canonicalvoting_amd import _lib
from tests import decode_scene_cases as sc

EINVAL = -22
NEW = ("cv_decode_scenes_workspace_bytes", "cv_decode_scenes_f32", "cv_detect_scenes_f32", "cv_sizeof_decode_scene_job",
       "cv_sizeof_scenes_desc", "cv_sizeof_scenes_result")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_symbols_are_exported_and_sizes_match(built_lib):
    L = ctypes.CDLL(built_lib)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _lib.SIGNATURES, s
    L = _lib.lib()
    assert L.cv_sizeof_decode_scene_job() == ctypes.sizeof(_lib.DecodeSceneJob)
    assert L.cv_sizeof_scenes_desc() == ctypes.sizeof(_lib.ScenesDesc)
    assert L.cv_sizeof_scenes_result() == ctypes.sizeof(_lib.ScenesResult)
    assert _lib.MAX_SCENES == 16 and L.cv_abi_version() == 6
    # the descriptor IS the one-scene descriptor plus the count
    assert _lib.ScenesDesc.scene.offset == 0 and _lib.ScenesDesc.num_scenes.offset >= ctypes.sizeof(_lib.SceneDesc)


def jobs_of(dims_n):
    jobs = (_lib.DecodeSceneJob * len(dims_n))()
    row = 0
    for j, (dims, n) in zip(jobs, dims_n):
        j.dims = (ctypes.c_int * 3)(*dims)
        j.row0, j.n = row, n
        row += n
    return jobs


def test_decode_workspace_is_monotone_in_B_and_the_single_query_at_1(built_lib):
    L = _lib.lib()
    shapes = [((174, 88, 174), 80000), ((40, 30, 40), 3000), ((3, 3, 3), 1), ((301, 101, 301), 300000)] * 4
    for m in (8, 512):
        jobs = jobs_of(shapes)
        singles = [L.cv_decode_workspace_bytes((ctypes.c_int * 3)(*d), n, m) for d, n in shapes]
        assert L.cv_decode_scenes_workspace_bytes(jobs, 1, m) == singles[0]
        sizes = [L.cv_decode_scenes_workspace_bytes(jobs, b, m) for b in range(1, 17)]
        assert sizes == [sum(singles[:b]) for b in range(1, 17)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        assert L.cv_decode_scenes_workspace_bytes(jobs, 0, m) == 0 and L.cv_decode_scenes_workspace_bytes(jobs, 17, m) == 0
        assert L.cv_decode_scenes_workspace_bytes(None, 4, m) == 0
    assert L.cv_decode_scenes_workspace_bytes(jobs_of(shapes), 4, 0) == 0


def test_decode_scenes_refuses_bad_input_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every refusal below comes from a host-side check
    p = _lib.DecodeParams(60.0, 10.0, 0.2, 2, 0.3, 1, 8, 0.3)
    ni = (ctypes.c_int * 16)()
    i64 = (ctypes.c_int64 * 256)()
    i32 = (ctypes.c_int32 * 256)()
    f32 = (ctypes.c_float * 4096)()

    def fresh():
        jobs = jobs_of([((9, 5, 7), 700), ((16, 4, 12), 50), ((3, 3, 3), 1)])
        for j in jobs:
            j.d_grid_obj = j.d_grid_rot = j.d_grid_scale = 4096
        return jobs

    def dec(jobs, b=3, pts=fake, cls=fake, prm=ctypes.byref(p), out=ni, ws=1 << 30):
        return L.cv_decode_scenes_f32(jobs, b, ctypes.c_float(0.03), pts, fake, fake, cls, prm, 0, fake, ws, out, i64, i32, ni, f32,
                                      f32, i32, ni, None)

    for b in (0, -1, 17):
        assert dec(fresh(), b) == EINVAL and b"num_scenes" in L.cv_last_error()
    assert dec(None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(fresh(), pts=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(fresh(), cls=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(fresh(), prm=None) == EINVAL and b"null" in L.cv_last_error()
    assert dec(fresh(), out=None) == EINVAL and b"null" in L.cv_last_error()
    jobs = fresh()
    jobs[1].d_grid_rot = None
    assert dec(jobs) == EINVAL and b"scene 1" in L.cv_last_error()
    jobs = fresh()
    jobs[2].n = 0
    assert dec(jobs) == EINVAL and b"scene 2" in L.cv_last_error()
    jobs = fresh()
    jobs[0].dims[1] = 0
    assert dec(jobs) == EINVAL and b"scene 0" in L.cv_last_error()
    assert dec(fresh(), ws=1024) == -12 and b"workspace" in L.cv_last_error()
    p.max_iters = 0
    assert dec(fresh()) == EINVAL and b"max_iters" in L.cv_last_error()
    p.max_iters, p.thresh_high = 8, 0.0
    assert dec(fresh()) == EINVAL and b"thresh_high" in L.cv_last_error()


def scenes_desc(B):
    d, r = _lib.ScenesDesc(), _lib.ScenesResult()
    fake = ctypes.c_void_p(4096)
    s = d.scene
    for f in ("d_coords4", "d_feats", "d_points", "ops", "bufs", "d_out_feats", "h_pinned", "d_ws", "h_boxes", "h_scores",
              "h_classes", "h_cand_idx", "h_verdict", "h_pick"):
        setattr(s, f, fake)
    s.n, s.n_ops, s.n_bufs, s.out_ld, s.out_channels, s.pinned_bytes, s.max_candidates = 100, 10, 5, 96, 96, 4096, 8
    d.num_scenes = B
    return d, r


def test_scenes_call_refuses_bad_descriptors_before_touching_the_gpu(built_lib):
    """every field is validated before the first device call: the fake pointers are never dereferenced and no GPU is needed"""
    L = _lib.lib()
    call = lambda d, r: L.cv_detect_scenes_f32(ctypes.byref(d), ctypes.byref(r), None)
    d, r = scenes_desc(3)
    assert L.cv_detect_scenes_f32(None, ctypes.byref(r), None) == EINVAL
    assert L.cv_detect_scenes_f32(ctypes.byref(d), None, None) == EINVAL
    for b in (0, -2, 17):
        d.num_scenes = b
        assert call(d, r) == EINVAL and b"num_scenes" in L.cv_last_error() and str(b).encode() in L.cv_last_error()
    for f, word in (("d_coords4", b"descriptor"), ("d_feats", b"descriptor"), ("d_points", b"descriptor"), ("ops", b"descriptor"),
                    ("d_out_feats", b"output"), ("h_pinned", b"pinned"), ("d_ws", b"workspace"), ("h_boxes", b"result arrays"),
                    ("h_scores", b"result arrays"), ("h_classes", b"result arrays"), ("h_cand_idx", b"result arrays"),
                    ("h_verdict", b"result arrays"), ("h_pick", b"result arrays")):
        d, r = scenes_desc(3)
        setattr(d.scene, f, None)
        assert call(d, r) == EINVAL and word in L.cv_last_error(), f
    d, r = scenes_desc(3)
    d.scene.pinned_bytes = 256 + 64 * 3 - 1                 # the per-scene bounds land behind the one-scene call's 256 bytes
    assert call(d, r) == EINVAL and b"pinned" in L.cv_last_error()
    for f in ("conv_split_target", "vote_part_records"):
        d, r = scenes_desc(3)
        setattr(d.scene, f, -1)
        r.host_us[0] = 7.0
        assert call(d, r) == EINVAL and b"negative launch sizing" in L.cv_last_error() and r.host_us[0] == 0.0
    for algo in (-1, 3):
        d, r = scenes_desc(3)
        d.scene.vote_algo = algo
        assert call(d, r) == EINVAL and b"vote_algo" in L.cv_last_error()
    d, r = scenes_desc(1)
    d.scene.n = 0
    assert call(d, r) == EINVAL and b"descriptor" in L.cv_last_error()
    assert L.cv_hv_set_part_records_thread(0) == 0 and L.cv_sp_set_split_target_thread(0) == 0      # nothing left behind


def test_per_scene_result_layout():
    """scene b's entries of the host arrays at b * max_candidates (boxes: * 24 floats): what pipeline.detect_scenes_c reads as
    row b of [B, M] arrays; the result's per-scene fields are arrays of CV_MAX_SCENES"""
    B, M = 3, 8
    for dtype, tail, per in ((np.int64, (), 1), (np.int32, (), 1), (np.float32, (), 1), (np.float32, (8, 3), 24)):
        a = np.zeros((B, M) + tail, dtype)            # (how pipeline._SceneHost allocates them for a scene axis)
        assert a.flags["C_CONTIGUOUS"]
        flat = a.reshape(-1)
        flat[:] = np.arange(flat.size) % 251
        for b in range(B):
            assert np.array_equal(a[b].reshape(-1), flat[b * M * per:(b + 1) * M * per])
    r = _lib.ScenesResult()
    for f in ("n_cand", "n_boxes", "n_det", "truncated", "row0", "rows", "d_grid_obj", "d_grid_rot", "d_grid_scale"):
        assert len(getattr(r, f)) == _lib.MAX_SCENES, f
    assert len(r.dims) == _lib.MAX_SCENES and len(r.dims[0]) == 3 and len(r.corner[15]) == 3
    r.dims[2][1] = 5
    assert np.ctypeslib.as_array(r.dims).reshape(-1)[2 * 3 + 1] == 5


def test_hand_made_decode_jobs_are_what_they_claim():
    jobs = sc.batch()
    assert [c.grid_obj.shape for c in jobs] == list(sc.DIMS) and [len(c.pts) for c in jobs] == list(sc.POINTS)
    sc.claims(sc.expected(jobs))
    pts, xyz, prob, cls, ranges = sc.concat(jobs)
    assert ranges == [(0, 700), (700, 750), (750, 751), (751, 3751)] and len(pts) == 3751
    assert [(-(-(hi - lo) // 256)) for lo, hi in ranges] == [3, 1, 1, 12]      # back-projection workgroups per job


def test_eval_joint_takes_scenes_per_call():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_joint.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "--scenes-per-call" in r.stdout
