"""Voxelisation of raw clouds, the parts that need no GPU: the host-side argument checks of cv_sp_quantize_f32 / _f64, the
torch and return_inverse faces of ME.utils.sparse_quantize on the host path, and the synthetic raw scenes.

Expected values come from an inline restatement of the numpy path (np.floor(c / q), np.unique(axis=0, return_index=True),
np.sort) - never from the code under test."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, synth
from canonicalvoting_amd.me import utils as me_utils


def unique_restated(points, q):
    """the host sparse_quantize as it stood before the device path existed"""
    c = np.asarray(points)
    if q is not None:
        c = np.floor(c / q)
    c = c.astype(np.int32)
    _, idx = np.unique(c, axis=0, return_index=True)
    idx = np.sort(idx)
    return c, idx


def surface_cloud(seed, m, dtype=np.float32, shift=0.0):
    """points on the faces of a 5.2 x 2.6 x 5.2 m room with 5 mm jitter"""
    rng = np.random.default_rng(seed)
    p = rng.random((m, 3)) * np.array([5.2, 2.6, 5.2])
    face = rng.integers(0, 3, m)
    p[np.arange(m), face] = np.where(rng.random(m) < 0.5, 0.0, np.array([5.2, 2.6, 5.2])[face])
    p += rng.normal(0, 0.005, p.shape) + shift
    return p.astype(dtype)


def call(fn, real, **kw):
    a = dict(points=4096, m=100, ld=3, q=0.03, floor_only=0, offsets=None, n_clouds=0, coords4=4096, index=4096, inverse=None,
             counts=4096, h_counts=None, ws=4096, ws_bytes=1 << 40, stream=None)        # fake pointers: never dereferenced
    a.update(kw)
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    off = None if a["offsets"] is None else (ctypes.c_int64 * len(a["offsets"]))(*a["offsets"])
    return fn(vp(a["points"]), a["m"], a["ld"], real(a["q"]), a["floor_only"], off, a["n_clouds"], vp(a["coords4"]), vp(a["index"]),
              vp(a["inverse"]), vp(a["counts"]), a["h_counts"], vp(a["ws"]), a["ws_bytes"], a["stream"])


@pytest.mark.parametrize("name", ["cv_sp_quantize_f32", "cv_sp_quantize_f64"])
def test_quantize_call_refuses_bad_arguments_before_touching_the_gpu(built_lib, name):
    L = _lib.lib()
    fn = getattr(L, name)
    real = float
    for null in ("points", "coords4", "index", "counts", "ws"):
        assert call(fn, real, **{null: None}) == -22 and b"null pointer" in L.cv_last_error()
    for off in (4, 8, 12, 1):                     # coords4 rows are stored as 16-byte words
        assert call(fn, real, coords4=4096 + off) == -22 and b"16-byte aligned" in L.cv_last_error()
    for m in (0, -5):
        assert call(fn, real, m=m) == -22 and b"point count" in L.cv_last_error()
    for q in (0.0, -0.03, float("nan"), float("inf")):
        assert call(fn, real, q=q) == -22 and b"quantization_size" in L.cv_last_error()
    assert call(fn, real, ld=2) == -22 and b"row stride" in L.cv_last_error()
    assert call(fn, real, offsets=[0, 60, 40], n_clouds=3) == -22 and b"not sorted" in L.cv_last_error()
    assert call(fn, real, offsets=[0, 50, 101], n_clouds=3) == -22 and b"out of range" in L.cv_last_error()
    assert call(fn, real, offsets=[0, -1, 50], n_clouds=3) == -22 and b"out of range" in L.cv_last_error()
    assert call(fn, real, offsets=[5, 50], n_clouds=2) == -22 and b"start at row 0" in L.cv_last_error()
    assert call(fn, real, offsets=[0], n_clouds=0) == -22 and b"cloud count" in L.cv_last_error()
    assert call(fn, real, offsets=[0], n_clouds=257) == -22 and b"cloud count" in L.cv_last_error()
    need = L.cv_sp_quantize_workspace_bytes(100)
    assert need >= L.cv_sp_table_capacity(100) * 12 + 400
    assert call(fn, real, ws_bytes=need - 1) == -12 and b"workspace too small" in L.cv_last_error()
    assert L.cv_sp_quantize_workspace_bytes(0) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("q", [0.03, 0.05, None])
def test_numpy_calls_return_what_they_did(dtype, q):
    p = surface_cloud(1, 20000, dtype, shift=-1.3)
    feats = np.random.default_rng(2).random((p.shape[0], 3)).astype(np.float32)
    labels = np.arange(p.shape[0])
    c, idx = unique_restated(p, q)
    got = me_utils.sparse_quantize(p, quantization_size=q)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, c[idx])
    got = me_utils.sparse_quantize(p, feats, quantization_size=q)
    assert len(got) == 2 and np.array_equal(got[0], c[idx]) and np.array_equal(got[1], feats[idx])
    got = me_utils.sparse_quantize(p, feats, labels, quantization_size=q)
    assert len(got) == 3 and np.array_equal(got[0], c[idx]) and np.array_equal(got[1], feats[idx]) and np.array_equal(got[2], labels[idx])
    got = me_utils.sparse_quantize(p, quantization_size=q, return_index=True)
    assert len(got) == 2 and np.array_equal(got[0], c[idx]) and np.array_equal(got[1], idx) and got[1].dtype == idx.dtype
    got = me_utils.sparse_quantize(p, feats, quantization_size=q, return_index=True)       # (return_index wins, as it did)
    assert len(got) == 2 and np.array_equal(got[1], idx)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpu_torch_tensors_take_the_host_path_and_come_back_as_torch(dtype):
    p = surface_cloud(3, 20000, dtype)
    feats = np.random.default_rng(4).random((p.shape[0], 3)).astype(np.float32)
    labels = np.random.default_rng(5).integers(0, 10, p.shape[0])
    c, idx = unique_restated(p, 0.03)
    coords, f, l = me_utils.sparse_quantize(torch.from_numpy(p), torch.from_numpy(feats), torch.from_numpy(labels), quantization_size=0.03)
    assert all(torch.is_tensor(t) and t.device.type == "cpu" for t in (coords, f, l))
    assert coords.dtype == torch.int32 and np.array_equal(coords.numpy(), c[idx])
    assert np.array_equal(f.numpy(), feats[idx]) and np.array_equal(l.numpy(), labels[idx])
    coords, index = me_utils.sparse_quantize(torch.from_numpy(p), quantization_size=0.03, return_index=True)
    assert torch.is_tensor(index) and np.array_equal(index.numpy(), idx) and np.array_equal(coords.numpy(), c[idx])
    # numpy in with device="cpu": torch out as well (the call shape of sunrgbd/brnetcanon.py:218 with another device)
    coords, f = me_utils.sparse_quantize(p, features=feats, quantization_size=0.03, device="cpu")
    assert torch.is_tensor(coords) and torch.is_tensor(f) and np.array_equal(coords.numpy(), c[idx]) and np.array_equal(f.numpy(), feats[idx])
    # and the result feeds batched_coordinates
    b = me_utils.batched_coordinates([coords, coords[:7]])
    assert b.shape == (coords.shape[0] + 7, 4) and b[-1, 0] == 1 and torch.equal(b[:coords.shape[0], 1:], coords)


@pytest.mark.parametrize("as_torch", [False, True])
@pytest.mark.parametrize("q", [0.03, None])
def test_host_inverse_maps_every_point_to_its_voxel(as_torch, q):
    p = surface_cloud(6, 30000, np.float32, shift=-2.0)
    c, idx = unique_restated(p, q)
    arg = torch.from_numpy(p) if as_torch else p
    coords, index, inverse = me_utils.sparse_quantize(arg, quantization_size=q, return_index=True, return_inverse=True)
    if as_torch:
        coords, index, inverse = coords.numpy(), index.numpy(), inverse.numpy()
    assert np.array_equal(coords, c[idx]) and np.array_equal(index, idx)
    assert inverse.shape == (p.shape[0],)
    assert np.array_equal(coords[inverse], c)                       # every point lands in the voxel of floor(p / q)
    assert np.all(index[inverse] <= np.arange(p.shape[0]))          # whose first point is not after it
    assert np.array_equal(inverse[index], np.arange(index.size))
    got = me_utils.sparse_quantize(arg, quantization_size=q, return_inverse=True)        # inverse is the last element
    assert len(got) == 2 and np.array_equal(np.asarray(got[1]), inverse)
    got = me_utils.sparse_quantize(arg, arg, quantization_size=q, return_inverse=True)
    assert len(got) == 3 and np.array_equal(np.asarray(got[2]), inverse)


# sha256 of the arrays' bytes, recorded from make_scene before make_raw_scene shared its sampler
MAKE_SCENE_SHA = {
    (0, 80000): dict(coords="1120eba72050bb82426f4a9242e196cdd3a7b8f7cc18e982c07b7d5c48ccd888",
                     feats="0e497869c9742d2dba230567c315fea6c2f6da2755cb2119793b35462635d80c",
                     xyz_labels="ec968bf727904f347d8a45a0bfb800e83c96be3589776e262fe631bd99e744db",
                     scale_labels="ddcdaa8cfc5a2f2c77c1debce4bcfc2a6691d332c4844209d737925b016f991a",
                     class_labels="33c6f727633ba96003bd2f4a9bfded176c9013826e3dcdc27aa5a8afe8c4f02c",
                     boxes="05e891620f4995193b8bd63670d0a1d146a6859e001a40a20ba62f83e0ca05a5"),
    (3, 20000): dict(coords="71fb7560a2e4e04ebc4d3277a3d104a66cab7c37ca0ea8360eae75d9070b2bae",
                     feats="dbcb278c569b7430992ca4eb33e1cd4ef166970edee39d35d75ceaa7b33f27d9",
                     xyz_labels="4138797c9d41b8cf87a8e7de7e19b2987e75c31d53ee891dbfb4595cde3d55ce",
                     scale_labels="fe6538d2aa8306c3164ac6ff47d6a92fafecef4a85e14dd09b2c411cbf612126",
                     class_labels="3f547366b6d0830c334ddfb364dca403156d564763ba093843d3f14c6264bf68",
                     boxes="370aec2b6afdbe98f395bb3892e39e4bac9d11fef26a933790fe2d51a2f0e3f0"),
}


@pytest.mark.parametrize("seed,n", sorted(MAKE_SCENE_SHA))
def test_make_scene_is_unchanged(seed, n):
    s = synth.make_scene(seed, n)
    for field, want in MAKE_SCENE_SHA[(seed, n)].items():
        a = np.ascontiguousarray(getattr(s, field))
        assert hashlib.sha256(a.tobytes()).hexdigest() == want, field


def test_make_raw_scene_is_deterministic_and_quantises_like_a_scene():
    a, b, c = synth.make_raw_scene(0, 50000), synth.make_raw_scene(0, 50000), synth.make_raw_scene(1, 50000)
    for f in ("points", "feats", "xyz_labels", "scale_labels", "class_labels", "boxes"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert not np.array_equal(a.points, c.points)
    assert a.points.shape == (50000, 3) and a.points.dtype == np.float64 and a.feats.dtype == np.float32
    assert a.class_labels.shape == (50000,) and set(np.unique(a.class_labels)) <= set(range(10))
    assert (a.class_labels != synth.BACKGROUND).sum() > 1000 and a.boxes.shape == (12, 8)
    # several samples per voxel: the unique step has something to do
    _, idx = unique_restated(a.points, 0.03)
    assert 10000 < idx.size < 50000
    # same layout as make_scene(seed): the ground-truth boxes before the origin shift
    assert np.array_equal(a.boxes, synth.make_scene(0, 20000, origin_shift=False).boxes)
    xyz, scale, prob, cls = synth.synth_predictions(a)
    assert xyz.shape == (50000, 3) and prob.shape == (50000,) and cls.dtype == np.int32
