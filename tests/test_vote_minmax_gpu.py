"""The two small reductions in front of every vote (hv_vote.hip), through the C ABI: cv_hv_minmax_f32 / _async_f32, which
give every grid its shape, and cv_hv_count_votes_f32.  Until now the first was only checked through the grid shape that
follows from it, and the second never took the second trip of its grid-stride loop (2048 workgroups of 256: n R > 524 288).

minmax_partial runs min(256, ceil(n / 256)) workgroups of 256 threads that stride over the points: n = 255 / 256 / 257 are the
sides of one workgroup, 65 536 / 65 537 those of the second trip.  The points are a slice of a NaN-filled buffer (a read
outside it makes the result NaN) and the extremes sit at index 0, at n - 1 and, where there is one, at an index >= 65 536.
min / max select, they do not round: the results are compared by == with numpy's (which does not tell -0.0 from 0.0)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from canonicalvoting_amd import _lib, hv_cuda
from tests.test_vote_fallbacks_gpu import _rings

gpu = pytest.mark.gpu
f32 = np.float32
GUARD = 4096
CV_ENOMEM = -12
SIZES = [1, 255, 256, 257, 65536, 65537, 200003]
DENORMAL = f32(1e-40)


def cloud(n, kind):
    """[n, 3] points in (-3, 5); the extremes of x at index 0 (min) and n - 1 (max), those of y the other way round, those of z
    at an index >= 65 536 where there is one (else in the middle).  negative: everything below -1, so a reduction that starts
    from 0 instead of -inf finds a wrong maximum.  tiny: x is negative but for one denormal (its maximum), y positive but for
    one -0.0 (its minimum)"""
    rng = np.random.default_rng(n)
    pts = rng.uniform(-3, 5, (n, 3)).astype(f32)
    if n > 1:
        pts[0, 0], pts[n - 1, 0] = -3.5, 5.5
        pts[0, 1], pts[n - 1, 1] = 5.25, -3.25
        pts[65536 + (n - 65536) // 2 if n > 65536 else n // 2, 2] = 6.0
        pts[65536 if n > 65537 else 0, 2] = -4.0
    if kind == "negative":
        pts = (-np.abs(pts) - 1).astype(f32)
    if kind == "tiny":
        pts[:, 0] = -np.abs(pts[:, 0]) - 1
        pts[:, 1] = np.abs(pts[:, 1]) + 1
        pts[n // 3, 0] = DENORMAL
        pts[n // 2, 1] = -0.0
    return pts


def guarded_points(cuda, pts):
    buf = torch.full((2 * GUARD + pts.size,), float("nan"), dtype=torch.float32, device=cuda)
    view = buf[GUARD:GUARD + pts.size].view(-1, 3)
    view.copy_(torch.from_numpy(pts))
    return buf, view


def minmax(cuda, view, ws=None, ws_bytes=None):
    L = _lib.lib()
    need = L.cv_hv_minmax_workspace_bytes()
    if ws is None:
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=cuda)
    mn, mx = (ctypes.c_float * 3)(), (ctypes.c_float * 3)()
    with torch.cuda.device(cuda):
        rc = L.cv_hv_minmax_f32(hv_cuda._ptr(view), view.shape[0], mn, mx, hv_cuda._ptr(ws), need if ws_bytes is None else ws_bytes,
                                hv_cuda._stream(cuda))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "bytes behind the reported workspace size were written"
    return rc, np.array(mn, f32), np.array(mx, f32)


@gpu
@pytest.mark.parametrize("n,kind", [(n, "plain") for n in SIZES] + [(257, "negative"), (65537, "negative"), (255, "tiny"),
                                                                   (65537, "tiny")])
def test_minmax_equals_numpy(cuda, built_lib, n, kind):
    pts = cloud(n, kind)
    buf, view = guarded_points(cuda, pts)
    rc, mn, mx = minmax(cuda, view)
    assert rc == 0
    want_mn, want_mx = pts.min(0), pts.max(0)
    print("n %d %s: min %s max %s" % (n, kind, mn, mx))
    assert np.array_equal(mn, want_mn) and np.array_equal(mx, want_mx), (mn, want_mn, mx, want_mx)
    if kind == "plain" and n > 1:
        assert list(mn) == [-3.5, -3.25, -4.0] and list(mx) == [5.5, 5.25, 6.0]
    if kind == "negative":
        assert (mx < 0).all()
    if kind == "tiny":
        assert mx[0] == DENORMAL and mx[0] > 0 and mn[1] == 0          # the denormal survives; the zero's sign is not asserted
    omn, omx, _ = oracle.grid_geometry(pts, 1.0)
    assert np.array_equal(omn, mn) and np.array_equal(omx, mx)
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


@gpu
def test_prefetched_geometry_is_the_synchronous_one(cuda, built_lib):
    """cv_hv_minmax_async_f32 through hv_cuda.prefetch_geometry: grid_geometry picks the six floats up, and they are those of
    the synchronous entry"""
    pts = cloud(65537, "plain")
    _, view = guarded_points(cuda, pts)
    want = hv_cuda.grid_geometry(view, 0.05)
    hv_cuda.prefetch_geometry(view)
    assert (hv_cuda.threading.get_ident(), view.data_ptr()) in hv_cuda._prefetched
    got = hv_cuda.grid_geometry(view, 0.05)
    assert (hv_cuda.threading.get_ident(), view.data_ptr()) not in hv_cuda._prefetched        # it was the prefetched result
    assert got == want
    assert got[0] == [float(v) for v in pts.min(0)] and got[1] == [float(v) for v in pts.max(0)]


@gpu
def test_minmax_below_its_workspace_size_launches_nothing(cuda, built_lib):
    L = _lib.lib()
    need = L.cv_hv_minmax_workspace_bytes()
    _, view = guarded_points(cuda, cloud(257, "plain"))
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=cuda)
    rc, mn, mx = minmax(cuda, view, ws, need - 1)
    assert rc == CV_ENOMEM and b"workspace" in L.cv_last_error()
    assert bool((ws == 0xA5).all()) and not mn.any() and not mx.any()
    host = torch.full((6,), 7.0).pin_memory()
    with torch.cuda.device(cuda):
        rc = L.cv_hv_minmax_async_f32(hv_cuda._ptr(view), 257, ctypes.c_void_p(host.data_ptr()), hv_cuda._ptr(ws), need - 1,
                                      hv_cuda._stream(cuda))
    torch.cuda.synchronize()
    assert rc == CV_ENOMEM and bool((ws == 0xA5).all()) and bool((host == 7.0).all())


@gpu
def test_count_votes_takes_the_second_trip_of_its_stride_loop(cuda, built_lib):
    """n = 6000, R = 120: 720 000 (point, rotation) pairs for 2048 x 256 threads.  The grid is a 96 x 6 x 64 box that cuts the
    cloud (cells of 1, origin (2.5, -1.25, 4)); the count is the oracle's"""
    n, R, dims = 6000, 120, [96, 6, 64]
    assert n * R > 2048 * 256
    rng = np.random.default_rng(11)
    rad = rng.uniform(0, 40, n)
    rad[::5] = 0.0
    pts, xyz, scale = _rings(rng, rng.uniform(-30, 125, n), rng.uniform(-1.5, 6.5, n), rng.uniform(-30, 93, n), rad)
    origin = np.array([2.5, -1.25, 4.0], f32)
    pts = (pts + origin).astype(f32)
    corners = np.stack([origin, origin + (np.asarray(dims, f32) - 1)]).astype(f32)
    vin = oracle.hv_forward(pts, xyz, scale, np.ones(n, f32), 1.0, R, corners=corners, return_vin=True)[3]
    assert 0.05 * n * R < vin < 0.6 * n * R
    # the pairs of the second trip hold in-bounds votes of their own
    from oracle import hv_numpy
    pi, ri, _, _, _ = hv_numpy.vote_geometry(pts, xyz, scale, 1.0, R, origin, dims)
    assert len(pi) == vin and int((pi * R + ri >= 2048 * 256).sum()) > 1000
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    assert hv_cuda.count_votes(t(pts), t(xyz), t(scale), 1.0, R, origin, dims) == vin
