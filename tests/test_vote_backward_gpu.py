"""hv_bwd (hv_vote.hip), the gradient of the vote, as a pure function of its inputs through the C ABI: every element against
the float64 oracle with a bound of its own (oracle/hv_numpy.py hv_backward64, VOTE_BWD_ERROR_MODEL; pinned on the CPU by
tests/test_vote_bound.py, which also asserts the geometry every case here is built for).

All five inputs and grad are carved from the middle of NaN-filled device buffers (GUARD floats of NaN on both sides), the
three outputs too: a read outside an array poisons the result, an element that was not written stays NaN, and the guards
must still be all NaN afterwards.  A second call must give the same bits (one wave per point, a butterfly: no atomics).

  sweep      R = 1 ... 256 over the trip counts of `for (i = lane; i < R; i += 64)`, n = 1 ... 1023 over the waves of the last
             workgroup that return at c >= n; a 9 x 6 x 13 grid
  cut        the grid is a box that cuts the cloud on all six sides: points with all, some and none of their votes in bounds
  big        a box larger than the cloud whose origin is not the cloud's minimum; objectness 0 and negative
  thin1/2    Y = 1 (no vote can be in bounds: every output is exactly 0) and Y = 2 (a single layer of cells)
  nodes      xyz = 0 and points on the nodes: all fractional parts 0; a vote at dims - 1 is out, one at the largest float
             below it is in and reads the last cell
  one-hot    a single cell of grad is 1, R = 1, xyz = 0: d_obj is the point's trilinear weight to that cell, to the bit
  large      n = 2^18 + 1: 65 537 workgroups
"""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from oracle import hv_numpy
from canonicalvoting_amd import _lib, hv_cuda
from canonicalvoting_amd.hough import HVFunction, HoughVoting

gpu = pytest.mark.gpu
f32 = np.float32
GUARD = 4096
NAMES = ("d_xyz", "d_scale", "d_obj")
RATIOS = {}                 # output -> worst error-to-bound ratio of this run (test_zz_report prints them)
T0 = time.time()

SWEEP = [(1, 1), (7, 3), (63, 4), (64, 5), (65, 1023), (120, 1), (128, 3), (129, 5), (256, 1023)]      # (R, n)
SWEEP_DIMS, SWEEP_RES, SWEEP_CORNER = [9, 6, 13], 0.07, [-0.31, 0.2, 1.03]
CUT_DIMS, CUT_RES, CUT_CORNER = [12, 7, 17], 0.125, [-0.75, 0.5, 1.25]       # exact in fp32: corners[1] = corner + (dims - 1) res


def _cloud(seed, n, dims, res, corner, widen, rad, R):
    """n points uniform over the box [corner, corner + (dims - 1) res] widened by `widen` cells on every side, votes on
    rings of up to `rad` cells (every fifth xyz = 0) lifted by up to half a cell in y; grad ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    corner = np.asarray(corner, f32)
    lo, hi = -float(widen), np.asarray(dims, np.float64) - 1 + widen
    cells = rng.uniform(lo, hi, (n, 3))
    r = rng.uniform(0, rad, n)
    r[::5] = 0.0
    phi = rng.uniform(0, 2 * np.pi, n)
    off = np.stack([r * np.cos(phi), rng.uniform(-0.5, 0.5, n) * (r > 0), r * np.sin(phi)], 1) * res
    scale = rng.uniform(0.5, 1.5, (n, 3)).astype(f32)
    return dict(pts=(corner + cells * res).astype(f32), xyz=(off / scale).astype(f32), scale=scale,
                obj=rng.uniform(0.1, 1.0, n).astype(f32), grad=rng.normal(0, 1, tuple(dims)).astype(f32),
                corner=corner, dims=list(dims), res=res, R=R)


def case_sweep(R, n):
    return _cloud(100 + R, n, SWEEP_DIMS, SWEEP_RES, SWEEP_CORNER, -0.5, 2.5, R)      # inside the box: most rotations are in


def case_cut():
    return _cloud(7, 1500, CUT_DIMS, CUT_RES, CUT_CORNER, 4.0, 5.0, 60)


def cut_corners():
    lo = np.asarray(CUT_CORNER, f32)
    return np.stack([lo, lo + (np.asarray(CUT_DIMS, f32) - 1) * f32(CUT_RES)]).astype(f32)


def case_big():
    """a 15 x 9 x 11 box around a cloud that fills its middle; every third objectness 0, every third negative"""
    c = _cloud(8, 777, [15, 9, 11], 0.11, [3.3, -1.7, 0.45], -2.5, 3.0, 36)
    c["obj"][0::3] = 0.0
    c["obj"][1::3] *= -1.0
    return c


def case_thin(Y):
    c = _cloud(20 + Y, 500, [9, Y, 13], 0.07, SWEEP_CORNER, 1.0, 2.5, 24)
    if Y == 2:                                       # the single layer: y votes inside [0, 1) cells for most points
        c["pts"][:, 1] = (c["corner"][1] + np.random.default_rng(3).uniform(-0.2, 1.2, 500) * c["res"]).astype(f32)
        c["xyz"][:, 1] *= f32(0.2)
    return c


def case_nodes():
    """res = 1, corner 0, a 5 x 4 x 6 grid, xyz = 0: every node of the grid (the last one of an axis is out of bounds) and,
    for every axis, points at the largest float below dims - 1"""
    dims = [5, 4, 6]
    nodes = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3).astype(f32)
    below = []
    for k in range(3):
        p = np.array([1, 2, 3], f32)
        p[k] = np.nextafter(f32(dims[k] - 1), f32(0))
        below.append(p)
    pts = np.concatenate([nodes, np.stack(below)]).astype(f32)
    n = len(pts)
    rng = np.random.default_rng(5)
    return dict(pts=pts, xyz=np.zeros((n, 3), f32), scale=rng.uniform(0.5, 1.5, (n, 3)).astype(f32),
                obj=rng.uniform(0.1, 1.0, n).astype(f32), grad=rng.normal(0, 1, tuple(dims)).astype(f32),
                corner=np.zeros(3, f32), dims=dims, res=1.0, R=7)


def case_one_hot():
    """R = 1 (theta = 0), xyz = 0, res = 1, corner 0: grid_pos is the point itself.  grad is 1 at (3, 2, 4) of 7 x 5 x 11"""
    dims, hot = [7, 5, 11], (3, 2, 4)
    rng = np.random.default_rng(6)
    n = 203
    pts = (np.asarray(hot) + rng.uniform(-1.15, 1.15, (n, 3))).astype(f32)
    pts[::7] = np.round(pts[::7])
    grad = np.zeros(dims, f32)
    grad[hot] = 1.0
    return dict(pts=pts, xyz=np.zeros((n, 3), f32), scale=np.ones((n, 3), f32), obj=rng.uniform(0.1, 1.0, n).astype(f32),
                grad=grad, corner=np.zeros(3, f32), dims=dims, res=1.0, R=1, hot=hot)


def case_large():
    """the last point, the only wave of workgroup 65 536 that does not return, votes where it stands in the middle of the box"""
    c = _cloud(9, (1 << 18) + 1, [15, 9, 21], 0.125, [0.5, -0.25, 2.0], 2.0, 4.0, 3)
    c["pts"][-1] = c["corner"] + f32(0.125) * np.array([7.3, 4.2, 10.6], f32)
    c["xyz"][-1] = 0.0
    return c


CASES = dict([("sweep_R%d_n%d" % rn, functools.partial(case_sweep, *rn)) for rn in SWEEP],
             cut=case_cut, big=case_big, thin1=functools.partial(case_thin, 1), thin2=functools.partial(case_thin, 2),
             nodes=case_nodes, one_hot=case_one_hot, large=case_large)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """hv_backward64 of the case and its bounds, computed once and left unchanged"""
    c = case(name)
    ref = hv_numpy.hv_backward64(c["grad"], c["pts"], c["xyz"], c["scale"], c["obj"], c["res"], c["R"], c["corner"])
    return ref, hv_numpy.vote_bwd_bounds(ref)


def guarded(cuda, a):
    """(buffer, view): a in the middle of a NaN-filled device buffer; without a, a NaN-filled window of that shape"""
    size = int(np.prod(a.shape if hasattr(a, "shape") else a))
    buf = torch.full((2 * GUARD + size,), float("nan"), dtype=torch.float32, device=cuda)
    view = buf[GUARD:GUARD + size]
    if hasattr(a, "shape"):
        view.copy_(torch.from_numpy(np.ascontiguousarray(a, f32).ravel()))
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def backward(cuda, c, twice=True):
    """cv_hv_backward_f32 on guarded buffers, on the current stream -> (d_xyz [n,3], d_scale [n,3], d_obj [n]) as numpy"""
    L = _lib.lib()
    n = len(c["pts"])
    ins = [guarded(cuda, c[k]) for k in ("grad", "pts", "xyz", "scale", "obj")]
    keep = [v.clone() for _, v in ins]

    def once():
        outs = [guarded(cuda, shape) for shape in ((n, 3), (n, 3), (n,))]
        args = [hv_cuda._ptr(v) for _, v in ins] + [n, ctypes.c_float(c["res"]), c["R"], hv_cuda._f3(c["corner"]),
                                                   (ctypes.c_int * 3)(*c["dims"])] + [hv_cuda._ptr(v) for _, v in outs]
        with torch.cuda.device(cuda):
            _lib.check(L.cv_hv_backward_f32(*args, hv_cuda._stream(cuda)), "cv_hv_backward_f32")
        torch.cuda.current_stream(cuda).synchronize()
        for buf, _ in ins + outs:
            assert guards_intact(buf), "a guard word was written"
        for (_, v), k in zip(ins, keep):
            assert torch.equal(v.view(torch.int32), k.view(torch.int32)), "an input was written"
        return [v.clone() for _, v in outs]

    first = once()
    if twice:
        for a, b, name in zip(first, once(), NAMES):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name + ": the second call differs"
    return first[0].cpu().numpy().reshape(n, 3), first[1].cpu().numpy().reshape(n, 3), first[2].cpu().numpy()


def assert_within(got, name, tag=None):
    """every element inside its bound, rows without a vote in bounds exact zeros; records the worst ratios"""
    ref, bounds = reference(name)
    none = ref["votes"] == 0
    for key, g in zip(NAMES, got):
        assert not np.isnan(g).any(), "%s %s: %d elements were not written (or read a guard)" % (name, key, int(np.isnan(g).sum()))
        assert np.isfinite(g).all(), (name, key)
        assert not g[none].any(), "%s %s: a point without a vote in bounds has a gradient" % (name, key)
        ratio = np.abs(g.astype(np.float64) - ref[key]) / bounds[key]
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio[i]))
        print("%s %s: worst error %.3f of its bound" % (tag or name, key, float(ratio[i])))
        assert ratio[i] <= 1.0, "%s %s: element %s off by %.3g x its bound (got %r, fp64 %r, bound %.3g, votes %d)" % (
            tag or name, key, i, float(ratio[i]), float(g[i]), float(ref[key][i]), float(bounds[key][i]), int(ref["votes"][i[0]]))


@gpu
@pytest.mark.parametrize("name", [k for k in CASES if k not in ("one_hot", "large")])
def test_backward_is_inside_the_bound(cuda, built_lib, name):
    got = backward(cuda, case(name))
    assert_within(got, name)
    c = case(name)
    if name == "thin1":
        assert not any(g.any() for g in got)
    if name == "big":
        zero = c["obj"] == 0
        assert zero.sum() > 200 and (c["obj"] < 0).sum() > 200
        assert not got[0][zero].any() and not got[1][zero].any()           # d_xyz / d_scale carry the objectness ...
        assert np.count_nonzero(got[2][zero]) > 100                        # ... d_obj does not


@gpu
def test_one_hot_grad_gives_the_trilinear_weight_to_the_bit(cuda, built_lib):
    """a known answer that does not pass through the oracle: with R = 1, xyz = 0, res = 1 and corner 0 the vote is the point,
    and d_obj = ((wx * wy) * wz) of the hot cell in fp32 - the other seven terms are products with 0"""
    c = case("one_hot")
    got = backward(cuda, c)
    p, dims = c["pts"], c["dims"]
    inb = np.all((p >= 0) & (p < (np.asarray(dims, f32) - 1)), 1)
    fl = np.floor(p)
    fr = (p - fl).astype(f32)
    w = np.ones(len(p), f32)
    for k in range(3):
        rel = c["hot"][k] - fl[:, k]                   # 0: the low cell (weight 1 - fr), 1: the high cell (fr), else none
        wk = np.where(rel == 0, (f32(1) - fr[:, k]).astype(f32), np.where(rel == 1, fr[:, k], f32(0))).astype(f32)
        w = (w * wk).astype(f32)
    want = np.where(inb, w, f32(0)).astype(f32)
    assert np.count_nonzero(want) > 50 and (want == 0).sum() > 20 and (want == 1).sum() >= 1
    assert np.array_equal(got[2], want)
    assert_within(got, "one_hot")


@gpu
def test_more_than_65535_workgroups(cuda, built_lib):
    c = case("large")
    assert (len(c["pts"]) + 3) // 4 == 65537
    got = backward(cuda, c, twice=False)
    assert_within(got, "large")


@gpu
def test_on_a_side_stream(cuda, built_lib):
    c = case("cut")
    want = backward(cuda, c, twice=False)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        got = backward(cuda, c, twice=False)
    side.synchronize()
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert_within(got, "cut", "cut (side stream)")


@gpu
def test_through_autograd_with_corners(cuda, built_lib):
    """HoughVoting(...)(p, x, s, o, corners=cut box).backward(): the gradients are the bits of the direct call with the grid
    origin corners[0]; HVFunction.backward returns seven values, None for corners"""
    c = case("cut")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    p, x, s, o = t(c["pts"]), t(c["xyz"]), t(c["scale"]), t(c["obj"])
    x.requires_grad_(True); s.requires_grad_(True); o.requires_grad_(True)
    corners = t(cut_corners())
    hv = HoughVoting(c["res"], c["R"])
    g_obj = hv(p, x, s, o, corners=corners)[0]
    assert list(g_obj.shape) == c["dims"]
    (g_obj * t(c["grad"])).sum().backward()
    torch.cuda.synchronize()
    direct = backward(cuda, c, twice=False)
    for got, want, name in zip((x.grad, s.grad, o.grad), direct, NAMES):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), name
    assert_within(direct, "cut", "cut (autograd)")

    class Ctx:
        saved_tensors = (p, x.detach(), s.detach(), o.detach(), hv.res, hv.num_rots)
    Ctx.corners = corners
    out = HVFunction.backward(Ctx, t(c["grad"]), None, None)
    assert len(out) == 7 and out[0] is None and all(v is None for v in out[4:])
    for got, want in zip(out[1:4], direct):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # without the corners the origin is the minimum of the points: another grid, other numbers
    other = hv_cuda.backward(t(c["grad"]), p, x.detach(), s.detach(), o.detach(), hv.res, hv.num_rots)
    assert not np.array_equal(other[2].cpu().numpy(), direct[2])


@gpu
def test_zz_report():
    """not a check of its own: the worst error-to-bound ratio per output of this run and the module's wall time"""
    for k in sorted(RATIOS):
        print("ratio %-8s %.3f" % (k, RATIOS[k]))
    print("module wall time %.1f s" % (time.time() - T0))
