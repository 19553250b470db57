"""Votes into a box given by `corners` that CUTS the cloud (what proposals.HoughVotingModule does on every call), against the
CPU oracle.  Every other vote test takes the points' own bounding box as the grid, so the tile algorithm has never met a
point outside it: there the ring centre (ux, uz) is negative or beyond the last tile, which is what the tile clamps of
hv_list_pass, ring_touches, ring_arc and the streaming cull of hv_tile_item (hv_vote.hip) have to get right - the direct
kernel and hv_count_votes share only the bounds test with them.

res = 1 and cell units as in tests/test_vote_fallbacks_gpu.py (whose _rings makes the votes), explicit corners, no anchor
points.  The points are uniform over the box widened by 40 cells in x / z and 1.5 in y, the rings 0 to 60 cells, every fifth
xyz = 0, every tenth point on the x / z nodes.  tests/test_vote_bound.py asserts on the CPU that in-bounds votes from points
outside the box are a large share of every case.

  stream   64 x 6 x 96: 12 tiles, streaming launch
  queue    256 x 6 x 256: 128 tiles, queue launch with work lists (list_ctl read back from a workspace the test owns)
  shifted  the same box with its origin at (-3.5, 10.25, 7.75)
           (both: the entry total of the work lists is that of a numpy restatement of ring_touches - an over-inclusive cull
           changes no grid value, only this number and the time)
  small    33 x 2 x 65, R = 7

Per case, for the direct kernel (algo 1) and the tile algorithm (algo 2): the grids under the bounds of
tests/test_vote_gpu.py (assert_grids_close), the exact vote count, a second call on the used workspace (equal bits from the
tile algorithm; the direct kernel adds fp32 atomics in the order of arrival and is held to the bounds again), and for the tile
algorithm the peaks entry."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import hv_numpy
from canonicalvoting_amd import _lib, hv_cuda
from tests.test_vote_fallbacks_gpu import (RES, TAIL, _rings, assert_launch, assert_tail_untouched, equal_bits, list_ctl_words,
                                           pattern_workspace, ring_entries, takes_queue_launch)
from tests.test_vote_gpu import assert_grids_close, dev_inputs
from tests.test_vote_peaks_gpu import assert_peaks_equal_full

gpu = pytest.mark.gpu
f32 = np.float32

# name -> (dims, origin, points, R, launch)
CASES = {
    "stream": ([64, 6, 96], [0.0, 0.0, 0.0], 3000, 120, "stream"),
    "queue": ([256, 6, 256], [0.0, 0.0, 0.0], 4000, 120, "queue"),
    "shifted": ([256, 6, 256], [-3.5, 10.25, 7.75], 4000, 120, "queue"),
    "small": ([33, 2, 65], [0.0, 0.0, 0.0], 1500, 7, "stream"),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    dims, origin, n, R, _ = CASES[name]
    X, Y, Z = dims
    rng = np.random.default_rng(X + Z + n)
    rad = rng.uniform(0, 60, n)
    rad[::5] = 0.0
    cells = rng.uniform(-40, X - 1 + 40, n), rng.uniform(-1.5, Y - 1 + 1.5, n), rng.uniform(-40, Z - 1 + 40, n)
    pts, xyz, scale = _rings(rng, *cells, rad)
    pts[::10, 0::2] = np.round(pts[::10, 0::2])
    origin = np.asarray(origin, f32)
    pts = (pts + origin).astype(f32)                       # (the rounded x / z stay on the nodes: the origin is in quarters)
    corners = np.stack([origin, origin + (np.asarray(dims, f32) - 1)]).astype(f32)
    return dict(pts=pts, xyz=xyz, scale=scale, prob=rng.uniform(0.5, 1.0, n).astype(f32), dims=dims, R=R, corners=corners)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's grids, its in-bounds vote count and the contributions per cell, computed once and left unchanged"""
    c = case(name)
    ref = oracle.hv_forward(c["pts"], c["xyz"], c["scale"], c["prob"], RES, c["R"], corners=c["corners"], return_vin=True)
    counts = hv_numpy.contribution_counts(c["pts"], c["xyz"], c["scale"], RES, c["R"], c["corners"][0], c["dims"])
    return ref[:3], ref[3], counts


@functools.lru_cache(maxsize=None)
def list_entries(name):
    """numpy restatement of the work-list total (ring_entries of tests/test_vote_fallbacks_gpu.py) with the ring centres in
    cell units, (p - corner) / res as hv_prep_scatter stores them"""
    c = case(name)
    return ring_entries(dict(c, pts=(c["pts"] - c["corners"][0]).astype(f32)))


def vote(cuda, c, ws, ws_bytes, algo, thresh=None):
    """cv_hv_forward_f32 (thresh None) or cv_hv_forward_peaks_f32 with the grid of c["corners"] on the caller's workspace,
    the grids pre-filled with NaN"""
    L = _lib.lib()
    p, x, s, o = dev_inputs(cuda, c["pts"], c["xyz"], c["scale"], c["prob"])
    dims = (ctypes.c_int * 3)()
    _lib.check(L.cv_hv_grid_dims_f32(hv_cuda._f3(c["corners"][0]), hv_cuda._f3(c["corners"][1]), ctypes.c_float(RES), dims), "dims")
    assert list(dims) == c["dims"]
    X, Y, Z = c["dims"]
    grids = [torch.full((X, Y, Z) + tail, float("nan"), dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    ptr = hv_cuda._ptr
    args = [ptr(p), ptr(x), ptr(s), ptr(o), len(c["pts"]), ctypes.c_float(RES), c["R"], hv_cuda._f3(c["corners"][0]), dims]
    args += [ptr(g) for g in grids] + [ptr(ws), ws_bytes, algo] + ([] if thresh is None else [ctypes.c_float(thresh)])
    fn = "cv_hv_forward_f32" if thresh is None else "cv_hv_forward_peaks_f32"
    with torch.cuda.device(cuda):
        _lib.check(getattr(L, fn)(*args, hv_cuda._stream(cuda)), fn)
    torch.cuda.synchronize()
    return grids


@gpu
@pytest.mark.parametrize("algo", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_vote_into_a_box_that_cuts_the_cloud(cuda, built_lib, name, algo):
    c, launch = case(name), CASES[name][4]
    ref, vin, counts = reference(name)
    n = len(c["pts"])
    cdims = (ctypes.c_int * 3)(*c["dims"])
    size = _lib.lib().cv_hv_forward_workspace_bytes(n, c["R"], cdims, algo)
    assert size > 0
    ws = pattern_workspace(cuda, size)
    first = vote(cuda, c, ws, size, algo)
    assert_tail_untouched(ws, size, name)
    if algo == 2:
        words = list_ctl_words(ws, n)
        print("%s: list_ctl %s, in-bounds votes %d" % (name, words, vin))
        assert takes_queue_launch(c["dims"]) == (launch == "queue")
        assert_launch(words, launch, c, name)
        if launch == "queue":
            # the cull itself: a ring_touches that keeps too much leaves every grid value as it is (the arcs only get longer)
            # and shows here alone.  Not asserted to the unit: a (ring, tile) pair whose radius is within an fp32 rounding
            # of dmin - tol or dmax + tol may fall either way (relative width 1e-7 of 1e5 candidate pairs)
            assert abs(words[0] - list_entries(name)) <= 2, (name, words[0], list_entries(name))
    assert_grids_close([g.cpu().numpy() for g in first], ref, "%s algo %d" % (name, algo), counts=counts)
    p, x, s, _ = dev_inputs(cuda, c["pts"], c["xyz"], c["scale"], c["prob"])
    assert hv_cuda.count_votes(p, x, s, RES, c["R"], c["corners"][0], c["dims"]) == vin
    again = vote(cuda, c, ws, size, algo)
    if algo == 2:
        assert equal_bits(first, again), name + ": the second call differs"
    else:       # fp32 atomics in the order of arrival: not the same bits run to run, the same bounds
        assert_grids_close([g.cpu().numpy() for g in again], ref, "%s algo 1, second call" % name, counts=counts)
    assert_tail_untouched(ws, size, name)
    if algo == 2:
        top = np.sort(np.partition(ref[0].ravel(), -41)[-41:])
        th = float(f32(0.5 * (float(top[0]) + float(top[1]))))
        assert th > 0
        peaks = vote(cuda, c, ws, size, algo, thresh=th)
        hot = assert_peaks_equal_full(first, peaks, th, name)
        assert 10 < hot < 200, (name, hot, th)
        everywhere = vote(cuda, c, ws, size, algo, thresh=float("-inf"))
        assert equal_bits(first, everywhere), name + ": thresh -inf"
        assert_tail_untouched(ws, size, name)


@gpu
def test_drop_in_forward_with_corners_gives_the_same_bits(cuda, built_lib):
    """hv_cuda.forward(..., corners) (its own scratch, algo auto) on the shifted box: the bits of the C call above"""
    c = case("shifted")
    n = len(c["pts"])
    size = _lib.lib().cv_hv_forward_workspace_bytes(n, c["R"], (ctypes.c_int * 3)(*c["dims"]), 0)
    want = vote(cuda, c, torch.zeros(size + TAIL, dtype=torch.uint8, device=cuda), size, 0)
    p, x, s, o = dev_inputs(cuda, c["pts"], c["xyz"], c["scale"], c["prob"])
    res = torch.tensor(RES, dtype=torch.float32, device=cuda)
    rots = torch.tensor(c["R"], dtype=torch.int32, device=cuda)
    got = hv_cuda.forward(p, x, s, o, res, rots, torch.from_numpy(c["corners"]).to(cuda))
    torch.cuda.synchronize()
    assert equal_bits(want, got)
    assert hv_cuda.recent_corner(got[0]) == [float(v) for v in c["corners"][0]]
