"""The vote tile kernel's workgroup-wide survivor list (hv_vote.hip, hv_fwd_tiles): rounds of cull / arcs / expand.

Every case is compared with the CPU oracle the way tests/test_vote_gpu.py::test_forward_matches_oracle_small does (touched
set and in-bounds vote count exact, the same bounds on the values) and with the recorded bits of the per-wave chunk kernel
that preceded it: tests/golden/vote_parent_bits.json holds the sha256 of the bytes of the three grids of every case as that
kernel wrote them.  All six channels accumulate as 2^-36 fixed-point integers, whose sums do not depend on the order or the
grouping of the votes, so the hashes are expected to be EQUAL.

The overflow of the work-list array (list mode falling back to streaming) and the other launch shapes that no case here takes
(more than 4096 planes, the tile-count bounds of the queue launch, more than 256 rotations) are in
tests/test_vote_fallbacks_gpu.py."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import oracle
from canonicalvoting_amd import _lib, hv_cuda
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.synth import make_scene, synth_predictions
from tests.test_vote_gpu import assert_grids_close, dev_inputs, run_hip

pytestmark = pytest.mark.gpu
BITS = os.path.join(os.path.dirname(__file__), "golden", "vote_parent_bits.json")
RES = 0.03


def _rings(rng, cx, cy, cz, rad):
    """points at grid positions (cx, cy, cz) [cells] whose votes form rings of radius rad [cells] in their y plane"""
    n = len(cx)
    pts = (np.stack([cx, cy, cz], 1) * RES).astype(np.float32)
    phi = rng.uniform(0, 2 * np.pi, n)
    off = np.stack([rad * np.cos(phi), np.zeros(n), rad * np.sin(phi)], 1) * RES
    scale = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    xyz = (off / scale).astype(np.float32)
    prob = rng.uniform(0.5, 1.0, n).astype(np.float32)
    return pts, xyz, scale, prob


def _with_anchors(case, hi):
    """two more points with xyz = 0 (a ring of radius 0) that span the grid [0, hi] cells"""
    pts, xyz, scale, prob = case
    a = (np.array([[0, 0, 0], hi], np.float64) * RES).astype(np.float32)
    return (np.concatenate([pts, a]), np.concatenate([xyz, np.zeros((2, 3), np.float32)]),
            np.concatenate([scale, np.ones((2, 3), np.float32)]), np.concatenate([prob, np.ones(2, np.float32)]))


def case_rounds():
    """3000 points in one y cell and a 10 x 20-cell patch, rings of 3 to 12 cells, R = 120: the tiles of planes 2 and 3
    around the patch keep far more than the 512 survivors a round holds, and the list fills up inside a chunk"""
    rng = np.random.default_rng(101)
    n = 3000
    c = _rings(rng, rng.uniform(15, 25, n), rng.uniform(2.2, 2.8, n), rng.uniform(20, 40, n), rng.uniform(3, 12, n))
    return _with_anchors(c, [40, 6, 60]) + (RES, 120)


def case_corner():
    """64 points in one corner of a grid of three tiles, one lone point with xyz = 0 in the middle tile: workgroups with
    no survivor and with a single one"""
    rng = np.random.default_rng(102)
    n = 64
    c = _rings(rng, rng.uniform(2, 7, n), rng.uniform(0.5, 2.5, n), rng.uniform(2, 7, n), rng.uniform(0.5, 2, n))
    pts, xyz, scale, prob = c
    lone = (np.array([[24.25, 1.5, 16.5]]) * RES).astype(np.float32)
    c = (np.concatenate([pts, lone]), np.concatenate([xyz, np.zeros((1, 3), np.float32)]),
         np.concatenate([scale, np.ones((1, 3), np.float32)]), np.concatenate([prob, np.ones(1, np.float32)]))
    return _with_anchors(c, [47, 4, 31]) + (RES, 120)


def case_inside():
    """ring centres inside the tile (full arcs of R rotations) and xyz = 0 (a ring of radius 0: all 120 votes of a point
    into one cell)"""
    rng = np.random.default_rng(103)
    n = 300
    rad = rng.uniform(0.05, 6, n)
    rad[::5] = 0.0
    c = _rings(rng, rng.uniform(3, 12, n), rng.uniform(0.5, 3.5, n), rng.uniform(4, 27, n), rad)
    c[0][::10] = np.round(c[0][::10] / RES) * np.float32(RES)       # some of them on the nodes
    return _with_anchors(c, [15, 5, 31]) + (RES, 120)


def case_parts():
    """10 000 points in one plane: its two bins hold 10 000 records, three parts at 4096 records per part"""
    rng = np.random.default_rng(104)
    n = 10000
    c = _rings(rng, rng.uniform(8, 56, n), rng.uniform(3.1, 3.9, n), rng.uniform(8, 56, n), rng.uniform(1, 7, n))
    return _with_anchors(c, [64, 8, 64]) + (RES, 120)


def _small_scene(R):
    sc = make_scene(4, n_points=777, res=0.06, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
    xyz, scale, prob, _ = synth_predictions(sc)
    return sc.points, xyz, scale, prob, sc.res, R


def case_r7():
    return _small_scene(7)


def case_r256():
    """MAX_R_TILES rotations"""
    return _small_scene(256)


def case_lists():
    """4000 points in a 16 m x 4 m room at res 0.03: about 170 tiles, the work-queue launch with per-(bin, tile) lists"""
    sc = make_scene(6, n_points=4000, room=(16.0, 2.0, 4.0), n_boxes=8)
    xyz, scale, prob, _ = synth_predictions(sc)
    return sc.points, xyz, scale, prob, sc.res, 120


def case_huge():
    """contributions above the fast fixed-point conversion's range, in a batch with ordinary ones"""
    sc = make_scene(14, n_points=1500, res=0.06, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
    xyz, scale, prob, _ = synth_predictions(sc)
    scale = scale.copy()
    scale[::7] *= 1.0e5
    xyz = (xyz * 1e-5 * (scale > 1e3) + xyz * (scale <= 1e3)).astype(np.float32)
    return sc.points, xyz, scale, prob, sc.res, 24


CASES = {"rounds": case_rounds, "corner": case_corner, "inside": case_inside, "parts": case_parts, "r7": case_r7,
         "r256": case_r256, "lists": case_lists, "huge": case_huge}


def grid_hashes(grids):
    return {k: hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest() for k, g in zip(("obj", "rot", "scale"), grids)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and the oracle's grids, computed once"""
    pts, xyz, scale, prob, res, R = CASES[name]()
    ref = oracle.hv_forward(pts, xyz, scale, prob, res, R, return_vin=True)
    return (pts, xyz, scale, prob, res, R), ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_oracle_and_the_recorded_bits(cuda, built_lib, name):
    (pts, xyz, scale, prob, res, R), ref = _case(name)
    hip = run_hip(cuda, pts, xyz, scale, prob, res, R, 2)
    if name == "huge":
        # (the bounds of test_huge_scale_contributions_take_the_exact_slow_path: the per-contribution quantum bound of
        # assert_grids_close is stated for contributions inside the fast conversion's range)
        assert np.array_equal(hip[0] == 0, ref[0] == 0)
        np.testing.assert_allclose(hip[0], ref[0], rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ref[0]).max())))
        live = ref[0] > 1e-3 * max(1.0, float(np.abs(ref[0]).max()))
        np.testing.assert_allclose(hip[2][live], ref[2][live], rtol=1e-4, atol=1e-4)
        assert float(np.abs(ref[2]).max()) > 2e4                    # the slow path was exercised
    else:
        assert_grids_close(hip, ref[:3], name, inputs=(pts, xyz, scale, res, R))
    corner, _, dims = oracle.grid_geometry(pts, res)
    p, x, s, _ = dev_inputs(cuda, pts, xyz, scale, prob)
    assert hv_cuda.count_votes(p, x, s, res, R, corner, dims) == ref[3]
    with open(BITS) as f:
        want = json.load(f)[name]
    assert grid_hashes(hip) == want, name + ": the grids are not the bits the per-wave chunk kernel wrote"


def test_case_shapes_are_what_they_claim(built_lib):
    """the geometry the cases rely on: tile counts (16 x 32-cell tiles), one bin, the work-queue threshold of 128 tiles"""
    tiles = lambda d: -(-d[0] // 16) * -(-d[2] // 32)
    dims = {k: oracle.grid_geometry(CASES[k]()[0], CASES[k]()[4])[2] for k in ("rounds", "corner", "parts", "lists")}
    assert tiles(dims["corner"]) == 3
    assert tiles(dims["rounds"]) < 128 and tiles(dims["parts"]) < 128 and tiles(dims["lists"]) >= 128
    pts = CASES["rounds"]()[0][:-2]
    assert len(pts) == 3000 and len(np.unique(np.floor(pts[:, 1] / np.float32(RES)))) == 1
    pts = CASES["parts"]()[0][:-2]
    assert len(pts) == 10000 and len(np.unique(np.floor(pts[:, 1] / np.float32(RES)))) == 1


def test_parts_give_the_same_grids_at_every_part_size(cuda, built_lib):
    """10 000 records of one plane at 4096 (three parts), 12288 and 16384 (one part, twenty rounds) records per part"""
    (pts, xyz, scale, prob, res, R), _ = _case("parts")
    args = dev_inputs(cuda, pts, xyz, scale, prob)
    L = _lib.lib()
    hv = HoughVoting(res, R)
    hv_cuda.set_algorithm(2)
    before = L.cv_hv_set_part_records(4096)
    try:
        grids = []
        for records in (4096, 12288, 16384):
            L.cv_hv_set_part_records(records)
            with torch.no_grad():
                grids.append(hv(*args))
            torch.cuda.synchronize()
    finally:
        L.cv_hv_set_part_records(before)
        hv_cuda.set_algorithm(0)
    assert float(grids[0][0].max()) > 0
    for other in grids[1:]:
        for a, b in zip(grids[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", ["parts", "lists"])
def test_writes_nothing_beyond_the_workspace_size_it_reports(cuda, built_lib, name, K):
    """cv_hv_forward_cat_f32 on a workspace of exactly cv_hv_forward_cat_workspace_bytes bytes: the 64 KB behind it (part of the
    same allocation, so nothing can fault) keep their fill pattern, and the grids are the bits of the same call on a roomy
    workspace.  `parts`: streaming launch with a plane split into parts; `lists`: work-queue launch; K = 2: a second category
    (half the offsets) one category stride behind the first.  The workspace arrives filled with the pattern, not zeroed."""
    import ctypes
    (pts, xyz, scale, prob, res, R), _ = _case(name)
    p, x, s, o = dev_inputs(cuda, pts, xyz, scale, prob)
    x = torch.stack([x, x * 0.5][:K]).contiguous()
    s = torch.stack([s, s][:K]).contiguous()
    o = torch.stack([o, o][:K]).contiguous()
    L = _lib.lib()
    n = p.shape[0]
    mn, _, dims = hv_cuda.grid_geometry(p, res)
    cdims = (ctypes.c_int * 3)(*dims)
    X, Y, Z = dims
    size = L.cv_hv_forward_cat_workspace_bytes(n, R, cdims, 2, K)
    assert size == K * L.cv_hv_forward_workspace_bytes(n, R, cdims, 2) > 0
    TAIL, PATTERN = 65536, 0xA5

    def vote(ws, ws_bytes):
        grids = [torch.empty((K, X, Y, Z) + tail, dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
        with torch.cuda.device(cuda):
            _lib.check(L.cv_hv_forward_cat_f32(hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), n,
                                               ctypes.c_float(res), R, hv_cuda._f3(mn), cdims, K, hv_cuda._ptr(grids[0]),
                                               hv_cuda._ptr(grids[1]), hv_cuda._ptr(grids[2]), hv_cuda._ptr(ws), ws_bytes, 2,
                                               hv_cuda._stream(cuda)), "cv_hv_forward_cat_f32")
        torch.cuda.synchronize()
        return grids

    tight = torch.full((size + TAIL,), PATTERN, dtype=torch.uint8, device=cuda)
    got = vote(tight, size)
    assert bool((tight[size:] == PATTERN).all()), "bytes behind the reported workspace size were written"
    assert not bool((tight[:size] == PATTERN).all())
    roomy = torch.zeros((2 * size + TAIL,), dtype=torch.uint8, device=cuda)
    want = vote(roomy, roomy.numel())
    assert float(want[0][K - 1].max()) > 0
    for a, b in zip(got, want):
        assert torch.equal(a, b)
