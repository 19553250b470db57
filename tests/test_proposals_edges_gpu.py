"""Edges of the device proposal sampler that the hand-made cases of tests/test_proposals_device_gpu.py do not reach: the
clamps and the NaN rule of cv_prop_select_desc's contract (include/cv_hip.h) with the seeds spread over two LDS tiles,
cv_prop_cloud_ranges_i32 through the C ABI against numpy, proposals.cloud_corners on empty clouds and with a border, and one
sample of the reference's own sizes (1024 vote points, num_proposal = 512) through the columns, both select modes and
HoughVotingModule.propose.  Every comparison is of bytes or of integers.  (The seed-tile cases themselves are part of
proposal_cases.select_cases and run in test_select_draws_equal_the_oracle.)"""
import ctypes
from fractions import Fraction
from itertools import accumulate

import numpy as np
import pytest
import torch

from oracle import proposal_oracle as po
from canonicalvoting_amd import _lib, proposals
from canonicalvoting_amd.proposals import HoughVotingModule
from tests import proposal_cases as pc
from tests.test_proposals_device import cell_in_bracket
from tests.test_proposals_device_gpu import (SELECT_CASES, SENTINEL, _cells_of, _gpu_grids, _margin, _numpy_draws, _sync,
                                             run_columns, run_select)
from tests.test_proposals_gpu import _scene

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _case(name):
    return next(c for c in SELECT_CASES if c.name == name)


def _with(case, seeds=None, P=None):
    return pc.Case(case.name, case.grid, case.grid_scale, case.corner, case.res, case.seeds if seeds is None else seeds,
                   case.draws, case.P if P is None else P, case.pow)


def _far(case):
    """the case with one seed 1000 m away and P = S: the first round keeps all its draws, in draw order"""
    return _with(case, seeds=np.full((1, 3), 1e3), P=case.S)


def _select_equals_contract(cuda, case, yidx_d, yidx_ref, draws, draws_ref=None):
    """run cv_prop_select_f32 in draws mode and compare rows, sentinel rows and info with select_contract on
    (yidx_ref, draws_ref) -> (cand, scale, info) of the device"""
    cand, scale, info = run_select(cuda, case, yidx_d, draws=draws, with_host=True)
    cand, scale = cand.cpu().numpy(), scale.cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref_c, ref_s, filled, used = pc.select_contract(yidx_ref, case.grid_scale, case.corner, case.res, case.seeds,
                                                        draws if draws_ref is None else draws_ref, case.P)
    assert info == [filled, used]
    assert cand[:filled].tobytes() == ref_c[:filled].tobytes() and scale[:filled].tobytes() == ref_s[:filled].tobytes()
    assert (cand[filled:] == np.float32(SENTINEL)).all() and (scale[filled:] == np.float32(SENTINEL)).all()
    return cand, scale, info


# ------------------------------------------------------------------------------------------------------- NaN and Inf seeds
@pytest.mark.parametrize("at", [1024, 3], ids=["second_tile", "first_tile"])
def test_select_nan_seed_keeps_every_draw_and_inf_seed_counts_for_nothing(cuda, built_lib, at):
    case = _case("tile_V1025")
    n, Z = case.grid.shape[0] * case.grid.shape[2], case.grid.shape[2]
    yidx_d = run_columns(cuda, case.grid, case.pow)[1]
    yidx = yidx_d[:n].cpu().numpy()
    seeds = case.seeds.copy()
    seeds[at] = np.nan
    # a NaN wins the minimum of every draw: no draw is near, every round keeps all of its draws
    for P, want in ((case.P, [case.P, 1]), (300, [300, 2])):
        cand, _, info = _select_equals_contract(cuda, _with(case, seeds, P), yidx_d, yidx, case.draws)
        assert info == want
        assert cand[:P].tobytes() == pc.world_of(case.draws.reshape(-1)[:P], yidx, Z, case.res, case.corner).tobytes()
    # +Inf gives d2 = inf, which neither wins nor poisons the minimum: the result of the list without that seed
    seeds[at] = np.inf
    cand, scale, info = _select_equals_contract(cuda, _with(case, seeds), yidx_d, yidx, case.draws)
    cand2, scale2, info2 = _select_equals_contract(cuda, _with(case, np.delete(case.seeds, at, 0)), yidx_d, yidx, case.draws)
    assert info == info2 and info[1] == 3
    assert cand.tobytes() == cand2.tobytes() and scale.tobytes() == scale2.tobytes()


# ------------------------------------------------------------------------------------------------------- the clamps
def test_select_clamps_draws_outside_the_map(cuda, built_lib):
    case = _case("tile_V1025")
    n = case.grid.shape[0] * case.grid.shape[2]
    yidx_d = run_columns(cuda, case.grid, case.pow)[1]
    yidx = yidx_d[:n].cpu().numpy()
    planted = [((0, 0), -1, 0), ((0, 5), -2 ** 40, 0), ((0, 7), n, n - 1), ((0, 100), 2 ** 40, n - 1),
               ((1, 3), n, n - 1), ((1, 4), -1, 0), ((2, 1), -2 ** 40, 0), ((2, 2), 2 ** 40, n - 1)]
    outside, inside = case.draws.copy(), case.draws.copy()
    for at, bad, good in planted:
        outside[at], inside[at] = bad, good
    # with the case's seeds (cell 0 is near and kept, cell n - 1 is far) and with every draw of round 0 kept
    for c in (case, _far(case)):
        got = _select_equals_contract(cuda, c, yidx_d, yidx, outside, draws_ref=inside)
        want = _select_equals_contract(cuda, c, yidx_d, yidx, inside)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    # in the kept-all run the planted draws of round 0 are rows 0, 5, 7 and 100
    Z = case.grid.shape[2]
    world = pc.world_of(np.array([0, n - 1]), yidx, Z, case.res, case.corner)
    assert got[0][[0, 5]].tobytes() == world[[0, 0]].tobytes() and got[0][[7, 100]].tobytes() == world[[1, 1]].tobytes()


def test_select_clamps_yidx_outside_the_map(cuda, built_lib):
    case = _case("tile_V1025")
    X, Y, Z = case.grid.shape
    n = X * Z
    yidx_d = run_columns(cuda, case.grid, case.pow)[1]
    yidx = yidx_d[:n].cpu().numpy()
    # drawn cells: the near columns 0 and 1 and the first far draws of round 0
    far = [int(c) for c in dict.fromkeys(case.draws[0].tolist()) if c > 2][:6]
    low, high = [0] + far[:3], [1] + far[3:]
    assert all(c in case.draws[0] for c in low + high)
    outside, inside = yidx.copy(), yidx.copy()
    outside[low], inside[low] = -5, 0
    outside[high], inside[high] = Y + 3, Y - 1
    assert (inside != yidx).any()
    t = lambda a: torch.cat([torch.from_numpy(a).to(cuda), yidx_d[n:]])
    for c in (case, _far(case)):
        got = _select_equals_contract(cuda, c, t(outside), inside, case.draws)
        want = _select_equals_contract(cuda, c, t(inside), inside, case.draws)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    # in the kept-all run: the up coordinate and the scale row of a clamped draw are those of y = 0 and y = Y - 1
    rows = {c: case.draws[0].tolist().index(c) for c in low + high}
    for cells, y in ((low, 0), (high, Y - 1)):
        for c in cells:
            assert got[0][rows[c], 1] == np.float32(y) * np.float32(case.res) + case.corner[1]
            assert got[1][rows[c]].tobytes() == case.grid_scale[c // Z, y, c % Z].tobytes()


# ------------------------------------------------------------------------------------------------------- cloud ranges
def run_ranges(cuda, coords4, n_clouds, with_host=False):
    """cv_prop_cloud_ranges_i32 on torch's current stream into rows 1 .. n_clouds of a sentinel-filled [n_clouds + 2, 8]
    buffer -> the [n_clouds, 8] int32 rows; the guard row on either side must still hold the sentinel"""
    L = _lib.lib()
    c = torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(cuda)
    out = torch.full((n_clouds + 2, 8), -7, dtype=torch.int32, device=cuda)
    h_out = torch.full((n_clouds, 8), -9, dtype=torch.int32).pin_memory() if with_host else None
    _lib.check(L.cv_prop_cloud_ranges_i32(_lib.ptr(c), c.shape[0], n_clouds, _lib.ptr(out[1:]), _lib.ptr(h_out),
                                          _lib.stream(cuda)), "cv_prop_cloud_ranges_i32")
    torch.cuda.current_stream().synchronize()
    out = out.cpu().numpy()
    assert (out[0] == -7).all() and (out[-1] == -7).all()
    if with_host:
        assert np.array_equal(h_out.numpy(), out[1:-1])
    return out[1:-1]


def ranges_reference(coords4, n_clouds):
    """numpy on the same array: searchsorted on the batch column, min / max per slice, the documented row of an empty cloud"""
    coords4 = np.asarray(coords4, np.int32)
    edges = np.searchsorted(coords4[:, 0], np.arange(n_clouds + 1), side="left")
    out = np.empty((n_clouds, 8), np.int32)
    for b in range(n_clouds):
        rows = coords4[edges[b]:edges[b + 1], 1:]
        out[b, :2] = edges[b], edges[b + 1]
        out[b, 2:5] = rows.min(0) if len(rows) else I32_MAX
        out[b, 5:8] = rows.max(0) if len(rows) else I32_MIN
    return out


LO, HI = -32704, 32703                                      # the coordinate window of the quantiser


def _batch(sizes, ids=None, seed=81):
    rng = np.random.default_rng(seed)
    ids = range(len(sizes)) if ids is None else ids
    rows = [np.concatenate([np.full((m, 1), b), rng.integers(LO, HI + 1, (m, 3))], 1) for b, m in zip(ids, sizes)]
    return np.concatenate(rows).astype(np.int32)


def _sized_batch():
    """clouds of 1, 255, 256, 257, 513 and 4000 rows; both window edges, and extrema at the rows the strided read and the
    tree reach last: the last row of a cloud (lane 0's second or third trip) and lane 255's only row"""
    sizes = [1, 255, 256, 257, 513, 4000]
    c = _batch(sizes)
    first = np.cumsum([0] + sizes)
    c[first[0], 1:] = [LO, HI, -5]                           # the cloud of one row
    c[first[1]:first[2], 1] = np.clip(c[first[1]:first[2], 1], -1000, -3)      # all negative in x
    c[first[1] + 254, 1:] = [-1001, HI, LO]                  # lane 254, the last row of 255
    c[first[2] + 255, 1:] = [HI, LO, 7]                      # lane 255, the last row of 256
    c[first[3] + 255, 2] = HI                                # lane 255's only row of 257
    c[first[3] + 256, 1:] = [LO, 11, HI]                     # lane 0's second row, the last of 257
    c[first[4] + 512, 1:] = [HI, HI, LO]                     # lane 0's third row, the last of 513
    c[first[5] + 3999, 3] = LO
    c[first[5], 3] = HI
    return c, len(sizes)


RANGE_CASES = {
    "sizes": _sized_batch,
    "one_cloud": lambda: (_batch([1031], seed=82), 1),
    "300_clouds_of_3": lambda: (_batch([3] * 300, seed=83), 300),
    "gaps": lambda: (_batch([200, 257, 5], ids=[0, 2, 5], seed=84), 7),
}


@pytest.mark.parametrize("name", list(RANGE_CASES))
def test_cloud_ranges_equal_numpy(cuda, built_lib, name):
    coords4, n_clouds = RANGE_CASES[name]()
    assert coords4[:, 1:].min() >= LO and coords4[:, 1:].max() <= HI and (np.diff(coords4[:, 0]) >= 0).all()
    ref = ranges_reference(coords4, n_clouds)
    got = run_ranges(cuda, coords4, n_clouds, with_host=True)
    assert np.array_equal(got, ref)
    assert ref[0, 0] == 0 and ref[-1, 1] == len(coords4)
    if name == "sizes":
        assert (ref[:, 2:5].min(), ref[:, 5:8].max()) == (LO, HI) and ref[1, 5] < 0
    if name == "gaps":                                       # the documented row of a cloud without rows, 6 behind the last row
        for b, at in ((1, 200), (3, 457), (4, 457), (6, 462)):
            assert got[b].tolist() == [at, at] + [I32_MAX] * 3 + [I32_MIN] * 3


def test_cloud_ranges_same_bytes_on_every_run_and_stream(cuda, built_lib):
    coords4, n_clouds = _sized_batch()
    first = run_ranges(cuda, coords4, n_clouds).tobytes()
    again = run_ranges(cuda, coords4, n_clouds).tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run_ranges(cuda, coords4, n_clouds, with_host=True).tobytes()
    assert first == again == other


def test_cloud_corners_raises_on_an_empty_cloud_and_widens_x_and_z(cuda, built_lib):
    gaps, n_gaps = RANGE_CASES["gaps"]()
    good, n_good = _sized_batch()
    t = lambda a: torch.from_numpy(a).to(cuda).contiguous()
    q = 0.03
    with pytest.raises(RuntimeError, match="cloud 1 has no voxel"):
        proposals.cloud_corners(t(gaps), n_gaps, q)
    # the call behind the raise: the pool of page-locked landing buffers is intact
    ranges, corners = proposals.cloud_corners(t(good), n_good, q)
    ref = ranges_reference(good, n_good)
    assert ranges == [(int(r[0]), int(r[1])) for r in ref]
    plain = np.stack([ref[:, 2:5].astype(np.float32) * np.float32(q), ref[:, 5:8].astype(np.float32) * np.float32(q)], 1)
    assert plain.dtype == np.float32 and np.stack([c.numpy() for c in corners]).tobytes() == plain.tobytes()
    # border = 0.1 moves x and z of both corners by float32(0.1), and y not at all
    ranges_b, corners_b = proposals.cloud_corners(t(good), n_good, q, border=0.1)
    wide = plain.copy()
    wide[:, 0, [0, 2]] -= np.float32(0.1)
    wide[:, 1, [0, 2]] += np.float32(0.1)
    assert ranges_b == ranges and np.stack([c.numpy() for c in corners_b]).tobytes() == wide.tobytes()
    assert all(c.dtype == torch.float32 and c.shape == (2, 3) for c in corners_b)
    assert (wide[:, :, 1] == plain[:, :, 1]).all() and (wide[:, :, [0, 2]] != plain[:, :, [0, 2]]).all()
    # an empty cloud behind the last row raises as well
    with pytest.raises(RuntimeError, match="cloud 6 has no voxel"):
        proposals.cloud_corners(t(good), n_good + 1, q)


# ------------------------------------------------------------------------------------------------------- the reference's sizes
def _exact(values):
    """fp32 / fp64 values as exact integers in units of 2^-1074 (every finite one is a multiple of it)"""
    return [int(Fraction(float(v)) * (1 << 1074)) for v in values]


def test_production_sample_columns_and_both_select_modes(cuda, built_lib):
    """100 x 40 x 101 cells of 0.05 m, 1024 seeds, P = 512, S = 768: all three trips of the seed staging loop on every draw"""
    case = _case("production")
    X, Y, Z = case.grid.shape
    n = X * Z
    assert (case.grid.shape, len(case.seeds), case.S, case.P) == ((100, 40, 101), 1024, 768, 512)
    dist_d, yidx_d, cdf_d, flags = run_columns(cuda, case.grid, case.pow)
    _sync()
    dist, yidx, cdf = dist_d.cpu().numpy(), yidx_d.cpu().numpy(), cdf_d.cpu().numpy()
    assert (dist[n:] == np.float32(SENTINEL)).all() and (yidx[n:] == -7).all() and (cdf[n:] == SENTINEL).all()
    ref_dist, ref_yidx, _, uniform, _ = pc.columns_contract(case.grid, case.pow)
    assert not uniform and flags.cpu().numpy()[:2].tolist() == [0, 0]
    assert np.array_equal(yidx[:n], ref_yidx) and dist[:n].tobytes() == ref_dist.tobytes()
    # the prefix sums: non-decreasing and within n * 2^-53 * total of the exact ones (integers: fp32 values are dyadic)
    assert (np.diff(cdf[:n]) >= 0).all()
    prefix = list(accumulate(_exact(dist[:n])))
    err = max(abs(a - b) for a, b in zip(_exact(cdf[:n]), prefix))
    print("cdf error %.3g of bound %.3g" % (err / (1 << 1074), n * prefix[-1] / (1 << 1127)))
    assert err * 2 ** 53 <= n * prefix[-1]
    # draws mode against the contract on the device's own yidx
    _, _, info = _select_equals_contract(cuda, case, yidx_d, yidx[:n], case.draws)
    assert info[0] == case.P
    # uniform mode: 0, the largest fp32 below 1, one ulp either side of three cdf steps, random ones
    rng = np.random.default_rng(91)
    c64 = cdf[:n]
    us = [0.0, 0.99999994]
    for step in (0, n // 2, n - 2):
        centre = np.float32(c64[step] / c64[-1])
        us += [float(np.nextafter(centre, np.float32(0))), float(centre), float(np.nextafter(centre, np.float32(1)))]
    us = np.array(us, np.float32)
    assert ((us >= 0) & (us < 1)).all()
    us = np.concatenate([us, rng.random(case.S - len(us), dtype=np.float32)])[None]
    cells = _cells_of(cuda, case, yidx_d, cdf_d, us)
    assert np.array_equal(cells, pc.cell_of_uniform(us[0], c64))
    for c, u in zip(cells, us[0]):
        assert cell_in_bracket(int(c), u, dist[:n]), (c, u)
    assert cells[0] == 0 and cells[1] == n - 1


# (scene seed, draw seed): on the CPU oracle's grid every evaluated draw is > 5e-3 clear of the 0.3 m radius and the argmax over
# the up axis of every drawn column leads by > 1e-3 of its value; (6, 6) needs two trips
PRODUCTION_SEEDS = [(5, 28), (6, 6), (7, 20)]


@pytest.mark.parametrize("seed,draw_seed", PRODUCTION_SEEDS)
def test_propose_with_1024_votes_and_512_proposals(cuda, built_lib, seed, draw_seed):
    sc, pts, xyz, scale, prob, corners, _, t = _scene(cuda, seed)
    rng = np.random.default_rng(1000 + seed)
    votes = (pts[rng.choice(len(pts), 1024, replace=False)] + rng.normal(0, 0.05, (1024, 3))).astype(np.float32)
    hv = HoughVotingModule(res=0.05, nms_size=0.3, thresh=0, num_proposal=512, num_rots=60)
    assert hv.per_round == 768
    grid_obj, grid_scale = _gpu_grids(hv, t, pts, xyz, scale, prob, corners)
    draws = _numpy_draws(draw_seed, grid_obj.shape[0] * grid_obj.shape[2], S=768)
    ref_c, ref_s, _, used = po.sample_proposals(grid_obj, grid_scale, corners[0], 0.05, votes, draws, 512)
    margin = _margin(grid_obj, corners, votes, draws[:used])
    print("seed %d / %d: %d trips, nearest-seed margin %.3g" % (seed, draw_seed, used, margin))
    assert margin > 1e-3                                     # the case condition, on the GPU's own grids
    cand, probs, scales = hv.propose(t(pts), t(xyz), t(scale), t(prob), torch.from_numpy(corners), t(votes), draws=draws)
    assert cand.shape == (512, 3) and scales.shape == (512, 3) and probs.shape == (512,) and float(probs.abs().max()) == 0.0
    assert hv.last_rounds_used == [used]
    assert cand.cpu().numpy().tobytes() == ref_c.tobytes() and scales.cpu().numpy().tobytes() == ref_s.tobytes()
