"""The device proposal sampler without a GPU: the C ABI surface and its host-side validation, the SUN RGB-D caller's
imports, and the contract itself - a numpy restatement of cv_prop_select_f32 in the kernel's precision against the fp64
oracle on every hand-made case, the case conditions that make that comparison decidable, and eight named wrong results."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from oracle import proposal_oracle as po
from canonicalvoting_amd import _lib
from tests import proposal_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT_CASES = pc.select_cases()


def test_symbols_exported_and_abi_version_unchanged(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ("cv_prop_columns_f32", "cv_prop_select_f32", "cv_prop_workspace_bytes", "cv_prop_cloud_ranges_i32"):
        assert hasattr(L, name), "libcvhip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "cv_hip.h")).read()
    header_version = int(re.search(r"#define\s+CV_ABI_VERSION\s+(\d+)", header).group(1))
    assert _lib.lib().cv_abi_version() == header_version == _lib.ABI_VERSION == 6       # the change only adds symbols
    assert _lib.lib().cv_sizeof_prop_select_desc() == ctypes.sizeof(_lib.PropSelectDesc)
    assert _lib.lib().cv_prop_workspace_bytes(1536) >= 1536 * 4 and _lib.lib().cv_prop_workspace_bytes(0) == 0


def test_reference_caller_imports():
    """utils/minkunet.py:30 of the reference, the import the SUN RGB-D caller reaches through its model file"""
    from MinkowskiEngine.modules.resnet_block import BasicBlock, Bottleneck
    assert BasicBlock.expansion == 1 and Bottleneck.expansion == 4


def _fake(n=1):
    """a non-NULL address that is never dereferenced: validation fails before the first device call"""
    return ctypes.c_void_p(0x1000 * n)


def _valid_desc():
    d = _lib.PropSelectDesc()
    d.d_grid_scale, d.d_yidx, d.d_cdf, d.d_seeds = _fake(1), _fake(2), _fake(3), _fake(4)
    d.d_cand, d.d_scale, d.d_info, d.d_ws = _fake(5), _fake(6), _fake(7), _fake(8)
    d.dims = (ctypes.c_int * 3)(4, 3, 5)
    d.res, d.radius, d.n_seeds = 0.05, 0.3, 7
    d.d_draws = _fake(9)
    d.rounds, d.per_round, d.num_proposal, d.start, d.ws_bytes = 2, 3, 2, 0, 4096
    return d


def test_entry_points_validate_on_the_host(built_lib):
    L = _lib.lib()
    EINVAL = -22
    dims = (ctypes.c_int * 3)(4, 3, 5)
    args = [_fake(1), dims, 0.5, _fake(2), _fake(3), _fake(4), _fake(5), None]
    for null_at in (0, 1, 3, 4, 5, 6):
        a = list(args)
        a[null_at] = None
        assert L.cv_prop_columns_f32(*a) == EINVAL and b"null" in L.cv_last_error()
    for bad in ((0, 3, 5), (4, -1, 5), (4, 3, 0), (1 << 16, 1, 1 << 16)):
        a = list(args)
        a[1] = (ctypes.c_int * 3)(*bad)
        assert L.cv_prop_columns_f32(*a) == EINVAL and b"dims" in L.cv_last_error()
    a = list(args)
    a[2] = float("nan")
    assert L.cv_prop_columns_f32(*a) == EINVAL

    assert L.cv_prop_select_f32(None, None) == EINVAL and b"null" in L.cv_last_error()
    for field in ("d_grid_scale", "d_yidx", "d_seeds", "d_cand", "d_scale", "d_info"):
        d = _valid_desc()
        setattr(d, field, None)
        assert L.cv_prop_select_f32(ctypes.byref(d), None) == EINVAL and b"null" in L.cv_last_error(), field

    def rejected(word, **fields):
        d = _valid_desc()
        for k, v in fields.items():
            setattr(d, k, v)
        rc = L.cv_prop_select_f32(ctypes.byref(d), None)
        assert rc == EINVAL and word in L.cv_last_error(), (fields, rc, L.cv_last_error())

    rejected(b"dims", dims=(ctypes.c_int * 3)(4, 0, 5))
    rejected(b"dims", dims=(ctypes.c_int * 3)(-4, 3, 5))
    rejected(b"both", d_uniform=_fake(10))                          # draws and uniforms
    rejected(b"neither", d_draws=None)
    rejected(b"d_cdf", d_draws=None, d_uniform=_fake(10), d_cdf=None)   # uniform mode reads the prefix sums
    rejected(b"start", start=3)                                     # start > num_proposal
    rejected(b"start", start=-1)
    rejected(b"start", num_proposal=0)
    rejected(b"rounds", rounds=0)
    rejected(b"rounds", per_round=0)
    rejected(b"seeds", n_seeds=0)
    d = _valid_desc()
    d.ws_bytes = 0
    assert L.cv_prop_select_f32(ctypes.byref(d), None) == -12 and b"workspace" in L.cv_last_error()

    assert L.cv_prop_cloud_ranges_i32(None, 5, 1, _fake(1), None, None) == EINVAL
    assert L.cv_prop_cloud_ranges_i32(_fake(1), 0, 1, _fake(2), None, None) == EINVAL
    assert L.cv_prop_cloud_ranges_i32(_fake(1), 5, 0, _fake(2), None, None) == EINVAL


def _oracle(case, draws=None):
    return po.sample_proposals(case.grid, case.grid_scale, case.corner, case.res, case.seeds,
                               list(case.draws if draws is None else draws), case.P, pow=case.pow)


@pytest.mark.parametrize("case", SELECT_CASES, ids=repr)
def test_case_condition_every_draw_is_decidable(case):
    """|nearest seed distance - 0.3| > 1e-5 in fp64 for every draw: more than 50 x the fp32 evaluation error of a distance
    below 0.5 m, and beyond that only the nearest seed matters - so `near` is the same in fp32 and fp64"""
    assert pc.case_margin(case) > 1e-5


@pytest.mark.parametrize("case", SELECT_CASES, ids=repr)
def test_numpy_contract_equals_the_oracle(case):
    dist, yidx, _, uniform, _ = pc.columns_contract(case.grid, case.pow)
    cand, scale, filled, used = pc.select_contract(yidx, case.grid_scale, case.corner, case.res, case.seeds, case.draws, case.P)
    ref_c, ref_s, ref_dist, ref_used = _oracle(case)
    assert filled == case.P and used == ref_used
    assert cand.tobytes() == ref_c.astype(np.float32).tobytes() and scale.tobytes() == ref_s.astype(np.float32).tobytes()
    assert uniform == bool(np.all(ref_dist == 1.0))
    if not uniform:                                                 # (the oracle raises in fp32, the contract in fp64: 1 ulp)
        np.testing.assert_allclose(dist, ref_dist, rtol=2.0 ** -22)


def _case(name):
    return next(c for c in SELECT_CASES if c.name == name)


def test_short_budget_and_continuation_in_the_contract():
    case = _case("short")
    _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
    a = (case.grid_scale, case.corner, case.res, case.seeds)
    c1, s1, filled, used = pc.select_contract(yidx, *a, case.draws[:2], case.P)
    assert filled == 20 and used == 2 and np.isnan(c1[20:]).all()
    c2, s2, filled2, used2 = pc.select_contract(yidx, *a, case.draws[2:], case.P, start=filled, rows=(c1, s1))
    ref_c, ref_s, _, ref_used = _oracle(case)
    assert filled2 == case.P and used + used2 == ref_used == 5
    assert c2.tobytes() == ref_c.tobytes() and s2.tobytes() == ref_s.tobytes()


def test_scripted_rounds_do_what_their_names_say():
    for name, used in (("mid_round", 2), ("round_end", 2), ("no_near_round", 2), ("no_near_first", 1), ("chunks", 3)):
        assert _oracle(_case(name))[3] == used, name


def test_named_wrong_results_are_outside_the_contract():
    # 1. last instead of first argmax: the column of ties
    case = _case("grid_ties")
    _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
    Y = case.grid.shape[1]
    last = (Y - 1 - case.grid[:, ::-1, :].argmax(1)).reshape(-1).astype(np.int32)
    assert (last != yidx).any()
    ties = np.flatnonzero(last != yidx)
    draws = case.draws.copy()
    draws[0, :len(ties)] = ties                                     # make sure the tied columns are drawn
    ref_c = _oracle(case, draws)[0]
    a = (case.grid_scale, case.corner, case.res, case.seeds, draws, case.P)
    assert pc.select_contract(yidx, *a)[0].tobytes() == ref_c.tobytes()
    assert pc.select_contract(last, *a)[0].tobytes() != ref_c.tobytes()
    # 2. fused multiply-add in `world`: one rounding instead of two moves some coordinate of some case
    moved = 0
    for case in SELECT_CASES[:10]:
        _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
        a = (case.grid_scale, case.corner, case.res, case.seeds, case.draws, case.P)
        moved += pc.select_contract(yidx, *a, wrong="fused_world")[0].tobytes() != _oracle(case)[0].tobytes()
    assert moved >= 5
    # 3. keeping nothing when no draw is near; 4. not truncating at P
    case = _case("no_near_round")
    _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
    a = (case.grid_scale, case.corner, case.res, case.seeds, case.draws, case.P)
    ref_c, _, _, ref_used = _oracle(case)
    wrong_c, _, _, wrong_used = pc.select_contract(yidx, *a, wrong="keep_nothing")
    assert wrong_used != ref_used and wrong_c.tobytes() != ref_c.tobytes()
    assert pc.select_contract(yidx, *a, wrong="no_truncation")[0].shape[0] > case.P == ref_c.shape[0]
    # 5. an off-by-one cell at u -> 1
    dist = pc.columns_contract(pc.distinct_grid(np.random.default_rng(3), (3, 2, 5)), 0.5)[0]
    cdf = np.cumsum(dist.astype(np.float64))
    u = np.float32(0.99999994)
    assert cell_in_bracket(pc.cell_of_uniform(u, cdf), u, dist)
    assert not cell_in_bracket(pc.cell_of_uniform(u, cdf, wrong="off_by_one"), u, dist)
    # 6. - 8. a seed list read in part: the first trip of the staging loop (341 seeds), the first tile (1024), two tiles
    # (2048).  Every seed-tile case rejects each one that is shorter than its list.
    applied = {w: 0 for w in pc.SEED_CUTS}
    for case in TILE_CASES:
        _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
        a = (case.grid_scale, case.corner, case.res, case.seeds, case.draws, case.P)
        ref_c, ref_s, _, _ = _oracle(case)
        assert pc.select_contract(yidx, *a)[0].tobytes() == ref_c.tobytes()
        for w, cut in pc.SEED_CUTS.items():
            if len(case.seeds) > cut:
                wrong_c, wrong_s, _, _ = pc.select_contract(yidx, *a, wrong=w)
                assert wrong_c.tobytes() != ref_c.tobytes() and wrong_s.tobytes() != ref_s.tobytes(), (case, w)
                applied[w] += 1
    assert applied == {"first_trip_only": 8, "first_tile_only": 4, "second_tile_short": 3}


TILE_CASES = [c for c in SELECT_CASES if c.name.startswith("tile_")]


def test_seed_tile_cases_are_what_their_table_says():
    """every V of the table and the long-round case; the near seeds at the listed positions and nowhere else; all three
    rounds evaluated, so the tile loop is walked with a full budget; the nearest-seed margin of the layout is the radius"""
    assert [len(c.seeds) for c in TILE_CASES] == list(pc.TILE_SEEDS) + [2049]
    assert [(c.S, c.P) for c in TILE_CASES] == [(192, 128)] * 7 + [(1536, 1024)]
    for case in TILE_CASES:
        near_at = pc.TILE_SEEDS[len(case.seeds)]
        assert np.flatnonzero((case.seeds != 100.0).any(1)).tolist() == list(near_at)
        assert case.grid.shape == (32, 5, 33) and case.res == 1.0 and _oracle(case)[3] == 3 == len(case.draws)
        assert abs(pc.case_margin(case) - 0.3) < 1e-6


@pytest.mark.parametrize("at", [1024, 3])
def test_nan_seed_in_the_contract_keeps_every_draw(at):
    """a NaN wins the minimum: no draw is near, every round keeps all its draws; +Inf neither wins nor poisons it"""
    case = _case("tile_V1025")
    _, yidx, _, _, _ = pc.columns_contract(case.grid, case.pow)
    Z = case.grid.shape[2]
    seeds = case.seeds.copy()
    seeds[at] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.isnan(pc.nearest_f32(pc.world_of(case.draws[0], yidx, Z, case.res, case.corner), seeds)).all()
        cand, _, filled, used = pc.select_contract(yidx, case.grid_scale, case.corner, case.res, seeds, case.draws, 300)
    assert (filled, used) == (300, 2)
    assert cand.tobytes() == pc.world_of(case.draws.reshape(-1)[:300], yidx, Z, case.res, case.corner).tobytes()
    seeds[at] = np.inf
    a = (yidx, case.grid_scale, case.corner, case.res)
    with_inf = pc.select_contract(*a, seeds, case.draws, case.P)
    without = pc.select_contract(*a, np.delete(case.seeds, at, 0), case.draws, case.P)
    assert with_inf[0].tobytes() == without[0].tobytes() and with_inf[1].tobytes() == without[1].tobytes()
    assert with_inf[2:] == without[2:] and with_inf[3] == 3


def cell_in_bracket(c, u, dist):
    """fsum(dist[:c]) - tol <= u * total <= fsum(dist[:c+1]) + tol with tol = n * 2^-52 * total, for a cell inside the map"""
    n = len(dist)
    if not 0 <= c < n:
        return False
    d = dist.astype(np.float64)
    total = math.fsum(d)
    tol = n * 2.0 ** -52 * total
    t = float(np.float32(u)) * total
    return math.fsum(d[:c]) - tol <= t <= math.fsum(d[:c + 1]) + tol
