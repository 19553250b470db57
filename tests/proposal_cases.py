"""Hand-made cases for the device proposal sampler (cv_prop_columns_f32 / cv_prop_select_f32), numpy only and without a vote:
grids, scale grids, seeds and draws from seeded generators, plus a numpy restatement of the contract of include/cv_hip.h in
the kernel's own precision.  Shared by tests/test_proposals_device.py (CPU: the restatement against the oracle, the case
conditions), tests/test_proposals_device_gpu.py (the kernels against the oracle) and tests/test_proposals_edges_gpu.py."""
import math

import numpy as np

F32 = np.float32
RADIUS = 0.3
SHAPES = [(1, 1, 1), (3, 2, 5), (16, 7, 16), (17, 3, 15), (1, 4, 257), (32, 5, 33)]
# seed counts either side of the constants the select kernel has, or had: 256 was its lane count when the seeds were staged
# one per lane (SEED_COUNTS, the random and scripted cases), and today it stages SEED_TILE = 1024 seeds (3072 words) per LDS
# tile with 1024 lanes, so the staging loop takes its second trip at 342 seeds and its third at 683, and a second tile
# starts at seed 1024 (TILE_SEEDS, the seed-tile cases)
SEED_COUNTS = [1, 255, 256, 257]
# V -> positions of the near seeds in the seed list, on both sides of 341 | 342, 682 | 683, 1023 | 1024 and 2047 | 2048
TILE_SEEDS = {342: (0, 340, 341), 683: (341, 342, 682), 1023: (0, 682, 1022), 1024: (682, 683, 1023), 1025: (683, 1023, 1024),
              2049: (1024, 1025, 2047, 2048), 3000: (2047, 2048, 2999)}
# the named wrong results that read only a part of the seed list: the first trip of the staging loop, the first tile, two tiles
SEED_CUTS = {"first_trip_only": 341, "first_tile_only": 1024, "second_tile_short": 2048}
PRODUCTION_SEED = 5                                           # (case_margin of the draws it gives: 3e-4)
BUDGETS = [(1, 1), (3, 2), (192, 128), (1536, 1024)]          # (per_round S, num_proposal P), S = int(1.5 P)


class Case:
    """one select case: grid [X,Y,Z], grid_scale [X,Y,Z,3], corner [3], res, seeds [V,3], draws [rounds][S], P, pow"""

    def __init__(self, name, grid, grid_scale, corner, res, seeds, draws, P, pow=0.5):
        self.name, self.grid, self.grid_scale = name, np.ascontiguousarray(grid, F32), np.ascontiguousarray(grid_scale, F32)
        self.corner, self.res, self.seeds = np.asarray(corner, F32), float(F32(res)), np.ascontiguousarray(seeds, F32)
        self.draws, self.P, self.pow = np.ascontiguousarray(draws, np.int64), int(P), pow
        self.S = self.draws.shape[1]

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------- grids for the column pass
def distinct_grid(rng, shape):
    """distinct random fp32 values in [0, 4)"""
    n = int(np.prod(shape))
    return (rng.permutation(n).astype(F32) * F32(4.0 / n)).reshape(shape)


def column_cases():
    """(name, grid, pow, expect uniform, expect non-finite) for cv_prop_columns_f32"""
    rng = np.random.default_rng(7)
    out = []
    for shape in SHAPES:
        out.append(("distinct%s" % (shape,), distinct_grid(rng, shape), 0.5, False, False))
    out.append(("distinct_pow2", distinct_grid(rng, (17, 3, 15)), 2.0, False, False))
    out.append(("distinct_pow0.3", distinct_grid(rng, (16, 7, 16)), 0.3, False, False))
    ties = distinct_grid(rng, (3, 4, 5))
    ties[1, :, 2] = F32(9.0)                                   # a column of ties: the first wins
    ties[2, 1:3, 0] = F32(8.0)
    out.append(("ties", ties, 0.5, False, False))
    out.append(("all_equal", np.full((3, 2, 5), 0.25, F32), 0.5, False, False))
    nan = distinct_grid(rng, (16, 7, 16))
    nan[5, 3, 9] = np.nan
    nan[5, 5, 9] = np.nan                                      # the first NaN of the column wins
    out.append(("nan_cell", nan, 0.5, True, True))
    inf = distinct_grid(rng, (17, 3, 15))
    inf[16, 2, 14] = np.inf
    out.append(("inf_cell", inf, 0.5, True, True))
    out.append(("zeros_pow2", np.zeros((16, 7, 16), F32), 2.0, True, False))      # sum = 256e-14 < 1e-7: uniform
    out.append(("zeros_pow0.5", np.zeros((16, 7, 16), F32), 0.5, False, False))   # sum = 256 * 3.2e-4: not uniform
    return out


def columns_contract(grid, pow):
    """(dist [X*Z] f32 after the uniform overwrite, yidx [X*Z] i32, raw dist, uniform taken, non-finite seen)"""
    grid = np.asarray(grid, F32)
    m = grid.max(1)                                            # NaN propagates
    yidx = grid.argmax(1).astype(np.int32)                     # the first maximum, the first NaN when there is one
    b = (m + F32(1e-7)).astype(F32)
    with np.errstate(invalid="ignore"):
        raw = (np.sqrt(b.astype(np.float64)) if pow == 0.5 else np.power(b.astype(np.float64), float(pow))).astype(F32).reshape(-1)
    nonfinite = not np.all(np.isfinite(raw))
    uniform = nonfinite or math.fsum(raw.astype(np.float64)) < float(F32(1e-7))
    return (np.ones_like(raw) if uniform else raw), yidx.reshape(-1), raw, uniform, nonfinite


# ---------------------------------------------------------------------------------------------- the select contract in numpy
def world_of(cells, yidx, Z, res, corner, fused=False):
    ix, iz = cells // Z, cells % Z
    idx = np.stack([ix, yidx[cells], iz], -1)
    if fused:                                                  # a WRONG result: one rounding instead of two
        return (idx.astype(np.float64) * float(F32(res)) + np.asarray(corner, np.float64)).astype(F32)
    return (idx.astype(F32) * F32(res)).astype(F32) + np.asarray(corner, F32)


def nearest_f32(world, seeds):
    """sqrtf of the fp32 minimum of ((dx*dx + dy*dy) + dz*dz)"""
    d = world[:, None, :].astype(F32) - np.asarray(seeds, F32)[None]
    d2 = ((d[..., 0] * d[..., 0]).astype(F32) + (d[..., 1] * d[..., 1]).astype(F32)).astype(F32) + (d[..., 2] * d[..., 2]).astype(F32)
    return np.sqrt(d2.astype(F32).min(1)).astype(F32)


def nearest_f64(world, seeds):
    d = world[:, None, :].astype(np.float64) - np.asarray(seeds, np.float64)[None]
    return np.sqrt((d ** 2).sum(-1)).min(1)


def select_contract(yidx, grid_scale, corner, res, seeds, draws, P, start=0, rows=None, wrong=None):
    """cv_prop_select_f32 in draws mode: (cand [P,3], scale [P,3], filled, rounds_used); rows beyond ``filled`` keep what
    ``rows`` = (cand, scale) held (NaN without).  wrong: one of the named wrong results ("fused_world", "keep_nothing",
    "no_truncation", the seed-list cuts of SEED_CUTS; "last_argmax" is a wrong yidx and lives in the caller)."""
    X, Y, Z = grid_scale.shape[:3]
    if wrong in SEED_CUTS:                                     # a WRONG result: only the front of the seed list is read
        seeds = seeds[:SEED_CUTS[wrong]]
    cand = np.full((P, 3), np.nan, F32) if rows is None else rows[0].copy()
    scale = np.full((P, 3), np.nan, F32) if rows is None else rows[1].copy()
    got_c, got_s = [cand[:start]], [scale[:start]]
    filled, used = start, 0
    for s in np.asarray(draws, np.int64):
        if filled >= P:
            break
        used += 1
        s = np.clip(s, 0, X * Z - 1)
        world = world_of(s, yidx, Z, res, corner, fused=wrong == "fused_world")
        sc = grid_scale[s // Z, yidx[s], s % Z, :]
        near = nearest_f32(world, seeds) < F32(RADIUS)
        keep = near if (near.any() or wrong == "keep_nothing") else np.ones_like(near)
        got_c.append(world[keep]); got_s.append(sc[keep])
        filled += int(keep.sum())
    all_c, all_s = np.concatenate(got_c), np.concatenate(got_s)
    if wrong == "no_truncation":
        return all_c, all_s, filled, used
    filled = min(filled, P)
    cand[:filled], scale[:filled] = all_c[:filled], all_s[:filled]
    return cand, scale, filled, used


def cell_of_uniform(u, cdf, wrong=None):
    """uniform mode: t = u * cdf[last] in fp64, the first cell whose cdf exceeds t, the last cell when none does"""
    t = np.asarray(u, F32).astype(np.float64) * cdf[-1]
    c = np.searchsorted(cdf, t, side="right")
    if wrong == "off_by_one":                                  # a WRONG result: the cell behind, unclamped
        return c + 1
    return np.minimum(c, len(cdf) - 1)


# ---------------------------------------------------------------------------------------------- select cases
def _random_case(rng, name, shape, V, S, P, rounds, res, pow=0.5, grid=None):
    X, Y, Z = shape
    grid = distinct_grid(rng, shape) if grid is None else grid
    gs = rng.uniform(0.1, 2.0, shape + (3,)).astype(F32)
    corner = rng.uniform(-2, 2, 3).astype(F32)
    ext = np.array(shape, np.float64) * res
    seeds = (corner + rng.uniform(0, 1, (V, 3)) * ext).astype(F32)
    # as many rounds as the walk needs (at most `rounds`) and one more, which must stay unevaluated
    draws = rng.integers(0, X * Z, (rounds, S))
    yidx = columns_contract(grid, pow)[1]
    filled, used = select_contract(yidx, gs, corner, res, seeds, draws, P)[2:]
    assert filled == P, "case %s: %d rounds do not fill %d proposals" % (name, rounds, P)
    return Case(name, grid, gs, corner, res, seeds, draws[:used + 1], P, pow)


def _layout(rng, shape, V, res=1.0, near_at=None):
    """a grid whose columns with flat index below n / 2 are near (a seed sits on their cell) and the others at least `res`
    = 1 m away from every seed; seeds beyond the near columns are 100 m away.  near_at: the positions in the seed list of
    the near seeds (the seed at near_at[j] sits on column j, every other seed is 100 m away); the front of the list without"""
    X, Y, Z = shape
    n = X * Z
    grid = distinct_grid(rng, shape)
    gs = rng.uniform(0.1, 2.0, shape + (3,)).astype(F32)
    corner = np.array([0.5, -1.0, 2.0], F32)
    yidx = grid.argmax(1).reshape(-1)
    near_cells = np.arange(min(n // 2, V) if near_at is None else len(near_at))
    seeds = np.full((V, 3), 100.0, F32)
    seeds[np.arange(len(near_cells)) if near_at is None else np.asarray(near_at)] = world_of(near_cells, yidx, Z, res, corner)
    return grid, gs, corner, seeds, len(near_cells), n


def _scripted(rng, name, shape, V, S, P, near_counts, res=1.0, near_at=None):
    """draws with exactly near_counts[r] near draws in round r, at random places of the round"""
    grid, gs, corner, seeds, n_near, n = _layout(rng, shape, V, res, near_at)
    draws = np.empty((len(near_counts), S), np.int64)
    for r, k in enumerate(near_counts):
        row = rng.integers(n_near, n, S)                       # far columns
        row[rng.choice(S, k, replace=False)] = rng.integers(0, n_near, k)
        draws[r] = row
    return Case(name, grid, gs, corner, res, seeds, draws, P)


def select_cases():
    rng = np.random.default_rng(11)
    out = []
    # every shape, cycling the seed counts and budgets; res chosen so that a good part of the map is beyond the radius
    for i, shape in enumerate(SHAPES):
        V = SEED_COUNTS[i % 4]
        S, P = BUDGETS[i % 4]
        out.append(_random_case(rng, "random%s_V%d_P%d" % (shape, V, P), shape, V, S, P, 64, res=0.23))
    for j, (S, P) in enumerate(BUDGETS):
        V = SEED_COUNTS[(j + 2) % 4]
        out.append(_random_case(rng, "budget_S%d_P%d_V%d" % (S, P, V), (32, 5, 33), V, S, P, 64, res=0.2))
    out.append(_random_case(rng, "pow2", (17, 3, 15), 257, 192, 128, 64, res=0.3, pow=2.0))
    # scripted rounds on the 16 x 7 x 16 map (128 near columns), S = 192, P = 128
    out.append(_scripted(rng, "mid_round", (16, 7, 16), 256, 192, 128, [100, 60, 50]))       # P reached inside round 2
    out.append(_scripted(rng, "round_end", (16, 7, 16), 255, 192, 128, [100, 28, 50]))       # exactly at the end of round 2
    out.append(_scripted(rng, "no_near_round", (16, 7, 16), 257, 192, 128, [10, 0, 50]))     # round 2 keeps all its draws
    out.append(_scripted(rng, "no_near_first", (16, 7, 16), 1, 192, 128, [0, 5]))
    out.append(_scripted(rng, "short", (16, 7, 16), 256, 192, 128, [10, 10, 40, 40, 40, 40]))  # two rounds leave 20 rows
    out.append(_scripted(rng, "chunks", (32, 5, 33), 257, 1536, 1024, [500, 300, 400]))      # rounds longer than the workgroup
    # draws on the special grids of the column pass
    for name, grid, pow, _, _ in column_cases():
        if name in ("ties", "all_equal", "nan_cell", "inf_cell", "zeros_pow2", "zeros_pow0.5"):
            shape = grid.shape
            out.append(_random_case(rng, "grid_" + name, shape, 255, 192, 128, 64, res=0.23, pow=pow, grid=grid))
    # (generators of their own from here on: the cases above keep their bytes)
    # seed tiles: a few near seeds at the list positions of TILE_SEEDS, three rounds of 60 near draws each (P inside round 3)
    rng = np.random.default_rng(12)
    for V, near_at in TILE_SEEDS.items():
        out.append(_scripted(rng, "tile_V%d" % V, (32, 5, 33), V, 192, 128, [60, 60, 60], near_at=near_at))
    # rounds longer than the workgroup over two tiles and a seed: a lane without a draw in the last chunk still stages seeds
    out.append(_scripted(rng, "tile_chunks_V2049", (32, 5, 33), 2049, 1536, 1024, [500, 300, 400], near_at=TILE_SEEDS[2049]))
    # the reference's own sizes (BRNet: 1024 vote points per sample, num_proposal = 512) on a 5 m x 2 m x 5 m map
    out.append(_random_case(np.random.default_rng(PRODUCTION_SEED), "production", (100, 40, 101), 1024, 768, 512, 64, res=0.05))
    return out


def case_margin(case):
    """min over every draw of |nearest seed distance in fp64 - 0.3| (the case condition: > 1e-5)"""
    _, yidx, _, _, _ = columns_contract(case.grid, case.pow)
    Z = case.grid.shape[2]
    cells = np.unique(case.draws.reshape(-1))
    return float(np.abs(nearest_f64(world_of(cells, yidx, Z, case.res, case.corner), case.seeds) - RADIUS).min())
