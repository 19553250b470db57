"""CPU pin of the float64 vote-backward oracle and its per-element bound (oracle/hv_numpy.py hv_backward64,
VOTE_BWD_ERROR_MODEL) that tests/test_vote_backward_gpu.py holds hv_bwd to, and of the geometry its cases and those of
tests/test_vote_corners_gpu.py are built for.

  - the fp32-sequential C oracle (oracle.hv_backward) is inside the bound on every element, at every trip count of the
    kernel's lane loop and with the grid given by a box larger than the cloud and by one that cuts it
  - hv_backward64 itself against float64 autograd of an independent restatement of grid_obj, on the cut box
  - five named wrong results, built from the oracle's own per-vote terms, are >= 10 x outside the bound; the bar the suite
    held the backward to before (1e-4 of the largest element of the output) accepts hundreds of their wrong elements"""
import functools

import numpy as np
import pytest

import oracle
from oracle import hv_numpy
from canonicalvoting_amd.synth import make_scene, synth_predictions

OLD_RTOL = 1e-4      # tests/test_vote_gpu.py: atol = RTOL * max(1, max |ref|), rtol = RTOL
NAMES = ("d_xyz", "d_scale", "d_obj")


@functools.lru_cache(maxsize=None)
def scene():
    """the scene of tests/test_vote_gpu.py::test_backward_through_autograd"""
    sc = make_scene(5, n_points=1500, res=0.06, room=(1.5, 0.9, 1.5), n_boxes=2, margin=0.5, box_scale=0.4)
    xyz, scale, prob, _ = synth_predictions(sc)
    return sc.points, xyz, scale, prob, sc.res


def box_of(kind, pts, res):
    """(corner, dims) of the grid: the cloud's own box, one larger than the cloud, one that cuts it"""
    mn, mx = pts.min(0), pts.max(0)
    if kind == "own":
        corner, _, dims = oracle.grid_geometry(pts, res)
        return corner, dims
    ext = mx - mn
    lo, hi = (mn - 0.2, mx + 0.3) if kind == "big" else (mn + 0.3 * ext, mx - 0.25 * ext)
    lo, hi = lo.astype(np.float32), hi.astype(np.float32)
    dims = [int(np.float32(np.float32(hi[k] - lo[k]) / np.float32(res))) + 1 for k in range(3)]
    return lo, dims


CASES = [(R, "own") for R in (1, 7, 36, 64, 65, 120, 129, 256)] + [(60, "big"), (60, "cut")]


@functools.lru_cache(maxsize=None)
def case(R, kind, dims=None):
    pts, xyz, scale, prob, res = scene()
    corner, bdims = box_of(kind, pts, res)
    dims = list(dims or bdims)
    grad = np.random.default_rng(0).normal(0, 1, tuple(dims)).astype(np.float32)
    return grad, corner, dims


def ratios(got, ref):
    """worst |got - ref| / bound per output, and the assertion that rows without a vote are exact zeros"""
    bounds = hv_numpy.vote_bwd_bounds(ref)
    none = ref["votes"] == 0
    out = {}
    for name, g in zip(NAMES, got):
        g = np.asarray(g)
        assert g.dtype == np.float32 and np.isfinite(g).all(), name
        assert not g[none].any(), name + ": a point without a vote in bounds has a gradient"
        out[name] = float((np.abs(g.astype(np.float64) - ref[name]) / bounds[name]).max())
    return out


def old_bar_passes(got, ref32):
    """the bar of test_forward_backward_match_golden / test_backward_through_autograd"""
    return all(bool(np.all(np.abs(g - r) <= OLD_RTOL * max(1.0, float(np.abs(r).max())) + OLD_RTOL * np.abs(r)))
               for g, r in zip(got, ref32))


@pytest.mark.parametrize("R,kind", CASES)
def test_c_oracle_is_inside_the_bound(R, kind):
    """fp32, sequential: the ratios are recorded in LABNOTES.md (worst 0.30, at R = 1 and in the cut box)"""
    pts, xyz, scale, prob, res = scene()
    grad, corner, dims = case(R, kind)
    ref = hv_numpy.hv_backward64(grad, pts, xyz, scale, prob, res, R, corner)
    got = oracle.hv_backward(grad, pts, xyz, scale, prob, res, R, corner=None if kind == "own" else corner)
    r = ratios(got, ref)
    print("R %d %s box: votes %d, points without %d, worst ratio %s" % (
        R, kind, int(ref["votes"].sum()), int((ref["votes"] == 0).sum()), r))
    assert max(r.values()) <= 1.0, r
    assert ref["votes"].max() <= R and ref["votes"].sum() > 0
    if kind == "own":
        assert np.array_equal(oracle.hv_backward(grad, pts, xyz, scale, prob, res, R, corner=corner)[0], got[0])
    if kind == "cut":
        assert (ref["votes"] == 0).sum() >= 100 and (ref["votes"] > 0).sum() >= 100
    # the float64 sums are inside their own magnitudes
    for name in NAMES:
        assert (np.abs(ref[name]) <= ref["m_" + name[2:]] * (1 + 1e-12)).all()


def test_float64_oracle_matches_autograd_of_a_restatement_on_the_cut_box():
    """tests/test_oracle_vote.py::test_backward_matches_autograd_of_restatement with a corner argument, against
    hv_backward64.  Tolerance from there: d_xyz / d_scale are the true gradients times res (the reference omits the 1 / res
    factor), and the fp32 geometry moves a few votes across cell edges."""
    import torch
    pts, xyz, scale, prob, res = scene()
    R = 16
    corner, dims = box_of("cut", pts, res)
    grad = np.random.default_rng(1).normal(0, 1, dims).astype(np.float32)
    ref = hv_numpy.hv_backward64(grad, pts, xyz, scale, prob, res, R, corner)
    assert (ref["votes"] > 0).sum() >= 100

    ct, st = hv_numpy.rot_table(R)
    t64 = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=g)
    P, X, S, O, G, C, Sn, cr = t64(pts), t64(xyz, True), t64(scale, True), t64(prob, True), t64(grad), t64(ct), t64(st), t64(corner)
    corr = X * S
    ox = -C[None] * corr[:, 0:1] + Sn[None] * corr[:, 2:3]
    oy = (-corr[:, 1:2]).expand_as(ox)
    oz = -Sn[None] * corr[:, 0:1] - C[None] * corr[:, 2:3]
    g = [(P[:, k:k + 1] + o - cr[k]) / float(np.float32(res)) for k, o in enumerate((ox, oy, oz))]
    ok = (g[0] >= 0) & (g[1] >= 0) & (g[2] >= 0) & (g[0] < dims[0] - 1) & (g[1] < dims[1] - 1) & (g[2] < dims[2] - 1)
    fl = [torch.floor(a).long().clamp(0, d - 2) for a, d in zip(g, dims)]
    fr = [a - torch.floor(a) for a in g]
    total = 0
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                w = (fr[0] if bx else 1 - fr[0]) * (fr[1] if by else 1 - fr[1]) * (fr[2] if bz else 1 - fr[2])
                total = total + (w * O[:, None] * G[fl[0] + bx, fl[1] + by, fl[2] + bz] * ok).sum()
    total.backward()
    np.testing.assert_allclose(ref["d_obj"], O.grad.numpy(), rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(ref["d_xyz"], X.grad.numpy() * res, rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(ref["d_scale"], S.grad.numpy() * res, rtol=2e-3, atol=2e-3)
    assert float(np.abs(ref["d_xyz"]).max()) > 0.1


def _wrong(name):
    """(case, wrong result [3 float64 arrays], reference) of a named wrong result, from the oracle's per-vote terms"""
    pts, xyz, scale, prob, res = scene()
    R, dims = {"last_rotation": (65, None), "upper_lanes": (120, None), "strides": (36, (7, 5, 11))}.get(name, (36, None))
    if dims is None:
        grad, corner, dims = case(R, "own")
    else:
        # a 7 x 5 x 11 grid over the middle of the cloud (cells of `res`), so that X, Y and Z all differ
        mid = (0.5 * (pts.min(0) + pts.max(0))).astype(np.float32)
        corner = (mid - np.float32(res) * np.array([3.1, 2.2, 5.3], np.float32)).astype(np.float32)
        grad = np.random.default_rng(0).normal(0, 1, dims).astype(np.float32)
    pi, ri, fl, w0, w1 = hv_numpy.vote_geometry(pts, xyz, scale, res, R, corner, dims)
    cells = hv_numpy.gather_cells(grad, fl)
    sums = lambda **kw: hv_numpy.backward_sums(**dict(dict(cells=cells, w0=w0, w1=w1, pi=pi, ri=ri, xyz=xyz, scale=scale, obj=prob,
                                                           num_rots=R), **kw))
    ref = sums()
    if name == "last_rotation":           # `i < R - 1`: the last in-bounds rotation of every point
        last = np.full(len(pts), -1)
        np.maximum.at(last, pi, ri)
        keep = ri != last[pi]
        bad = sums(cells=cells[:, keep], w0=[a[keep] for a in w0], w1=[a[keep] for a in w1], pi=pi[keep], ri=ri[keep])
    elif name == "upper_lanes":           # no __shfl_xor(..., 32): lane 0 never sees lanes 32 ... 63
        keep = (ri % 64) < 32
        bad = sums(cells=cells[:, keep], w0=[a[keep] for a in w0], w1=[a[keep] for a in w1], pi=pi[keep], ri=ri[keep])
    elif name == "strides":               # sx and sy swapped in b + sx + sy + 1
        X, Y, Z = dims
        b = (fl[0] * Y + fl[1]) * Z + fl[2]
        flat = grad.ravel().astype(np.float64)
        bad = sums(cells=np.stack([flat[b + bx * Z + by * Y * Z + bz] for bx, by, bz in hv_numpy.CELLS]))
    elif name == "wy":                    # w0y and w1y swapped
        bad = sums(w0=[w0[0], w1[1], w0[2]], w1=[w1[0], w0[1], w1[2]])
    else:                                 # `dx *= ob` missing: d_xyz / d_scale without the objectness
        assert name == "no_obj"
        bad = dict(ref, **{k: v for k, v in sums(obj=np.ones_like(prob)).items() if k in ("d_xyz", "d_scale")})
    return [bad[k] for k in NAMES], ref


WRONG = ("last_rotation", "upper_lanes", "strides", "wy", "no_obj")


@pytest.mark.parametrize("name", WRONG)
def test_named_wrong_results_are_far_outside_the_bound(name):
    """Each is >= 10 x outside the bound on some element.  Against the old bar (|error| <= 1e-4 max(1, max |ref|) + 1e-4 |ref|
    per element): taken over the whole array of this 1500-point scene NONE of the five passes it - a wrong result that
    touches every point meets a few large elements; what the old bar cannot see is the single element.  Of the elements
    >= 10 x outside the bound it accepts (d_xyz, d_scale, d_obj): last_rotation 393 / 1154 / 3 of 3234 / 3234 / 1071,
    upper_lanes 118 / 517 / 1 of 3236 / 3236 / 1079, wy 129 / 380 / 2, no_obj 7 / 30 / 0, strides 1 / 0 / 0 - so a fault
    confined to a few points (one lane count, one workgroup) can pass it whole."""
    bad, ref = _wrong(name)
    bounds = hv_numpy.vote_bwd_bounds(ref)
    worst, accepted = 0.0, 0
    for k, b in zip(NAMES, bad):
        err = np.abs(b - ref[k])
        worst = max(worst, float((err / bounds[k]).max()))
        old_tol = OLD_RTOL * max(1.0, float(np.abs(ref[k]).max())) + OLD_RTOL * np.abs(ref[k])
        accepted += int(((err >= 10 * bounds[k]) & (err <= old_tol)).sum())
    old = old_bar_passes([b.astype(np.float32) for b in bad], [ref[k].astype(np.float32) for k in NAMES])
    print("%s: %.3g x the bound; old bar %s as a whole, accepts %d elements >= 10 x outside the bound" % (
        name, worst, "passes" if old else "fails", accepted))
    assert worst >= 10.0, (name, worst)
    assert not old, name
    if name in ("last_rotation", "upper_lanes", "wy"):
        assert accepted >= 100, (name, accepted)


# ---- the geometry the GPU cases are built for (a seed change must not hollow them out) ---------------------------------------
def test_backward_gpu_cases_have_the_geometry_they_are_built_for():
    from tests import test_vote_backward_gpu as bw
    # the sweep: every trip-count edge of the lane loop and every n, n % 4 != 0 among them, a non-cubic grid, votes in the last trip of the lane loop
    assert {r for r, _ in bw.SWEEP} == {1, 7, 63, 64, 65, 120, 128, 129, 256} and {n for _, n in bw.SWEEP} == {1, 3, 4, 5, 1023}
    assert len(set(bw.SWEEP_DIMS)) == 3
    for R, n in bw.SWEEP:
        name = "sweep_R%d_n%d" % (R, n)
        c, (ref, _) = bw.case(name), bw.reference(name)
        assert len(c["pts"]) == n and ref["votes"].max() > 0, name
        pi, ri, _, _, _ = hv_numpy.vote_geometry(c["pts"], c["xyz"], c["scale"], c["res"], R, c["corner"], c["dims"])
        assert ri.max() == R - 1 and (ri // 64 == (R - 1) // 64).sum() > 0, name          # the last trip has in-bounds votes
        if n == 1023:
            assert (ref["votes"] == R).sum() > 100 and (ref["votes"] < R).sum() > 100, name
    # the cut box: points beyond all six faces; with votes, without, and outside the box but with votes
    c, (ref, _) = bw.case("cut"), bw.reference("cut")
    cells = (c["pts"] - c["corner"]) / np.float32(c["res"])
    hi = np.asarray(c["dims"]) - 1
    assert (cells < 0).any(0).all() and (cells > hi).any(0).all()
    outside = ((cells < 0) | (cells > hi)).any(1)
    print("cut: %d of %d points have votes, %d of them lie outside the box" % (
        (ref["votes"] > 0).sum(), len(outside), (outside & (ref["votes"] > 0)).sum()))
    assert (ref["votes"] > 0).sum() >= 100 and (ref["votes"] == 0).sum() >= 100
    assert (outside & (ref["votes"] > 0)).sum() >= 1
    assert (ref["votes"] == c["R"]).sum() >= 1 and ((ref["votes"] > 0) & (ref["votes"] < c["R"])).sum() >= 100
    corners = bw.cut_corners()
    assert np.array_equal(corners[0], c["corner"])
    assert [int(np.float32(np.float32(corners[1][k] - corners[0][k]) / np.float32(c["res"]))) + 1 for k in range(3)] == c["dims"]
    # the big box: its origin is not the cloud's minimum, nearly every point has all its votes
    c, (ref, _) = bw.case("big"), bw.reference("big")
    assert (c["pts"].min(0) > c["corner"] + c["res"]).all() and (ref["votes"] > 0).all() and (ref["votes"] == c["R"]).mean() > 0.9
    # thin grids
    assert bw.reference("thin1")[0]["votes"].sum() == 0 and bw.case("thin1")["dims"][1] == 1
    v = bw.reference("thin2")[0]["votes"]
    assert bw.case("thin2")["dims"][1] == 2 and (v > 0).sum() >= 100 and (v == 0).sum() >= 50
    # nodes: all fractional parts 0; a coordinate at dims - 1 excludes the point, the largest float below it does not
    c, (ref, _) = bw.case("nodes"), bw.reference("nodes")
    last = (c["pts"] == np.asarray(c["dims"], np.float32) - 1).any(1)
    assert last.sum() > 50 and (ref["votes"][last] == 0).all() and (ref["votes"][~last] == c["R"]).all()
    pi, ri, fl, w0, w1 = hv_numpy.vote_geometry(c["pts"], c["xyz"], c["scale"], c["res"], c["R"], c["corner"], c["dims"])
    on_node = pi < len(c["pts"]) - 3
    assert all((w[on_node] == 0).all() for w in w1) and all((w[on_node] == 1).all() for w in w0)
    for k in range(3):
        mine = pi == len(c["pts"]) - 3 + k
        assert mine.sum() == c["R"] and (fl[k][mine] == c["dims"][k] - 2).all() and (w1[k][mine] > 0.999).all()
    # the large case
    c, (ref, _) = bw.case("large"), bw.reference("large")
    assert len(c["pts"]) == 2 ** 18 + 1 and c["R"] == 3 and 1000 < np.prod(c["dims"]) < 10000
    assert (ref["votes"] > 0).sum() > 50000 and (ref["votes"] == 0).sum() > 50000 and ref["votes"][-1] > 0


def test_corner_box_cases_have_votes_from_points_outside_the_box():
    from tests import test_vote_corners_gpu as cb
    from tests.test_vote_fallbacks_gpu import ntiles_of, takes_queue_launch
    assert ntiles_of(cb.CASES["stream"][0]) == 12 and ntiles_of(cb.CASES["queue"][0]) == 128
    for name in cb.NAMES:
        c = cb.case(name)
        dims, origin, n, R, launch = cb.CASES[name]
        assert takes_queue_launch(dims) == (launch == "queue") and len(c["pts"]) == n
        cells = c["pts"] - c["corners"][0]
        hi = np.asarray(dims) - 1
        assert (cells < 0).any(0).all() and (cells > hi).any(0).all(), name          # points beyond each of the six faces
        outside = ((cells < 0) | (cells > hi)).any(1)
        pi, _, _, _, _ = hv_numpy.vote_geometry(c["pts"], c["xyz"], c["scale"], 1.0, R, c["corners"][0], dims)
        vin = cb.reference(name)[1]
        from_outside = int(outside[pi].sum())
        print("%s: %d of %d in-bounds votes come from points outside the box" % (name, from_outside, vin))
        assert len(pi) == vin
        if R == 120:
            assert from_outside >= 10000 and from_outside >= 0.05 * vin, name
        else:
            assert from_outside > 0, name
    assert np.array_equal(cb.case("shifted")["corners"][0], np.array([-3.5, 10.25, 7.75], np.float32))
    # the work lists of the queue cases fit (no overflow flag), and the points left of / in front of tile 0 matter to the total
    from tests.test_vote_fallbacks_gpu import list_capacity
    for name in ("queue", "shifted"):
        assert 5000 < cb.list_entries(name) < list_capacity(cb.CASES[name][2], 128) // 4
