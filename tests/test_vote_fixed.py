"""CPU: the exact restatement of the vote tile algorithm (oracle/hv_numpy.hv_forward_fixed) and the direct kernel's error model
(hv_forward64 / vote_fwd_bounds), pinned before tests/test_vote_exact_gpu.py holds the kernels to them.

  - the restatement's sha256 hashes are those of tests/golden/vote_parent_bits.json (bits a GPU wrote) on all eight dense cases;
  - it lies inside the old bar (assert_grids_close against the C oracle), and the C oracle - fp32, sequential - inside the
    direct kernel's derived bound;
  - named wrong results built from the restatement's own per-contribution terms differ from it in bits; the ones marked
    "accepted" pass the old bar all the same, which is what that bar could not see;
  - the new cases of tests/vote_cases.py are what they claim."""
import functools
import json

import numpy as np
import pytest

import oracle
from oracle import hv_numpy
from tests import test_vote_dense_gpu as dense
from tests import vote_cases
from tests.test_vote_gpu import assert_grids_close

f32 = np.float32
WRONG_CASES = ["rounds", "r7", "lists"]


def words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def differing_words(a, b):
    return sum(int((words(x) != words(y)).sum()) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def inputs(name):
    return (dense.CASES[name] if name in dense.CASES else vote_cases.CASES[name])()


@functools.lru_cache(maxsize=None)
def geometry(name):
    pts, _, _, _, res, _ = inputs(name)
    corner, _, dims = hv_numpy.grid_dims(pts, f32(res))
    assert dims == oracle.grid_geometry(pts, res)[2]
    return corner, dims


@functools.lru_cache(maxsize=None)
def c_oracle(name):
    pts, xyz, scale, prob, res, R = inputs(name)
    return oracle.hv_forward(pts, xyz, scale, prob, res, R)


@functools.lru_cache(maxsize=None)
def sums(name):
    """(cells, int64 sums [6, c], counts) of the restatement, computed once and left unchanged"""
    pts, xyz, scale, prob, res, R = inputs(name)
    return hv_numpy.fixed_sums(pts, xyz, scale, prob, res, R, *geometry(name))


@functools.lru_cache(maxsize=None)
def fixed(name):
    cells, s, _ = sums(name)
    return hv_numpy.dense_grids(cells, *hv_numpy.fixed_store(s), geometry(name)[1])


@functools.lru_cache(maxsize=None)
def counts(name):
    pts, xyz, scale, _, res, R = inputs(name)
    return hv_numpy.contribution_counts(pts, xyz, scale, res, R)


def grids_of(cells, s, dims, **kw):
    return hv_numpy.dense_grids(cells, *hv_numpy.fixed_store(s, **kw), dims)


def assert_old_bar(grids, name):
    """what the forward-vote tests asserted of the tile kernel before the exact reference (tests/test_vote_dense_gpu.py)"""
    ref = c_oracle(name)
    if name == "huge":
        assert np.array_equal(grids[0] == 0, ref[0] == 0)
        np.testing.assert_allclose(grids[0], ref[0], rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ref[0]).max())))
        live = ref[0] > 1e-3 * max(1.0, float(np.abs(ref[0]).max()))
        np.testing.assert_allclose(grids[2][live], ref[2][live], rtol=1e-4, atol=1e-4)
    else:
        assert_grids_close(grids, ref, name, counts=counts(name))


@pytest.mark.parametrize("name", sorted(dense.CASES))
def test_restatement_has_the_recorded_bits_and_meets_the_old_bar(name):
    """hv_forward_fixed (the public entry, not the cached parts) hashes to what the GPU wrote for every dense case"""
    pts, xyz, scale, prob, res, R = inputs(name)
    got = hv_numpy.hv_forward_fixed(pts, xyz, scale, prob, res, R)
    with open(dense.BITS) as f:
        want = json.load(f)[name]
    assert dense.grid_hashes(got) == want, name
    assert differing_words(got, fixed(name)) == 0
    cells, _, cnt = sums(name)
    assert np.array_equal(np.bincount(cells, weights=cnt, minlength=counts(name).size).astype(np.int64),
                          counts(name).ravel().astype(np.int64))
    assert_old_bar(got, name)


@pytest.mark.parametrize("name", sorted(dense.CASES))
def test_c_oracle_is_inside_the_direct_kernels_bound(name):
    """the fp32 sequential C oracle is one admissible order of the direct kernel's sums: every element inside vote_fwd_bounds of
    hv_forward64, exact zeros at cells without contributions.  Prints the worst ratios (LABNOTES.md records them)."""
    pts, xyz, scale, prob, res, R = inputs(name)
    assert (prob >= 0).all()
    ref = hv_numpy.hv_forward64(pts, xyz, scale, prob, res, R)
    b = hv_numpy.vote_fwd_bounds(ref)
    touched = ref["count"] > 0
    assert np.array_equal(ref["count"], counts(name))
    assert (b["margin"][touched] > 0).all(), name
    got = c_oracle(name)
    worst = {}
    for g, key in zip(got, ("obj", "rot", "scale")):
        assert not g[~touched].any(), (name, key)
        worst[key] = float((np.abs(g.astype(np.float64) - b[key])[touched] / b["b_" + key][touched]).max())
    print("%s: C oracle at %.3f (obj) %.3f (rot) %.3f (scale) of the bound, n_c up to %d" % (
        name, worst["obj"], worst["rot"], worst["scale"], int(ref["count"].max())))
    assert max(worst.values()) <= 1.0, (name, worst)


def test_vote_fwd_bounds_formula():
    """the model on a hand-made cell: two terms, n_c = 2"""
    u = 2.0 ** -24
    ref = dict(sum=np.array([[[[2.0, 1.0, -1.0, 4.0, 0.0, 0.5]]]]), mag=np.array([[[[2.0, 3.0, 1.0, 4.0, 0.0, 0.5]]]]),
               count=np.array([[[2]]]))
    b = hv_numpy.vote_fwd_bounds(ref)
    gam = 2 * u / (1 - 2 * u)
    bD = gam * 2.0 + 2 * 2.0 ** -126
    assert b["b_obj"][0, 0, 0] == bD and b["margin"][0, 0, 0] == 2.0 + 1e-7 - bD
    q = 1.0 / (2.0 + 1e-7)
    want = (gam * 3.0 + 2 * 2.0 ** -126 + q * bD) / (2.0 + 1e-7 - bD) + 2 * u * q + 2.0 ** -149
    assert b["rot"][0, 0, 0, 0] == q and abs(b["b_rot"][0, 0, 0, 0] - want) <= 1e-22
    # a channel without magnitude keeps the flushed subnormals of its two additions and the quotient's one
    assert b["b_scale"][0, 0, 0, 1] == 2 * 2.0 ** -126 / (2.0 + 1e-7 - bD) + 2.0 ** -149


@functools.lru_cache(maxsize=None)
def contributions(name):
    """every contribution of the case: (cell [m], fp32 terms [6, m], words [6, m] int64)"""
    pts, xyz, scale, prob, res, R = inputs(name)
    parts = list(hv_numpy.vote_contributions(pts, xyz, scale, prob, res, R, *geometry(name)))
    cell, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts], 1)
    q = np.stack([hv_numpy.obj_quantum(t[0])] + [hv_numpy.fx_quantum(v) for v in t[1:]])
    return cell, t, q


@functools.lru_cache(maxsize=None)
def grazing(name):
    """index of the contribution with the largest w / (weight of its cell) below 1e-5: a grazing vote into a busy cell"""
    cell, t, _ = contributions(name)
    weight = fixed(name)[0].ravel()[cell].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(weight > 0, t[0].astype(np.float64) / weight, 0.0)
    ratio[(ratio >= 1e-5) | (t[0] <= 0)] = 0.0
    i = int(np.argmax(ratio))
    assert 1e-6 < ratio[i] < 1e-5, (name, ratio[i])
    return i, float(ratio[i]), float(weight[i])


def with_contribution(name, i, times):
    """the restatement's grids with contribution i counted 1 + times times (times = -1: dropped)"""
    cell, _, q = contributions(name)
    cells, s, _ = sums(name)
    s = s.copy()
    at = np.searchsorted(cells, cell[i])
    assert cells[at] == cell[i]
    s[:, at] += times * q[:, i]
    return hv_numpy.dense_grids(cells, *hv_numpy.fixed_store(s), geometry(name)[1])


@pytest.mark.parametrize("name", WRONG_CASES)
def test_wrong_results_the_old_bar_accepted_differ_in_bits(name):
    pts, xyz, scale, prob, res, R = inputs(name)
    corner, dims = geometry(name)
    cells, s, _ = sums(name)
    i, ratio, weight = grazing(name)
    wrong = {
        "one contribution dropped": with_contribution(name, i, -1),
        "one contribution counted twice": with_contribution(name, i, +1),
        "quanta truncated": grids_of(*hv_numpy.fixed_sums(pts, xyz, scale, prob, res, R, corner, dims, truncate=True)[:2], dims),
        "divided by the double sum": grids_of(cells, s, dims, double_divisor=True),
    }
    print("%s: grazing contribution %.3g into a cell of weight %.4g (ratio %.3g)" % (name, ratio * weight, weight, ratio))
    for what, grids in wrong.items():
        n = differing_words(grids, fixed(name))
        print("%s, %s: %d words differ" % (name, what, n))
        assert n >= 1, (name, what)
        assert_old_bar(grids, name)                 # accepted by the 1e-4 bar
    # the objectness channel's non-zero rule changes no word of these cases (it needs `tiny`)
    c2, s2, _ = hv_numpy.fixed_sums(pts, xyz, scale, prob, res, R, corner, dims, nonzero_rule=False)
    assert np.array_equal(c2, cells) and np.array_equal(s2, s)


@pytest.mark.parametrize("name", WRONG_CASES)
def test_wrong_sums_leave_the_direct_kernels_bound_where_few_terms_meet(name):
    """the same errors on the float64 sums against vote_fwd_bounds, whose width goes with n_c: a dropped or doubled contribution
    is outside it by the printed factor at the cell where |w| / b_obj is largest (asserted: more than 10 x); truncated quanta
    move a sum by less than n_c 2^-36 against gamma(n_c) sum |t|, outside only at cells whose mean term is below 2^-12 (the
    factor is printed; asserted > 1 on the objectness channel where such a cell exists).  Dividing by the double sum moves a
    quotient by at most u |q|, always inside the 2 u |q| the model grants the division - only the bit comparison sees it."""
    pts, xyz, scale, prob, res, R = inputs(name)
    ref = hv_numpy.hv_forward64(pts, xyz, scale, prob, res, R)
    b = hv_numpy.vote_fwd_bounds(ref)
    cell, t, q = contributions(name)
    b_obj = b["b_obj"].ravel()[cell]
    factor = np.abs(t[0].astype(np.float64)) / b_obj
    i = int(np.argmax(factor))
    print("%s: dropping or doubling one contribution (w %.3g, n_c %d) is %.3g x the bound of its cell" % (
        name, float(t[0][i]), int(ref["count"].ravel()[cell[i]]), float(factor[i])))
    assert factor[i] > 10.0
    j, ratio, weight = grazing(name)
    print("%s: the grazing contribution (ratio %.3g, n_c %d) is %.3g x the bound of its busy cell" % (
        name, ratio, int(ref["count"].ravel()[cell[j]]), float(factor[j])))
    lost = np.abs(t[0].astype(np.float64) - np.trunc(t[0].astype(np.float64) * 2.0 ** 36) * 2.0 ** -36)
    n = ref["count"].size
    trunc_err = np.bincount(cell, weights=lost, minlength=n)
    touched = ref["count"].ravel() > 0
    tf = trunc_err[touched] / b["b_obj"].ravel()[touched]
    small_terms = (ref["mag"][..., 0].ravel()[touched] < 2.0 ** -13 * ref["count"].ravel()[touched]) & (trunc_err[touched] > 0)
    print("%s: truncation up to %.3g x the bound (%d cells with a mean term below 2^-13)" % (name, float(tf.max()), int(small_terms.sum())))
    if small_terms.any():
        assert tf.max() > 1.0


def test_tiny_case_needs_the_non_zero_rule():
    pts, xyz, scale, prob, res, R = inputs("tiny")
    corner, dims = geometry("tiny")
    assert len(pts) <= 600 and -(-dims[0] // 16) <= 3 and -(-dims[2] // 32) <= 3 and R == 24
    cell, t, q = contributions("tiny")
    sub = (hv_numpy.fx_quantum(t[0]) == 0) & (t[0] != 0)
    assert sub.sum() > 1000 and (np.abs(q[0][sub]) == 1).all()
    assert set(np.sign(t[0][sub])) == {-1.0, 1.0}
    # they vote into busy cells and into cells nothing else reaches
    others = np.bincount(cell[~sub], minlength=int(np.prod(dims)))
    assert (others[cell[sub]] > 0).any() and (others[cell[sub]] == 0).any()
    cells, s, _ = sums("tiny")
    c2, s2, _ = hv_numpy.fixed_sums(pts, xyz, scale, prob, res, R, corner, dims, nonzero_rule=False)
    wrong = hv_numpy.dense_grids(c2, *hv_numpy.fixed_store(s2), dims)
    right = fixed("tiny")
    assert differing_words(wrong, right) >= 1
    assert not np.array_equal(wrong[0] == 0, right[0] == 0), "the touched-cell set must change without the rule"
    # cells that only the sub-quantum points reach hold whole quanta with the rule
    alone = np.unique(cell[sub][others[cell[sub]] == 0])
    held = right[0].ravel()[alone].astype(np.float64) * 2.0 ** 36
    assert (held != 0).sum() > 20 and np.array_equal(held, np.rint(held)) and float(np.abs(held).max()) <= 8 * 24 * 27
    assert not wrong[0].ravel()[alone].any()


def test_signed_case_has_cells_whose_sums_cancel():
    pts, _, _, prob, _, _ = inputs("signed")
    dims = geometry("signed")[1]
    assert len(pts) <= 600 and -(-dims[0] // 16) <= 3 and -(-dims[2] // 32) <= 3
    assert (prob > 0).sum() > 100 and (prob < 0).sum() > 100
    cell, t, q = contributions("signed")
    cells, s, cnt = sums("signed")
    moved = np.bincount(np.searchsorted(cells, cell), weights=np.abs(q[0]).astype(np.float64), minlength=len(cells))
    cancelled = (s[0] == 0) & (moved > 0)
    assert cancelled.sum() >= 50 and (cnt[cancelled] > 0).all()
    right = fixed("signed")
    assert (right[0] < 0).any() and (right[0] > 0).any() and np.isfinite(right[1]).all() and np.isfinite(right[2]).all()


def test_clamp_case_reaches_the_clamp():
    pts, _, scale, _, _, _ = inputs("clamp")
    assert len(pts) == 1500 and float(scale.max()) == 1e9
    cell, t, q = contributions("clamp")
    beyond = np.abs(t[3:]) > 6e7
    assert beyond.sum() >= 100
    assert (np.abs(q[3:][beyond]) == int(6e7 * 2 ** 36)).all()
    # three clamped terms in one cell pass 2^63 quanta: some 64-bit sums of this case wrap around, in the restatement's int64
    # as in the kernel's unsigned words
    assert max(float(np.bincount(cell, weights=np.abs(v).astype(np.float64)).max()) for v in q[3:]) > 2.0 ** 63
    # (a clamped sum is not the C oracle's: only the objectness grid, which the scale does not enter, is compared with it)
    ref = c_oracle("clamp")[0]
    assert np.array_equal(fixed("clamp")[0] == 0, ref == 0)
    np.testing.assert_allclose(fixed("clamp")[0], ref, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ref).max())))
