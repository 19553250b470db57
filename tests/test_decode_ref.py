"""CPU, always on: the decode oracle (oracle/decode_oracle.c) against the full-grid torch restatement of tests/decode_ref.py on
its edge cases, the claims each case exists for, the named wrong results, and both against what the reference's own lines
produced (tests/golden/decode_ref_*.npz, decode_edge_ref.npz).

The oracle shares structure and fp conventions with the kernels of csrc/hv_decode.hip; the restatement shares neither (whole
grid, torch.argmax, clamped meshgrid, masked indexing, no fused multiply-add).  Integer results, scores and the mutated grid
must be exactly equal; boxes within 2e-6 absolute, the margin tests/test_decode_gpu.py gives the reference's lines."""
import os

import numpy as np
import pytest

import oracle
from tests import decode_ref as dr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BOX_TOL = 2e-6


def oracle_decode(c, **over):
    kw = dict(c.kw, **over)
    okw = {}
    for k, v in kw.items():
        if k == "separate_variant":
            okw["elim_hi_plus1"] = 0 if v else 1
        elif k == "max_candidates":
            okw["max_iters"] = v
        else:
            okw[k] = v
    return oracle.decode(*c.args(), oracle.DecodeParams.default(**okw))


def differences(a, b, box_tol=BOX_TOL):
    """names of the result fields in which two decodes differ (exact, except boxes)"""
    out = [k for k in ("cand_idx", "verdict", "classes") if list(a[k]) != list(b[k])]
    out += [k for k in ("scores", "grid_obj_after") if not np.array_equal(a[k], b[k])]
    if a["boxes"].shape != b["boxes"].shape or (len(a["boxes"]) and np.abs(a["boxes"] - b["boxes"]).max() > box_tol):
        out.append("boxes")
    return out


def zeroed_cells(before, after):
    return np.flatnonzero((before != 0) & (after == 0))


@pytest.mark.parametrize("name", list(dr.CASES))
def test_oracle_equals_the_restatement(name):
    c, want = dr.case(name), dr.expected(name)
    got = oracle_decode(c)
    assert differences(got, want) == []
    # what the case is for
    assert c.listed() == c.claims["listed"]
    assert not np.isnan(c.grid_obj).any() and c.cls.min() >= 0 and c.cls.max() < 64 and c.prob.min() >= 0
    if not c.allow_truncation:
        assert not want["truncated"] and len(want["cand_idx"]) <= c.kw.get("max_candidates", 512)
    for k in ("verdict", "classes", "cand"):
        if k in c.claims:
            assert list(want["cand_idx" if k == "cand" else k]) == list(c.claims[k]), k
    if "truncated" in c.claims:
        assert want["truncated"] == c.claims["truncated"]


def test_len_family_lists_exactly_L_cells_and_reaches_every_verdict():
    seen = set()
    for L in dr.LEN_SMALL + dr.LEN_BIG:
        c, want = dr.case("len_%d" % L), dr.expected("len_%d" % L)
        assert int((c.grid_obj >= 60).sum()) == L and int((c.grid_obj >= 60).sum()) == c.listed()
        assert c.grid_obj.shape == ((20, 12, 20) if L <= 4097 else (40, 20, 40))
        vals = np.unique(c.grid_obj[c.grid_obj >= 60])
        assert set(vals) <= {60.0, 61.0, 62.0, 63.0} and (L < 63 or len(vals) == 4)         # heavy ties
        assert 1 <= len(want["cand_idx"]) <= 400                                                # tens to low hundreds
        seen |= set(want["verdict"].tolist())
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name", ["faces_0", "faces_0_sep", "faces_0_in", "faces_0_out"])
def test_faces_put_listed_cells_exactly_on_a_face(name):
    """yaw 0: the cell k = |scale| / res steps from the peak along x has |t| == |s| bit for bit, is listed, and survives the
    peak (the grid after that one candidate) while the cell one step nearer dies.  One ulp outward kills it, one ulp inward changes nothing."""
    c, want = dr.case(name), dr.expected(name)
    px, py, pz = dr.FACE_PEAK
    res, s = np.float32(c.res), c.grid_scale[dr.FACE_PEAK]
    assert want["cand_idx"][0] == dr.flat_of(dr.FACE_DIMS, dr.FACE_PEAK)
    after = dr.decode(*c.args(), **dict(c.kw, max_candidates=1))["grid_obj_after"]        # the peak's suppression alone
    on_face = 0
    for axis, k in enumerate(dr.FACE_PEAK_SCALE):
        k = abs(k)
        for sign in (1, -1):
            cell, near = [px, py, pz], [px, py, pz]
            cell[axis] += sign * k
            near[axis] += sign * (k - 1)
            t = np.float32(sign * k) * res                                   # (x - cx) * res, then * cos = 1
            assert c.grid_obj[tuple(cell)] >= 60
            nudged = axis == 0 and c.claims["nudge"]
            if not nudged:
                assert np.abs(t).view(np.uint32) == np.abs(s[axis]).view(np.uint32)
                on_face += 1
            killed = nudged == "out"
            assert after[tuple(cell)] == (0 if killed else 61)
            assert after[tuple(near)] == 0
    assert on_face >= 4
    if name == "faces_0_in":
        assert differences(want, dr.expected("faces_0")) == []
    if name == "faces_0_out":
        assert "cand_idx" in differences(want, dr.expected("faces_0"))


@pytest.mark.parametrize("dims", dr.CORNER_DIMS)
def test_corner_peaks_are_examined_first(dims):
    for e, p in dr.CORNER_ELIM:
        name = "corners_%dx%dx%d_e%d%s" % (dims + (e, "p" if p else ""))
        c, want = dr.case(name), dr.expected(name)
        corners = c.claims["corners"]
        assert len(corners) == 2 ** sum(d > 1 for d in dims)
        assert want["cand_idx"][0] in corners and not want["grid_obj_after"].ravel()[corners].any()
        if dims == (9, 7, 11) and e < 50:          # no corner's cube or box reaches another corner: all eight come first
            assert sorted(want["cand_idx"][:8].tolist()) == sorted(corners)
        if e == 50 and max(dims) <= 50:
            assert len(want["cand_idx"]) == 1 and not want["grid_obj_after"].any()
    if max(dims) == 300:
        ax = dims.index(300)
        assert (np.array(np.unravel_index(dr.expected("corners_%dx%dx%d_e2p" % dims)["cand_idx"], dims))[ax] > 255).any()


def test_values_case_order_and_threshold():
    c, want = dr.case("values"), dr.expected("values")
    assert list(want["cand_idx"]) == c.claims["order"]                       # +inf, the 61s, then both cells == thresh_high
    assert np.isinf(c.grid_obj).sum() == 1 and (c.grid_obj == 60).sum() == 2
    below = np.nextafter(np.float32(60), np.float32(0))
    assert want["grid_obj_after"].ravel()[c.claims["never"]] == below and c.grid_obj.ravel()[c.claims["never"]] == below
    eq = dr.expected("values_equal")
    assert (np.diff(eq["cand_idx"]) > 0).all() and eq["cand_idx"][0] == 0    # pure flat-index order


def test_lattice_accepts_on_both_sides_of_candidate_256():
    want = dr.expected("lattice_291_m512")
    assert len(want["cand_idx"]) == 291 and want["verdict"][255] == 0 and want["verdict"][258] == 0
    assert 63 in want["classes"] and len(want["boxes"]) == 97
    assert differences(dr.expected("lattice_291_m291"), want) == [] and not dr.expected("lattice_291_m291")["truncated"]
    cut = dr.expected("lattice_291_m290t")
    assert cut["truncated"] and list(cut["cand_idx"]) == list(want["cand_idx"][:290])
    grow = dr.LATTICE_GROW()
    assert grow.kw["max_candidates"] == 9 and not grow.allow_truncation
    assert np.array_equal(grow.grid_obj, dr.case("lattice_291_m512").grid_obj)


def test_verdict_edge_cases_hold_what_they_claim():
    assert np.float32(0.3) in dr.case("ve_prob_eq").prob
    assert np.float32(0.25) * np.float32(8) == np.float32(2)
    for n in (1, 255, 256, 257):
        assert len(dr.case("ve_npts_%d" % n).pts) == n
    c = dr.case("ve_face_points")
    assert sorted(np.abs(c.pts[:12]).max(1).tolist()) == [float(np.nextafter(np.float32(c.res), np.float32(0)))] * 6 + [c.res] * 6


@pytest.mark.parametrize("name", list(dr.CATEGORY_CASES))
def test_categories_mixed_lists_per_category(name):
    cats = dr.CATEGORY_CASES[name]()
    assert [c.listed() for c in cats] == ([0, 300, 4097] if name.endswith("a") else [0, 1537, 24577])
    for c in cats:
        assert c.pts is cats[0].pts and not c.cls.any()
        want = dr.decode(*c.args(), **c.kw)
        assert differences(oracle_decode(c), want) == []
        assert (len(want["cand_idx"]) == 0) == (c.listed() == 0)


# every named wrong result changes the outcome of the cases named next to it: a wrong= that no case told apart would be a
# missing case
REJECTED_BY = {
    "tie_highest_index": ("values_equal", "len_64", "lattice_291_m512"),
    "face_inclusive": ("faces_0", "faces_45_sep", "corners_9x7x11_e0", "ve_face_points"),
    "cube_plus1_swapped": ("corners_9x7x11_e2", "corners_9x7x11_e2p", "corners_300x2x7_e50p", "zero_scale_separate"),
    "valid_ratio_inclusive": ("ve_ratio_pass",),
    "thresh_low_inclusive": ("ve_low_pass", "ve_npts_1"),
    "class_tie_highest": ("ve_class_tie",),
    "prob_mask_inclusive": ("ve_prob_eq",),
    "listed_strict": ("values",),
    "mean_over_in_box": ("ve_mean_mask", "values_equal"),
    "rotation_transposed": ("faces_90", "len_1", "corners_1x1x1_e0"),
}


@pytest.mark.parametrize("wrong", dr.WRONG)
def test_named_wrong_results_are_rejected(wrong):
    assert set(REJECTED_BY) == set(dr.WRONG)
    for name in REJECTED_BY[wrong]:
        c = dr.case(name)
        assert differences(dr.decode(*c.args(), wrong=wrong, **c.kw), dr.expected(name)) != [], (wrong, name)


@pytest.mark.parametrize("name", ["decode_ref_8k", "decode_ref_5k"])
def test_restatement_matches_reference_lines_executed_on_cpu(name):
    """the restatement is pinned by the reference's lines as the oracle is (tests/test_oracle_decode.py)"""
    from tests.golden.make_decode_golden import make_case
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    sc, _ = make_case(int(z["seed"]), int(z["n"]), 1.0)
    res = float(z["res"])
    pts = (sc.coords * np.float32(res)).astype(np.float32)
    g = oracle.hv_forward(pts, z["xyz_pred"], z["scale_pred"], z["prob_pred"], res, 120)
    corner, _, _ = oracle.grid_geometry(pts, res)
    th, tl, vr, el = z["consts"]
    d = dr.decode(g[0], g[1], g[2], corner, res, pts, z["xyz_pred"], z["prob_pred"], z["class_pred"], thresh_high=th,
                  thresh_low=tl, valid_ratio=vr, elimination=int(el))
    assert len(d["boxes"]) == len(z["boxes"]) and list(d["classes"]) == list(z["classes"])
    np.testing.assert_allclose(d["boxes"], z["boxes"], rtol=0, atol=BOX_TOL)
    np.testing.assert_allclose(d["scores"], z["scores"], rtol=1e-6)
    assert np.array_equal(zeroed_cells(g[0], d["grid_obj_after"]), z["zeroed"])


def check_edge_fixture(z, name, c, got):
    """a decode result against what eval_joint.py:195-263 produced for the case (exact arithmetic: exact equality)"""
    nb = int((got["verdict"] == 0).sum())
    assert nb == len(got["boxes"]) == len(z[name + "__boxes"])
    assert list(got["classes"]) == list(z[name + "__classes"])
    assert np.array_equal(got["scores"], z[name + "__scores"])
    np.testing.assert_allclose(got["boxes"].reshape(-1, 8, 3), z[name + "__boxes"], rtol=0, atol=BOX_TOL)
    assert np.array_equal(zeroed_cells(c.grid_obj, got["grid_obj_after"]), z[name + "__zeroed"])


@pytest.mark.parametrize("name", list(dr.GOLDEN_CASES))
def test_edge_fixture_from_the_reference_lines(name):
    z = np.load(os.path.join(GOLDEN, "decode_edge_ref.npz"))
    c = dr.case(name)
    assert np.array_equal(c.pts.min(0), c.corner)           # the reference takes the corner from the points (:201)
    check_edge_fixture(z, name, c, dr.expected(name))
    check_edge_fixture(z, name, c, oracle_decode(c))
