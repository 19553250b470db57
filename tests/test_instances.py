"""cv_decode_instances_f32 without a device: the exported symbols, every refusal, and the contract itself as a numpy fp32
restatement (``contract``) that the GPU tests (tests/test_instances_gpu.py) compare the kernels with bit for bit.

The restatement follows the kernels' operation order (include/cv_hip.h, csrc/hv_decode.hip ``inst_boxes`` / ``inside_box``):
rot = f32(atan2(f64 r1, f64 r0)), cs / sn = f32(cos / sin(f64 rot)), centre = corner + res * cell in fp32,
t0 = fma(d2, sn, fma(d1, 0, d0 * cs)), t1 = fma(d2, 0, fma(d1, 1, d0 * 0)), t2 = fma(d2, cs, fma(d1, 0, d0 * -sn)), member when
|t| < |scale| on all three axes (and prob > prob_thresh with confident support), owner = the first box of the list.

The geometry of every GPU case is generated here, with fixed seeds.  The device's and numpy's double atan2 / cos / sin may
differ in the last ulp, which could move a verdict only for a point that sits on a face to within rounding: the rotated
cases therefore ASSERT (``face_margin``) that in fp64 no point lies within 1e-4 relative of any face of any box.  Random
scales cannot meet that (a 1000-point, 130-box case has ~4e5 point-face pairs, each inside the 1e-4 band with probability
~1e-4), so the generator places every box's scale in the middle of a gap between two consecutive |t| of the case's points:
nothing is dropped or filtered, and the assertion checks the construction.  The on-face cases (``special_case``) use the rot
vectors (1, 0) and (-1, 0) only and put every on-face point at the centre's coordinate on the other rotated axis, so that the
one inexact value (sin of f32(pi)) is multiplied by an exact zero."""
import ctypes
import os
import re

import numpy as np
import pytest

from canonicalvoting_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS = (12, 6, 10)
GROUP = 64                      # INST_GROUP of csrc/hv_decode.hip: boxes staged in LDS at a time
N_SWEEP = (1, 63, 64, 65, 255, 256, 257, 1000)
B_SWEEP = (0, 1, 63, 64, 65, 130)            # around GROUP and two groups


# ---- the contract ------------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """RN_f32(a * b + c) with ONE rounding, elementwise: the product of two f32 is exact in f64, the f64 sum is rounded to
    odd (its error from the two-sum), and rounding that to f32 then equals rounding the exact value (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def box_geometry(grid_rot, grid_scale, corner, res, cell, use_corner=True):
    """(centre [3], cs, sn, scale [3]) in f32 of the box the decode proposes at flat grid cell ``cell``"""
    X, Y, Z = grid_rot.shape[:3]
    c = (cell // (Z * Y), (cell // Z) % Y, cell % Z)
    r0, r1 = grid_rot[c]
    rot = f32(np.arctan2(np.float64(r1), np.float64(r0)))
    cs, sn = f32(np.cos(np.float64(rot))), f32(np.sin(np.float64(rot)))
    step = np.array([f32(res) * f32(c[d]) for d in range(3)], f32)
    centre = (np.asarray(corner, f32) + step) if use_corner else step
    return centre.astype(f32), cs, sn, np.asarray(grid_scale[c], f32)


def inside(points, centre, cs, sn, sc, strict=True):
    with np.errstate(all="ignore"):
        d = (np.asarray(points, f32) - centre).astype(f32)
        d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
        zero, one = f32(0), f32(1)
        t0 = fma32(d2, sn, fma32(d1, zero, d0 * cs))
        t1 = fma32(d2, zero, fma32(d1, one, d0 * zero))
        t2 = fma32(d2, cs, fma32(d1, zero, d0 * f32(-sn)))
        lt = (lambda a, b: a < b) if strict else (lambda a, b: a <= b)
        return lt(np.abs(t0), abs(sc[0])) & lt(np.abs(t1), abs(sc[1])) & lt(np.abs(t2), abs(sc[2]))


def contract(grid_rot, grid_scale, corner, res, points, prob, cells, label_of=None, confident=True, prob_thresh=0.3,
             strict=True, prob_ge=False, last=False, use_corner=True):
    """One category: (owner [n] int32, count_in [B], count_owned [B]).  The four keyword switches after ``prob_thresh`` are the
    named WRONG results (non-strict faces, >= on prob_thresh, last containing box, centre without the corner)."""
    n, B = len(points), len(cells)
    label_of = np.arange(B, dtype=np.int32) if label_of is None else np.asarray(label_of, np.int32)
    owner = np.full(n, -1, np.int32)
    owned_by = np.full(n, -1, np.int64)
    cin, cown = np.zeros(B, np.int32), np.zeros(B, np.int32)
    with np.errstate(invalid="ignore"):
        conf = np.ones(n, bool) if not confident else ((prob >= f32(prob_thresh)) if prob_ge else (prob > f32(prob_thresh)))
    for j, cell in enumerate(cells):
        m = inside(points, *box_geometry(grid_rot, grid_scale, corner, res, int(cell), use_corner), strict=strict) & conf
        cin[j] = m.sum()
        take = m if last else (m & (owned_by < 0))
        owned_by[take] = j
    has = owned_by >= 0
    owner[has] = label_of[owned_by[has]]
    cown[:] = np.bincount(owned_by[has], minlength=B)[:B]
    return owner, cin, cown


# ---- cases (fixed seeds; shared with tests/test_instances_gpu.py) -----------------------------------------------------------------

def face_margin(case):
    """fp64: the smallest | |t| - |s| | / |s| over every point, box and axis of a case (inf without boxes or points)"""
    worst = np.inf
    p = case["points"].astype(np.float64)
    for cell in case["cells"]:
        centre, cs, sn, sc = [np.asarray(v, np.float64) for v in box_geometry(case["grid_rot"], case["grid_scale"], case["corner"],
                                                                               case["res"], int(cell))]
        d = p - centre
        t = np.stack([d[:, 0] * cs + d[:, 2] * sn, d[:, 1], -d[:, 0] * sn + d[:, 2] * cs], 1)
        if t.size:
            worst = min(worst, float((np.abs(np.abs(t) - np.abs(sc)) / np.abs(sc)).min()))
    return worst


def make_case(seed, n, n_boxes, dims=DIMS, points=None, scale=(0.15, 0.45)):
    """A rotated case: random rot vectors, points uniform over the grid's extent (or the given ``points``), ``n_boxes``
    distinct cells; each box's scale sits in the middle of a gap of its points' |t|, the gap nearest to a draw from ``scale``
    (see the module docstring)"""
    rng = np.random.default_rng(seed)
    X, Y, Z = dims
    res, corner = f32(0.1), np.array([-0.35, 0.2, 1.05], f32)
    grid_rot = rng.normal(size=(X, Y, Z, 2)).astype(f32)
    grid_scale = rng.uniform(0.1, 0.5, (X, Y, Z, 3)).astype(f32)
    if points is None:
        points = (corner + rng.uniform(0, 1, (n, 3)) * (np.array(dims) * float(res))).astype(f32)
    prob = rng.uniform(0, 1, n).astype(f32)
    cells = rng.choice(X * Y * Z, n_boxes, replace=False).astype(np.int64)
    case = dict(grid_rot=grid_rot, grid_scale=grid_scale, corner=corner, res=res, points=points, prob=prob, cells=cells)
    for cell in cells:
        centre, cs, sn, _ = [np.asarray(v, np.float64) for v in box_geometry(grid_rot, grid_scale, corner, res, int(cell))]
        d = points.astype(np.float64) - centre
        t = np.abs(np.stack([d[:, 0] * cs + d[:, 2] * sn, d[:, 1], -d[:, 0] * sn + d[:, 2] * cs], 1))
        c = (int(cell) // (Z * Y), (int(cell) // Z) % Y, int(cell) % Z)
        for a in range(3):
            edges = np.concatenate([[0.0], np.sort(t[:, a]), [t[:, a].max() + 0.4]])
            mid, half = (edges[:-1] + edges[1:]) / 2, (edges[1:] - edges[:-1]) / 2
            good = np.flatnonzero((half >= 4e-4 * mid) & (mid >= scale[0] / 2))
            grid_scale[c][a] = f32(mid[good[np.argmin(np.abs(mid[good] - rng.uniform(*scale)))]])
    return case


def special_case():
    """The on-face and special-value case: rot vectors (1, 0) and (-1, 0), everything exactly representable.  Returns the
    case and the expected owners by hand.  res 0.5, corner (1, 0, 0); boxes (cells of a 4x4x4 grid):
      A cell (1,1,1) rot ( 1,0) centre (1.5,.5,.5) scale (.5,.5,.5)     x in (1, 2)
      B cell (2,1,1) rot (-1,0) centre (2.0,.5,.5) scale (.5,.5,.5)     x in (1.5, 2.5)
      C cell (0,3,3) rot ( 1,0) centre (1.0,1.5,1.5) scale (.5,0,.5)    a zero scale component: no members"""
    dims = (4, 4, 4)
    grid_rot = np.zeros(dims + (2,), f32)
    grid_rot[..., 0] = 1
    grid_rot[2, 1, 1] = (-1, 0)
    grid_scale = np.full(dims + (3,), 0.5, f32)
    grid_scale[0, 3, 3] = (0.5, 0, 0.5)
    cell = lambda x, y, z: (x * 4 + y) * 4 + z
    nan, inf = np.nan, np.inf
    rows = [                                                      # x, y, z, prob, owner
        (1.25, .5, .5, .9, 0),                                    # A only
        (1.75, .5, .5, .9, 0),                                    # A and B: the first
        (2.25, .5, .5, .9, 1),                                    # B only
        (2.0, .5, .5, .9, 1),                                     # on A's +x face (z = the centres' z): B only
        (1.0, .5, .5, .9, -1),                                    # on A's -x face
        (1.5, .5, .5, .9, 0),                                     # on B's face (|t0| = .5 exactly, cs = -1), inside A
        (2.5, .5, .5, .9, -1),                                    # on B's other face
        (1.25, 1.0, .5, .9, -1),                                  # on A's +y face
        (1.25, .5, 0.0, .9, -1),                                  # on A's -z face (x off B)
        (1.25, .5, .5, .3, -1),                                   # prob == prob_thresh (as f32): not confident
        (1.25, .5, .5, nan, -1),                                  # NaN prob
        (nan, .5, .5, .9, -1), (1.25, nan, .5, .9, -1), (1.25, .5, nan, .9, -1),
        (inf, .5, .5, .9, -1), (-inf, .5, .5, .9, -1), (1.25, inf, .5, .9, -1), (1.25, .5, -inf, .9, -1),
        (1.0, 1.5, 1.5, .9, -1),                                  # at C's centre
        (3.5, .5, .5, .9, -1),                                    # outside everything
    ]
    a = np.array(rows, np.float64)
    want = a[:, 4].astype(np.int32)
    case = dict(grid_rot=grid_rot, grid_scale=grid_scale, corner=np.array([1, 0, 0], f32), res=f32(0.5),
                points=a[:, :3].astype(f32), prob=a[:, 3].astype(f32),
                cells=np.array([cell(1, 1, 1), cell(2, 1, 1), cell(0, 3, 3)], np.int64))
    return case, want


def run_contract(case, cells=None, **kw):
    return contract(case["grid_rot"], case["grid_scale"], case["corner"], case["res"], case["points"], case["prob"],
                    case["cells"] if cells is None else cells, **kw)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_abi_version_is_still_6(built_lib):
    text = open(os.path.join(ROOT, "include", "cv_hip.h")).read()
    L = _lib.lib()
    for name in ("cv_decode_instances_workspace_bytes", "cv_decode_instances_f32"):
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared in include/cv_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # the header's parameter list and the ctypes table agree in length
    decl = re.search(r"int cv_decode_instances_f32\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["cv_decode_instances_f32"][1]) == 21
    assert int(re.search(r"#define\s+CV_ABI_VERSION\s+(\d+)", text).group(1)) == 6 == _lib.ABI_VERSION == L.cv_abi_version()
    assert L.cv_decode_instances_workspace_bytes(3, 130) >= 3 * 130 * 9 * 4
    assert L.cv_decode_instances_workspace_bytes(0, 4) == 0 and L.cv_decode_instances_workspace_bytes(_lib.MAX_CATEGORIES + 1, 4) == 0


def _call(L, **over):
    """cv_decode_instances_f32 on made-up device addresses (nothing may be launched: there is no device here)"""
    fake = lambda: _lib.vp(0x1000)
    K, M = over.pop("K", 2), over.pop("M", 4)
    a = dict(rot=fake(), scale=fake(), dims=(ctypes.c_int * 3)(4, 4, 4), corner=(ctypes.c_float * 3)(0, 0, 0), res=0.5, points=fake(),
             prob=fake(), n=10, K=K, cells=np.zeros((max(K, 1), M), np.int64), label=np.zeros((max(K, 1), M), np.int32),
             n_boxes=np.array([2] * max(K, 1), np.int32), M=M, thresh=0.3, confident=1, owner=fake(), cin=None, cown=None, ws=fake(),
             ws_bytes=L.cv_decode_instances_workspace_bytes(max(min(K, _lib.MAX_CATEGORIES), 1), M))
    a.update(over)
    return L.cv_decode_instances_f32(a["rot"], a["scale"], a["dims"], a["corner"], ctypes.c_float(a["res"]), a["points"], a["prob"],
                                     a["n"], a["K"], a["cells"].ctypes.data_as(_lib.c_i64_p), a["label"].ctypes.data_as(_lib.c_i32_p),
                                     a["n_boxes"].ctypes.data_as(_lib.c_int_p), a["M"], ctypes.c_float(a["thresh"]), a["confident"],
                                     a["owner"], a["cin"], a["cown"], a["ws"], a["ws_bytes"], None)


def _cells_with(value):
    c = np.zeros((2, 4), np.int64)
    c[1, 1] = value
    return c


@pytest.mark.parametrize("tag,over,text", [
    ("null rot grid", dict(rot=None), "null"),
    ("null scale grid", dict(scale=None), "null"),
    ("null points", dict(points=None), "null"),
    ("null owner", dict(owner=None), "null"),
    ("null prob with confident_only", dict(prob=None), "d_prob"),
    ("negative n", dict(n=-1), "n out of range"),
    ("no category", dict(K=0), "num_cats"),
    ("too many categories", dict(K=_lib.MAX_CATEGORIES + 1), "num_cats"),
    ("negative box count", dict(n_boxes=np.array([2, -1], np.int32)), "n_boxes[1]"),
    ("more boxes than max_boxes", dict(n_boxes=np.array([5, 2], np.int32)), "n_boxes[0]"),
    ("negative cell", dict(cells=_cells_with(-1)), "outside the grid"),
    ("cell == X*Y*Z", dict(cells=_cells_with(64)), "outside the grid"),
    ("workspace one byte short", dict(ws_bytes=2 * 4 * 12 * 4 - 1), "workspace too small"),
    ("null workspace", dict(ws=None), "workspace too small"),
])
def test_refusals_return_einval_without_a_device(built_lib, tag, over, text):
    L = _lib.lib()
    assert _call(L, **over) == -22, tag
    assert text in L.cv_last_error().decode(), (tag, L.cv_last_error())


def test_accepted_edge_arguments_without_a_device(built_lib):
    """what is NOT refused, on the one path that launches nothing: n == 0 (a no-op success), also with a NULL prob when the
    support is 'inside' and with cells on the grid's last cell"""
    L = _lib.lib()
    assert _call(L, n=0) == 0
    assert _call(L, n=0, prob=None, confident=0) == 0
    assert _call(L, n=0, cells=_cells_with(63)) == 0
    assert _call(L, n=0, cells=_cells_with(64), n_boxes=np.array([2, 1], np.int32)) == 0      # beyond n_boxes[1]: not read


def test_fma32_rounds_once():
    # 1 + 2^-24 + 2^-48 lies just above the tie between 1 and 1 + 2^-23: one rounding gives 1 + 2^-23; rounding the f64 sum
    # (which drops nothing here) and cases built from products that need all 48 bits
    a = f32(1 + 2.0 ** -12)
    assert fma32(a, a, f32(0)) == f32(1 + 2.0 ** -11)              # a*a = 1 + 2^-11 + 2^-24: a tie broken to even -> 1 + 2^-11
    assert fma32(a, a, f32(2.0 ** -60)) == f32(1 + 2.0 ** -11 + 2.0 ** -23)     # a hair above the tie: up (f64 alone would lose the hair)
    assert fma32(a, a, f32(-2.0 ** -60)) == f32(1 + 2.0 ** -11)
    # against exact rational arithmetic: the result is the f32 nearest to the exact value
    from fractions import Fraction
    rng = np.random.default_rng(0)
    x, y, z = [(rng.normal(size=512) * 2.0 ** rng.integers(-12, 12, 512)).astype(f32) for _ in range(3)]
    got = fma32(x, y, z)
    for xi, yi, zi, g in zip(x, y, z, got):
        exact = Fraction(float(xi)) * Fraction(float(yi)) + Fraction(float(zi))
        mine = abs(Fraction(float(g)) - exact)
        for other in (np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(-np.inf))):
            assert mine <= abs(Fraction(float(other)) - exact), (xi, yi, zi, g)
    assert np.isnan(fma32(f32(np.inf), f32(0), f32(1))) and fma32(f32(np.inf), f32(1), f32(1)) == np.inf


def test_known_answer_by_hand():
    case, want = special_case()
    owner, cin, cown = run_contract(case)
    assert owner.tolist() == want.tolist()
    # members: A rows 0, 1, 5; B rows 1, 2, 3; C none
    assert cin.tolist() == [3, 3, 0] and cown.tolist() == [3, 2, 0]
    # support 'inside': the two rows that failed on prob alone join A
    owner_in, cin_in, cown_in = run_contract(case, confident=False)
    assert [i for i in range(len(want)) if owner_in[i] != want[i]] == [9, 10] and owner_in[9] == owner_in[10] == 0
    assert cin_in.tolist() == [5, 3, 0] and cown_in.tolist() == [5, 2, 0]
    # label_of is what the owner array holds
    assert run_contract(case, label_of=[7, -5, 9])[0].tolist() == [{0: 7, 1: -5, -1: -1}[v] for v in want]


@pytest.mark.parametrize("wrong,rows", [
    (dict(strict=False), [3, 4, 6, 7, 8, 18]),   # non-strict faces: every on-face row changes hands but 5 (A's either way); 18 joins C
    (dict(prob_ge=True), [9]),                # >= on prob_thresh
    (dict(last=True), [1]),                   # the last containing box instead of the first
    (dict(use_corner=False), None),           # the centre without the corner
])
def test_named_wrong_results_differ_from_the_contract(wrong, rows):
    case, want = special_case()
    got = run_contract(case, **wrong)[0]
    diff = [i for i in range(len(want)) if got[i] != want[i]]
    assert diff, wrong
    if rows is not None:
        assert diff == rows, (wrong, diff)


def gpu_cases():
    """name -> rotated case, every one of the GPU file's (built once per process): n<N> the point-count sweep on five boxes,
    b<B> the box-count sweep on 600 points, k0..k2 three categories (70, 0 and 9 boxes) on shared points"""
    if not _CASES:
        for n in N_SWEEP:
            _CASES["n%d" % n] = make_case(100 + n, n, 5)
        for b in B_SWEEP:
            _CASES["b%d" % b] = make_case(200 + b, 600, b, scale=(0.05, 0.2))      # small boxes: the last of 130 still owns points
        pts = make_case(300, 300, 0)["points"]
        for k, b in enumerate((70, 0, 9)):
            _CASES["k%d" % k] = make_case(301 + k, 300, b, points=pts)
    return _CASES


_CASES = {}


def test_rotated_gpu_cases_keep_every_point_clear_of_every_face():
    cases = gpu_cases()
    assert len(cases) == len(N_SWEEP) + len(B_SWEEP) + 3
    for name, case in cases.items():
        assert face_margin(case) >= 1e-4, (name, face_margin(case))
    # and they are not trivial: boxes overlap (shared points exist) and own a fair share of the points
    big = cases["b130"]
    owner, cin, cown = run_contract(big, confident=False)
    assert (owner >= 0).mean() > 0.5 and cin.sum() > cown.sum() and (cin > 0).sum() > 100 and (owner >= 2 * GROUP).any()
    assert (run_contract(cases["b65"], confident=False)[0] == GROUP).any()           # the one box of the second group owns points
    assert np.array_equal(cases["k0"]["points"], cases["k2"]["points"])
