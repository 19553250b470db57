"""Independent numpy restatement of the reference vote op -- TEST INFRASTRUCTURE.

Cross-check for oracle/hv_oracle.c ("C restatement vs an independent
restatement").  Vectorised over (point, rotation); per-vote contributions are
formed in fp32 with the same operation order as hv_cuda_kernel.cu:29-59 and
accumulated in float64 with np.add.at, so it also serves as a high-precision
sum against which both the fp32-sequential C oracle and the fp32-atomic HIP
kernel can be measured.

Follows houghvoting/src/hv_cuda_kernel.cu:25-96 (vote), :106-118 (average),
:129-134 (grid dims).

Below the restatement: the float64 reference and error model of the vote's gradient (hv_backward64, VOTE_BWD_ERROR_MODEL), the
exact restatement of the tile algorithm's 2^-36 fixed-point sums (hv_forward_fixed: the bits hv_fwd_tiles must write) and the
float64 reference and error model of the direct forward kernel (hv_forward64, VOTE_FWD_ERROR_MODEL).
"""
import numpy as np

f32 = np.float32


def grid_dims(points, res):
    pts = np.asarray(points, f32)
    mn = pts.min(0)
    mx = pts.max(0)
    diff = ((mx - mn).astype(f32) / f32(res)).astype(f32)     # :131 fp32 tensor ops
    dims = [int(np.trunc(d)) + 1 for d in diff]               # :132 .to<int>() + 1
    return mn, mx, dims


def rot_table(num_rots):
    rot_interval = f32(f32(2) * f32(3.141592654)) / f32(num_rots)   # :35
    theta = (np.arange(num_rots).astype(f32) * rot_interval).astype(f32)  # :37
    return np.cos(theta.astype(np.float64)).astype(f32), np.sin(theta.astype(np.float64)).astype(f32)


def vote_geometry(points, xyz, scale, res, num_rots, corner, dims):
    """The in-bounds votes of hv_bwd / hv_fwd (hv_vote.hip) in fp32 with their operation order (the library is built with
    -ffp-contract=off, so these are the kernel's bits): (pi, ri, fl[3] int64, w0[3] f32, w1[3] f32) - point and rotation of
    every in-bounds vote, its floor cell and its two trilinear weights per axis, w0 = 1 - fr rounded to fp32."""
    pts = np.asarray(points, f32)
    xyz = np.asarray(xyz, f32)
    scale = np.asarray(scale, f32)
    res = f32(res)
    corner = np.asarray(corner, f32)
    X, Y, Z = dims
    ct, st = rot_table(num_rots)
    corr = (xyz * scale).astype(f32)
    cx, cy, cz = corr[:, 0:1], corr[:, 1:2], corr[:, 2:3]
    ox = ((-ct)[None] * cx).astype(f32) + (st[None] * cz).astype(f32)
    oy = np.broadcast_to(-cy, ox.shape)
    oz = ((-st)[None] * cx).astype(f32) - (ct[None] * cz).astype(f32)
    g = [(((pts[:, k:k + 1] + o).astype(f32) - corner[k]).astype(f32) / res).astype(f32)
         for k, o in enumerate((ox, oy, oz))]
    ok = (g[0] >= 0) & (g[1] >= 0) & (g[2] >= 0) & (g[0] < f32(X - 1)) & (g[1] < f32(Y - 1)) & (g[2] < f32(Z - 1))
    pi, ri = np.nonzero(ok)
    gv = [a[pi, ri] for a in g]
    fl = [np.trunc(a).astype(np.int64) for a in gv]
    w1 = [(a - np.floor(a)).astype(f32) for a in gv]
    w0 = [(f32(1) - a).astype(f32) for a in w1]
    return pi, ri, fl, w0, w1


def hv_forward(points, xyz, scale, obj, res, num_rots, acc_dtype=np.float64):
    pts = np.asarray(points, f32)
    scale = np.asarray(scale, f32)
    obj = np.asarray(obj, f32)
    corner, _, dims = grid_dims(pts, f32(res))
    X, Y, Z = dims
    ct, st = rot_table(num_rots)
    pi, ri, fl, w0, w1 = vote_geometry(pts, xyz, scale, res, num_rots, corner, dims)   # :29-50
    o = obj[pi]
    g_obj = np.zeros(X * Y * Z, acc_dtype)
    g_rot = np.zeros((X * Y * Z, 2), acc_dtype)
    g_scale = np.zeros((X * Y * Z, 3), acc_dtype)
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                wx = (w1 if bx else w0)[0]
                wy = (w1 if by else w0)[1]
                wz = (w1 if bz else w0)[2]
                w = (((wx * wy).astype(f32) * wz).astype(f32) * o).astype(f32)   # :52-59
                cell = ((fl[0] + bx) * Y + (fl[1] + by)) * Z + (fl[2] + bz)
                np.add.at(g_obj, cell, w.astype(acc_dtype))
                np.add.at(g_rot[:, 0], cell, (w * ct[ri]).astype(f32).astype(acc_dtype))
                np.add.at(g_rot[:, 1], cell, (w * st[ri]).astype(f32).astype(acc_dtype))
                for j in range(3):
                    np.add.at(g_scale[:, j], cell, (w * scale[pi, j]).astype(f32).astype(acc_dtype))
    # :112-117  x /= w + 1e-7 (double), stored as float.  The grid weight the
    # reference divides by is the fp32-accumulated one; mirror that rounding.
    w32 = g_obj.astype(f32)
    d = w32.astype(np.float64) + 1e-7
    g_rot = (g_rot.astype(f32).astype(np.float64) / d[:, None]).astype(f32)
    g_scale = (g_scale.astype(f32).astype(np.float64) / d[:, None]).astype(f32)
    return (w32.reshape(X, Y, Z), g_rot.reshape(X, Y, Z, 2), g_scale.reshape(X, Y, Z, 3), len(pi))


def contribution_counts(points, xyz, scale, res, num_rots, corner=None, dims=None, chunk=20000):
    """int32 [X,Y,Z]: how many (vote, corner) contributions each cell receives (hv_cuda_kernel.cu:41-96: eight per
    in-bounds vote).  Tests use it to state the accumulated-rounding bound of a cell's sums; the geometry is vote_geometry's,
    chunked over points so that a 300k-point scene stays within a few hundred MB."""
    pts = np.asarray(points, f32)
    xyz = np.asarray(xyz, f32)
    scale = np.asarray(scale, f32)
    if corner is None:
        corner, _, dims = grid_dims(pts, f32(res))
    X, Y, Z = dims
    counts = np.zeros(X * Y * Z, np.int64)
    for a in range(0, len(pts), chunk):
        _, _, fl, _, _ = vote_geometry(pts[a:a + chunk], xyz[a:a + chunk], scale[a:a + chunk], res, num_rots, corner, dims)
        base = (fl[0] * Y + fl[1]) * Z + fl[2]
        for bx in (0, 1):
            for by in (0, 1):
                for bz in (0, 1):
                    counts += np.bincount(base + (bx * Y + by) * Z + bz, minlength=X * Y * Z)
    return counts.reshape(X, Y, Z).astype(np.int32)


# the eight cells of a vote in the order hv_bwd reads them (lll llh lhl lhh hll hlh hhl hhh): (bx, by, bz)
CELLS = [(bx, by, bz) for bx in (0, 1) for by in (0, 1) for bz in (0, 1)]


def gather_cells(grad, fl):
    """float64 [8, votes]: grad at the eight cells of every vote, CELLS order"""
    grad = np.asarray(grad, f32)
    return np.stack([grad[fl[0] + bx, fl[1] + by, fl[2] + bz] for bx, by, bz in CELLS]).astype(np.float64)


def backward_sums(cells, w0, w1, pi, ri, xyz, scale, obj, num_rots):
    """The sums of hv_bwd over the given votes in float64, and the same sums with every product replaced by its absolute
    value.  cells [8, votes] float64 (gather_cells), w0 / w1 the fp32 weights, pi / ri the point and rotation of each vote.
    -> dict(d_xyz [n,3], d_scale [n,3], d_obj [n], m_xyz, m_scale, m_obj, votes [n])"""
    f64 = np.float64
    xyz = np.asarray(xyz, f32).astype(f64)
    scale = np.asarray(scale, f32).astype(f64)
    obj = np.asarray(obj, f32).astype(f64)
    n = len(obj)
    ct, st = (a.astype(f64)[ri] for a in rot_table(num_rots))
    W = [[a.astype(f64) for a in w0], [a.astype(f64) for a in w1]]
    dob = np.zeros(len(pi)); mob = np.zeros(len(pi))
    d = [np.zeros(len(pi)) for _ in range(3)]
    m = [np.zeros(len(pi)) for _ in range(3)]
    for g, b in zip(cells, CELLS):
        t = g * W[b[0]][0] * W[b[1]][1] * W[b[2]][2]
        dob += t
        mob += np.abs(t)
        for k in range(3):                      # d/d(axis k): the other two weights, - for the low cell, + for the high
            a, c = [j for j in range(3) if j != k]
            t = g * W[b[a]][a] * W[b[c]][c]
            d[k] += t if b[k] else -t
            m[k] += np.abs(t)
    ob = obj[pi]
    d = [v * ob for v in d]
    m = [v * np.abs(ob) for v in m]
    dc = [-ct * d[0] - st * d[2], -d[1], st * d[0] - ct * d[2]]
    mc = [np.abs(ct) * m[0] + np.abs(st) * m[2], m[1], np.abs(st) * m[0] + np.abs(ct) * m[2]]

    def per_point(v):
        return np.bincount(pi, weights=v, minlength=n)

    out = dict(d_obj=per_point(dob), m_obj=per_point(mob), votes=np.bincount(pi, minlength=n).astype(np.int64))
    for name, other in (("xyz", scale), ("scale", xyz)):
        out["d_" + name] = np.stack([per_point(dc[k] * other[pi, k]) for k in range(3)], 1)
        out["m_" + name] = np.stack([per_point(mc[k] * np.abs(other[pi, k])) for k in range(3)], 1)
    return out


def hv_backward64(grad, points, xyz, scale, obj, res, num_rots, corner):
    """float64 reference of the vote's gradient (hv_bwd of hv_vote.hip, hv_cuda_kernel.cu:183-260).  The geometry - offsets,
    grid_pos, the bounds test, trunc, fr and w0 = 1 - fr - is fp32 in hv_forward's operation order, which is the kernel's bit
    for bit; everything after the weights is float64.  grad.shape gives the grid, corner its origin.
    -> dict(d_xyz, d_scale, d_obj, m_xyz, m_scale, m_obj, votes): per point the sums, their magnitudes (every product
    replaced by its absolute value) and the number of in-bounds rotations."""
    grad = np.asarray(grad, f32)
    pi, ri, fl, w0, w1 = vote_geometry(points, xyz, scale, res, num_rots, corner, grad.shape)
    return backward_sums(gather_cells(grad, fl), w0, w1, pi, ri, xyz, scale, obj, num_rots)


U24 = 2.0 ** -24
VOTE_BWD_C0 = {"d_obj": 3, "d_xyz": 14, "d_scale": 14}
VOTE_BWD_K = {"d_obj": 8, "d_xyz": 1, "d_scale": 1}
VOTE_BWD_ERROR_MODEL = """Error model of hv_bwd (hv_vote.hip), per output element, against hv_backward64.  u = 2^-24.

    bound = (c0 + k * votes) * u * magnitude + 2^-149

votes is the number of in-bounds rotations of the point, magnitude the output's sum with every product replaced by its
absolute value.  The weights are the kernel's own bits (vote_geometry), so the only error is the rounding of the fp32
products and additions behind them.  An output is a sum of terms t; the kernel computes sum t * prod (1 + d_j), |d_j| <= u,
one factor for each rounded operation a term passes through, so |error| <= ((1 + u)^p - 1) * sum |t| with p the longest
such path - whatever the order of the additions, hence nothing here knows of the lane loop or the butterfly.

  d_obj    term = grad * w * w * w: 3 products.  8 terms per vote, 8 * votes terms in all; summed in any order a term passes
           through at most 8 * votes - 1 additions (one less than the number of terms).  p <= 3 + 8 * votes - 1.
           c0 = 3, k = 8.
  d_xyz    term = grad * w * w * obj * cos|sin * scale.  Longest path, through d_xyz[0] / [2]: 2 products, the 7 additions
  d_scale  of the eight-term dx / dz, * obj, * cos|sin, the addition of the two halves of dcx / dcz, * scale (or * xyz): 13.
           Then one such value per vote is summed: at most votes - 1 additions.  p <= 12 + votes; d_xyz[1] has three less.
           c0 = 14, k = 1 (two roundings of margin over the count).

(1 + u)^p - 1 <= p u / (1 - p u); the spare rounding of d_obj and the two of d_xyz cover the second-order part while
p^2 u < 1, that is up to 511 in-bounds votes of a point for d_obj (R <= 511) and every R the op takes for the others.
2^-149 is the one fp32 subnormal a flushed or underflowed term can cost; the C oracle (fp32, sequential) stays below 0.3 of
the bound on the cases of tests/test_vote_bound.py."""


def vote_bwd_bounds(ref):
    """dict(d_xyz, d_scale, d_obj) of per-element bounds for a result of hv_backward64 (VOTE_BWD_ERROR_MODEL)"""
    out = {}
    for name in ("d_xyz", "d_scale", "d_obj"):
        v = ref["votes"].astype(np.float64)
        if name != "d_obj":
            v = v[:, None]
        out[name] = (VOTE_BWD_C0[name] + VOTE_BWD_K[name] * v) * U24 * ref["m_" + name[2:]] + 2.0 ** -149
    return out


# ---------------------------------------------------------------------------
# forward vote: the exact restatement of the tile algorithm, and the direct kernel's float64 reference and error model
# ---------------------------------------------------------------------------
FX_SCALE = 2.0 ** 36           # hv_vote.hip: every fp32 contribution is rounded once to a multiple of 2^-36
FX_CLAMP = f32(6.0e7)          # fx_from_float: contributions beyond it are clamped


def fx_quantum(v, truncate=False):
    """int64 round(clip(v, -6e7, 6e7) * 2^36), ties to even: the word fx_from_float (hv_vote.hip) adds for the fp32
    contribution v.  v * 2^36 is exact in float64, so both of the kernel's conversions - the magic-number fma inside
    |v| < 2^15 and __double2ll_rn of the clamped value - give this word.  truncate: towards zero instead (a named wrong
    result of tests/test_vote_fixed.py, not the kernel)."""
    d = np.clip(np.asarray(v, f32), -FX_CLAMP, FX_CLAMP).astype(np.float64) * FX_SCALE
    return (np.trunc(d) if truncate else np.rint(d)).astype(np.int64)


def vote_contributions(points, xyz, scale, obj, res, num_rots, corner, dims, chunk=2000):
    """Generator over chunks of points: (cell int64 [m], t f32 [6, m], point int64 [m]) - every (in-bounds vote, corner)
    contribution: its flat cell, the six fp32 terms in channel order (objectness weight, w cos, w sin, w s0, w s1, w s2) and the
    point it comes from.  w = ((wx wy) wz) obj and t = w c are single fp32 operations in the order of hv_fwd_direct and
    drain_vote (hv_vote.hip) on vote_geometry's bits, so the terms are the kernels' bits."""
    pts = np.asarray(points, f32)
    xyz = np.asarray(xyz, f32)
    scale = np.asarray(scale, f32)
    obj = np.asarray(obj, f32)
    X, Y, Z = dims
    ct, st = rot_table(num_rots)
    for a in range(0, len(pts), chunk):
        pi, ri, fl, w0, w1 = vote_geometry(pts[a:a + chunk], xyz[a:a + chunk], scale[a:a + chunk], res, num_rots, corner, dims)
        pi = pi + a
        o = obj[pi]
        chan = (ct[ri], st[ri], scale[pi, 0], scale[pi, 1], scale[pi, 2])
        base = (fl[0] * Y + fl[1]) * Z + fl[2]
        cells, terms = [], []
        for bx, by, bz in CELLS:
            w = ((((w1 if bx else w0)[0] * (w1 if by else w0)[1]).astype(f32) * (w1 if bz else w0)[2]).astype(f32) * o).astype(f32)
            cells.append(base + (bx * Y + by) * Z + bz)
            terms.append(np.stack([w] + [(w * c).astype(f32) for c in chan]))
        yield np.concatenate(cells), np.concatenate(terms, 1), np.tile(pi, 8)


def obj_quantum(w, truncate=False, nonzero_rule=True):
    """the objectness channel's word (lds_add_obj): fx_quantum, but a non-zero weight never rounds to zero - it adds one
    quantum of its sign"""
    q = fx_quantum(w, truncate)
    if nonzero_rule:
        q = np.where((q == 0) & (w != 0), np.sign(w).astype(np.int64), q)
    return q


def reduce_by_cell(cell, values):
    """(sorted unique cells, int64 sums [C, cells]) of values [C, m] - sort and np.add.reduceat, one channel at a time;
    int64 addition wraps as the kernel's does"""
    if len(cell) == 0:
        return cell.astype(np.int64), np.zeros((len(values), 0), np.int64)
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    starts = np.concatenate([[0], np.flatnonzero(sc[1:] != sc[:-1]) + 1])
    return sc[starts], np.stack([np.add.reduceat(v[order], starts) for v in values])


def fixed_sums(points, xyz, scale, obj, res, num_rots, corner, dims, truncate=False, nonzero_rule=True, chunk=2000):
    """(cells int64 [c] sorted, sums int64 [6, c], counts int64 [c]): the tile algorithm's six integer sums at every cell that
    receives a contribution, and how many it receives.  Memory goes with a chunk's contributions, not with the grid."""
    ucells, usums = [], []
    for cell, t, _ in vote_contributions(points, xyz, scale, obj, res, num_rots, corner, dims, chunk):
        q = [obj_quantum(t[0], truncate, nonzero_rule)] + [fx_quantum(v, truncate) for v in t[1:]]
        c, s = reduce_by_cell(cell, q + [np.ones(len(cell), np.int64)])
        ucells.append(c)
        usums.append(s)
    if not ucells:
        return np.zeros(0, np.int64), np.zeros((6, 0), np.int64), np.zeros(0, np.int64)
    c, s = reduce_by_cell(np.concatenate(ucells), list(np.concatenate(usums, 1)))
    return c, s[:6], s[6]


def fixed_store(sums, double_divisor=False):
    """(obj32 [c], quot f32 [5, c]) the tile kernel stores for the integer sums [6, c]: obj32 = float(sum0 2^-36), each quotient
    float(double(float(sum_k 2^-36)) / (double(obj32) + 1e-7)).  double_divisor: divide by the unrounded double sum instead
    (a named wrong result, not the kernel)."""
    val = sums.astype(np.float64) * (1.0 / FX_SCALE)
    obj32 = val[0].astype(f32)
    d = (val[0] if double_divisor else obj32.astype(np.float64)) + 1e-7
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (val[1:].astype(f32).astype(np.float64) / d).astype(f32)
    return obj32, quot


def dense_grids(cells, obj32, quot, dims):
    """the three dense float32 grids of sparse results, zeros elsewhere"""
    X, Y, Z = dims
    g_obj = np.zeros(X * Y * Z, f32)
    g_rot = np.zeros((X * Y * Z, 2), f32)
    g_scale = np.zeros((X * Y * Z, 3), f32)
    g_obj[cells] = obj32
    g_rot[cells] = quot[:2].T
    g_scale[cells] = quot[2:].T
    return g_obj.reshape(X, Y, Z), g_rot.reshape(X, Y, Z, 2), g_scale.reshape(X, Y, Z, 3)


def hv_forward_fixed(points, xyz, scale, obj, res, num_rots, corner=None, dims=None, thresh=None):
    """The bits hv_fwd_tiles (hv_vote.hip) must write, whatever its launch shape: (grid_obj, grid_rot, grid_scale) float32.

    Per in-bounds vote and corner the six fp32 terms of vote_contributions; each is rounded once to an int64 multiple of 2^-36
    (fx_quantum; objectness: obj_quantum), the words are summed per cell and channel as integers - exact and independent of
    the order, so no cull, work list, part or round of the kernel may show in them - and stored by fixed_store.  Cells
    without a contribution are zeros.  corner / dims: the grid of a vote into a box (default: the points' bounding box).
    thresh (cv_hv_forward_peaks_f32): a fourth value, the mask grid_obj >= thresh; the quotients are defined only there."""
    pts = np.asarray(points, f32)
    if corner is None:
        corner, _, dims = grid_dims(pts, f32(res))
    cells, sums, _ = fixed_sums(pts, xyz, scale, obj, res, num_rots, corner, dims)
    grids = dense_grids(cells, *fixed_store(sums), dims)
    if thresh is None:
        return grids
    return grids + (grids[0] >= f32(thresh),)


def hv_forward64(points, xyz, scale, obj, res, num_rots, corner=None, dims=None):
    """float64 reference of the forward vote's sums before the division: dict(sum [X,Y,Z,6], mag [X,Y,Z,6], count [X,Y,Z]) -
    per cell and channel (objectness, cos, sin, s0, s1, s2) the float64 sum of the fp32 terms of vote_contributions (the
    kernels' bits), the sum of their absolute values, and the number of contributions n_c (contribution_counts)."""
    pts = np.asarray(points, f32)
    if corner is None:
        corner, _, dims = grid_dims(pts, f32(res))
    X, Y, Z = dims
    n = X * Y * Z
    total = np.zeros((6, n))
    mag = np.zeros((6, n))
    count = np.zeros(n, np.int64)
    for cell, t, _ in vote_contributions(pts, xyz, scale, obj, res, num_rots, corner, dims):
        count += np.bincount(cell, minlength=n)
        for k in range(6):
            v = t[k].astype(np.float64)
            total[k] += np.bincount(cell, weights=v, minlength=n)
            mag[k] += np.bincount(cell, weights=np.abs(v), minlength=n)
    return dict(sum=total.T.reshape(X, Y, Z, 6).copy(), mag=mag.T.reshape(X, Y, Z, 6).copy(), count=count.reshape(X, Y, Z))


VOTE_FWD_ERROR_MODEL = """Error model of the direct forward vote (hv_fwd_direct + hv_normalise, hv_vote.hip), per output element,
against hv_forward64.  u = 2^-24, gamma(n) = n u / (1 - n u).

The terms are the kernel's own bits (vote_contributions), so the only errors are those of the fp32 atomic additions, in whatever
order they arrive, and of the division.

  a sum of n_c terms t (grid_obj, and the numerators N of the quotients):
      b = gamma(n_c) * sum |t| + n_c * 2^-126
    Summed in any order a term passes through at most n_c - 1 additions, each (1 + d), |d| <= u: the error is at most
    ((1 + u)^(n_c - 1) - 1) sum |t| <= gamma(n_c - 1) sum |t|; gamma(n_c) leaves one rounding spare.  The second part covers an
    atomic unit that flushes a subnormal operand or result to zero: at most the smallest normal number per addition.

  a quotient q = N / D, D = sum_obj + 1e-7 (hv_normalise: float(double(N32) / (double(D32) + 1e-7))):
      b_q = (b_N + |q| b_D) / (D - b_D) + 2 u |q| + 2^-149
    |N32 / D32' - N / D| <= (|N32 - N| + |q| |D32' - D|) / D32' and D32' >= D - b_D, valid where D - b_D > 0 (the tests assert
    it at every touched cell; it holds wherever objectness >= 0).  The division is double, its result rounded once to fp32:
    u |q'| <= 2 u |q| while the first part is below |q|, and one subnormal.

  cells without a contribution: exact zeros in all three grids (0 / 1e-7)."""


def vote_fwd_bounds(ref):
    """dict(obj, rot, scale: the float64 values the direct kernel approximates; b_obj, b_rot, b_scale: their per-element bounds
    (VOTE_FWD_ERROR_MODEL); margin [X,Y,Z]: D - b_D, which must be > 0 wherever count > 0) for a result of hv_forward64"""
    n = ref["count"].astype(np.float64)[..., None]
    b = n * U24 / (1.0 - n * U24) * ref["mag"] + n * 2.0 ** -126
    D = ref["sum"][..., 0:1] + 1e-7
    bD = b[..., 0:1]
    margin = D - bD
    q = ref["sum"][..., 1:] / D
    with np.errstate(divide="ignore", invalid="ignore"):
        bq = (b[..., 1:] + np.abs(q) * bD) / margin + 2 * U24 * np.abs(q) + 2.0 ** -149
    bq = np.where(margin > 0, bq, np.nan)
    return dict(obj=ref["sum"][..., 0], rot=q[..., :2], scale=q[..., 2:], b_obj=b[..., 0], b_rot=bq[..., :2],
                b_scale=bq[..., 2:], margin=margin[..., 0])
