"""A full-grid, sequential restatement of the detection decode in CPU torch, and hand-made edge cases for it.

Shared by tests/test_decode_ref.py (CPU: the cases' claims, oracle/decode_oracle.c against this restatement, named wrong
results, the reference's own lines through tests/golden/*.npz) and tests/test_decode_edge_gpu.py (the kernels of
csrc/hv_decode.hip against this restatement).  It calls into neither `oracle` nor the HIP library.

  1. Restatement (`decode`).  The tensor operations of the reference loop (eval_joint.py:195-263, the eval_separate.py:209
     slice as a switch), one after the other, on the WHOLE grid: torch.argmax over the full grid (first maximum = lowest flat
     index), the cube zeroed by slicing with max(c - e, 0), the box cells from a meshgrid clamped to the grid (:223), both masks
     as -1 < w < 1, masked boolean indexing, torch.unique(return_counts=True) + argmax for the class, max over the in-box
     probabilities for the score.  The kernels and oracle/decode_oracle.c work on a compacted list of cells >= thresh_high,
     with division-free box tests, histograms and clamped loop bounds instead: none of that structure is shared here.
     fp32 conventions (those the head of oracle/decode_oracle.c documents, and only those): atan2 / cos / sin in double and
     rounded to float; [.,3] @ [3,3] as three separately rounded products summed in k order, (d0 R0j + d1 R1j) + d2 R2j, no
     fused multiply-add; x / res as x * float32(1 / float32(res)); true division by the scale; the masked mean summed in
     double; valid_ratio * n_in in fp32.
  2. `wrong=`: named wrong results (WRONG), each a one-line deviation a kernel could plausibly have.
  3. Cases (CASES: name -> generator of a Case).  All seeded; grids hold no NaN, class ids lie in [0, 64), probabilities >= 0.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

F32 = np.float32
WRONG = ("tie_highest_index", "face_inclusive", "cube_plus1_swapped", "valid_ratio_inclusive", "thresh_low_inclusive",
         "class_tie_highest", "prob_mask_inclusive", "listed_strict", "mean_over_in_box", "rotation_transposed")
RAW = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, -1], [-1, 1, 1], [1, -1, 1], [1, -1, -1], [-1, -1, -1], [-1, -1, 1]], F32)


# ====================================================================================================== 1. restatement
def matmul3(a, B):
    """a [M,3] @ B [3,3] in fp32: three separately rounded products per element, summed in k order"""
    return (a[:, 0:1] * B[0:1] + a[:, 1:2] * B[1:2]) + a[:, 2:3] * B[2:3]


def strictly_inside(w, inclusive=False):
    if inclusive:
        return ((-1 <= w) & (w <= 1)).all(-1)
    return ((-1 < w) & (w < 1)).all(-1)


def decode(grid_obj, grid_rot, grid_scale, corner, res, points, xyz_pred, prob_pred, class_pred=None, thresh_high=60.0,
           thresh_low=10.0, valid_ratio=0.2, elimination=2, prob_thresh=0.3, err_thresh=0.3, separate_variant=False,
           max_candidates=512, wrong=None):
    """Returns dict(cand_idx, verdict, boxes [K,8,3], scores, classes, grid_obj_after, truncated).  verdict: 0 accepted,
    1 too few (confident) points (:246-247), 2 LCC error (:252-253).  `truncated`: the walk stopped at max_candidates with
    a cell >= thresh_high still in the grid (the reference has no cap; this is the capped walk the kernels define).
    class_pred None: class 0 everywhere."""
    assert wrong is None or wrong in WRONG, wrong
    g = torch.from_numpy(np.array(grid_obj, F32, copy=True))
    X, Y, Z = g.shape
    shape = torch.tensor([X, Y, Z])
    g_rot = torch.from_numpy(np.ascontiguousarray(grid_rot, F32))
    g_scale = torch.from_numpy(np.ascontiguousarray(grid_scale, F32))
    pts = torch.from_numpy(np.ascontiguousarray(points, F32))
    xyz = torch.from_numpy(np.ascontiguousarray(xyz_pred, F32))
    prob = torch.from_numpy(np.ascontiguousarray(prob_pred, F32))
    cls = torch.zeros(len(pts), dtype=torch.int64) if class_pred is None else torch.from_numpy(np.asarray(class_pred, np.int64))
    corner = torch.from_numpy(np.ascontiguousarray(corner, F32))
    res32 = torch.tensor(res, dtype=torch.float32)
    inv_res = torch.tensor(1.0, dtype=torch.float32) / res32
    raw = torch.from_numpy(RAW)
    th_high, th_low, vr = F32(thresh_high), torch.tensor(thresh_low, dtype=torch.float32), torch.tensor(valid_ratio, dtype=torch.float32)
    pth = torch.tensor(prob_thresh, dtype=torch.float32)
    e = int(elimination)
    plus1 = 0 if separate_variant else 1
    if wrong == "cube_plus1_swapped":
        plus1 = 1 - plus1
    incl = wrong == "face_inclusive"
    cand_idx, verdict, boxes, scores, classes = [], [], [], [], []
    truncated = False
    while True:
        flat = int(torch.argmax(g))                                                   # :205 first maximum in flat order
        if wrong == "tie_highest_index":
            flat = int(torch.nonzero(g.reshape(-1) == g.max())[-1])
        cx, cy, cz = flat // (Y * Z), flat // Z % Y, flat % Z
        top = g[cx, cy, cz].item()
        if top < th_high or (wrong == "listed_strict" and top <= th_high):            # :208-209
            break
        if len(cand_idx) >= max_candidates:
            truncated = True
            break
        cand_idx.append(flat)
        cand = torch.tensor([cx, cy, cz])
        cw = corner + res32 * cand.float()                                            # :206
        g[max(cx - e, 0):cx + e + plus1, max(cy - e, 0):cy + e + plus1, max(cz - e, 0):cz + e + plus1] = 0   # :211
        r0, r1 = float(g_rot[cx, cy, cz, 0]), float(g_rot[cx, cy, cz, 1])
        rot = float(F32(math.atan2(r1, r0)))                                          # :214
        c, s = float(F32(math.cos(rot))), float(F32(math.sin(rot)))
        R = torch.tensor([[c, 0, -s], [0, 1, 0], [s, 0, c]], dtype=torch.float32)     # :215
        if wrong == "rotation_transposed":
            R = R.T.contiguous()
        sc = g_scale[cx, cy, cz]                                                      # :216
        M = R * sc[None, :]                                                           # R @ diag(scale)
        bbox = matmul3(raw, M.T.contiguous())                                         # :219
        lo, hi = bbox.min(0)[0], bbox.max(0)[0]
        blo, bhi = (lo * inv_res).int(), (hi * inv_res).int()                         # :220 (truncation towards zero)
        cc = torch.stack(torch.meshgrid(*[torch.arange(int(blo[k]), int(bhi[k]) + 1) for k in range(3)], indexing="ij"),
                         -1).reshape(-1, 3) + cand                                    # :221-222
        cc = torch.max(torch.min(cc, shape - 1), torch.zeros(3, dtype=torch.int64))   # :223
        w_cells = matmul3((cc - cand).float() * res32, R) / sc                        # :225
        inb = cc[strictly_inside(w_cells, incl)]                                      # :226-229
        w_pts = matmul3(pts - cw, R) / sc                                             # :231
        in_world = strictly_inside(w_pts, incl)                                       # :232-234
        g[inb[:, 0], inb[:, 1], inb[:, 2]] = 0                                        # :243
        in_prob = prob[in_world]
        mask = in_prob >= pth if wrong == "prob_mask_inclusive" else in_prob > pth    # :245
        n_in, n_mask = in_world.sum().float(), mask.sum().float()
        few = n_mask <= vr * n_in if wrong == "valid_ratio_inclusive" else n_mask < vr * n_in
        low = n_in <= th_low if wrong == "thresh_low_inclusive" else n_in < th_low
        if bool(few) or bool(low):                                                    # :246-247
            verdict.append(1)
            continue
        d = xyz[in_world][mask] - w_pts[in_world][mask]                               # :249-250
        q = d * d
        term = torch.sqrt((q[:, 0] + q[:, 1]) + q[:, 2]) * in_prob[mask]
        denom = n_in if wrong == "mean_over_in_box" else n_mask
        error = float(F32(float(term.double().sum()) / float(denom)))
        if error > err_thresh:                                                        # :252-253
            verdict.append(2)
            continue
        elems, counts = torch.unique(cls[in_world][mask], return_counts=True)         # :255-256
        pick = int(torch.nonzero(counts == counts.max())[-1]) if wrong == "class_tie_highest" else int(torch.argmax(counts))
        verdict.append(0)
        classes.append(int(elems[pick]))
        scores.append(float(in_prob.max()))                                           # :258
        boxes.append((bbox + cw).numpy())                                             # :259
    return dict(cand_idx=np.array(cand_idx, np.int64), verdict=np.array(verdict, np.int32),
                boxes=np.array(boxes, F32).reshape(-1, 8, 3), scores=np.array(scores, F32),
                classes=np.array(classes, np.int32), grid_obj_after=g.numpy(), truncated=truncated)


# ============================================================================================================= 3. cases
@dataclass
class Case:
    grid_obj: np.ndarray
    grid_rot: np.ndarray
    grid_scale: np.ndarray
    corner: np.ndarray
    res: float
    pts: np.ndarray
    xyz: np.ndarray
    prob: np.ndarray
    cls: np.ndarray
    kw: dict = field(default_factory=dict)        # decode keywords (the names of decode_boxes and of `decode` above)
    allow_truncation: bool = False                # the capped walk is what the case is about
    claims: dict = field(default_factory=dict)    # what the case exists for; tests/test_decode_ref.py asserts each

    def args(self):
        return self.grid_obj, self.grid_rot, self.grid_scale, self.corner, self.res, self.pts, self.xyz, self.prob, self.cls

    def listed(self):
        return int((self.grid_obj >= F32(self.kw.get("thresh_high", 60.0))).sum())


def rot_of(yaw, dims):
    yaw = np.broadcast_to(np.asarray(yaw, np.float64), dims)
    return np.stack([np.cos(yaw), np.sin(yaw)], -1).astype(F32)


def flat_of(dims, c):
    return (c[0] * dims[1] + c[1]) * dims[2] + c[2]


LEN_SMALL = (1, 63, 64, 65, 511, 512, 513, 1535, 1536, 1537, 4095, 4096, 4097)
LEN_BIG = (24575, 24576, 24577)


def len_parts(L, dims, seed):
    """exactly L cells of integer value 60..63 at the places a seeded permutation picks, every other cell below 60; random
    yaw and scale 0.1 .. 0.3 m per cell (res 0.05: a candidate suppresses hundreds of cells).  Predictions: probabilities
    around prob_thresh and canonical coordinates of zero put the confident fraction near valid_ratio and the error near
    err_thresh, so all three verdicts occur."""
    rng = np.random.default_rng(seed)
    G = dims[0] * dims[1] * dims[2]
    g = rng.integers(20, 60, G).astype(F32)
    g[rng.permutation(G)[:L]] = rng.integers(60, 64, L).astype(F32)
    g = g.reshape(dims)
    assert int((g >= 60).sum()) == L
    rot = rot_of(rng.uniform(-np.pi, np.pi, dims), dims)
    scale = rng.uniform(0.1, 0.3, dims + (3,)).astype(F32)
    xyz = rng.normal(0, 0.05, (600, 3)).astype(F32)
    prob = rng.uniform(0.1, 0.36, 600).astype(F32)
    return g, rot, scale, xyz, prob


def len_points(dims, res=0.05):
    rng = np.random.default_rng(77)
    pts = (rng.uniform(0, 1, (600, 3)) * (np.array(dims) * res)).astype(F32)
    return pts, rng.integers(0, 64, 600).astype(np.int32)


def len_case(L):
    dims = (20, 12, 20) if L <= 4800 else (40, 20, 40)
    g, rot, scale, xyz, prob = len_parts(L, dims, 1000 + L)
    pts, cls = len_points(dims)
    return Case(g, rot, scale, np.zeros(3, F32), 0.05, pts, xyz, prob, cls, kw=dict(max_candidates=1024), claims=dict(listed=L))


FACE_YAWS = {"0": (1.0, 0.0), "90": (0.0, 1.0), "m90": (0.0, -1.0), "180": (-1.0, 0.0),
             "45": (math.cos(math.pi / 4), math.sin(math.pi / 4))}
FACE_DIMS, FACE_PEAK, FACE_RES = (13, 7, 13), (6, 3, 6), 0.0625
FACE_PEAK_SCALE = (4, -2, 3)          # in cells


def faces_case(yaw, separate=False, nudge=None):
    """every cell 61 against thresh_high 60 and one peak; every scale a signed integer multiple of res = 1/16, elimination 0:
    the box test alone decides.  At yaw 0 a cell k = |scale| / res steps from the candidate along an axis has |t| == |s| bit
    for bit and survives; `nudge` moves the peak's x scale one ulp inward / outward (outward: its face cells die)."""
    rng = np.random.default_rng(5)
    dims, res = FACE_DIMS, FACE_RES
    g = np.full(dims, 61, F32)
    g[FACE_PEAK] = 100
    rot = np.broadcast_to(np.array(FACE_YAWS[yaw], F32), dims + (2,)).copy()
    scale = (rng.integers(1, 4, dims + (3,)) * rng.choice([-1, 1], dims + (3,)) * res).astype(F32)
    scale[FACE_PEAK] = np.array(FACE_PEAK_SCALE, F32) * F32(res)
    if nudge:
        scale[FACE_PEAK][0] = np.nextafter(scale[FACE_PEAK][0], F32(0 if nudge == "in" else 1))
    n = 200
    pts = (rng.integers(0, 16 * 13, (n, 3)) / 256.0).astype(F32)      # exact multiples of res / 16
    pts[0] = 0
    xyz = (rng.integers(-8, 9, (n, 3)) / 64.0).astype(F32)
    prob = (rng.integers(0, 33, n) / 64.0).astype(F32)
    cls = rng.integers(0, 64, n).astype(np.int32)
    return Case(g, rot, scale, np.zeros(3, F32), res, pts, xyz, prob, cls,
                kw=dict(elimination=0, separate_variant=separate, max_candidates=2048, thresh_low=3),
                claims=dict(listed=dims[0] * dims[1] * dims[2], yaw=yaw, nudge=nudge))


CORNER_DIMS = ((9, 7, 11), (5, 300, 3), (300, 2, 7), (40, 1, 40), (1, 1, 1))
CORNER_ELIM = ((0, False), (0, True), (2, True), (2, False), (50, True))      # (elimination, the joint variant's +1)


def corners_case(dims, elim, plus1):
    """peaks at the eight corners of the grid (fewer where an axis has one cell), every other cell 60..62: cube and box
    bounds are clamped at every border.  Scales are signed multiples (2..4) of res = 1/16.  9x7x11: yaw 0 everywhere, else a
    random yaw per cell.  Axes of 300 cells put values above 255 into the coordinate packing."""
    rng = np.random.default_rng(sum(dims) * 7 + elim)
    res = 0.0625
    g = rng.integers(60, 63, dims).astype(F32)
    corners = sorted({(x, y, z) for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)})
    for i, c in enumerate(corners):
        g[c] = 100 + i % 3                    # ties among the corners too
    yaw = 0.0 if dims == (9, 7, 11) else rng.uniform(-np.pi, np.pi, dims)
    rot = rot_of(yaw, dims)
    scale = (rng.integers(2, 5, dims + (3,)) * rng.choice([-1, 1], dims + (3,)) * res).astype(F32)
    n = 300
    pts = np.stack([rng.integers(0, 16 * d, n) for d in dims], -1).astype(F32) / F32(256)     # multiples of res / 16
    pts[0] = 0
    xyz = (rng.integers(-8, 9, (n, 3)) / 64.0).astype(F32)
    prob = (rng.integers(0, 33, n) / 64.0).astype(F32)
    cls = rng.integers(0, 64, n).astype(np.int32)
    return Case(g, rot, scale, np.zeros(3, F32), res, pts, xyz, prob, cls,
                kw=dict(elimination=elim, separate_variant=not plus1, max_candidates=2048, thresh_low=2),
                claims=dict(listed=dims[0] * dims[1] * dims[2], corners=[flat_of(dims, c) for c in corners]))


def values_case(equal=False):
    """mixed: one +inf cell, two cells exactly thresh_high = 60.0 (examined), one the float just below (never examined), a
    few 61s; tiny boxes so nothing suppresses anything else.  equal: every cell 61 - pure flat-index order."""
    rng = np.random.default_rng(11)
    dims, res = (6, 5, 7), 0.0625
    n = 40
    pts = (rng.integers(0, 16 * 5, (n, 3)) / 256.0).astype(F32)
    pts[0] = 0
    xyz = (rng.integers(-8, 9, (n, 3)) / 64.0).astype(F32)
    prob = (rng.integers(0, 65, n) / 64.0).astype(F32)
    cls = rng.integers(0, 64, n).astype(np.int32)
    rot = rot_of(0.0, dims)
    if equal:
        g = np.full(dims, 61, F32)
        scale = np.full(dims + (3,), 2 * res, F32)
        return Case(g, rot, scale, np.zeros(3, F32), res, pts, xyz, prob, cls, kw=dict(thresh_low=1),
                    claims=dict(listed=6 * 5 * 7))
    g = np.full(dims, 10, F32)
    scale = np.full(dims + (3,), res / 4, F32)
    INF, T1, T2, BELOW = (4, 2, 3), (5, 4, 6), (0, 0, 0), (2, 2, 2)
    g[INF] = np.inf
    g[T1] = 60.0
    g[T2] = 60.0
    g[BELOW] = np.nextafter(F32(60), F32(0))
    g[1, 4, 1] = 61
    g[3, 0, 5] = 61
    return Case(g, rot, scale, np.zeros(3, F32), res, pts, xyz, prob, cls, kw=dict(thresh_low=1, elimination=0),
                claims=dict(listed=5, order=[flat_of(dims, c) for c in (INF, (1, 4, 1), (3, 0, 5), T2, T1)],
                            never=flat_of(dims, BELOW)))


def zero_scale_separate_case():
    """DELIBERATE DEVIATION FROM THE REFERENCE: one peak whose scale is 0, elimination 0, separate variant.  The cube is empty
    and 0 / 0 is inside no box, so the candidate never zeroes itself: eval_separate.py's loop would not terminate here.  The
    capped walk is what this project defines: the same cell is examined max_candidates = 5 times and the walk is truncated."""
    dims, res = (5, 4, 6), 0.0625
    g = np.full(dims, 10, F32)
    g[2, 1, 3] = 90
    scale = np.zeros(dims + (3,), F32)
    pts = np.zeros((4, 3), F32)
    return Case(g, rot_of(0.0, dims), scale, np.zeros(3, F32), res, pts, pts.copy(), np.full(4, 0.5, F32), np.zeros(4, np.int32),
                kw=dict(elimination=0, separate_variant=True, max_candidates=5), allow_truncation=True,
                claims=dict(listed=1, cand=[flat_of(dims, (2, 1, 3))] * 5))


LATTICE_DIMS, LATTICE_RES = (48, 12, 48), 0.0625
LATTICE_CORNER = (-1.5, 0.25, 2.0)


def lattice_case(n_peaks=291, max_candidates=512, allow_truncation=False):
    """n_peaks isolated peaks (boxes smaller than a cell, three cells apart) with a non-zero grid corner; values tie in
    threes; exactly one point at each peak's world position.  In candidate order the point kinds cycle: confident and right
    (accepted), not confident (verdict 1), confident and wrong (verdict 2), with thresh_low = 1 - so accepted boxes lie on
    both sides of candidate 256, and 291 is no multiple of 8.  Candidate i's point has class i % 64."""
    rng = np.random.default_rng(291)
    dims, res = LATTICE_DIMS, LATTICE_RES
    sites = [(x, y, z) for x in range(0, dims[0], 3) for y in range(0, dims[1], 3) for z in range(0, dims[2], 3)]
    pick = [0] + sorted(1 + rng.permutation(len(sites) - 1)[:n_peaks - 1])      # site (0, 0, 0): the points' minimum is the corner
    cells = np.array([sites[i] for i in pick])
    g = np.full(dims, 10, F32)
    vals = 200 - (rng.permutation(n_peaks) // 3)
    g[cells[:, 0], cells[:, 1], cells[:, 2]] = vals
    flat = (cells[:, 0] * dims[1] + cells[:, 1]) * dims[2] + cells[:, 2]
    order = np.lexsort((flat, -vals))                                            # candidate order: value down, flat index up
    corner = np.array(LATTICE_CORNER, F32)
    scale = np.full(dims + (3,), res / 4, F32)
    pts = (corner[None] + F32(res) * cells[order].astype(F32)).astype(F32)
    kind = np.arange(n_peaks) % 3
    prob = np.where(kind == 1, 0.125, 0.875).astype(F32)
    xyz = np.where((kind == 2)[:, None], 1.0, 0.0).astype(F32) * np.ones((1, 3), F32)
    cls = (np.arange(n_peaks) % 64).astype(np.int32)
    n_cand = min(n_peaks, max_candidates) if allow_truncation else n_peaks
    return Case(g, rot_of(0.0, dims), scale, corner, res, pts, xyz, prob, cls,
                kw=dict(thresh_low=1, max_candidates=max_candidates), allow_truncation=allow_truncation,
                claims=dict(listed=n_peaks, cand=flat[order][:n_cand].tolist(), verdict=(np.arange(n_cand) % 3).tolist(),
                            truncated=allow_truncation and max_candidates < n_peaks))


VE_RES = 0.0625


def one_box(offsets, prob, cls=None, xyz=None, peak=(2, 2, 2), far=0, **kw):
    """one peak on a 5x5x5 grid, yaw 0, box half extent one cell (res = 1/16) centred on the world origin; points at
    `offsets` from the centre, `far` surplus points far outside, and one more at the grid corner (outside the box unless the
    peak is cell (0, 0, 0)).  All arithmetic is exact."""
    dims, res = (5, 5, 5), VE_RES
    g = np.full(dims, 10, F32)
    g[peak] = 90
    scale = np.full(dims + (3,), res, F32)
    corner = (-F32(res) * np.array(peak, F32)).astype(F32)
    offsets = np.asarray(offsets, F32).reshape(-1, 3)
    n = len(offsets)
    far_pts = corner[None] + 4.0 + np.arange(far, dtype=F32)[:, None] * F32(0.25) * np.ones((1, 3), F32)
    pts = np.concatenate([offsets, far_pts.reshape(-1, 3), corner[None]]).astype(F32)
    pad = far + 1
    prob = np.concatenate([np.asarray(prob, F32), np.full(pad, 0.875, F32)])
    cls = np.concatenate([np.zeros(n, np.int32) if cls is None else np.asarray(cls, np.int32), np.full(pad, 5, np.int32)])
    # (default predictions: each point's own canonical coordinates, offset / scale, exact - error 0)
    xyz = np.concatenate([offsets / F32(res) if xyz is None else np.asarray(xyz, F32), np.zeros((pad, 3), F32)])
    assert np.array_equal(pts.min(0), corner)
    return Case(g, rot_of(0.0, dims), scale, corner, res, pts, xyz, prob, cls, kw=kw, claims=dict(listed=1))


def _inner(n):
    """n distinct offsets strictly inside the unit-cell box, multiples of res / 16"""
    k = np.arange(n)
    return np.stack([(k % 15) - 7, (k // 15 % 15) - 7, (k // 225) - 3], -1).astype(F32) * F32(VE_RES / 16)


def ve(n_in, n_conf, verdict, **kw):
    prob = np.r_[np.full(n_conf, 0.875), np.full(n_in - n_conf, 0.125)]
    c = one_box(_inner(n_in), prob, **kw)
    c.claims.update(verdict=[verdict])
    return c


def ve_prob_eq():
    """eight points in the box, one confident and one with prob == float32(0.3) exactly: the mask holds one point, below
    valid_ratio 0.25 * 8 = 2 -> rejected (a `>=` mask would hold two and accept)"""
    prob = np.r_[0.875, F32(0.3), np.full(6, 0.125)]
    c = one_box(_inner(8), prob, valid_ratio=0.25, thresh_low=1)
    c.claims.update(verdict=[1])
    return c


def ve_mean():
    """eight points in the box, four of them confident and each 0.5 off in x: the mean over the MASK is 0.5 * 0.875 > 0.3
    (verdict 2); divided by the in-box count it would be 0.21875 and pass"""
    offs = _inner(8)
    xyz = offs / F32(VE_RES) + F32([0.5, 0, 0])
    c = one_box(offs, np.r_[np.full(4, 0.875), np.full(4, 0.125)], xyz=xyz, thresh_low=1)
    c.claims.update(verdict=[2])
    return c


def ve_class(classes, want):
    c = one_box(_inner(len(classes)), np.full(len(classes), 0.875), cls=classes, thresh_low=1)
    c.claims.update(verdict=[0], classes=[want])
    return c


def ve_face_points():
    """six confident points one ulp inside the faces and six unconfident ones exactly on them (w == +-1: outside).  thresh_low
    = 6 rejects if an inner point is lost, valid_ratio = 0.75 rejects if a face point is counted (6 < 0.75 * 7)"""
    s = F32(VE_RES)
    inner = np.nextafter(s, F32(0))
    offs = []
    for k in range(3):
        for sign in (1, -1):
            a = np.zeros(3, F32); a[k] = sign * s; offs.append(a)
            b = np.zeros(3, F32); b[k] = sign * inner; offs.append(b)
    c = one_box(np.array(offs), np.tile(F32([0.125, 0.875]), 6), thresh_low=6, valid_ratio=0.75)
    c.claims.update(verdict=[0], n_in=6)
    return c


def ve_npts(n):
    """n scan points in all: the first (and the grid corner itself) at the centre of a box on cell (0, 0, 0), two more inside
    where n allows, the rest far outside"""
    inside = np.array([[0, 0, 0], [1, 2, 3], [3, 1, 0]], F32)[:min(n - 1, 3)] * F32(VE_RES / 16) if n > 1 else np.zeros((0, 3), F32)
    m = len(inside)
    c = one_box(inside, np.full(m, 0.875), peak=(0, 0, 0), far=n - 1 - m, thresh_low=1)
    assert len(c.pts) == n
    c.claims.update(verdict=[0], n_points=n)
    return c


def categories_case(which):
    """three categories on one grid shape, listed lengths 0 / 300 / 4097 (a) or 0 / 1537 / 24577 (b): an empty list and two
    different walks side by side in one launch.  Scan points shared, no class input.  Returns (list of Case, shared points)."""
    lens, dims = ((0, 300, 4097), (20, 12, 20)) if which == "a" else ((0, 1537, 24577), (40, 20, 40))
    pts, _ = len_points(dims)
    out = []
    for L in lens:
        g, rot, scale, xyz, prob = len_parts(L, dims, 2000 + L)
        out.append(Case(g, rot, scale, np.zeros(3, F32), 0.05, pts, xyz, prob, np.zeros(600, np.int32),
                        kw=dict(max_candidates=1024), claims=dict(listed=L)))
    return out


def _cases():
    C = {}
    for L in LEN_SMALL + LEN_BIG:
        C["len_%d" % L] = functools.partial(len_case, L)
    for yaw in FACE_YAWS:
        C["faces_%s" % yaw] = functools.partial(faces_case, yaw)
        C["faces_%s_sep" % yaw] = functools.partial(faces_case, yaw, True)
    C["faces_0_in"] = functools.partial(faces_case, "0", False, "in")
    C["faces_0_out"] = functools.partial(faces_case, "0", False, "out")
    for dims in CORNER_DIMS:
        for e, p in CORNER_ELIM:
            C["corners_%dx%dx%d_e%d%s" % (dims + (e, "p" if p else ""))] = functools.partial(corners_case, dims, e, p)
    C["values"] = values_case
    C["values_equal"] = functools.partial(values_case, True)
    C["zero_scale_separate"] = zero_scale_separate_case
    C["lattice_291_m512"] = functools.partial(lattice_case, 291, 512)
    C["lattice_291_m291"] = functools.partial(lattice_case, 291, 291)
    C["lattice_291_m290t"] = functools.partial(lattice_case, 291, 290, True)
    C["ve_ratio_pass"] = functools.partial(ve, 8, 2, 0, valid_ratio=0.25, thresh_low=1)
    C["ve_ratio_reject"] = functools.partial(ve, 8, 1, 1, valid_ratio=0.25, thresh_low=1)
    C["ve_low_pass"] = functools.partial(ve, 10, 10, 0)
    C["ve_low_reject"] = functools.partial(ve, 9, 9, 1)
    C["ve_prob_eq"] = ve_prob_eq
    C["ve_mean_mask"] = ve_mean
    C["ve_class_tie"] = functools.partial(ve_class, [7, 7, 2, 2], 2)
    C["ve_class_63"] = functools.partial(ve_class, [63, 0, 63, 62, 63, 0], 63)
    C["ve_face_points"] = ve_face_points
    for n in (1, 255, 256, 257):
        C["ve_npts_%d" % n] = functools.partial(ve_npts, n)
    return C


CASES = _cases()
# lattice_291 with max_candidates = 9 and no allow_truncation: the capacity grows (9 -> 72 -> 576); the grid is not mutated
LATTICE_GROW = functools.partial(lattice_case, 291, 9)
CATEGORY_CASES = {"categories_mixed_a": functools.partial(categories_case, "a"),
                  "categories_mixed_b": functools.partial(categories_case, "b")}
# the cases whose arithmetic is exact whatever the summation order, joint variant: executed by the reference's own lines
# (tests/golden/make_decode_golden.py -> tests/golden/decode_edge_ref.npz)
GOLDEN_CASES = dict({k: CASES[k] for k in ("faces_0", "corners_9x7x11_e0p", "corners_9x7x11_e2p", "corners_9x7x11_e50p", "values",
                                           "values_equal")},
                    **{k: v for k, v in CASES.items() if k.startswith("ve_")}, lattice_30=functools.partial(lattice_case, 30, 512))


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case, built once (callers must not modify its arrays)"""
    if name in CASES:
        return CASES[name]()
    return GOLDEN_CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result for a named case, computed once and shared (treat as read-only)"""
    c = case(name)
    return decode(*c.args(), **c.kw)
