"""Hand-made jobs for the decode over a scene axis (cv_decode_scenes_f32): four scenes that share nothing but the decode
parameters, at the smallest shapes that can still go wrong - grids of (9, 5, 7), (16, 4, 12), (3, 3, 3) and (24, 6, 24) cells,
700, 50, 1 and 3000 points (3, 1, 1 and 12 back-projection workgroups).  tests/decode_ref.py says what each job decodes to;
`claims()` is what the jobs exist for and is asserted on the CPU (tests/test_scene_batch.py) and again on the GPU."""
import numpy as np

from tests import decode_ref as dr

F32 = np.float32
RES = 0.1
MAX_CANDIDATES = 6
KW = dict(thresh_high=60.0, thresh_low=3.0, valid_ratio=0.2, elimination=1, prob_thresh=0.3, err_thresh=0.3,
          max_candidates=MAX_CANDIDATES)
DIMS = ((9, 5, 7), (16, 4, 12), (3, 3, 3), (24, 6, 24))
POINTS = (700, 50, 1, 3000)


def _box_points(rng, corner, cell, yaw, scale, n, wrong):
    """n points strictly inside the box the decode forms at `cell`, and their canonical coordinates as predictions
    (`wrong`: shifted by one box width, an LCC error of about one)"""
    w = rng.uniform(-0.85, 0.85, (n, 3))
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    centre = np.asarray(corner, np.float64) + RES * np.asarray(cell, np.float64)
    pts = centre + (w * np.asarray(scale)) @ R.T
    return pts.astype(F32), (w + (1.0 if wrong else 0.0)).astype(F32)


def _job(seed, dims, n, corner, peaks, far):
    """peaks: (cell, value, yaw, scale, points, wrong); the remaining points lie `far` away from every box"""
    rng = np.random.default_rng(seed)
    g_obj = rng.uniform(0.0, 20.0, dims).astype(F32)
    g_rot = dr.rot_of(rng.uniform(-3.0, 3.0, dims), dims)
    g_scale = rng.uniform(0.04, 0.06, dims + (3,)).astype(F32)
    pts, xyz = [], []
    for cell, value, yaw, scale, k, wrong in peaks:
        g_obj[cell] = value
        g_rot[cell] = (np.cos(yaw), np.sin(yaw))
        g_scale[cell] = scale
        if k:
            p, x = _box_points(rng, corner, cell, yaw, scale, k, wrong)
            pts.append(p)
            xyz.append(x)
    rest = n - sum(len(p) for p in pts)
    assert rest >= 0
    pts.append((np.asarray(corner) + far + rng.uniform(0, 1, (rest, 3))).astype(F32))
    xyz.append(rng.uniform(-1, 1, (rest, 3)).astype(F32))
    pts, xyz = np.concatenate(pts), np.concatenate(xyz)
    order = rng.permutation(n)
    return dr.Case(g_obj, g_rot, g_scale, np.asarray(corner, F32), RES, pts[order], xyz[order],
                   rng.uniform(0.35, 0.99, n).astype(F32), rng.integers(0, 9, n).astype(np.int32), dict(KW), True)


def job_a(seed=1):
    """(9, 5, 7), 700 points: an accepted box whose neighbour cell (>= thresh_high) it suppresses, a box rejected for its LCC
    error, a peak without points"""
    peaks = [((2, 2, 2), 100.0, 0.3, (0.16, 0.12, 0.15), 300, False), ((3, 2, 2), 70.0, 0.0, (0.05, 0.05, 0.05), 0, False),
             ((6, 2, 4), 90.0, -0.7, (0.13, 0.14, 0.12), 250, True), ((7, 4, 6), 80.0, 1.1, (0.05, 0.05, 0.05), 0, False)]
    return _job(seed, DIMS[0], POINTS[0], (-0.4, 0.1, 1.3), peaks, 50.0)


def job_trunc(seed=2):
    """(16, 4, 12), 50 points: ten isolated peaks, more live cells than max_candidates - the walk is cut"""
    peaks = [((1 + 3 * (i % 5), 1, 2 + 6 * (i // 5)), 100.0 - i, 0.2 * i, (0.05, 0.05, 0.05), 5 if i < 4 else 0, False)
             for i in range(10)]
    return _job(seed, DIMS[1], POINTS[1], (2.0, -1.0, 0.0), peaks, 50.0)


def job_empty(seed=3):
    """(3, 3, 3), one point: no cell >= thresh_high"""
    return _job(seed, DIMS[2], POINTS[2], (0.0, 0.0, 0.0), [], 50.0)


def job_big(seed=4):
    """(24, 6, 24), 3000 points: three accepted boxes, one rejected for its error, one for too few points"""
    peaks = [((4, 2, 5), 120.0, 0.5, (0.21, 0.18, 0.2), 600, False), ((12, 3, 12), 110.0, -1.2, (0.25, 0.2, 0.22), 500, False),
             ((19, 2, 6), 95.0, 2.0, (0.2, 0.22, 0.18), 400, False), ((6, 3, 19), 85.0, 0.1, (0.2, 0.2, 0.2), 300, True),
             ((20, 4, 20), 75.0, 0.9, (0.2, 0.2, 0.2), 2, False)]
    return _job(seed, DIMS[3], POINTS[3], (-3.0, 0.5, -1.0), peaks, 50.0)


def batch():
    """the four distinct jobs"""
    return [job_a(), job_trunc(), job_empty(), job_big()]


def batch_twins():
    """slots 0 and 3 hold the same data"""
    return [job_a(), job_trunc(), job_empty(), job_a()]


def expected(jobs):
    return [dr.decode(*c.args(), **c.kw) for c in jobs]


def claims(want):
    """what the four jobs of batch() exist for, on their tests/decode_ref.py results"""
    a, t, e, b = want
    assert (a["verdict"] == 0).sum() >= 1 and (a["verdict"] == 2).sum() >= 1 and (a["verdict"] == 1).sum() >= 1 and not a["truncated"]
    assert (3 * 5 + 2) * 7 + 2 not in a["cand_idx"]                    # cell (3, 2, 2) went with its neighbour's cube
    assert t["truncated"] and len(t["cand_idx"]) == MAX_CANDIDATES
    assert len(e["cand_idx"]) == 0 and not e["truncated"]
    assert (b["verdict"] == 0).sum() >= 3 and (b["verdict"] == 2).sum() >= 1 and (b["verdict"] == 1).sum() >= 1 and not b["truncated"]
    assert len(b["cand_idx"]) <= MAX_CANDIDATES


def concat(jobs):
    """the shared arrays and the row ranges"""
    ends = np.cumsum([len(c.pts) for c in jobs])
    ranges = [(int(e - len(c.pts)), int(e)) for c, e in zip(jobs, ends)]
    cat = lambda f: np.concatenate([f(c) for c in jobs])
    return cat(lambda c: c.pts), cat(lambda c: c.xyz), cat(lambda c: c.prob), cat(lambda c: c.cls), ranges
