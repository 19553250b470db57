"""Small vote cases for the exact tests of the tile algorithm (tests/test_vote_fixed.py on the CPU, tests/test_vote_exact_gpu.py on
the GPU) that the dense cases of tests/test_vote_dense_gpu.py do not have: contributions below the fixed-point quantum,
objectness of both signs, contributions beyond the clamp.  Each returns (points, xyz, scale, prob, res, num_rots) like the dense
cases; at most 600 points (`clamp`: the 1500 of `huge`) and 3 x 3 tiles of 16 x 32 cells.  tests/test_vote_fixed.py asserts that each is what it claims."""
import numpy as np

RES = 0.03
f32 = np.float32


def _rings(rng, cx, cy, cz, rad):
    """points at grid positions (cx, cy, cz) [cells] whose votes form rings of radius rad [cells] in their y plane"""
    n = len(cx)
    pts = (np.stack([cx, cy, cz], 1) * RES).astype(f32)
    phi = rng.uniform(0, 2 * np.pi, n)
    off = np.stack([rad * np.cos(phi), np.zeros(n), rad * np.sin(phi)], 1) * RES
    scale = rng.uniform(0.5, 1.5, (n, 3)).astype(f32)
    return pts, (off / scale).astype(f32), scale


def _static(rng, n, lo, hi):
    """n points uniform in the box [lo, hi] [cells] that vote where they stand (xyz = 0), scale 1"""
    pts = (rng.uniform(lo, hi, (n, 3)) * RES).astype(f32)
    return pts, np.zeros((n, 3), f32), np.ones((n, 3), f32)


def _join(parts, probs, hi):
    """the parts, then two anchors of weight 1 with xyz = 0 that span the grid [0, hi] cells"""
    a = (np.array([[0, 0, 0], hi], np.float64) * RES).astype(f32)
    parts = list(parts) + [(a, np.zeros((2, 3), f32), np.ones((2, 3), f32))]
    pts, xyz, scale = (np.concatenate([p[i] for p in parts]) for i in range(3))
    prob = np.concatenate(list(probs) + [np.ones(2)]).astype(f32)
    return pts, xyz, scale, prob


TINY_OBJ = (1e-12, 3e-12, -1e-12)          # all below half a quantum (2^-37 = 7.3e-12) whatever the trilinear weight


def case_tiny():
    """300 ordinary ring points around cells (5..20, 1..4, 5..30), rings of at most 5 cells, plus 51 points of objectness
    1e-12 / 3e-12 / -1e-12 with xyz = 0: 24 inside the busy region, 27 in the corner (28..38, 1..4, 40..58) that nothing else
    reaches.  Every contribution of those points rounds to zero quanta; the objectness channel's non-zero rule alone makes
    their cells touched.  Grid 41 x 6 x 61 (3 x 2 tiles), R = 24."""
    rng = np.random.default_rng(201)
    n = 300
    rings = _rings(rng, rng.uniform(5, 20, n), rng.uniform(1, 4, n), rng.uniform(5, 30, n), rng.uniform(0, 5, n))
    busy = _static(rng, 24, (6, 1, 6), (19, 4, 29))
    empty = _static(rng, 27, (28, 1, 40), (38, 4, 58))
    tiny = np.tile(np.array(TINY_OBJ), 17)
    return _join([rings, busy, empty], [rng.uniform(0.5, 1.0, n), tiny[:24], tiny[24:]], [40, 5, 60]) + (RES, 24)


def case_signed():
    """300 ring points with objectness uniform in +-[0.5, 1], and 60 pairs of identical points with objectness +p and -p - 30
    rings among the others, 30 with xyz = 0 in a corner of their own, where the integer sums of whole cells are exactly 0.
    Grid 41 x 6 x 61, R = 24."""
    rng = np.random.default_rng(202)
    n = 300
    rings = _rings(rng, rng.uniform(5, 20, n), rng.uniform(1, 4, n), rng.uniform(5, 30, n), rng.uniform(0, 5, n))
    prob = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    pair_rings = _rings(rng, rng.uniform(5, 20, 30), rng.uniform(1, 4, 30), rng.uniform(5, 30, 30), rng.uniform(0, 5, 30))
    pair_static = _static(rng, 30, (28, 1, 40), (38, 4, 58))
    pairs = tuple(np.concatenate([a, b]) for a, b in zip(pair_rings, pair_static))
    p = rng.uniform(0.5, 1.0, 60)
    return _join([rings, pairs, pairs], [prob, p, -p], [40, 5, 60]) + (RES, 24)


def case_clamp():
    """the `huge` case of tests/test_vote_dense_gpu.py with point 3 given a scale of 1e9 (its xyz scaled down so that its votes
    stay where they were): w * s exceeds 6e7 and is clamped by the fixed-point conversion"""
    from tests.test_vote_dense_gpu import case_huge
    pts, xyz, scale, prob, res, R = case_huge()
    xyz, scale = xyz.copy(), scale.copy()
    corr = xyz[3] * scale[3]
    scale[3] = f32(1e9)
    xyz[3] = (corr / scale[3]).astype(f32)
    return pts, xyz, scale, prob, res, R


CASES = {"tiny": case_tiny, "signed": case_signed, "clamp": case_clamp}
