"""An independent reference of the voxeliser (cv_sp_quantize_f32 / _f64, section 6 of csrc/sparse_coords.hip) and hand-made
adversarial clouds, numpy and Python only.  Nothing here imports the library.

Shared by tests/test_quantize_ref.py (CPU: what the cases claim, the two references against each other and against the host
path of ME.utils, named wrong restatements) and tests/test_quantize_edge_gpu.py (the kernels through the C ABI).

  1. Reference.  `reference` is a plain loop over the rows with a dict keyed by (cloud, vx, vy, vz): nothing is packed, no
     table, no run shortcut.  `reference_vec` restates it with a packed key and np.unique for the one case of 2^20 rows.
     `reference(..., wrong=name)` gives the named WRONG results: what a voxeliser with one specific mistake would write.
  2. Table claims.  mix64, packed_key, home_slots, occupancy and wrapped_run are coord_ref's, with the batch column set to the
     cloud index.  They construct collision cases and verify their claims; they are never the expected value of an output.
  3. Cases.  Functions of no arguments returning a Case: points [m, 3] of the case's dtype, q, floor_only, offsets, ld and
     what the case claims of itself in `.claims`.
"""
import bisect
import functools

import numpy as np

from tests import coord_ref as cr

WINDOW_LO, WINDOW_HI = cr.WINDOW_LO, cr.WINDOW_HI
MAX_CLOUDS = 256                                   # CV_QUANTIZE_MAX_CLOUDS (include/cv_hip.h)
WAVE, GROUP, SCAN_BLOCK, TRIP = 64, 256, 1024, 1 << 20     # lanes; quantize_insert's workgroup; scan block; grid-stride trip
WRONG = ("truncate", "reciprocal", "f32_for_f64", "window_plus_one", "window_minus_one", "run_ignores_cloud", "no_wrap",
         "last_point", "lexicographic", "rejected_removed_first")


# ====================================================================================================== 1. reference
def row_voxel(p, q, floor_only, wrong=None):
    """(voxel as three Python ints, or None when the row is rejected) of one row `p` of numpy scalars.  The quotient is the
    scalar division of the row's own dtype; the window check is made on the floats, before any conversion to int."""
    T = type(p[0])
    if wrong == "f32_for_f64":
        T = np.float32
    lo, hi = WINDOW_LO, WINDOW_HI
    if wrong == "window_plus_one":
        lo, hi = lo - 1, hi + 1
    if wrong == "window_minus_one":
        lo, hi = lo + 1, hi - 1
    rnd = np.trunc if wrong == "truncate" else np.floor
    v = []
    for x in p:
        if not np.isfinite(x):
            return None
        x = T(x)
        if floor_only:
            f = rnd(x)
        elif wrong == "reciprocal":
            f = rnd(x * (T(1) / T(q)))
        else:
            f = rnd(x / T(q))
        if not (f >= lo and f <= hi):              # (false for NaN)
            return None
        v.append(int(f))
    return tuple(v)


def cloud_of(i, offsets):
    """the last cloud whose first row is <= i"""
    return 0 if offsets is None else bisect.bisect_right(list(offsets), i) - 1


def reference(points, q, floor_only=0, offsets=None, wrong=None):
    """dict(coords4 [N, 4] (cloud, x, y, z), index [N], inverse [m], n, rejected), int64 arrays.  Output order = order of
    first appearance, index = first row of every voxel, inverse[i] = output row of row i's voxel or -1 for a rejected row."""
    assert wrong is None or wrong in WRONG
    points = np.asarray(points)
    m = len(points)
    with np.errstate(all="ignore"):
        vox = [row_voxel(points[i], q, floor_only, wrong) for i in range(m)]
    keys = [None if v is None else (cloud_of(i, offsets),) + v for i, v in enumerate(vox)]
    if wrong == "run_ignores_cloud":               # a lane whose VOXEL equals its left neighbour's takes that neighbour's key
        for i in range(m):
            if i % WAVE and keys[i] is not None and keys[i - 1] is not None and keys[i][1:] == keys[i - 1][1:]:
                keys[i] = keys[i - 1]
    lost = set()
    if wrong == "no_wrap":                         # keys whose probe runs off the end of the table are dropped
        distinct = list(dict.fromkeys(k for k in keys if k is not None))
        table = set(cr.occupancy(np.array(distinct, np.int64).reshape(-1, 4), cr.table_capacity(m), wrap=False))
        lost = {k for k, pk in zip(distinct, cr.packed_key(np.array(distinct, np.int64).reshape(-1, 4)).tolist()) if pk not in table}
    seen, coords4, index, inverse, rejected = {}, [], [], [], 0
    for i, key in enumerate(keys):
        if key is None:
            rejected += 1
            inverse.append(-1)
            continue
        if key in lost:
            inverse.append(-1)
            continue
        r = seen.get(key)
        if r is None:
            r = seen[key] = len(index)
            coords4.append(key)
            index.append(i)
        elif wrong == "last_point":
            index[r] = i
        inverse.append(r)
    coords4 = np.array(coords4, np.int64).reshape(-1, 4)
    index, inverse = np.array(index, np.int64), np.array(inverse, np.int64)
    if wrong == "lexicographic" and len(index):
        order = np.lexsort(coords4.T[::-1])
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        coords4, index, inverse = coords4[order], index[order], np.where(inverse >= 0, rank[inverse], -1)
    if wrong == "rejected_removed_first":          # row numbers of the cloud with its rejected rows taken out
        shift = np.cumsum(np.array([k is None for k in keys], np.int64))
        index = index - shift[index]
    return dict(coords4=coords4, index=index, inverse=inverse, n=len(index), rejected=rejected)


def reference_vec(points, q, floor_only=0, offsets=None):
    """`reference` restated with arrays: packed key (coord_ref.packed_key, cloud in the batch field), np.unique"""
    p = np.asarray(points)
    m, T = len(p), p.dtype.type
    with np.errstate(all="ignore"):
        v = np.floor(p) if floor_only else np.floor(p / T(q))
        ok = np.isfinite(p).all(1) & ((v >= WINDOW_LO) & (v <= WINDOW_HI)).all(1)
    rows = np.nonzero(ok)[0]
    b = np.zeros(len(rows), np.int64) if offsets is None else np.searchsorted(np.asarray(offsets, np.int64), rows, side="right") - 1
    c4 = np.concatenate([b[:, None], v[rows].astype(np.int64)], 1)
    _, first, inv = np.unique(cr.packed_key(c4), return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    inverse = np.full(m, -1, np.int64)
    inverse[rows] = rank[np.asarray(inv).reshape(-1)]
    return dict(coords4=c4[first[order]], index=rows[first[order]].astype(np.int64), inverse=inverse, n=len(first),
                rejected=int(m - len(rows)))


ARRAYS = ("coords4", "index", "inverse")


def same_result(a, b):
    return a["n"] == b["n"] and a["rejected"] == b["rejected"] and all(cr.same(a[k], b[k]) for k in ARRAYS)


# ================================================================================================================ 2. cases
class Case:
    def __init__(self, name, points, q=0.03, floor_only=0, offsets=None, ld=3, big=False, **claims):
        self.name, self.points = name, np.ascontiguousarray(points)
        assert self.points.ndim == 2 and self.points.shape[1] == 3 and self.points.dtype in (np.float32, np.float64)
        self.dtype, self.m = self.points.dtype, len(self.points)
        T = self.dtype.type
        self.q = float(T(q))                       # what the C call receives as float / double
        self.floor_only, self.ld, self.big, self.claims = floor_only, ld, big, claims
        self.offsets = None if offsets is None else [int(o) for o in offsets]
        assert self.offsets is None or (self.offsets[0] == 0 and self.offsets == sorted(self.offsets)
                                        and self.offsets[-1] <= self.m and 1 <= len(self.offsets) <= MAX_CLOUDS)
        assert self.m > 0 and ld >= 3 and (floor_only or (self.q > 0 and np.isfinite(self.q)))      # a valid call

    def __repr__(self):
        return self.name

    def laid_out(self):
        """(flat array, first element): the rows with stride ld, columns 3.. NaN, one element past the start of the buffer
        when ld > 3 (the buffer's start is at least 16-byte aligned on the device)"""
        if self.ld == 3:
            return self.points.reshape(-1), 0
        flat = np.full(1 + self.m * self.ld, np.nan, self.dtype)
        flat[1:].reshape(self.m, self.ld)[:, :3] = self.points
        return flat, 1


def to_points(vox, dtype, q=0.03):
    """points in the middle of the voxels `vox` [m, 3]; the quotient of the dtype floors to the voxel (asserted)"""
    T = np.dtype(dtype).type
    vox = np.asarray(vox, np.int64).reshape(-1, 3)
    p = ((vox + 0.5) * float(T(q))).astype(dtype)
    assert np.array_equal(np.floor(p / T(q)), vox.astype(dtype))
    return p


def pool(n, seed, shift=(0, 0, 0)):
    """n distinct voxels around the origin (negative ones included), shuffled"""
    return cr._thinned_block(-9, 10, n, seed)[:, 1:] + np.asarray(shift, np.int64)


RUN_SHIFT = (40, 0, 0)          # voxels of runs and special rows: outside the box of `pool`


def with_duplicates(m, seed):
    """voxels of m rows: about a third of the rows repeat an earlier row, the others are new"""
    rng = np.random.default_rng(seed)
    fresh = iter(pool(m, seed))
    rows = []
    for i in range(m):
        rows.append(rows[int(rng.integers(0, i))] if i and rng.random() < 1 / 3 else next(fresh))
    return np.array(rows, np.int64)


def dtype_tag(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


# ---- sizes and runs
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def sizes(m, dtype=np.float32):
    """m rows, about a third duplicates: the m_pad padding of the last wave, one and two scan blocks"""
    return Case("sizes_%d_%s" % (m, dtype_tag(dtype)), to_points(with_duplicates(m, 100 + m), dtype), branch="m_pad, scan blocks")


RUN_LENGTHS, RUN_LANES = (1, 2, 63, 64, 65, 130), (0, 1, 63)


def _place_runs():
    """[(first row, length)]: every length at every first lane, never adjacent to each other; four of them are made to cross
    rows 256, 1024, 1280 and 1792 (placed first)"""
    cross = {(2, 63): 256, (65, 63): 1024, (130, 0): 1280, (130, 1): 1792}
    want = [(ln, lane) for ln in RUN_LENGTHS for lane in RUN_LANES]
    used, out = set(), []
    for ln, lane in sorted(want, key=lambda t: t not in cross):
        c, s = cross.get((ln, lane)), lane
        while (set(range(s - 1, s + ln + 1)) & used) or not (c is None or s < c <= s + ln - 1):
            s += WAVE
            assert s < 4096
        used |= set(range(s, s + ln))
        out.append((s, ln))
    return sorted(out)


def runs(dtype=np.float32):
    """runs of one voxel (a new voxel per run) of every length in RUN_LENGTHS starting at every lane in RUN_LANES, separated
    by rows of other voxels"""
    placed = _place_runs()
    m = max(s + ln for s, ln in placed) + 7
    vox = pool(m, 21)
    special = pool(len(placed), 22, RUN_SHIFT)
    for j, (s, ln) in enumerate(placed):
        vox[s:s + ln] = special[j]
    return Case("runs_" + dtype_tag(dtype), to_points(vox, dtype), runs=placed, branch="run-leader shortcut")


def runs_aba(dtype=np.float32):
    """voxel A at rows 10 and 12 around B at 11 (one wave), both again at rows 600, 601 (a later workgroup); C at rows 63, 64
    (a run across a wave boundary) and again at 300"""
    vox = pool(700, 23)
    a, b, c = pool(3, 24, RUN_SHIFT)
    for r, v in ((10, a), (11, b), (12, a), (600, a), (601, b), (63, c), (64, c), (300, c)):
        vox[r] = v
    return Case("runs_aba_" + dtype_tag(dtype), to_points(vox, dtype), revisits={10: (12, 600), 11: (601,), 63: (64, 300)},
                branch="-2 - slot of a voxel visited again")


def runs_one_voxel(dtype=np.float32):
    """all 1300 rows in one voxel: two scan blocks, N = 1"""
    return Case("runs_one_voxel_" + dtype_tag(dtype), to_points(np.tile(pool(1, 25), (1300, 1)), dtype), branch="one run over every boundary")


def bad_values(dtype, q=0.03):
    """{kind: a coordinate that rejects its row}"""
    T = np.dtype(dtype).type
    return dict(nan=T(np.nan), pinf=T(np.inf), ninf=T(-np.inf), above=T((WINDOW_HI + 1.5) * float(T(q))),
                below=T((WINDOW_LO - 0.5) * float(T(q))))


KINDS = ("nan", "pinf", "ninf", "above", "below")


def runs_rejected(dtype=np.float32):
    """runs of one voxel broken by rejected rows; cloud 1 (rows 600..699) is rejected as a whole.  claims: `rejected` {row:
    kind}, `broken` [(rows of one voxel around rejected rows)], `late_first` (rejected row, the voxel's index)"""
    m = 700
    vox = with_duplicates(m, 26)
    v = pool(8, 27, RUN_SHIFT)
    for rows, w in ((range(5, 8), v[0]), (range(126, 131), v[1]), (range(189, 194), v[2]), (range(255, 321), v[3]), (range(400, 403), v[4])):
        vox[list(rows)] = w
    vox[450], vox[451] = (WINDOW_HI, 0, 1), (2, WINDOW_LO, 3)                 # the window's own edges are accepted
    p = to_points(vox, dtype)
    bad = bad_values(dtype)
    rejected = {6: "nan", 128: "pinf", 191: "ninf", 400: "nan", 460: "above", 461: "below", 462: "pinf", 463: "ninf"}
    rejected.update({r: KINDS[r % 5] for r in range(256, 320)})               # a whole wave
    rejected.update({r: KINDS[r % 5] for r in range(600, 700)})               # a whole cloud
    for r, kind in rejected.items():
        p[r, r % 3 if r != 400 else 2] = bad[kind]                            # (row 400: x, y of its voxel, z NaN)
    return Case("runs_rejected_" + dtype_tag(dtype), p, offsets=[0, 600], rejected=rejected,
                broken=[(5, 7), (126, 127, 129, 130), (189, 190, 192, 193), (255, 320), (401, 402)], late_first=(400, 401),
                branch="rejected rows: EMPTY_KEY lanes break runs, slot -1")


def all_rejected(dtype=np.float32):
    """130 rows, every one rejected"""
    p = to_points(pool(130, 28), dtype)
    bad = bad_values(dtype)
    for r in range(130):
        p[r, r % 3] = bad[KINDS[r % 5]]
    return Case("all_rejected_" + dtype_tag(dtype), p, rejected={r: KINDS[r % 5] for r in range(130)}, branch="N = 0")


# ---- hash table (claims through coord_ref's table restatement, cloud index in the batch column)
CHAIN_TAIL, CHAIN_LEN = 8, 40


def _cells(lo, hi, cloud=0):
    return cr._with_batch(cr._grid(lo, hi), cloud)


def _tail_chain(name, m, dtype):
    """rows 0..39: distinct voxels of the box [-16, 16)^3 homed in the last 8 slots of the table (the lanes of one wave insert
    them at once and most probe through the end of the table); rows 300..339: the same voxels in reverse order; filler homed
    away from both ends of the table elsewhere, a third of it duplicates"""
    cap = cr.table_capacity(m)
    box = _cells(-16, 16)
    home = cr.home_slots(box, cap)
    tail = box[home >= cap - CHAIN_TAIL]
    first = tail[cr.home_slots(tail, cap) == cap - CHAIN_TAIL][:1]            # the run starts at slot cap - 8 exactly
    assert len(first) == 1
    rest = np.array([t for t in tail.tolist() if t != first[0].tolist()], np.int64)
    chain = np.concatenate([first, rest[:CHAIN_LEN - 1]])
    assert len(chain) == CHAIN_LEN
    mid = box[(home >= 200) & (home < cap - 200)]
    mid = mid[np.random.default_rng(m).permutation(len(mid))]
    rng = np.random.default_rng(m + 1)
    vox = np.empty((m, 3), np.int64)
    nxt = 0
    for i in range(m):
        if i < CHAIN_LEN:
            vox[i] = chain[i, 1:]
        elif 300 <= i < 300 + CHAIN_LEN:
            vox[i] = chain[CHAIN_LEN - 1 - (i - 300), 1:]
        elif i > CHAIN_LEN + 5 and rng.random() < 1 / 3:
            vox[i] = vox[int(rng.integers(CHAIN_LEN, i))]
        else:
            vox[i], nxt = mid[nxt, 1:], nxt + 1
    return Case(name, to_points(vox, dtype), cap=cap, chain=chain, tail_cells=len(tail), branch="probe loop through the end of the table")


def tail_chain_1024(dtype=np.float32):
    return _tail_chain("tail_chain_1024_" + dtype_tag(dtype), 500, dtype)


def tail_chain_2048(dtype=np.float32):
    return _tail_chain("tail_chain_2048_" + dtype_tag(dtype), 1000, dtype)


def one_home_slot(dtype=np.float32):
    """the voxels of the box [-20, 20)^3 that share the most popular home slot of the 2048-slot table (at least 20), in
    adjacent lanes from row 64 on, and in reverse order two workgroups later (from row 576); 700 rows"""
    m = 700
    cap = cr.table_capacity(m)
    box = _cells(-20, 20)
    home = cr.home_slots(box, cap)
    slot = int(np.bincount(home, minlength=cap).argmax())
    group = box[home == slot][:48]
    vox = pool(m, 29, (60, 0, 0))
    vox[64:64 + len(group)] = group[:, 1:]
    vox[576:576 + len(group)] = group[::-1, 1:]
    return Case("one_home_slot_" + dtype_tag(dtype), to_points(vox, dtype), cap=cap, slot=slot, group=group,
                branch="one wave contends for one home slot")


# ---- clouds
def clouds_same_points(dtype=np.float32):
    """the same 150 rows in two clouds: equal voxels, different keys"""
    vox = with_duplicates(150, 30)
    return Case("clouds_same_points_" + dtype_tag(dtype), to_points(np.concatenate([vox, vox]), dtype), offsets=[0, 150],
                branch="cloud index in the key")


def clouds_empty(dtype=np.float32):
    """300 rows in 8 clouds of which 0, 2, 3, 6 and 7 are empty (equal offsets; the last two offsets equal m)"""
    vox = with_duplicates(300, 31)
    vox[95:105] = vox[95]                                  # a run over the boundary at row 100
    return Case("clouds_empty_" + dtype_tag(dtype), to_points(vox, dtype), offsets=[0, 0, 100, 100, 100, 257, 300, 300],
                empty=(0, 2, 3, 6, 7), branch="bisection with equal offsets")


def clouds_boundaries(dtype=np.float32):
    """boundaries at rows 128 (lane 0), 193 (lane 1) and 300 (lane 44), each inside a run of equal voxels"""
    vox = with_duplicates(400, 32)
    v = pool(3, 33, RUN_SHIFT)
    vox[126:131], vox[191:196], vox[290:311] = v[0], v[1], v[2]
    return Case("clouds_boundaries_" + dtype_tag(dtype), to_points(vox, dtype), offsets=[0, 128, 193, 300],
                split_runs=((126, 131, 128), (191, 196, 193), (290, 311, 300)), branch="same voxel, other cloud: a new leader")


def clouds_256(dtype=np.float32):
    """300 rows of 12 voxels in 256 clouds (some empty, some of several rows)"""
    rng = np.random.default_rng(34)
    offsets = [0] + sorted(rng.integers(0, 301, MAX_CLOUDS - 1).tolist())
    vox = pool(12, 35)[rng.integers(0, 12, 300)]
    return Case("clouds_256_" + dtype_tag(dtype), to_points(vox, dtype), offsets=offsets, branch="256-entry bisection")


# ---- arithmetic
def _edge_rows(valid, maybe, dtype):
    """rows of three values from `valid`, every value on every axis; then one row per value of `maybe` (values that may
    reject their row) on axis r % 3 with valid values on the other axes"""
    valid, maybe = np.asarray(valid, dtype), np.asarray(maybe, dtype)
    n = len(valid)
    i = np.arange(n)
    a = np.stack([valid[i], valid[(i * 7 + 3) % n], valid[(i * 13 + 5) % n]], 1)
    a = np.concatenate([a, a[:, [2, 0, 1]], a[:, [1, 2, 0]]])
    b = np.stack([valid[np.arange(len(maybe)) % n]] * 3, 1)
    b[np.arange(len(maybe)), np.arange(len(maybe)) % 3] = maybe
    return np.concatenate([a, b]).astype(dtype)


def _around(x, dtype, steps=3):
    """x as dtype and its `steps` neighbours on either side"""
    T = np.dtype(dtype).type
    out = [T(x)]
    for d in (T(np.inf), T(-np.inf)):
        y = T(x)
        for _ in range(steps):
            y = np.nextafter(y, d)
            out.append(y)
    return out


def quotient_edges_f32():
    """q = float32(0.03).  k * q for k in [-40, 40], whose fp32 quotients all floor AT k, and for the ten k of [-300, 300] whose
    quotient lies one ulp below k and floors to k - 1 (49, 81, 98, -171, ...), zeros, denormals (-1e-45
    lies in voxel -1), and the fp32 values around +-32704 * q, where the rounding of the division decides on the window"""
    q = np.float32(0.03)
    k = np.arange(-300, 301)
    k = k[(np.abs(k) <= 40) | (np.floor((k * q).astype(np.float32) / q) != k)]
    valid = list((k * q).astype(np.float32)) + [np.float32(x) for x in (-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38,
                                                                         -1.1754942e-38, 1.17549435e-38, -1.17549435e-38)]
    maybe = _around(np.float32(WINDOW_HI + 1) * q, np.float32) + _around(np.float32(WINDOW_LO) * q, np.float32)
    return Case("quotient_edges_f32", _edge_rows(valid, maybe, np.float32), q=q, k=k, n_valid=len(valid), maybe=maybe,
                branch="correctly rounded fp32 division, denormals, window by the quotient")


def quotient_edges_f64():
    """q = 0.03.  k * float32(0.03) and k * 0.03 for k in [-40, 40], zeros, denormals, values below the fp32 range (-1e-46 is
    voxel -1, its fp32 value is -0), around +-32704 * q, and 1e300 / -1e39 (rejected; beyond the fp32 range)"""
    q = 0.03
    k = np.arange(-40, 41)
    valid = list((k * np.float32(0.03)).astype(np.float64)) + list(k * q) + [-0.0, 0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-46, -1e-46,
                                                                             2.2250738585072014e-308, -2.2250738585072014e-308]
    maybe = _around((WINDOW_HI + 1) * q, np.float64) + _around(WINDOW_LO * q, np.float64) + [1e300, -1e39]
    return Case("quotient_edges_f64", _edge_rows(valid, maybe, np.float64), q=q, k=k, n_valid=len(valid), maybe=maybe,
                branch="fp64 division; fp32 would floor differently")


def quotient_tiny_q(dtype=np.float32):
    """a q so small that quotients of ordinary values overflow to inf (rejected); small values still have voxels"""
    f32 = np.dtype(dtype) == np.float32
    q = 2e-38 if f32 else 1e-300
    s = 1e-38 if f32 else 1e-300                           # about half a voxel / one voxel
    valid = [0.0, -0.0, s, -s, 50 * s, -50 * s, 30000 * s, -30000 * s] + ([1e-45, -1e-45] if f32 else [5e-324, -5e-324])
    maybe = [1.0, -1.0, 1e3, -1e3, 70000 * s, -70000 * s] + ([3e38, -3e38] if f32 else [1e300, -1e300, 1e10])
    return Case("quotient_tiny_q_" + dtype_tag(dtype), _edge_rows(valid, maybe, dtype), q=q, n_valid=len(valid), maybe=maybe,
                branch="quotient overflows to inf")


def quotient_huge_q(dtype=np.float32):
    """a q so large that every finite value lies in voxel 0 or -1"""
    f32 = np.dtype(dtype) == np.float32
    q, big = (3e38, 1e38) if f32 else (1e308, 1e307)
    valid = [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, big, -big, 12345.678, -0.03]
    return Case("quotient_huge_q_" + dtype_tag(dtype), _edge_rows(valid, [], dtype), q=q, n_valid=len(valid), maybe=[],
                branch="quotients underflow: voxel 0 or -1")


def floor_only(dtype=np.float32):
    """floor_only != 0: voxel = floor(p); q is garbage (0 for fp32, NaN for fp64) and must be ignored"""
    f32 = np.dtype(dtype) == np.float32
    valid = [-0.5, -1.0, -1.5, 0.0, -0.0, 0.5, 1.0, 2.999, 17.0, -17.0, 32703.0, 32703.5, -32704.0, -32703.5, -1e-45, 1e-45, 0.99999994]
    maybe = [32704.0, np.nextafter(np.dtype(dtype).type(32704.0), np.dtype(dtype).type(0)), -32704.5,
             np.nextafter(np.dtype(dtype).type(-32704.0), np.dtype(dtype).type(-np.inf)), -32705.0, np.nan, np.inf, 1e30]
    return Case("floor_only_" + dtype_tag(dtype), _edge_rows(valid, maybe, dtype), q=0.0 if f32 else float("nan"), floor_only=1,
                n_valid=len(valid), maybe=maybe, branch="floor(p), q ignored")


# ---- memory layout and thresholds
def strided(ld, dtype=np.float32):
    """row stride ld > 3, the first row one element past the buffer's start, NaN in every column that is not a coordinate"""
    return Case("strided_%d_%s" % (ld, dtype_tag(dtype)), to_points(with_duplicates(300, 36 + ld), dtype), ld=ld, branch="ld, unaligned base")


def above_2_20():
    """m = 2^20 + 321: two rows per scan thread (per = 2) and a second grid-stride trip of quantize_insert.  Rows below
    2^20 - 70: a random sequence of 4096 rows over 3000 voxels, repeated (every (first, not first) combination of a thread's
    two rows occurs in the first period).  Behind it, across row 2^20: a run of 50 rows of one voxel from 2^20 - 70, then a run
    of 40 rows of another from 2^20 - 20 with a rejected row at 2^20 - 1 (lane 63) and a cloud boundary at 2^20 + 3 inside it;
    the same voxel again at 2^20 + 65 behind a rejected row at 2^20 + 64; new voxels and repeats around them"""
    m, T = TRIP + 321, TRIP
    ids = np.random.default_rng(37).integers(0, 3000, 4096)
    ids = np.tile(ids, m // 4096 + 1)[:m]
    vox = np.stack([ids % 16, ids // 16 % 16, ids // 256], 1).astype(np.int64)
    tail = pool(400, 38, RUN_SHIFT)
    vox[T + 30:] = tail[np.random.default_rng(39).integers(2, 200, m - T - 30)]
    vox[T - 70:T - 20], vox[T - 20:T + 20] = tail[0], tail[1]
    vox[T + 64:T + 66] = tail[1]
    p = ((vox + 0.5) * float(np.float32(0.03))).astype(np.float32)
    p[T - 1, 1], p[T + 64, 0] = np.nan, np.inf
    return Case("above_2_20", p, offsets=[0, T + 3], big=True, rejected={T - 1: "nan", T + 64: "pinf"}, runs=((T - 70, 50), (T - 20, 40)),
                branch="per = 2, second grid-stride trip")


F32, F64 = np.float32, np.float64
_FAMILIES = [(sizes, [(m, F32) for m in SIZES] + [(65, F64), (1025, F64)]),
             (strided, [(4, F32), (7, F32), (4, F64), (7, F64)])]
_BOTH = (runs, runs_aba, runs_one_voxel, runs_rejected, all_rejected, tail_chain_1024, tail_chain_2048, one_home_slot,
         clouds_same_points, clouds_empty, clouds_boundaries, clouds_256, quotient_tiny_q, quotient_huge_q, floor_only)
CASES = {}
for _f, _args in _FAMILIES:
    for _a in _args:
        CASES["%s_%d_%s" % (_f.__name__, _a[0], dtype_tag(_a[1]))] = functools.partial(_f, *_a)
for _f in _BOTH:
    for _d in (F32, F64):
        CASES["%s_%s" % (_f.__name__, dtype_tag(_d))] = functools.partial(_f, _d)
CASES.update(quotient_edges_f32=quotient_edges_f32, quotient_edges_f64=quotient_edges_f64, above_2_20=above_2_20)
CASE_NAMES = sorted(CASES)
BIG_NAMES = ["above_2_20"]
SMALL_NAMES = [n for n in CASE_NAMES if n not in BIG_NAMES]


@functools.lru_cache(maxsize=None)
def case(name):
    """the case, built once per process and shared (callers must not write into its arrays)"""
    c = CASES[name]()
    assert c.name == name and c.big == (name in BIG_NAMES)
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the expected outputs of the case: the loop reference, the vectorised one for the case of 2^20 rows"""
    c = case(name)
    return (reference_vec if c.big else reference)(c.points, c.q, c.floor_only, c.offsets)
