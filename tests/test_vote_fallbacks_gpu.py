"""The launch shapes of the vote op (hv_vote.hip) that the benchmark scenes never take, each against the CPU oracle.

The op picks its launch from the grid and the data alone (tiles_layout, pick_algo, hv_list_scan).  Every other vote test of the
suite runs the two shapes tuned for the benchmark scenes; the cases here reach the others through the public entry points with
ordinary arguments:

  A   the work lists overflow, so the queue launch STREAMS the bins, hot (plane, tile) pairs split into parts by 64-record chunks
  A2  two categories in one call, one of them overflowing
  B   more than PREP_MAX_Y planes: y-bin count / scatter by global atomics (4096 planes: the LDS histogram exactly full)
  C   tile counts 120 / 128 / 4096 / 4128: both sides of the two bounds of the queue launch
  D   more than MAX_R_TILES rotations: algo 0 picks the direct kernel, algo 2 is refused

res = 1 and coordinates in cell units, so dims = (int)((max - min) / res) + 1 is exact; two anchor points with xyz = 0 span the
grid.  All six channels of the tile kernel are 2^-36 integers: the values are held to the bounds of tests/test_vote_gpu.py
(assert_grids_close) or to equality of bits, nothing new.  The calls go through the C ABI on a workspace the test owns (filled
with a byte pattern, 64 KB of sentinel behind the reported size), so that the three words of list_ctl can be read back: they say
which launch ran (list_ctl_words)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import hv_numpy
from canonicalvoting_amd import _lib, hv_cuda
from tests import test_vote_dense_gpu as dense
from tests.test_vote_gpu import assert_grids_close, dev_inputs, run_hip
from tests.test_vote_peaks_gpu import assert_peaks_equal_full

gpu = pytest.mark.gpu
RES = 1.0
R = 120
# hv_vote.hip
TX, TZ = 16, 32
QUEUE_MIN_TILES, LIST_MAX_TILES, PREP_MAX_Y, MAX_R_TILES, PART_VOTES = 128, 4096, 4096, 256, 32768
CV_EINVAL = -22
TAIL, PATTERN = 65536, 0xA5
PATTERN_WORD = int(np.full(4, PATTERN, np.uint8).view(np.int32)[0])


def _rings(rng, cx, cy, cz, rad):
    """points at (cx, cy, cz) [cells] whose votes form rings of radius rad [cells] in their y plane"""
    n = len(cx)
    pts = np.stack([cx, cy, cz], 1).astype(np.float32)
    phi = rng.uniform(0, 2 * np.pi, n)
    off = np.stack([rad * np.cos(phi), np.zeros(n), rad * np.sin(phi)], 1)
    scale = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    return pts, (off / scale).astype(np.float32), scale


def _static(pts):
    """points that vote where they stand (xyz = 0: all rotations of a point into the same cells)"""
    pts = np.asarray(pts, np.float64).astype(np.float32)
    return pts, np.zeros_like(pts), np.ones_like(pts)


def _case(rng, hi, *parts):
    """the parts, then the two anchors (0, 0, 0) and hi with xyz = 0; dims = hi + 1"""
    parts = parts + (_static([[0, 0, 0], hi]),)
    pts, xyz, scale = (np.concatenate([p[i] for p in parts]) for i in range(3))
    prob = np.concatenate([rng.uniform(0.5, 1.0, len(pts) - 2), np.ones(2)]).astype(np.float32)
    return dict(pts=pts, xyz=xyz, scale=scale, prob=prob, dims=[h + 1 for h in hi], R=R)


def case_overflow():
    """3000 rings of 250 to 330 cells around the middle of a 701 x 4 x 701 grid (968 tiles): each crosses about a hundred tiles,
    1.6 x the capacity of the work lists.  600 more points with xyz = 0 inside tile (21, 10): 600 x 120 arc steps > 2 PART_VOTES
    in planes 1 and 2 of that tile, which the queue therefore splits into three parts."""
    rng = np.random.default_rng(7)
    n = 3000
    cx, cy, cz = rng.uniform(300, 400, n), rng.uniform(1.1, 1.9, n), rng.uniform(300, 400, n)
    rings = _rings(rng, cx, cy, cz, rng.uniform(250, 330, n))
    hot = _static(np.stack([rng.uniform(340, 350, 600), rng.uniform(1.1, 1.9, 600), rng.uniform(330, 350, 600)], 1))
    return _case(rng, [700, 3, 700], rings, hot)


def case_overflow_small_rings():
    """category 1 of A2: the same points with xyz * 0.05, rings of about 15 cells - the lists fit"""
    c = case_overflow()
    return dict(c, xyz=(c["xyz"] * np.float32(0.05)).astype(np.float32))


def _case_tall(Y):
    """4000 points over a 21 x Y x 21 grid (two tiles), one stratum of (Y - 1) / 4000 of the height each: nearly every y-bin is
    populated, by 0, 1 or 2 records.  Rings of 0 to 6 cells, every fifth xyz = 0, every tenth point on the nodes."""
    rng = np.random.default_rng(4000 + Y)
    n = 4000
    cy = np.minimum((rng.permutation(n) + rng.uniform(0, 1, n)) * ((Y - 1) / n), Y - 1.01)
    rad = rng.uniform(0, 6, n)
    rad[::5] = 0.0
    rings = _rings(rng, rng.uniform(0, 20, n), cy, rng.uniform(0, 20, n), rad)
    rings[0][::10] = np.round(rings[0][::10])
    return _case(rng, [20, Y - 1, 20], rings)


def _case_wide(X, Y, Z):
    """2000 points scattered over an X x Y x Z grid, rings of 0 to 40 cells, every fifth xyz = 0, every tenth on the x / z nodes"""
    rng = np.random.default_rng(X + Z)
    n = 2000
    rad = rng.uniform(0, 40, n)
    rad[::5] = 0.0
    rings = _rings(rng, rng.uniform(0, X - 1, n), rng.uniform(0.1, Y - 1.1, n), rng.uniform(0, Z - 1, n), rad)
    rings[0][::10, 0::2] = np.round(rings[0][::10, 0::2])
    return _case(rng, [X - 1, Y - 1, Z - 1], rings)


# name -> (case, launch: "overflow" (queue launch, bins streamed), "queue" (queue launch, work lists), "stream" (streaming launch))
CASES = {
    "overflow": (case_overflow, "overflow"),
    "tall4096": (lambda: _case_tall(4096), "stream"),
    "tall4097": (lambda: _case_tall(4097), "stream"),
    "tall4160": (lambda: _case_tall(4160), "stream"),
    "tiles120": (lambda: _case_wide(128, 3, 480), "stream"),
    "tiles128": (lambda: _case_wide(128, 3, 512), "queue"),
    "tiles4096": (lambda: _case_wide(2048, 2, 1024), "queue"),
    "tiles4128": (lambda: _case_wide(2064, 2, 1024), "stream"),
}
NAMES = list(CASES)
DIMS = {"overflow": [701, 4, 701], "tall4096": [21, 4096, 21], "tall4097": [21, 4097, 21], "tall4160": [21, 4160, 21],
        "tiles120": [128, 3, 480], "tiles128": [128, 3, 512], "tiles4096": [2048, 2, 1024], "tiles4128": [2064, 2, 1024]}
NTILES = {"overflow": 968, "tall4096": 2, "tall4097": 2, "tall4160": 2, "tiles120": 120, "tiles128": 128, "tiles4096": 4096,
          "tiles4128": 4128}
# list_capacity(n, ntiles) = min(n * ntiles, 40 n + 65536) with the anchors counted in n (the streaming launches carve no lists)
CAPACITY = {"overflow": 40 * 3602 + 65536, "tall4096": 4002 * 2, "tall4097": 4002 * 2, "tall4160": 4002 * 2,
            "tiles120": 40 * 2002 + 65536, "tiles128": 40 * 2002 + 65536, "tiles4096": 40 * 2002 + 65536,
            "tiles4128": 40 * 2002 + 65536}


@functools.lru_cache(maxsize=None)
def case(name):
    return case_overflow_small_rings() if name == "overflow_small_rings" else CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's grids, its in-bounds vote count and the contributions per cell, computed once and left unchanged"""
    c = case(name)
    ref = oracle.hv_forward(c["pts"], c["xyz"], c["scale"], c["prob"], RES, c["R"], return_vin=True)
    counts = hv_numpy.contribution_counts(c["pts"], c["xyz"], c["scale"], RES, c["R"])
    return ref[:3], ref[3], counts


def ntiles_of(dims):
    return -(-dims[0] // TX) * -(-dims[2] // TZ)


def list_capacity(n, ntiles):
    return min(n * ntiles, 40 * n + 65536)


def takes_queue_launch(dims):
    # (tiles_layout's other two conditions - capacities below 2^31 - hold for every case here by orders of magnitude)
    return QUEUE_MIN_TILES <= ntiles_of(dims) <= LIST_MAX_TILES


def ring_entries(c):
    """numpy fp32 restatement of the work-list count (hv_list_pass / ring_touches of hv_vote.hip): the (record, tile) pairs whose
    ring can reach the tile's rectangle [x0 - 1, x0 + TX] x [z0 - 1, z0 + TZ], over the records with an in-bounds y"""
    f = np.float32
    X, Y, Z = c["dims"]
    corr = (c["xyz"] * c["scale"]).astype(f)
    gy = (c["pts"][:, 1] - corr[:, 1]).astype(f)          # corner 0, res 1
    keep = (gy >= 0) & (gy < f(Y - 1))
    ux, uz = c["pts"][keep, 0][:, None], c["pts"][keep, 2][:, None]
    r = np.sqrt((corr[keep, 0] * corr[keep, 0] + corr[keep, 2] * corr[keep, 2]).astype(f)).astype(f)[:, None]
    tol = (f(0.05) + f(1e-5) * (r + np.abs(ux) + np.abs(uz))).astype(f)
    z0 = np.arange(-(-Z // TZ), dtype=f)[None] * f(TZ)
    zlo, zhi = z0 - f(1), z0 + f(TZ)
    dzn = np.maximum(f(0), np.maximum(zlo - uz, uz - zhi))
    dzf = np.maximum(np.abs(uz - zlo), np.abs(uz - zhi))
    total = 0
    for tx in range(-(-X // TX)):
        xlo, xhi = f(tx * TX - 1), f(tx * TX + TX)
        dxn = np.maximum(f(0), np.maximum(xlo - ux, ux - xhi))
        dxf = np.maximum(np.abs(ux - xlo), np.abs(ux - xhi))
        dmin, dmax = np.sqrt(dxn * dxn + dzn * dzn), np.sqrt(dxf * dxf + dzf * dzf)
        total += int(((r >= dmin - tol) & (r <= dmax + tol)).sum())
    return total


def test_cases_have_the_geometry_their_branch_needs():
    """CPU: grid shape, tile count, launch shape and list capacity of every case; the y-bins of the tall grids; the overflow of
    case A restated in numpy (the device's own total is asserted by the GPU tests, this one says the seed is a sound choice)"""
    for name in NAMES:
        c, launch = case(name), CASES[name][1]
        dims = oracle.grid_geometry(c["pts"], RES)[2]
        assert dims == c["dims"] == DIMS[name], name
        assert ntiles_of(dims) == NTILES[name], name
        assert list_capacity(len(c["pts"]), NTILES[name]) == CAPACITY[name], name
        assert takes_queue_launch(dims) == (launch != "stream"), name
        assert np.prod(dims) <= 6.6e6 and len(c["pts"]) <= 4002, name
    assert NTILES["tiles120"] == QUEUE_MIN_TILES - 8 and NTILES["tiles128"] == QUEUE_MIN_TILES
    assert NTILES["tiles4096"] == LIST_MAX_TILES and NTILES["tiles4128"] > LIST_MAX_TILES
    # A: 3602 points, all records but the anchor's in bin 1; the 600 static points inside one tile
    c = case("overflow")
    n = len(c["pts"])
    cap = list_capacity(n, NTILES["overflow"])
    assert n == 3602 and cap == 40 * n + 65536 == 209616
    assert list_capacity(3000, 968) == 185536 and list_capacity(10, 968) == 9680
    entries = ring_entries(c)
    assert entries >= 1.5 * cap, (entries, cap)
    hot = c["pts"][3000:3600]
    assert len(np.unique(np.floor(hot[:, 0]) // TX)) == 1 and len(np.unique(np.floor(hot[:, 2]) // TZ)) == 1
    assert not c["xyz"][3000:].any() and 600 * R > 2 * PART_VOTES
    assert set(np.floor(c["pts"][:3600, 1])) == {1.0}
    # A2's second category fits
    small = case("overflow_small_rings")
    assert 0 < ring_entries(small) <= cap // 4
    # B: the bins on both sides of PREP_MAX_Y, most of them populated, by 0, 1 and 2 records
    for Y in (4096, 4097, 4160):
        c = case("tall%d" % Y)
        assert (Y <= PREP_MAX_Y) == (Y == 4096)
        assert not c["xyz"][:, 1].any()                            # the y cell of a vote is the point's
        fy = np.floor(c["pts"][:, 1]).astype(int)
        fy = fy[fy < Y - 1]
        occupancy = np.bincount(fy, minlength=Y - 1)
        assert (occupancy > 0).sum() > 3000 and {0, 1, 2} <= set(occupancy), Y
        assert fy.max() >= Y - 3
    # D
    assert dense.case_r256()[5] == MAX_R_TILES


def _ws_bytes(c, K=1, algo=0, num_rots=None):
    cdims = (ctypes.c_int * 3)(*c["dims"])
    return _lib.lib().cv_hv_forward_cat_workspace_bytes(len(c["pts"]), num_rots or c["R"], cdims, algo, K)


def pattern_workspace(cuda, size):
    return torch.full((size + TAIL,), PATTERN, dtype=torch.uint8, device=cuda)


def assert_tail_untouched(ws, size, tag):
    assert bool((ws[size:] == PATTERN).all()), tag + ": bytes behind the reported workspace size were written"


def list_ctl_words(ws, n, stride=0, k=0):
    """list_ctl[0..2] of category k = (entry total of the work lists, overflow flag, queue items), read from the caller's
    workspace.  tiles_layout (hv_vote.hip) carves fy[n] (int32), rec[13 n] (fp32), then list_ctl, each aligned to 256 bytes;
    category k's carve lies k * cv_hv_forward_workspace_bytes behind the first.  The queue launch zeroes the words with the
    per-call fill and writes all three; the streaming launch neither zeroes nor writes them."""
    a256 = lambda v: -(-v // 256) * 256
    at = a256(a256(4 * n) + 52 * n) + k * stride
    return [int(v) for v in ws[at:at + 12].view(torch.int32).cpu()]


def assert_launch(words, launch, c, tag):
    """the words say which launch ran (see list_ctl_words)"""
    total, flag, items = words
    n, (_, Y, _), ntiles = len(c["pts"]), c["dims"], ntiles_of(c["dims"])
    cap = list_capacity(n, ntiles)
    if launch == "stream":
        assert words == [PATTERN_WORD] * 3, (tag, words)
    elif launch == "queue":
        assert flag == 0 and 0 < total <= cap and items >= Y * ntiles, (tag, words, cap)
    else:
        assert flag == 1 and total >= 1.25 * cap and items >= Y * ntiles, (tag, words, cap)


def vote(cuda, c, ws, ws_bytes, thresh=None, cats=None, algo=0, num_rots=None):
    """cv_hv_forward_f32 (thresh None) or cv_hv_forward_peaks_f32 on the caller's workspace, rot / scale pre-filled with NaN;
    cats: a list of xyz arrays through the category entry points.  Returns the device grids."""
    L = _lib.lib()
    p, _, s, o = dev_inputs(cuda, c["pts"], c["xyz"], c["scale"], c["prob"])
    xs = [c["xyz"]] if cats is None else cats
    K = len(xs)
    x = torch.from_numpy(np.ascontiguousarray(np.stack(xs))).to(cuda)
    s, o = torch.stack([s] * K).contiguous(), torch.stack([o] * K).contiguous()
    n, rots = len(c["pts"]), num_rots or c["R"]
    mn, _, dims = hv_cuda.grid_geometry(p, RES)
    assert dims == c["dims"] and list(mn) == [0.0, 0.0, 0.0]
    X, Y, Z = dims
    grids = [torch.full((K, X, Y, Z) + tail, float("nan"), dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    ptr = hv_cuda._ptr
    head = [ptr(p), ptr(x), ptr(s), ptr(o), n, ctypes.c_float(RES), rots, hv_cuda._f3(mn), (ctypes.c_int * 3)(*dims)]
    tail = [ptr(g) for g in grids] + [ptr(ws), ws_bytes, algo] + ([] if thresh is None else [ctypes.c_float(thresh)])
    tail.append(hv_cuda._stream(cuda))
    if cats is None:
        fn = "cv_hv_forward_f32" if thresh is None else "cv_hv_forward_peaks_f32"
        args = head + tail
    else:
        fn = "cv_hv_forward_cat_f32" if thresh is None else "cv_hv_forward_peaks_cat_f32"
        args = head + [K] + tail
    with torch.cuda.device(cuda):
        _lib.check(getattr(L, fn)(*args), fn)
    torch.cuda.synchronize()
    return grids if cats is not None else [g[0] for g in grids]


def equal_bits(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@gpu
def test_list_ctl_is_where_the_helper_reads_it(cuda, built_lib):
    """the guard of list_ctl_words: on the `lists` case of tests/test_vote_dense_gpu.py (work-queue launch, lists that fit) the
    three words are a flag of 0, a total inside the capacity and at least one item per (plane, tile) - a change of the workspace
    layout fails here instead of making the tests below read other words"""
    pts, xyz, scale, prob, res, rots = dense.case_lists()
    dims = oracle.grid_geometry(pts, res)[2]
    ntiles = ntiles_of(dims)
    assert ntiles >= QUEUE_MIN_TILES
    p, x, s, o = dev_inputs(cuda, pts, xyz, scale, prob)
    L = _lib.lib()
    mn, _, ddims = hv_cuda.grid_geometry(p, res)
    assert ddims == dims
    cdims = (ctypes.c_int * 3)(*dims)
    n = len(pts)
    size = L.cv_hv_forward_workspace_bytes(n, rots, cdims, 0)
    ws = pattern_workspace(cuda, size)
    grids = [torch.empty(tuple(dims) + tail, dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    with torch.cuda.device(cuda):
        _lib.check(L.cv_hv_forward_f32(hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), n, ctypes.c_float(res),
                                       rots, hv_cuda._f3(mn), cdims, hv_cuda._ptr(grids[0]), hv_cuda._ptr(grids[1]),
                                       hv_cuda._ptr(grids[2]), hv_cuda._ptr(ws), size, 0, hv_cuda._stream(cuda)),
                   "cv_hv_forward_f32")
    torch.cuda.synchronize()
    total, flag, items = list_ctl_words(ws, n)
    assert flag == 0 and 0 < total <= list_capacity(n, ntiles) and items >= dims[1] * ntiles, (total, flag, items)
    assert_tail_untouched(ws, size, "lists")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_fallback_launch_matches_the_oracle(cuda, built_lib, name):
    """on a pattern-filled workspace of exactly the reported size: the launch the case is built for ran (list_ctl), the grids
    match the oracle under the bounds of the main path, the in-bounds vote count is the oracle's, a second call on the used
    workspace and a call on a roomy zeroed one give the same bits, and the 64 KB behind the reported size keep their pattern.
    (tall grids: the order of the records inside a bin is the atomic order of the scatter - the integer sums must hide it)"""
    c, launch = case(name), CASES[name][1]
    ref, vin, counts = reference(name)
    n = len(c["pts"])
    size = _ws_bytes(c)
    assert size > 0
    tight = pattern_workspace(cuda, size)
    first = vote(cuda, c, tight, size)
    words = list_ctl_words(tight, n)
    print("%s: list_ctl %s, capacity %d, in-bounds votes %d" % (name, words, list_capacity(n, ntiles_of(c["dims"])), vin))
    assert_tail_untouched(tight, size, name)
    assert not bool((tight[:size] == PATTERN).all())
    assert_launch(words, launch, c, name)
    assert_grids_close([g.cpu().numpy() for g in first], ref, name, counts=counts)
    p, x, s, _ = dev_inputs(cuda, c["pts"], c["xyz"], c["scale"], c["prob"])
    assert hv_cuda.count_votes(p, x, s, RES, c["R"], [0.0, 0.0, 0.0], c["dims"]) == vin
    again = vote(cuda, c, tight, size)
    assert equal_bits(first, again), name + ": the second call differs"
    assert list_ctl_words(tight, n) == words
    assert_tail_untouched(tight, size, name)
    del tight
    roomy = torch.zeros((size + (1 << 20) + TAIL,), dtype=torch.uint8, device=cuda)
    assert equal_bits(first, vote(cuda, c, roomy, roomy.numel())), name + ": a roomy workspace gives other grids"


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_fallback_launch_peaks_vote_writes_the_full_votes_bits(cuda, built_lib, name):
    """cv_hv_forward_peaks_f32 on the same launch: thresh = -inf writes all three grids of cv_hv_forward_f32, a threshold that a
    few hundred cells reach (chosen on the oracle) writes grid_obj everywhere and the quotients at those cells"""
    c, launch = case(name), CASES[name][1]
    ref = reference(name)[0]
    n = len(c["pts"])
    size = _ws_bytes(c)
    ws = pattern_workspace(cuda, size)
    full = vote(cuda, c, ws, size)
    everywhere = vote(cuda, c, ws, size, thresh=float("-inf"))
    assert_launch(list_ctl_words(ws, n), launch, c, name)
    for u, v, g in zip(full, everywhere, ("obj", "rot", "scale")):
        assert torch.equal(u, v), "%s: grid_%s at thresh -inf" % (name, g)
    top = np.sort(np.partition(ref[0].ravel(), -301)[-301:])
    th = float(np.float32(0.5 * (float(top[0]) + float(top[1]))))
    assert th > 0
    peaks = vote(cuda, c, ws, size, thresh=th)
    hot = assert_peaks_equal_full(full, peaks, th, name)
    assert 100 < hot < 600, (name, hot, th)
    assert bool(torch.isnan(peaks[1]).any()) and bool(torch.isnan(peaks[2]).any())     # not accumulated everywhere
    assert_launch(list_ctl_words(ws, n), launch, c, name)
    assert_tail_untouched(ws, size, name)


@gpu
def test_two_categories_one_of_them_overflowing(cuda, built_lib):
    """cv_hv_forward_cat_f32, K = 2: category 0 is case A (lists overflow, bins streamed), category 1 the same points with rings
    of a twentieth of the size (lists fit).  Each category's grids are the bits of its own single call, each carve has its own
    flag"""
    c, small = case("overflow"), case("overflow_small_rings")
    n, ntiles = len(c["pts"]), NTILES["overflow"]
    one = _ws_bytes(c)
    size = _ws_bytes(c, K=2)
    assert size == 2 * one
    ws = pattern_workspace(cuda, size)
    both = vote(cuda, c, ws, size, cats=[c["xyz"], small["xyz"]])
    assert_tail_untouched(ws, size, "two categories")
    w0, w1 = list_ctl_words(ws, n, one, 0), list_ctl_words(ws, n, one, 1)
    assert_launch(w0, "overflow", c, "category 0")
    assert_launch(w1, "queue", small, "category 1")
    single = pattern_workspace(cuda, one)
    for k, ck in enumerate((c, small)):
        alone = vote(cuda, ck, single, one)
        assert list_ctl_words(single, n) == (w0, w1)[k]
        assert float(alone[0].max()) > 0
        for u, v, g in zip(both, alone, ("obj", "rot", "scale")):
            assert torch.equal(u[k], v), "category %d: grid_%s" % (k, g)
    assert w0[0] > 4 * w1[0] and ntiles == ntiles_of(small["dims"])


def _scene_257():
    return dense._small_scene(MAX_R_TILES + 1)


@gpu
def test_auto_picks_the_direct_kernel_above_the_tile_kernels_rotations(cuda, built_lib):
    """R = 257 with algo 0: the reported workspace is the direct kernel's 256 bytes, the call leaves them untouched (the tile
    algorithm would have refused them as too small), and the grids meet the bounds test_forward_matches_oracle_small holds
    algo 1 to"""
    pts, xyz, scale, prob, res, rots = _scene_257()
    assert rots == 257
    L = _lib.lib()
    dims = oracle.grid_geometry(pts, res)[2]
    cdims = (ctypes.c_int * 3)(*dims)
    n = len(pts)
    assert L.cv_hv_forward_workspace_bytes(n, rots, cdims, 0) == 256 < L.cv_hv_forward_workspace_bytes(n, rots - 1, cdims, 0)
    ref = oracle.hv_forward(pts, xyz, scale, prob, res, rots, return_vin=True)
    p, x, s, o = dev_inputs(cuda, pts, xyz, scale, prob)
    mn, _, ddims = hv_cuda.grid_geometry(p, res)
    assert ddims == dims
    ws = pattern_workspace(cuda, 256)
    grids = [torch.full(tuple(dims) + tail, float("nan"), dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    with torch.cuda.device(cuda):
        _lib.check(L.cv_hv_forward_f32(hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), n, ctypes.c_float(res),
                                       rots, hv_cuda._f3(mn), cdims, hv_cuda._ptr(grids[0]), hv_cuda._ptr(grids[1]),
                                       hv_cuda._ptr(grids[2]), hv_cuda._ptr(ws), 256, 0, hv_cuda._stream(cuda)),
                   "cv_hv_forward_f32")
    torch.cuda.synchronize()
    assert bool((ws == PATTERN).all())
    assert_grids_close([g.cpu().numpy() for g in grids], ref[:3], "R 257, algo 0", inputs=(pts, xyz, scale, res, rots))
    assert hv_cuda.count_votes(p, x, s, res, rots, mn, dims) == ref[3]
    # the drop-in takes the same way
    assert_grids_close(run_hip(cuda, pts, xyz, scale, prob, res, rots, 0), ref[:3], "R 257, hv_cuda", inputs=(pts, xyz, scale, res, rots))


@gpu
def test_tiles_algorithm_refuses_more_rotations_and_leaves_the_stream_usable(cuda, built_lib):
    """R = 257 with algo 2: CV_EINVAL before anything is launched (the grids keep their pre-fill), and a following R = 120 call on
    the same stream matches the oracle"""
    pts, xyz, scale, prob, res, rots = _scene_257()
    L = _lib.lib()
    dims = oracle.grid_geometry(pts, res)[2]
    cdims = (ctypes.c_int * 3)(*dims)
    n = len(pts)
    p, x, s, o = dev_inputs(cuda, pts, xyz, scale, prob)
    mn, _, _ = hv_cuda.grid_geometry(p, res)
    size = L.cv_hv_forward_workspace_bytes(n, rots, cdims, 2)
    assert size > 256
    ws = pattern_workspace(cuda, size)
    grids = [torch.full(tuple(dims) + tail, float("nan"), dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    with torch.cuda.device(cuda):
        rc = L.cv_hv_forward_f32(hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), n, ctypes.c_float(res), rots,
                                 hv_cuda._f3(mn), cdims, hv_cuda._ptr(grids[0]), hv_cuda._ptr(grids[1]), hv_cuda._ptr(grids[2]),
                                 hv_cuda._ptr(ws), size, 2, hv_cuda._stream(cuda))
    assert rc == CV_EINVAL
    assert b"num_rots" in L.cv_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g).all()) for g in grids) and bool((ws == PATTERN).all())
    ref = oracle.hv_forward(pts, xyz, scale, prob, res, R, return_vin=True)
    hip = run_hip(cuda, pts, xyz, scale, prob, res, R, 2)
    assert_grids_close(hip, ref[:3], "R 120 after the refusal", inputs=(pts, xyz, scale, res, R))
    assert hv_cuda.count_votes(p, x, s, res, R, mn, dims) == ref[3]
