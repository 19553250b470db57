"""cv_hv_forward_peaks_f32 / cv_hv_forward_peaks_cat_f32 and cv_scene_desc.peak_quotients: the vote for a caller that only decodes
(hv_vote.hip: VOTE_OBJ, then VOTE_PEAKS over the tiles that hold a cell >= thresh) against the full vote.

All six sums of the tile kernel are 2^-36 fixed-point integers, so every comparison here is EQUALITY of bits: the objectness
grid everywhere, the rot / scale quotients at every cell with objectness >= thresh (elsewhere their content is unspecified: the
grids are pre-filled with NaN so that a cell the decode wrongly read would show), and everything cv_decode_f32 makes of the two
grid sets.  The CPU oracle is only asked whether a case is what it claims to be (how many cells reach the threshold, where they
lie); the reference of every comparison is the full vote of the same library."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from canonicalvoting_amd import _lib, decode, hv_cuda, pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_scene, synth_predictions

pytestmark = pytest.mark.gpu
RES = 0.03
TX, TZ = 16, 32                  # tile of hv_fwd_tiles (cells in x / z)
QUEUE_MIN_TILES = 128            # from this many tiles per plane on the work-queue launch, the streaming launch below
CAND_CAP = 512                   # candidate capacity of the decode calls below


def _t(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _scene_case(seed, n, R=120, **kw):
    sc = make_scene(seed, n_points=n, **kw)
    xyz, scale, prob, cls = synth_predictions(sc)
    return dict(pts=sc.points, xyz=xyz, scale=scale, prob=prob, cls=cls, res=sc.res, R=R)


@functools.lru_cache(maxsize=None)
def case_stream():
    """3000 points, 3 boxes, a grid of 3 x 2 tiles cut by the grid on both axes: the streaming launch"""
    return _scene_case(1, 3000, res=0.06, room=(2.0, 1.0, 2.0), n_boxes=3, margin=0.6, box_scale=0.5)


@functools.lru_cache(maxsize=None)
def case_queue():
    """4000 points in a 16 m x 4 m room at res 0.03, about 170 tiles per plane: the work-queue launch with its work lists,
    (plane, tile) pairs that receive nothing and pairs with several parts"""
    return _scene_case(6, 4000, room=(16.0, 2.0, 4.0), n_boxes=8)


def _clusters(centres, per, rng, spread=0.15):
    """`per` points around each centre [cells] that vote where they stand (xyz = 0: a ring of radius 0, all rotations into the
    same cells), objectness 1"""
    c = np.repeat(np.asarray(centres, np.float64), per, 0)
    c = c + rng.uniform(-spread, spread, c.shape)
    n = len(c)
    return (c * RES).astype(np.float32), np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32), np.ones(n, np.float32)


def _join(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def _anchors(hi):
    """two points with xyz = 0 and no weight that span the grid [0, hi] cells"""
    a = (np.array([[0, 0, 0], hi], np.float64) * RES).astype(np.float32)
    return a, np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32), np.zeros(2, np.float32)


BORDER_HI = (40, 4, 70)          # grid of 41 x 5 x 71 cells: 3 x 3 tiles, the last ones 9 and 7 cells wide
BORDER_CENTRES = [(15.5, 1.5, 10.5),      # cells 15 and 16 in x: both sides of the border between x tiles 0 and 1
                  (24.5, 2.5, 31.5),      # cells 31 and 32 in z: both sides of the border between z tiles 0 and 1
                  (39.5, 1.5, 50.5),      # cells 39 and 40 in x: the grid's last row
                  (20.5, 2.5, 69.5)]      # cells 69 and 70 in z: the grid's last column


@functools.lru_cache(maxsize=None)
def case_border():
    rng = np.random.default_rng(7)
    pts, xyz, scale, prob = _join(_clusters(BORDER_CENTRES, 6, rng), _anchors(BORDER_HI))
    return dict(pts=pts, xyz=xyz, scale=scale, prob=prob, cls=np.zeros(len(pts), np.int32), res=RES, R=120)


def _parts_case(hi):
    rng = np.random.default_rng(104)
    n = 10000
    cx, cy, cz, rad = rng.uniform(8, 56, n), rng.uniform(3.1, 3.9, n), rng.uniform(8, 56, n), rng.uniform(1, 7, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    off = np.stack([rad * np.cos(phi), np.zeros(n), rad * np.sin(phi)], 1) * RES
    scale = rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    rings = ((np.stack([cx, cy, cz], 1) * RES).astype(np.float32), (off / scale).astype(np.float32), scale,
             rng.uniform(0.005, 0.01, n).astype(np.float32))
    hot = _clusters([(12.5, 3.5, 12.5), (15.5, 3.5, 40.5), (40.5, 3.5, 31.5), (50.5, 3.5, 50.5)], 6, rng)
    pts, xyz, scale, prob = _join(rings, hot, _anchors(hi))
    return dict(pts=pts, xyz=xyz, scale=scale, prob=prob, cls=np.zeros(len(pts), np.int32), res=RES, R=120)


@functools.lru_cache(maxsize=None)
def case_parts():
    """10 000 points in one y cell, rings of 1 to 7 cells: the plane's two bins hold 10 000 records - three parts per tile at 4096
    records per part, one at 12288 - plus four clusters that make hot cells in the split planes.  A grid of 8 x 8 tiles (the
    streaming launch) and 9 planes: with the parts about 700 work items, more than the peaks launch has workgroups"""
    return _parts_case((127, 8, 255))


@functools.lru_cache(maxsize=None)
def case_queue_parts():
    """the same points in a grid of 16 x 8 = 128 tiles, the smallest that takes the work-queue launch: there the parts go by the
    summed arc lengths, and the eight tiles under the rings receive 10 000 x 120 / 8 = 150 000 steps each against 32 768 per part"""
    return _parts_case((255, 8, 255))


@functools.lru_cache(maxsize=None)
def oracle_obj(name):
    c = CASES[name]()
    return oracle.hv_forward(c["pts"], c["xyz"], c["scale"], c["prob"], c["res"], c["R"])[0]


CASES = {"stream": case_stream, "queue": case_queue, "border": case_border, "parts": case_parts, "queue_parts": case_queue_parts}
# the threshold of each case, chosen on the CPU oracle so that a few dozen cells reach it (the scenes: 40 and 56 cells; at the
# library's 60 the coarse 3000-point scenes have several hundred).  The cluster cases: 6 points of weight 1 x 120 rotations spread
# over the 8 cells around a centre, so each of them collects well over 20 and every other cell next to nothing
THRESH = {"stream": 100.0, "queue": 10.0, "border": 20.0, "parts": 20.0, "queue_parts": 20.0}


def check_case(name):
    """the case is what its docstring says (CPU oracle): launch shape, and a hot-cell count the decode comparison can hold"""
    c = CASES[name]()
    ref = oracle_obj(name)
    X, _, Z = ref.shape
    ntiles = -(-X // TX) * -(-Z // TZ)
    assert (ntiles >= QUEUE_MIN_TILES) == name.startswith("queue"), (name, ntiles)
    if name == "queue_parts":
        assert ntiles == QUEUE_MIN_TILES
    hot = int((ref >= THRESH[name]).sum())
    assert 0 < hot < CAND_CAP // 2, (name, hot)
    if name.startswith("queue"):         # some tile of some plane stays empty
        pad = np.zeros((-(-X // TX) * TX, ref.shape[1], -(-Z // TZ) * TZ), ref.dtype)
        pad[:X, :, :Z] = ref
        assert (pad.reshape(-1, TX, ref.shape[1], pad.shape[2] // TZ, TZ).max((1, 4)) == 0).any()
    return c, ref


def vote(cuda, c, thresh=None, part_records=0, cats=None):
    """the three grids of cv_hv_forward_f32 (thresh None) or cv_hv_forward_peaks_f32 (rot / scale pre-filled with NaN); cats: a
    list of (xyz, scale, prob) through the category entry points instead.  Returns device tensors and the grid corner."""
    L = _lib.lib()
    pts = _t(cuda, c["pts"])
    per_cat = cats if cats is not None else [(c["xyz"], c["scale"], c["prob"])]
    K = len(per_cat)
    xyz, scale, prob = (_t(cuda, np.stack([p[i] for p in per_cat])) for i in range(3))
    n, R, res = len(c["pts"]), c["R"], c["res"]
    mn, _, dims = hv_cuda.grid_geometry(pts, res)
    X, Y, Z = dims
    g_obj = torch.full((K, X, Y, Z), float("nan"), dtype=torch.float32, device=cuda)
    g_rot = torch.full((K, X, Y, Z, 2), float("nan"), dtype=torch.float32, device=cuda)
    g_scale = torch.full((K, X, Y, Z, 3), float("nan"), dtype=torch.float32, device=cuda)
    cdims = (ctypes.c_int * 3)(*dims)
    wsb = L.cv_hv_forward_cat_workspace_bytes(n, R, cdims, 0, K)
    assert wsb == K * L.cv_hv_forward_workspace_bytes(n, R, cdims, 0)
    ws = _lib.scratch(cuda, "hv_forward", wsb)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    head = [p(pts), p(xyz), p(scale), p(prob), n, ctypes.c_float(res), R, (ctypes.c_float * 3)(*mn), cdims]
    grids = [p(g_obj), p(g_rot), p(g_scale), p(ws), ws.numel(), 0]
    tail = ([] if thresh is None else [ctypes.c_float(thresh)]) + [ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)]
    if cats is None:
        fn = "cv_hv_forward_f32" if thresh is None else "cv_hv_forward_peaks_f32"
        args = head + grids + tail
    else:
        fn = "cv_hv_forward_cat_f32" if thresh is None else "cv_hv_forward_peaks_cat_f32"
        args = head + [K] + grids + tail
    before = L.cv_hv_set_part_records_thread(int(part_records))
    try:
        with torch.cuda.device(cuda):
            _lib.check(getattr(L, fn)(*args), fn)
    finally:
        L.cv_hv_set_part_records_thread(before)
    torch.cuda.synchronize()
    out = (g_obj, g_rot, g_scale) if cats is not None else (g_obj[0], g_rot[0], g_scale[0])
    return out, mn


def assert_peaks_equal_full(full, peaks, thresh, tag):
    """g_obj everywhere, rot / scale at every cell with g_obj >= thresh; returns the number of such cells"""
    assert not torch.isnan(full[0]).any() and not torch.isnan(full[1]).any() and not torch.isnan(full[2]).any(), tag
    assert torch.equal(full[0], peaks[0]), tag + ": grid_obj"
    hot = full[0] >= thresh
    assert torch.equal(full[1][hot], peaks[1][hot]), tag + ": grid_rot at the cells >= thresh"
    assert torch.equal(full[2][hot], peaks[2][hot]), tag + ": grid_scale at the cells >= thresh"
    return int(hot.sum())


def decode_of(cuda, c, grids, mn, thresh):
    # (the decode eliminates in grid_obj: it gets a copy)
    return decode.decode_boxes(grids[0].clone(), grids[1], grids[2], _t(cuda, c["pts"]), _t(cuda, c["xyz"]), _t(cuda, c["prob"]),
                               _t(cuda, c["cls"]), c["res"], corner=mn, thresh_high=thresh, max_candidates=CAND_CAP)


def assert_same_decode(a, b, tag):
    for k in ("cand_idx", "verdict", "boxes", "scores", "classes"):
        assert np.array_equal(a[k], b[k]), tag + ": " + k
    assert a["truncated"] == b["truncated"] is False, tag


@pytest.mark.parametrize("name", ["stream", "queue"])
def test_threshold_minus_infinity_writes_the_full_grids(cuda, built_lib, name):
    """every cell counts: all three grids equal everywhere - every tile, the edge tiles cut by the grid, the (plane, tile) pairs
    that receive nothing (the queue launch has them), on both instances of the launch"""
    c, _ = check_case(name)
    full, _ = vote(cuda, c)
    peaks, _ = vote(cuda, c, thresh=float("-inf"))
    for u, v, g in zip(full, peaks, ("obj", "rot", "scale")):
        assert torch.equal(u, v), "%s: grid_%s" % (name, g)


@pytest.mark.parametrize("name", ["stream", "queue"])
def test_decode_threshold_same_peaks_same_decode(cuda, built_lib, name):
    c, ref = check_case(name)
    th = THRESH[name]
    full, mn = vote(cuda, c)
    peaks, _ = vote(cuda, c, thresh=th)
    hot = assert_peaks_equal_full(full, peaks, th, name)
    assert 0 < hot < CAND_CAP // 2 and abs(hot - int((ref >= th).sum())) <= 0.1 * hot + 2, (hot, int((ref >= th).sum()))
    # the quotients were NOT accumulated everywhere: a tile without a hot cell keeps the pre-fill
    assert bool(torch.isnan(peaks[1]).any()) and bool(torch.isnan(peaks[2]).any())
    a, b = decode_of(cuda, c, full, mn, th), decode_of(cuda, c, peaks, mn, th)
    assert len(a["cand_idx"]) > 0, "the comparison saw no candidates"
    assert_same_decode(a, b, name)


def test_threshold_above_the_maximum(cuda, built_lib):
    c, ref = check_case("stream")
    th = float(np.ceil(ref.max() * 1.5))
    full, mn = vote(cuda, c)
    assert float(full[0].max()) < th
    peaks, _ = vote(cuda, c, thresh=th)
    assert torch.equal(full[0], peaks[0])
    assert bool(torch.isnan(peaks[1]).all()) and bool(torch.isnan(peaks[2]).all())      # nothing was written
    a, b = decode_of(cuda, c, full, mn, th), decode_of(cuda, c, peaks, mn, th)
    assert len(a["cand_idx"]) == len(b["cand_idx"]) == 0 and len(b["boxes"]) == 0
    assert_same_decode(a, b, "above the maximum")


@pytest.mark.parametrize("name", ["parts", "queue_parts"])
def test_split_planes_merge_to_the_same_bits(cuda, built_lib, name):
    """a plane whose two y-bins hold 10 000 records: three parts per tile at 4096 records per part, one at 12288 (streaming
    launch; the queue launch splits by arc steps either way).  At -inf every item of the launch is on the peaks launch's list -
    more items than it has workgroups, so a workgroup takes several, split ones among them"""
    c, ref = check_case(name)
    th = THRESH[name]
    ybin = np.floor((c["pts"][:, 1] - c["pts"][:, 1].min()) / RES).astype(int)
    assert np.bincount(ybin).max() > 2 * 4096
    full, mn = vote(cuda, c)
    want = None
    for part_records in (4096, 12288):
        assert all(torch.equal(u, v) for u, v in zip(full, vote(cuda, c, part_records=part_records)[0]))
        everywhere, _ = vote(cuda, c, thresh=float("-inf"), part_records=part_records)
        assert all(torch.equal(u, v) for u, v in zip(full, everywhere)), "part_records %d, thresh -inf" % part_records
        peaks, _ = vote(cuda, c, thresh=th, part_records=part_records)
        hot = assert_peaks_equal_full(full, peaks, th, "part_records %d" % part_records)
        assert hot > 0
        assert_same_decode(decode_of(cuda, c, full, mn, th), decode_of(cuda, c, peaks, mn, th), "part_records %d" % part_records)
        hot_cells = full[0] >= th
        got = (peaks[1][hot_cells].clone(), peaks[2][hot_cells].clone())
        if want is not None:
            assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        want = got
    # the same launches again on the same workspace: the arrival counters of the split planes were left as a call expects them
    peaks, _ = vote(cuda, c, thresh=th, part_records=4096)
    assert_peaks_equal_full(full, peaks, th, "second call")


def test_hot_cells_on_tile_borders_and_the_last_row_and_column(cuda, built_lib):
    c, ref = check_case("border")
    th = THRESH["border"]
    X, Y, Z = ref.shape
    assert (X, Y, Z) == tuple(h + 1 for h in BORDER_HI)
    # the oracle confirms where the clusters landed: both sides of an x and of a z tile border, the last row, the last column
    for cell in ((15, 1, 10), (16, 1, 10), (24, 2, 31), (24, 2, 32), (39, 1, 50), (X - 1, 1, 50), (20, 2, 69), (20, 2, Z - 1)):
        assert ref[cell] >= 1.5 * th, (cell, ref[cell])
    assert 15 % TX == TX - 1 and 32 % TZ == 0
    full, mn = vote(cuda, c)
    peaks, _ = vote(cuda, c, thresh=th)
    assert assert_peaks_equal_full(full, peaks, th, "border") == int((ref >= th).sum())
    assert_same_decode(decode_of(cuda, c, full, mn, th), decode_of(cuda, c, peaks, mn, th), "border")


def test_two_categories_equal_two_single_calls(cuda, built_lib):
    c, ref = check_case("stream")
    th = THRESH["stream"]
    # category 1: the same rings (xyz * scale unchanged) with 0.7 of the weight and other scales - fewer hot cells, other quotients
    s1 = (c["scale"] * np.float32(1.25)).astype(np.float32)
    x1 = (c["xyz"] * c["scale"] / s1).astype(np.float32)
    p1 = (c["prob"] * np.float32(0.7)).astype(np.float32)
    hot1 = int((oracle.hv_forward(c["pts"], x1, s1, p1, c["res"], c["R"])[0] >= th).sum())
    assert 0 < hot1 < int((ref >= th).sum())
    cats = [(c["xyz"], c["scale"], c["prob"]), (x1, s1, p1)]
    both, _ = vote(cuda, c, thresh=th, cats=cats)
    full2, _ = vote(cuda, c, cats=cats)
    counts = []
    for k, (xyz, scale, prob) in enumerate(cats):
        ck = dict(c, xyz=xyz, scale=scale, prob=prob)
        full, _ = vote(cuda, ck)
        single, _ = vote(cuda, ck, thresh=th)
        assert all(torch.equal(u[k], v) for u, v in zip(full2, full)), "category %d: full" % k
        counts.append(assert_peaks_equal_full(full, tuple(g[k] for g in both), th, "category %d" % k))
        hot = full[0] >= th
        assert torch.equal(single[1][hot], both[1][k][hot]) and torch.equal(single[2][hot], both[2][k][hot])
    assert counts[0] > counts[1] > 0


def _resident(case, cuda):
    sc = make_scene(case, n_points=3000, res=0.06, room=(2.0, 1.0, 2.0), n_boxes=3, margin=0.6, box_scale=0.5)
    c4 = torch.cat([torch.zeros((3000, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(cuda)
    feats = (_t(cuda, sc.feats) * 2 - 1).contiguous()
    pts = (c4[:, 1:] * sc.res).float().contiguous()
    xyz, scale, prob, cls = [_t(cuda, a) for a in synth_predictions(sc)]
    return sc, c4, feats, pts, (xyz, scale, prob, cls.int())


@pytest.mark.parametrize("in_flight", [None, 7])
def test_scene_call_without_keep_equals_the_call_with_keep(cuda, built_lib, in_flight):
    """detect_scene_c without ``keep`` takes the peaks vote (cv_scene_desc.peak_quotients), with ``keep`` the full one: the same
    detections, raw decode and network output, under both launch sizings; two scenes with different hot cells one after the other
    on the same workspace, so that a hot box left over from the previous scene would show"""
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(cuda).eval()
    policy = None if in_flight is None else pipeline.policy_for_scenes_in_flight(in_flight)
    scenes = [_resident(seed, cuda) for seed in (1, 2)]
    hv = HoughVoting(scenes[0][0].res, 120)
    want = []
    for sc, c4, feats, pts, teacher in scenes:
        keep = {}
        want.append(pipeline.detect_scene_c(model, hv, c4, feats, sc.res, scan_points=pts, predictions=teacher, keep=keep,
                                            thresh_high=20, policy=policy))
        assert "grids" in keep and not torch.isnan(keep["grids"][1]).any()
    assert not np.array_equal(want[0][1]["cand_idx"], want[1][1]["cand_idx"])
    assert all(len(w[1]["boxes"]) >= 2 and len(w[1]["cand_idx"]) > len(w[1]["boxes"]) for w in want)
    for rep in range(2):
        for (sc, c4, feats, pts, teacher), (dets0, raw0, y0) in zip(scenes, want):
            dets, raw, y = pipeline.detect_scene_c(model, hv, c4, feats, sc.res, scan_points=pts, predictions=teacher,
                                                   thresh_high=20, policy=policy)
            assert torch.equal(y, y0)
            assert_same_decode(raw0, raw, "scene %d, pass %d" % (sc.seed, rep))
            assert len(dets) == len(dets0) > 0
            for (c0, b0, s0), (c1, b1, s1) in zip(dets0, dets):
                assert c0 == c1 and s0 == s1 and np.array_equal(b0, b1)
