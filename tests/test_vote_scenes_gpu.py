"""cv_hv_forward_scenes_f32 / cv_hv_forward_peaks_scenes_f32 - B scenes' votes in one launch sequence - on the two batches of
tests/test_vote_scenes.py (their geometry is asserted there, without a GPU).  Everything is an EQUALITY on every 32-bit word:
a job's three grids against the integer restatement hv_numpy.hv_forward_fixed (tests/test_vote_exact_gpu.py: inputs, fixed,
assert_tile_bits) and against the single call on the same rows.

  batch A   res 0.03: three tiles / one plane in three parts / queue launch with work lists / 302 points
  batch B   res 1: 4097 planes (no LDS histogram) / streaming / queue / queue whose lists overflow, hot pairs in parts

The jobs are stored in another order than the job order, with gaps of heavy points between them that no job owns, and one job
starts at row 1.  The workspace is exactly the reported size, filled with a byte pattern (not zeroed), with 64 KB of sentinel
behind it; the B grid triples are carved from ONE buffer with 64 pattern floats around each, rot / scale pre-filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, decode, hv_cuda, pipeline
from tests import test_scene_batch_gpu as sb
from tests import test_vote_exact_gpu as ex
from tests import test_vote_fallbacks_gpu as fb
from tests import test_vote_scenes as vs

pytestmark = pytest.mark.gpu
GAP = 64          # pattern floats in front of, between and behind the grids
PATTERN_F = float(np.full(4, fb.PATTERN, np.uint8).view(np.float32)[0])


def upload(cuda, b):
    return [torch.from_numpy(b[k].copy()).to(cuda) for k in ("pts", "xyz", "scale", "prob")]          # (the batch's arrays are read-only)


def carve_grids(cuda, b):
    """one pattern-filled buffer; per job (obj, rot, scale) views with rot / scale set to NaN, and the mask of the gap floats
    (a grid of an odd number of cells is followed by one more gap float: grid_rot is an array of float pairs)"""
    cells = [int(np.prod(j[3])) for j in b["jobs"]]
    buf = torch.full((sum(6 * c + (c & 1) + GAP for c in cells) + GAP,), PATTERN_F, dtype=torch.float32, device=cuda)
    is_gap = torch.ones(buf.numel(), dtype=torch.bool, device=cuda)
    views, at = [], GAP
    for c, (_, _, _, dims) in zip(cells, b["jobs"]):
        r0 = at + c + (c & 1)
        obj, rot, scale = buf[at:at + c], buf[r0:r0 + 2 * c], buf[r0 + 2 * c:r0 + 5 * c]
        rot.fill_(float("nan"))
        scale.fill_(float("nan"))
        is_gap[at:at + c] = False
        is_gap[r0:r0 + 5 * c] = False
        views.append([obj.view(*dims), rot.view(*dims, 2), scale.view(*dims, 3)])
        at = r0 + 5 * c + GAP
    return buf, is_gap, views


def carve_offsets(b, order, algo=0):
    """byte offset of each listed job's workspace carve (job order of the call) and the total: the single sizes, summed"""
    sizes = [vs.single_bytes(b, k, algo) for k in order]
    return [vs.HEAD + sum(sizes[:i]) for i in range(len(order))], vs.HEAD + sum(sizes)


def vote_scenes(cuda, b, order=None, thresh=None, ws=None, algo=0, dev=None):
    """the scene call over the jobs `order` (default: all, in job order) -> ({job: [obj, rot, scale]}, workspace, its size)"""
    L = _lib.lib()
    order = list(range(len(b["jobs"]))) if order is None else order
    p, x, s, o = dev or upload(cuda, b)
    buf, is_gap, views = carve_grids(cuda, b)
    jobs = vs.job_table(b, [[g.data_ptr() for g in v] for v in views], order)
    size = L.cv_hv_forward_scenes_workspace_bytes(jobs, len(order), b["R"], algo)
    assert size == carve_offsets(b, order, algo)[1] > 0
    ws = fb.pattern_workspace(cuda, size) if ws is None else ws
    head = [jobs, len(order), hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), ctypes.c_float(b["res"]), b["R"],
            hv_cuda._ptr(ws), size, algo]
    with torch.cuda.device(cuda):
        if thresh is None:
            _lib.check(L.cv_hv_forward_scenes_f32(*head, hv_cuda._stream(cuda)), "cv_hv_forward_scenes_f32")
        else:
            _lib.check(L.cv_hv_forward_peaks_scenes_f32(*head, ctypes.c_float(thresh), hv_cuda._stream(cuda)),
                       "cv_hv_forward_peaks_scenes_f32")
    torch.cuda.synchronize()
    fb.assert_tail_untouched(ws, size, "scenes")
    assert bool((buf[is_gap].view(torch.int32) == fb.PATTERN_WORD).all()), "the floats around the grids were written"
    return {k: views[k] for k in order}, ws, size


def vote_alone(cuda, b, k, thresh=None, algo=0, dev=None):
    """the single call on job k's rows, corner and shape; rot / scale pre-filled with NaN"""
    L = _lib.lib()
    row0, n, corner, dims = b["jobs"][k]
    p, x, s, o = [t[row0:row0 + n] for t in (dev or upload(cuda, b))]
    cdims = (ctypes.c_int * 3)(*dims)
    size = L.cv_hv_forward_workspace_bytes(n, b["R"], cdims, algo)
    ws = fb.pattern_workspace(cuda, size)
    grids = [torch.full(tuple(dims) + tail, float("nan"), dtype=torch.float32, device=cuda) for tail in ((), (2,), (3,))]
    head = [hv_cuda._ptr(p), hv_cuda._ptr(x), hv_cuda._ptr(s), hv_cuda._ptr(o), n, ctypes.c_float(b["res"]), b["R"],
            hv_cuda._f3(corner), cdims] + [hv_cuda._ptr(g) for g in grids] + [hv_cuda._ptr(ws), size, algo]
    with torch.cuda.device(cuda):
        if thresh is None:
            _lib.check(L.cv_hv_forward_f32(*head, hv_cuda._stream(cuda)), "cv_hv_forward_f32")
        else:
            _lib.check(L.cv_hv_forward_peaks_f32(*head, ctypes.c_float(thresh), hv_cuda._stream(cuda)), "cv_hv_forward_peaks_f32")
    torch.cuda.synchronize()
    return grids


def same_words(a, b):
    """equality of every 32-bit word (NaN pre-fills included)"""
    return all(torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)) for u, v in zip(a, b))


def assert_launches(b, ws, order, fresh=True):
    """list_ctl of every job's carve, read at the carve's offset, says which launch the job took (the streaming launch leaves
    the words alone: on a workspace that was used before, `fresh` False, they say nothing)"""
    offs, _ = carve_offsets(b, order)
    for off, k in zip(offs, order):
        key = b["keys"][k]
        if not fresh and vs.LAUNCH[key] == "stream":
            continue
        _, n, _, dims = b["jobs"][k]
        words = fb.list_ctl_words(ws, n, off, 1)
        fb.assert_launch(words, vs.LAUNCH[key], dict(pts=np.empty((n, 3)), dims=dims), key)


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_job_is_the_restatement_and_the_single_call(cuda, built_lib, name):
    b = vs.batch(name)
    dev = upload(cuda, b)
    got, ws, _ = vote_scenes(cuda, b, dev=dev)
    assert_launches(b, ws, list(range(len(b["keys"]))))
    for k, key in enumerate(b["keys"]):
        want = ex.assert_tile_bits(got[k], key, "batch %s, job %d (%s)" % (name, k, key))
        assert want[0].any()
        assert same_words(got[k], vote_alone(cuda, b, k, dev=dev)), "batch %s, job %d (%s): not the single call's bits" % (name, k, key)


def peaks_thresh(b):
    """one threshold for the batch, from the restatement: half of the smallest of the jobs' maxima - every job has a cell at or
    above it and a touched cell below it (asserted)"""
    th = float(np.float32(0.5 * min(float(ex.fixed(key)[0].max()) for key in b["keys"])))
    for key in b["keys"]:
        obj = ex.fixed(key)[0]
        assert (obj >= th).any() and ((obj > 0) & (obj < th)).any(), (key, th)
    return th


@pytest.mark.parametrize("name", ["A", "B"])
def test_peaks_form_writes_the_quotients_at_the_cells_that_reach_the_threshold(cuda, built_lib, name):
    b = vs.batch(name)
    th = peaks_thresh(b)
    dev = upload(cuda, b)
    got, ws, _ = vote_scenes(cuda, b, thresh=th, dev=dev)
    assert_launches(b, ws, list(range(len(b["keys"]))))
    for k, key in enumerate(b["keys"]):
        tag = "batch %s peaks, job %d (%s)" % (name, k, key)
        want = ex.assert_tile_bits(got[k], key, tag, thresh=th)
        hot = torch.from_numpy(want[3].copy()).to(cuda)          # (the restatement is read-only)
        assert 0 < int(hot.sum()) < hot.numel()
        # the pre-fill survives at every other cell, as for the single peaks call - whose words these are
        assert bool(torch.isnan(got[k][1][~hot]).all()) and bool(torch.isnan(got[k][2][~hot]).all()), tag
        assert not bool(torch.isnan(got[k][1][hot]).any()) and not bool(torch.isnan(got[k][2][hot]).any()), tag
        assert same_words(got[k], vote_alone(cuda, b, k, thresh=th, dev=dev)), tag + ": not the single peaks call's bits"


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_second_call_with_the_jobs_permuted_finds_stale_state_and_gives_the_same_bits(cuda, built_lib, name):
    """the carves move onto each other's leftovers: every word a kernel relies on being zero is zeroed by the call"""
    b = vs.batch(name)
    dev = upload(cuda, b)
    first, ws, size = vote_scenes(cuda, b, dev=dev)
    first = {k: [g.clone() for g in v] for k, v in first.items()}
    order = [2, 3, 1, 0]
    assert carve_offsets(b, order)[0][1:] != carve_offsets(b, [0, 1, 2, 3])[0][1:]
    again, ws2, size2 = vote_scenes(cuda, b, order=order, ws=ws, dev=dev)
    assert size2 == size and ws2 is ws
    assert_launches(b, ws, order, fresh=False)
    for k, key in enumerate(b["keys"]):
        assert same_words(first[k], again[k]), "batch %s, job %d (%s): the second call differs" % (name, k, key)
    # the peaks form on the same leftovers
    th = peaks_thresh(b)
    peaks, _, _ = vote_scenes(cuda, b, order=[1, 0, 3, 2], thresh=th, ws=ws, dev=dev)
    for k, key in enumerate(b["keys"]):
        ex.assert_tile_bits(peaks[k], key, "batch %s peaks on a used workspace, job %d" % (name, k), thresh=th)


def test_twins_one_scene_and_sixteen_scenes(cuda, built_lib):
    a = vs.batch("A")
    # the same scene in slots 0 and 3
    twins = vs.batch("twins", ("dense:inside", "dense:corner", "dense:parts", "dense:inside"))
    got, _, _ = vote_scenes(cuda, twins)
    assert twins["jobs"][0][0] != twins["jobs"][3][0]
    assert same_words(got[0], got[3])
    for k, key in enumerate(twins["keys"]):
        ex.assert_tile_bits(got[k], key, "twins, job %d" % k)
    # B = 1 is the single call: the same bits, and the workspace of the single query
    for k in (1, 2):
        one, _, size = vote_scenes(cuda, a, order=[k])
        assert size == vs.single_bytes(a, k)
        assert same_words(one[k], vote_alone(cuda, a, k))
        ex.assert_tile_bits(one[k], a["keys"][k], "B = 1, job %d" % k)
    # B = 16
    many = vs.batch("sixteen", ("dense:corner",) * 16)
    got, _, _ = vote_scenes(cuda, many)
    for k in range(16):
        ex.assert_tile_bits(got[k], "dense:corner", "B = 16, job %d" % k)


def test_more_than_256_rotations_run_the_direct_kernel_job_after_job(cuda, built_lib):
    keys = ("dense:r7*r257", "small3*r257", "small0*r257")
    b = vs.batch("r257", keys)
    assert b["R"] == fb.MAX_R_TILES + 1
    got, ws, size = vote_scenes(cuda, b)
    assert size == 256 * len(keys) and bool((ws == fb.PATTERN).all())          # the direct kernel's workspace, untouched
    for k, key in enumerate(keys):
        assert (ex.inputs(key)[3] >= 0).all()
        ex.assert_direct_within_bounds(got[k], key, "R 257, job %d (%s)" % (k, key))


def test_python_wrapper_equals_forward_on_the_slices_and_feeds_the_scene_decode(cuda, built_lib):
    b = vs.batch("A")
    p, x, s, o = upload(cuda, b)
    ranges = [(r, r + n) for r, n, _, _ in b["jobs"]]
    res, R = b["res"], b["R"]
    got = hv_cuda.forward_scenes(p, x, s, o, ranges, res, R)
    alone = [hv_cuda.forward(p[a:e], x[a:e], s[a:e], o[a:e], torch.tensor(res, device=cuda), torch.tensor(R, device=cuda))
             for a, e in ranges]
    torch.cuda.synchronize()
    for k, key in enumerate(b["keys"]):
        assert same_words(got[k], alone[k]), key
        assert hv_cuda.recent_corner(got[k][0]) == hv_cuda.recent_corner(alone[k][0]) == [float(v) for v in b["jobs"][k][2]]
        ex.assert_tile_bits(got[k], key, "forward_scenes, job %d" % k)
    # the 7-argument form: a box of its own per scene, cutting the cloud
    boxes = []
    for (_, _, corner, dims) in b["jobs"]:
        lo = corner + np.float32(res) * np.float32([1.25, 0.5, 2.0])
        hi = corner + np.float32(res) * (np.asarray(dims, np.float32) - np.float32([3.5, 1.25, 2.75]))
        boxes.append(torch.from_numpy(np.stack([lo, hi]).astype(np.float32)).to(cuda))
    got_c = hv_cuda.forward_scenes(p, x, s, o, ranges, res, R, corners=boxes)
    for k, ((a, e), box) in enumerate(zip(ranges, boxes)):
        one = hv_cuda.forward(p[a:e], x[a:e], s[a:e], o[a:e], torch.tensor(res, device=cuda), torch.tensor(R, device=cuda), box)
        assert one[0].shape != alone[k][0].shape and float(one[0].max()) > 0
        assert same_words(got_c[k], one), "corners, job %d" % k
    # thresh selects the peaks entry point
    th = peaks_thresh(b)
    for k, tri in enumerate(hv_cuda.forward_scenes(p, x, s, o, ranges, res, R, thresh=th)):
        hot = got[k][0] >= th
        assert torch.equal(tri[0], got[k][0]) and torch.equal(tri[1][hot], got[k][1][hot]) and torch.equal(tri[2][hot], got[k][2][hot])
    # the result goes to the scene decode as it is: the origins travel on the grids
    cls = torch.zeros(len(b["pts"]), dtype=torch.int32, device=cuda)
    args = (ranges, p, x, o, cls, res)
    with_corners = decode.decode_boxes_scenes(got, [j[2] for j in b["jobs"]], *args, thresh_high=th)
    without = decode.decode_boxes_scenes(got, None, *args, thresh_high=th)
    assert sum(len(d["cand_idx"]) for d in without) >= len(b["keys"])
    for d0, d1 in zip(with_corners, without):
        for key in sb.RAW_KEYS:
            assert d0[key].tobytes() == d1[key].tobytes(), key
    # input checks
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        hv_cuda.forward_scenes(p.cpu(), x, s, o, ranges, res, R)
    with pytest.raises(RuntimeError, match="row range 1"):
        hv_cuda.forward_scenes(p, x, s, o, [ranges[0], (5, len(b["pts"]) + 1)], res, R)
    with pytest.raises(RuntimeError, match="zero points"):
        hv_cuda.forward_scenes(p, x, s, o, [ranges[0], (7, 7)], res, R)


@pytest.fixture(scope="module")
def world(cuda, built_lib):
    return sb.World(cuda)


@pytest.mark.parametrize("peak_quotients", [False, True])
def test_scene_call_on_three_unequal_rooms_equals_each_scan_alone(world, peak_quotients):
    """pipeline.detect_scenes_c with teacher predictions.  The call votes the rot / scale quotients at the decode's cells only
    (cv_scene_desc.peak_quotients) exactly when the caller does not ask for the grids: off - with ``keep`` - the three grids and
    the detections are compared, on - without it - the detections"""
    if not peak_quotients:
        got = world.batch(True)
        for b in range(len(sb.ROOMS)):
            one = world.alone(b, True)
            sb.same_keep(got["keep"][b], one["keep"], "scene %d" % b, net=False)
            assert float(got["keep"][b]["grids"][0].max()) > sb.THRESH
            sb.same_decode(got["out"][b][1], got["out"][b][0], one["raw"], one["dets"], "scene %d" % b)
        return
    out, _ = pipeline.detect_scenes_c(world.model, world.hv, world.c4, world.feats, sb.RES, len(sb.ROOMS), scan_points=world.pts,
                                      predictions=world.teacher, thresh_high=sb.THRESH)
    for b, r in enumerate(world.rooms):
        c4 = r["c4"].clone()
        c4[:, 0] = 0
        dets, raw, _ = pipeline.detect_scene_c(world.model, world.hv, c4, r["feats"], sb.RES, scan_points=r["pts"],
                                               predictions=r["teacher"], thresh_high=sb.THRESH)
        sb.same_decode(out[b][1], out[b][0], raw, dets, "scene %d (peak quotients)" % b)
        full = world.alone(b, True)
        sb.same_decode(out[b][1], out[b][0], full["raw"], full["dets"], "scene %d (peak quotients against full grids)" % b)
        assert len(raw["boxes"]) >= 2
