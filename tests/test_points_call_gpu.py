"""cv_detect_points_f32 / cv_detect_points_separate_f32 - voxelise, gather and detect in ONE C call (pipeline.detect_points_c,
detect_points_separate_c) - against the call-by-call path the parent has: pipeline.detect_points (ME.utils.quantize_device
+ torch gathers + detect_scene_c) and quantize_device + torch gathers + detect_scene_separate_c.  The same kernels in the
same order on the same arrays, so every comparison is exact (bytes or integers), and the expected side never runs the code
under test.

The cloud is the 3k scene of tests/test_scene_call_gpu.py before the unique step: 6000 raw samples, 3 746 voxels at
res = 0.06 (up to 8 points per voxel), a 35 x 18 x 35 grid, 27 candidates and 3 accepted boxes from teacher predictions."""
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.me import utils as me_utils
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_raw_scene, synth_predictions

pytestmark = pytest.mark.gpu

RES, THRESH, M = 0.06, 20, 6000
SMALL = dict(room=(2.0, 1.0, 2.0), n_boxes=3, margin=0.6, box_scale=0.5)
K = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cloud(seed, cuda, dtype=torch.float64):
    """(points [M, 3], feats in [0, 1], recentred feats, teacher predictions) of a small raw scene, on the device"""
    raw = make_raw_scene(seed, M, **SMALL)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    feats01 = t(raw.feats)
    teacher = tuple(t(a) for a in synth_predictions(raw))
    return t(raw.points).to(dtype), feats01, (feats01 * 2 - 1).contiguous(), teacher


@pytest.fixture(scope="module")
def model(cuda, built_lib):
    torch.manual_seed(0)
    return MinkUNet34C(3, 64).to(cuda).eval()


@pytest.fixture(scope="module")
def reference(cuda, model):
    """detect_points on the seed-1 cloud, per (dtype, predictions): computed once, never modified"""
    hv = HoughVoting(RES, 120)
    out = {}
    for dtype in (torch.float32, torch.float64):
        pts, _, feats, teacher = cloud(1, cuda, dtype)
        for pred, tag in ((teacher, "teacher"), (None, "network")):
            keep = {}
            dets, raw, y, index, inverse = pipeline.detect_points(model, hv, pts, feats, RES, predictions=pred, return_inverse=True,
                                                                  keep=keep, thresh_high=THRESH)
            out[dtype, tag] = dict(dets=dets, raw=raw, y=y, index=index, inverse=inverse, keep=keep)
    return out


def assert_same(want, got, keep, tag):
    dets, raw, y, index = got[:4]
    assert torch.equal(want["index"], index) and index.dtype == torch.int32, tag + ": index"
    if len(got) > 4:
        assert torch.equal(want["inverse"], got[4]), tag + ": inverse"
    assert y.shape == want["y"].shape and torch.equal(want["y"], y), tag + ": network output"
    for k in ("cand_idx", "verdict", "boxes", "scores", "classes"):
        assert want["raw"][k].tobytes() == raw[k].tobytes(), tag + ": " + k
    assert len(want["dets"]) == len(dets), tag + ": detection count"
    for (c0, b0, s0), (c1, b1, s1) in zip(want["dets"], dets):
        assert c0 == c1 and s0 == s1 and b0.tobytes() == b1.tobytes(), tag + ": detections"
    if keep is not None:
        wk = want["keep"]
        assert wk["dims"] == keep["dims"] and wk["corner"] == keep["corner"] and wk["level_rows"] == keep["level_rows"], tag
        for u, v, name in zip(wk["grids"], keep["grids"], ("obj", "rot", "scale")):
            assert u.shape == v.shape and torch.equal(u, v), tag + ": grid_" + name
        for u, v, name in zip(wk["net_pred"], keep["net_pred"], ("xyz", "scale", "prob", "class")):
            assert torch.equal(u, v), tag + ": head " + name


@pytest.mark.parametrize("tag", ["teacher", "network"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_call_equals_call_by_call(cuda, model, reference, dtype, tag):
    want = reference[dtype, tag]
    pts, _, feats, teacher = cloud(1, cuda, dtype)
    hv = HoughVoting(RES, 120)
    for rep in range(2):                # the second call runs on the grown scratch
        keep = {}
        got = pipeline.detect_points_c(model, hv, pts, feats, RES, predictions=teacher if tag == "teacher" else None,
                                       return_inverse=True, keep=keep, thresh_high=THRESH)
        assert_same(want, got, keep, "%s predictions, %s, call %d" % (tag, dtype, rep))
        n = got[3].shape[0]
        assert torch.equal(keep["scan_points"], (me_utils.quantize_device(pts, RES)[0][:, 1:] * RES).float())
        assert torch.equal(keep["feats"], feats[got[3].long()]) and keep["front_ws_bytes"] > 0 and keep["host_us_front"] > 0
    assert 3000 < n < M and int(torch.bincount(want["inverse"].long()).max()) > 1     # several points per voxel
    if tag == "teacher":                # the comparison saw accepted boxes and rejected candidates
        assert len(want["raw"]["boxes"]) >= 2
        assert len(want["raw"]["cand_idx"]) > len(want["raw"]["boxes"])
    assert len(pipeline.detect_points_c(model, hv, pts, feats, RES, thresh_high=THRESH)) == 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_strided_points(cuda, model, reference, dtype):
    pts, _, feats, teacher = cloud(1, cuda, dtype)
    wide = torch.full((M, 4), 7.0, dtype=dtype, device=cuda)
    wide[:, 0:3] = pts
    view = wide[:, 0:3]
    assert not view.is_contiguous()
    got = pipeline.detect_points_c(model, HoughVoting(RES, 120), view, feats, RES, predictions=teacher, return_inverse=True,
                                   thresh_high=THRESH)
    assert_same(reference[dtype, "teacher"], got, None, "row-strided points")
    # strided feature rows: a column block of a wider tensor
    fwide = torch.full((M, 5), 9.0, device=cuda)
    fwide[:, 1:4] = feats
    got = pipeline.detect_points_c(model, HoughVoting(RES, 120), pts, fwide[:, 1:4], RES, predictions=teacher, return_inverse=True,
                                   thresh_high=THRESH)
    assert_same(reference[dtype, "teacher"], got, None, "row-strided features")


def test_recentre_from_zero_on_features_in_the_unit_interval(cuda, model, reference):
    pts, feats01, feats, teacher = cloud(1, cuda, torch.float64)
    assert float(feats01.min()) >= 0 and float(feats01.max()) <= 1 and not torch.equal(feats01, feats)
    keep = {}
    got = pipeline.detect_points_c(model, HoughVoting(RES, 120), pts, feats01, RES, predictions=teacher, return_inverse=True,
                                   recentre_from=0, keep=keep, thresh_high=THRESH)
    assert_same(reference[torch.float64, "teacher"], got, keep, "recentre_from=0")
    assert torch.equal(keep["feats"], feats[got[3].long()])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_capacity_edge_one_point_per_voxel(cuda, model, dtype):
    """the voxel centres of the cloud: N == M, the output buffer is used to its last row"""
    pts, _, feats, teacher = cloud(1, cuda, torch.float64)
    c4, index, _ = me_utils.quantize_device(pts, RES)
    gi = index.long()
    centres = ((c4[:, 1:].double() + 0.5) * RES).to(dtype)
    f, pred = feats[gi].contiguous(), tuple(p[gi].contiguous() for p in teacher)
    m = centres.shape[0]
    hv = HoughVoting(RES, 120)
    wd, wr, wy, wi, winv = pipeline.detect_points(model, hv, centres, f, RES, predictions=pred, return_inverse=True, thresh_high=THRESH)
    got = pipeline.detect_points_c(model, hv, centres, f, RES, predictions=pred, return_inverse=True, thresh_high=THRESH)
    assert_same(dict(dets=wd, raw=wr, y=wy, index=wi, inverse=winv), got, None, "one point per voxel")
    assert got[2].shape[0] == m and torch.equal(got[3], torch.arange(m, dtype=torch.int32, device=cuda))
    assert len(wr["boxes"]) >= 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rejected_points_raise_and_leave_the_stream_usable(cuda, model, reference, dtype):
    pts, _, feats, teacher = cloud(1, cuda, dtype)
    bad = pts.clone()
    bad[10, 1] = float("nan")
    bad[700, 0] = float("inf")
    bad[M - 1, 2] = 40000 * RES
    hv = HoughVoting(RES, 120)
    with pytest.raises(RuntimeError, match=r"\b3 points rejected"):
        pipeline.detect_points_c(model, hv, bad, feats, RES, predictions=teacher, thresh_high=THRESH)
    got = pipeline.detect_points_c(model, hv, pts, feats, RES, predictions=teacher, return_inverse=True, thresh_high=THRESH)
    assert_same(reference[dtype, "teacher"], got, None, "after a rejected cloud")


def test_truncated_scene_returns_the_call_by_call_result(cuda, model, reference):
    want = reference[torch.float64, "teacher"]
    assert len(want["raw"]["cand_idx"]) > 4          # the capacity below really truncates the walk
    pts, _, feats, teacher = cloud(1, cuda, torch.float64)
    torch.cuda.synchronize()
    side, keep = torch.cuda.Stream(cuda), {}
    with torch.cuda.stream(side):       # (a stream of its own: the result arrays of a stream only grow, here they hold 4)
        got = pipeline.detect_points_c(model, HoughVoting(RES, 120), pts, feats, RES, predictions=teacher, return_inverse=True,
                                       max_candidates=4, keep=keep, thresh_high=THRESH)
        side.synchronize()
    _lib.release_scratch(cuda, side)
    assert "host_us_front" not in keep          # the scene was redone: the one-call path did not deliver this result
    assert_same(want, got, None, "truncated scene")


def test_two_host_threads_on_two_streams(cuda, model):
    work = [cloud(seed, cuda) for seed in (1, 2)]
    run = lambda w: pipeline.detect_points_c(model, HoughVoting(RES, 120), w[0], w[2], RES, predictions=w[3], return_inverse=True,
                                             thresh_high=THRESH)
    alone = [run(w) for w in work]
    torch.cuda.synchronize()
    assert not torch.equal(alone[0][3], alone[1][3])
    out, errors, start = [[None] * 4 for _ in work], [], threading.Barrier(2)

    def worker(i):
        try:
            torch.cuda.set_device(cuda)
            s = torch.cuda.Stream(cuda)
            with torch.cuda.stream(s):
                start.wait()
                for rep in range(4):
                    out[i][rep] = run(work[i])
            s.synchronize()
        except BaseException as e:      # noqa: BLE001
            errors.append(repr(e))
            start.abort()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:2]
    for i in range(2):
        a = alone[i]
        want = dict(dets=a[0], raw=a[1], y=a[2], index=a[3], inverse=a[4])
        for rep in range(4):
            assert_same(want, out[i][rep], None, "thread %d call %d" % (i, rep))


def test_five_events_are_recorded_in_order(cuda, model):
    pts, _, feats, teacher = cloud(1, cuda)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    pipeline.detect_points_c(model, HoughVoting(RES, 120), pts, feats, RES, predictions=teacher, events=ev, thresh_high=THRESH)
    torch.cuda.synchronize()
    times = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
    assert all(t > 0 for t in times), times


# ---- separate mode ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def separate_models(cuda, built_lib):
    out = {}
    for c in range(K):
        torch.manual_seed(100 + c)
        out[c] = MinkUNet34C(3, 8).to(cuda).eval()
    return out


def separate_teacher(seed, cuda):
    raw = make_raw_scene(seed, M, **SMALL)
    xyz, scale, prob, cls = synth_predictions(raw)
    rng = np.random.default_rng(seed)
    P = np.stack([np.where(cls == c, prob, rng.uniform(1e-3, 0.1, M)) for c in range(K)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)
    return t(np.stack([xyz] * K)), t(np.stack([scale] * K)), t(P)


@pytest.mark.parametrize("tag", ["teacher", "network"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_separate_mode_equals_quantise_gather_and_the_separate_scene_call(cuda, separate_models, dtype, tag):
    pts, _, feats, _ = cloud(1, cuda, dtype)
    teacher = separate_teacher(1, cuda) if tag == "teacher" else None
    hv = HoughVoting(RES, 120)
    # the parent's path: voxelise, gather with torch, one separate scene call
    c4, index, inverse = me_utils.quantize_device(pts, RES, None, True)
    gi = index.long()
    pred = None if teacher is None else tuple(p[:, gi].contiguous() for p in teacher)
    wkeep = {}
    want = pipeline.detect_scene_separate_c(separate_models, hv, c4, feats[gi], RES, predictions=pred, keep=wkeep, thresh_high=THRESH)
    if teacher is not None:
        assert sum(len(r["boxes"]) for r in wkeep["raw"]) >= 2
    for G in (0, 3):
        keep = {}
        dets, gindex, ginverse = pipeline.detect_points_separate_c(separate_models, hv, pts, feats, RES, predictions=teacher,
                                                                   models_per_pass=G, return_inverse=True, keep=keep,
                                                                   thresh_high=THRESH)
        tag2 = "%s predictions, %s, models_per_pass %d" % (tag, dtype, G)
        assert torch.equal(index, gindex) and torch.equal(inverse, ginverse) and torch.equal(c4, keep["coords4"]), tag2
        assert wkeep["dims"] == keep["dims"] and wkeep["corner"] == keep["corner"], tag2
        for k in range(K):
            assert torch.equal(wkeep["y"][k], keep["y"][k]), "%s: network output of model %d" % (tag2, k)
            for j, name in enumerate(("xyz", "scale", "prob")):
                assert torch.equal(wkeep["net_pred"][j][k], keep["net_pred"][j][k]), "%s: head %s of model %d" % (tag2, name, k)
            for j, name in enumerate(("obj", "rot", "scale")):
                assert torch.equal(wkeep["grids"][j][k], keep["grids"][j][k]), "%s: grid_%s of category %d" % (tag2, name, k)
            for f in ("cand_idx", "verdict", "boxes", "scores"):
                assert wkeep["raw"][k][f].tobytes() == keep["raw"][k][f].tobytes(), "%s: %s of category %d" % (tag2, f, k)
        assert len(want) == len(dets), tag2
        for (c0, b0, s0), (c1, b1, s1) in zip(want, dets):
            assert c0 == c1 and s0 == s1 and b0.tobytes() == b1.tobytes(), tag2 + ": detections"


# ---- the eval script --------------------------------------------------------------------------------------------------------------

def test_eval_script_raw_clouds_give_the_detections_of_detect_points(cuda, model):
    spec = importlib.util.spec_from_file_location("cv_eval_joint", os.path.join(ROOT, "scripts", "eval_joint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = {}
    res = mod.evaluate_raw(model, 2, M, seed0=300, res=RES, teacher=True, device=cuda, detections=got, thresh_high=THRESH, **SMALL)
    assert set(res) == {0.25, 0.5} and sorted(got) == ["synth0300", "synth0301"]
    hv = HoughVoting(RES)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    total = 0
    for i in range(2):
        raw = make_raw_scene(300 + i, M, **SMALL)
        want = pipeline.detect_points(model, hv, t(raw.points), t(raw.feats) * 2.0 - 1.0, RES,
                                      predictions=tuple(t(a) for a in synth_predictions(raw)), thresh_high=THRESH)[0]
        dets = got["synth%04d" % (300 + i)]
        assert len(want) == len(dets)
        for (c0, b0, s0), (c1, b1, s1) in zip(want, dets):
            assert c0 == c1 and s0 == s1 and b0.tobytes() == b1.tobytes()
        total += len(want)
    assert total >= 2
