"""cv_detect_scene_separate_f32 - one C call per separate-mode scene (plan once, K networks, K heads, one vote and one
decode over the category axis, NMS per category) - against the call-by-call path of eval_separate.py
(pipeline.detect_scene_separate and its stages): the same bits for every model's network output, head outputs, the K grids,
the raw decode and the detections."""
import threading

import numpy as np
import pytest
import torch

from canonicalvoting_amd import decode, pipeline
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_scene, synth_predictions

pytestmark = pytest.mark.gpu

K = 9
SEP = dict(separate_variant=True, err_thresh=float(np.float32(0.3)))


def separate_models(cuda, k=K):
    out = {}
    for c in range(k):
        torch.manual_seed(100 + c)
        out[c] = MinkUNet34C(3, 8).to(cuda).eval()
    return out


def resident(seed, n, cuda, small):
    kw = dict(res=0.06, room=(2.0, 1.0, 2.0), n_boxes=3, margin=0.6, box_scale=0.5) if small else {}
    sc = make_scene(seed, n_points=n, **kw)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)
    c4 = torch.cat([torch.zeros((n, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(cuda)
    feats = (t(sc.feats) * 2 - 1).contiguous()
    pts = (c4[:, 1:] * sc.res).float().contiguous()
    xyz, scale, prob, cls = synth_predictions(sc)
    rng = np.random.default_rng(seed)
    P = np.stack([np.where(cls == c, prob, rng.uniform(1e-3, 0.1, n)) for c in range(K)])
    teacher = (t(np.stack([xyz] * K)), t(np.stack([scale] * K)), t(P))
    return sc, c4, feats, pts, teacher


def by_calls(models, hv, c4, feats, pts, res, teacher, thresh_high, policy=None):
    """the stages of detect_scene_separate, one model after another, with everything kept for the comparison"""
    zeros = torch.zeros(pts.shape[0], dtype=torch.int32, device=pts.device)
    out = dict(y=[], pred=[], grids=[], raw=[], dets=[])
    with torch.no_grad(), pipeline.scene_policy(policy):
        x = ME.SparseTensor(feats, c4, device=feats.device)
        for k, (category, model) in enumerate(models.items()):
            y = model(x).F
            pred = pipeline.head_separate(y)
            use = pred if teacher is None else (teacher[0][k], teacher[1][k], teacher[2][k])
            g = hv(pts, use[0].contiguous(), use[1].contiguous(), use[2].contiguous())
            raw = decode.decode_boxes(g[0], g[1], g[2], pts, use[0].contiguous(), use[2].contiguous(), zeros, res,
                                      thresh_high=thresh_high, **SEP)
            out["y"].append(y); out["pred"].append(pred); out["grids"].append(g); out["raw"].append(raw)
            for i in decode.nms(raw["boxes"], raw["scores"], 0.3):
                out["dets"].append((category, raw["boxes"][i], float(raw["scores"][i])))
    return out


def same_dets(a, b, tag):
    assert len(a) == len(b), tag + ": detection count"
    for (c0, b0, s0), (c1, b1, s1) in zip(a, b):
        assert c0 == c1 and s0 == s1 and np.array_equal(b0, b1), tag + ": detections"


def assert_same(want, keep, dets, tag):
    for k in range(len(want["y"])):
        assert torch.equal(want["y"][k], keep["y"][k]), "%s: network output of model %d" % (tag, k)
        for j, name in enumerate(("xyz", "scale", "prob")):
            assert torch.equal(want["pred"][k][j], keep["net_pred"][j][k]), "%s: head %s of model %d" % (tag, name, k)
        for j, name in enumerate(("obj", "rot", "scale")):
            assert torch.equal(want["grids"][k][j], keep["grids"][j][k]), "%s: grid_%s of category %d" % (tag, name, k)
        for f in ("cand_idx", "verdict", "boxes", "scores"):
            assert np.array_equal(want["raw"][k][f], keep["raw"][k][f]), "%s: %s of category %d" % (tag, f, k)
    same_dets(want["dets"], dets, tag)


@pytest.mark.parametrize("in_flight", [None, 7])
@pytest.mark.parametrize("n,small,thresh", [(3000, True, 20), (80000, False, 60)])
def test_separate_scene_call_equals_the_call_by_call_path(cuda, built_lib, n, small, thresh, in_flight):
    models = separate_models(cuda)
    sc, c4, feats, pts, teacher = resident(1, n, cuda, small)
    hv = HoughVoting(sc.res, 120)
    policy = None if in_flight is None else pipeline.policy_for_scenes_in_flight(in_flight)
    for pred, tag in ((teacher, "teacher predictions"), (None, "network predictions")):
        want = by_calls(models, hv, c4, feats, pts, sc.res, pred, thresh, policy)
        for rep in range(2):            # the second call runs on the grown scratch
            keep = {}
            dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, predictions=pred, policy=policy, keep=keep,
                                                    thresh_high=thresh)
            assert_same(want, keep, dets, "%s (%d points, call %d)" % (tag, n, rep))
        if pred is not None:
            assert sum(len(r["boxes"]) for r in want["raw"]) >= 2
    # the public call-by-call function gives the same detections
    same_dets(pipeline.detect_scene_separate(models, hv, c4, feats, sc.res, thresh_high=thresh),
              pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, thresh_high=thresh), "detect_scene_separate")


def test_separate_scene_call_stage_events(cuda, built_lib):
    models = separate_models(cuda, 3)
    sc, c4, feats, pts, teacher = resident(2, 3000, cuda, True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    for e in ev:
        e.record()
    pipeline.detect_scene_separate_c(models, HoughVoting(sc.res, 120), c4, feats, sc.res, events=ev, thresh_high=20)
    torch.cuda.synchronize()
    assert all(ev[i].elapsed_time(ev[i + 1]) >= 0 for i in range(4))


def test_truncated_separate_scene_returns_the_call_by_call_result(cuda, built_lib):
    models = separate_models(cuda)
    sc, c4, feats, pts, teacher = resident(1, 80000, cuda, False)
    hv = HoughVoting(sc.res, 120)
    want = by_calls(models, hv, c4, feats, pts, sc.res, teacher, 60)
    assert max(len(r["cand_idx"]) for r in want["raw"]) > 4       # the capacity below really truncates a walk
    dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, predictions=teacher, max_candidates=4)
    same_dets(want["dets"], dets, "truncated scene")


def test_two_host_threads_run_separate_scenes(cuda, built_lib):
    models = separate_models(cuda)
    work = [resident(3, 3000, cuda, True), resident(4, 80000, cuda, False)]
    hv = [HoughVoting(w[0].res, 120) for w in work]
    thr = [20, 60]
    alone = [pipeline.detect_scene_separate_c(models, hv[i], w[1], w[2], w[0].res, predictions=w[4], thresh_high=thr[i])
             for i, w in enumerate(work)]
    out = [[None] * 3 for _ in work]
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream(cuda)
            w = work[i]
            with torch.cuda.stream(s):
                for rep in range(3):
                    out[i][rep] = pipeline.detect_scene_separate_c(models, hv[i], w[1], w[2], w[0].res, predictions=w[4],
                                                                   thresh_high=thr[i])
            s.synchronize()
        except Exception as e:          # pragma: no cover - reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(work))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for i in range(len(work)):
        assert len(alone[i]) > 0
        for rep in range(3):
            same_dets(alone[i], out[i][rep], "thread %d call %d" % (i, rep))
