"""Two branches of the scene calls in pipeline.py that the other tests do not reach, on the 3000-point scene of
tests/test_scene_call_gpu.py (K = 3 models for separate mode, the 6000-sample cloud of tests/test_points_call_gpu.py for the
raw-cloud call):

  * scratch growth - with the scratch floor at 1 MiB a call on a stream without scratch starts too small, the C call answers
    CV_ENOMEM with the size it needs, the scratch grows and the scene runs again: the same results as under the default floor;
  * the range-flag redo - a network input beyond the fp16 range (bn0's weight at 1e7) sends the scene to the call-by-call
    path on the bf16 triples: what detect_scene / detect_scene_separate return.

Every comparison is exact."""
import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests import test_points_call_gpu as raw_cloud
from tests import test_scene_call_gpu as joint
from tests import test_separate_scene_gpu as separate

pytestmark = pytest.mark.gpu
K, THRESH, RES, MIB = 3, 20, 0.06, 1 << 20


def _same_dets(a, b):
    assert len(a) == len(b)
    for (c0, b0, s0), (c1, b1, s1) in zip(a, b):
        assert c0 == c1 and s0 == s1 and b0.tobytes() == b1.tobytes()


def _same_raw(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _joint_scene(cuda):
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(cuda).eval()
    return (model,) + joint.resident(1, 3000, cuda, True)[1:]


def _separate_scene(cuda):
    _, c4, feats, pts, teacher = separate.resident(1, 3000, cuda, True)
    return separate.separate_models(cuda, K), c4, feats, pts, tuple(t[:K].contiguous() for t in teacher)


def _host(cuda, separate_mode):
    """the scene calls' host scratch of the current stream"""
    return pipeline._hosts.get((cuda.index, torch.cuda.current_stream(cuda).cuda_stream, separate_mode))


def _forget_stream(cuda, stream):
    """the stream handle may be one an earlier test used: drop its device scratch and the hosts that remember its size"""
    _lib.release_scratch(cuda, stream)
    for separate_mode in (False, True):
        pipeline._hosts.pop((cuda.index, stream.cuda_stream, separate_mode), None)


def test_scratch_grows_from_a_small_floor(cuda, built_lib, monkeypatch):
    model, c4, feats, pts, teacher = _joint_scene(cuda)
    models, s_c4, s_feats, _, s_teacher = _separate_scene(cuda)
    cloud, _, cloud_feats, cloud_teacher = raw_cloud.cloud(1, cuda)
    hv = HoughVoting(RES, 120)

    def calls():
        kj, kp, ks = {}, {}, {}
        a = pipeline.detect_scene_c(model, hv, c4, feats, RES, scan_points=pts, predictions=teacher, keep=kj, thresh_high=THRESH)
        b = pipeline.detect_points_c(model, hv, cloud, cloud_feats, RES, predictions=cloud_teacher, keep=kp, thresh_high=THRESH)
        c = pipeline.detect_scene_separate_c(models, hv, s_c4, s_feats, RES, predictions=s_teacher, keep=ks, thresh_high=THRESH)
        return (a, kj), (b, kp), (c, ks)

    want = calls()
    assert len(want[0][0][1]["boxes"]) >= 2
    torch.cuda.synchronize()
    monkeypatch.setattr(pipeline, "SCRATCH_FLOOR", MIB)
    side = torch.cuda.Stream(cuda)
    _forget_stream(cuda, side)
    with torch.cuda.stream(side):
        got = calls()
        side.synchronize()
        hints = [_host(cuda, False).ws_hint, _host(cuda, True).ws_hint]
    _forget_stream(cuda, side)
    assert min(hints) > MIB, hints               # the first attempt of each mode could not have fitted
    for (w, wk), (g, gk) in zip(want[:2], got[:2]):
        _same_dets(w[0], g[0])
        _same_raw(w[1], g[1])
        assert torch.equal(w[2], g[2]) and torch.equal(wk["y"], gk["y"])
        _same_raw(wk["raw"], gk["raw"])
    assert torch.equal(want[1][0][3], got[1][0][3])            # (index of the raw-cloud call)
    (w, wk), (g, gk) = want[2], got[2]
    _same_dets(w, g)
    for k in range(K):
        assert torch.equal(wk["y"][k], gk["y"][k])
        _same_raw(wk["raw"][k], gk["raw"][k])


def _beyond_fp16(model):
    with torch.no_grad():
        model.bn0.bn.weight.fill_(1e7)       # activations beyond the fp16 range: the pair format's range flag rises


def test_range_flag_redoes_the_joint_scene_call_by_call(cuda, built_lib):
    model, c4, feats, pts, _ = _joint_scene(cuda)
    _beyond_fp16(model)
    hv = HoughVoting(RES, 120)
    dets, raw, y = pipeline.detect_scene(model, hv, c4, feats, RES, thresh_high=THRESH)
    before = model.range_fallbacks
    assert before >= 1
    got = pipeline.detect_scene_c(model, hv, c4, feats, RES, thresh_high=THRESH)
    assert model.range_fallbacks == before + 1
    _same_dets(dets, got[0])
    _same_raw(raw, got[1])
    assert torch.equal(y.F, got[2])


def test_range_flag_redoes_the_separate_scene_call_by_call(cuda, built_lib):
    models, c4, feats, _, _ = _separate_scene(cuda)
    for m in models.values():
        _beyond_fp16(m)
    hv = HoughVoting(RES, 120)
    want = pipeline.detect_scene_separate(models, hv, c4, feats, RES, thresh_high=THRESH)
    keep = {}
    got = pipeline.detect_scene_separate_c(models, hv, c4, feats, RES, keep=keep, thresh_high=THRESH)
    assert keep["range_flag"] != 0 and "y" not in keep            # (the one-call path did not deliver this result)
    _same_dets(want, got)
