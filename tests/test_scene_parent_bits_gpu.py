"""The Python call layer of the eval path (pipeline.py's scene calls, hv_cuda.forward / forward_categories / backward,
decode.decode_boxes / decode_boxes_categories, pipeline.forward_models) against recorded bits:
tests/golden/scene_parent_bits.json holds, for every case, the sha256 of raw bytes as that layer produced them before its
joint / separate and single / K twins were folded.  The other tests of these calls compare the one-call paths with the
call-by-call paths; that refactor rewrote both sides, so "the same bits as before" is pinned here.  Every case was recorded
twice, in two processes, and is pinned because both agreed.

A case hashes everything its call returns: the detections (class or category, box bytes, score), every array of ``raw``,
the network outputs, ``index`` / ``inverse`` and, from ``keep``, ``y``, ``net_pred``, ``grids``, ``dims``, ``corner``,
``level_rows`` and ``raw`` (plus the gathered ``scan_points`` / ``feats`` / ``coords4`` of the raw-cloud calls).  Timings
(``host_us``) and scratch sizes are not results and are not hashed.

The refactor moved no arithmetic and no launch, so the hashes are expected to be EQUAL: there is no tolerance.

Scenes: the 3000-point scene of tests/test_scene_call_gpu.py and tests/test_separate_scene_gpu.py (seed 1, thresh_high 20,
K = 3 models for separate mode) and the 6000-sample raw cloud of tests/test_points_call_gpu.py."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from canonicalvoting_amd import decode, hv_cuda, pipeline
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from tests import test_points_call_gpu as raw_cloud
from tests import test_scene_call_gpu as joint
from tests import test_separate_scene_gpu as separate

pytestmark = pytest.mark.gpu
BITS = os.path.join(os.path.dirname(__file__), "golden", "scene_parent_bits.json")
K, THRESH, RES, ROTS = 3, 20, 0.06, 120
KEEP_KEYS = ("y", "net_pred", "grids", "dims", "corner", "level_rows", "raw", "scan_points", "feats", "coords4", "range_flag")


def _feed(h, v):
    """raw bytes of tensors and arrays; lists, tuples and dicts element by element (dicts in key order); numbers by repr"""
    if torch.is_tensor(v):
        h.update(v.detach().contiguous().cpu().numpy().tobytes())
    elif isinstance(v, np.ndarray):
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        for k in sorted(v):
            h.update(k.encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d]" % len(v))
        for e in v:
            _feed(h, e)
    else:
        assert v is None or isinstance(v, (bool, int, float, np.integer, np.floating)), type(v)
        h.update(repr(float(v) if isinstance(v, (float, np.floating)) else v if v is None else int(v)).encode())


def _hash(*items):
    h = hashlib.sha256()
    _feed(h, items)
    return h.hexdigest()


def _kept(keep):
    return {k: keep[k] for k in KEEP_KEYS if k in keep}


@functools.lru_cache(None)
def _joint(cuda):
    """(model, c4, feats, pts, teacher) of the joint 3000-point scene"""
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(cuda).eval()
    _, c4, feats, pts, teacher = joint.resident(1, 3000, cuda, True)
    return model, c4, feats, pts, teacher


@functools.lru_cache(None)
def _separate(cuda):
    """(models, c4, feats, pts, teacher [K, ...]) of the separate-mode 3000-point scene, K = 3"""
    _, c4, feats, pts, teacher = separate.resident(1, 3000, cuda, True)
    return separate.separate_models(cuda, K), c4, feats, pts, tuple(t[:K].contiguous() for t in teacher)


def _hv():
    return HoughVoting(RES, ROTS)


def _detect_scene(cuda):
    model, c4, feats, _, _ = _joint(cuda)
    dets, raw, y = pipeline.detect_scene(model, _hv(), c4, feats, RES, thresh_high=THRESH)
    return _hash(dets, raw, y.F)


def _detect_scene_c(teacher, with_keep):
    def run(cuda):
        model, c4, feats, pts, pred = _joint(cuda)
        keep = {} if with_keep else None
        dets, raw, y = pipeline.detect_scene_c(model, _hv(), c4, feats, RES, scan_points=pts, predictions=pred if teacher else None,
                                               keep=keep, thresh_high=THRESH)
        return _hash(dets, raw, y, _kept(keep) if with_keep else None)
    return run


def _detect_scene_separate(cuda):
    models, c4, feats, _, _ = _separate(cuda)
    return _hash(pipeline.detect_scene_separate(models, _hv(), c4, feats, RES, thresh_high=THRESH))


def _detect_scene_separate_c(teacher, models_per_pass):
    def run(cuda):
        models, c4, feats, _, pred = _separate(cuda)
        keep = {}
        dets = pipeline.detect_scene_separate_c(models, _hv(), c4, feats, RES, predictions=pred if teacher else None, keep=keep,
                                                models_per_pass=models_per_pass, thresh_high=THRESH)
        return _hash(dets, _kept(keep))
    return run


def _detect_points_c(teacher):
    def run(cuda):
        model = _joint(cuda)[0]
        pts, _, feats, pred = raw_cloud.cloud(1, cuda)
        keep = {}
        dets, raw, y, index, inverse = pipeline.detect_points_c(model, _hv(), pts, feats, RES, predictions=pred if teacher else None,
                                                                return_inverse=True, keep=keep, thresh_high=THRESH)
        return _hash(dets, raw, y, index, inverse, _kept(keep))
    return run


def _detect_points_separate_c(teacher, models_per_pass):
    def run(cuda):
        models = _separate(cuda)[0]
        pts, _, feats, _ = raw_cloud.cloud(1, cuda)
        keep = {}
        dets, index, inverse = pipeline.detect_points_separate_c(
            models, _hv(), pts, feats, RES, predictions=raw_cloud.separate_teacher(1, cuda) if teacher else None,
            models_per_pass=models_per_pass, return_inverse=True, keep=keep, thresh_high=THRESH)
        return _hash(dets, index, inverse, _kept(keep))
    return run


def _forward_models(models_per_pass):
    def run(cuda):
        models, c4, feats, _, _ = _separate(cuda)
        with torch.no_grad():
            return _hash(pipeline.forward_models(models.values(), ME.SparseTensor(feats, c4, device=cuda), models_per_pass))
    return run


def _vote_operands(cuda):
    _, _, _, pts, (xyz, scale, prob, _) = _joint(cuda)
    return pts, xyz, scale, prob, torch.tensor(RES, device=cuda), torch.tensor(ROTS, dtype=torch.int32, device=cuda)


def _hv_forward(with_corners):
    def run(cuda):
        pts, xyz, scale, prob, res, rots = _vote_operands(cuda)
        corners = None
        if with_corners:      # a box that cuts the cloud: votes fall outside it
            corners = torch.stack([pts.min(0).values + 0.17, pts.max(0).values - 0.11])
        g = hv_cuda.forward(pts, xyz, scale, prob, res, rots, corners)
        return _hash(g, list(g[0].shape), hv_cuda.recent_corner(g[0]))
    return run


def _hv_backward(cuda):
    pts, xyz, scale, prob, res, rots = _vote_operands(cuda)
    dims = hv_cuda.forward(pts, xyz, scale, prob, res, rots)[0].shape
    grad = torch.randn(*dims, generator=torch.Generator().manual_seed(3)).to(cuda)
    return _hash(hv_cuda.backward(grad, pts, xyz, scale, prob, res, rots))


def _category_operands(cuda, k):
    _, _, _, pts, teacher = _separate(cuda)
    return (pts,) + tuple(t[:k].contiguous() for t in teacher)


def _hv_forward_categories(k):
    def run(cuda):
        pts, xyz, scale, prob = _category_operands(cuda, k)
        g = hv_cuda.forward_categories(pts, xyz, scale, prob, RES, ROTS)
        return _hash(g, list(g[0].shape), hv_cuda.recent_corner(g[0]))
    return run


def _decode_boxes(max_candidates):
    def run(cuda):
        pts, xyz, scale, prob, res, rots = _vote_operands(cuda)
        g = hv_cuda.forward(pts, xyz, scale, prob, res, rots)
        raw = decode.decode_boxes(g[0], g[1], g[2], pts, xyz, prob, _joint(cuda)[4][3], RES, thresh_high=THRESH,
                                  max_candidates=max_candidates)
        assert len(raw["cand_idx"]) > 4 and len(raw["boxes"]) >= 2       # (with max_candidates = 4 the walk regrew)
        return _hash(raw)
    return run


def _decode_boxes_categories(k, max_candidates):
    def run(cuda):
        pts, xyz, scale, prob = _category_operands(cuda, k)
        g = hv_cuda.forward_categories(pts, xyz, scale, prob, RES, ROTS)
        raws = decode.decode_boxes_categories(g[0], g[1], g[2], pts, xyz, prob, RES, thresh_high=THRESH,
                                              max_candidates=max_candidates, **separate.SEP)
        assert len(raws) == k and (max_candidates > 4 or max(len(r["cand_idx"]) for r in raws) > 4)      # (4: a walk regrew)
        return _hash(raws)
    return run


CASES = {
    "detect_scene": _detect_scene,
    "detect_scene_c_teacher_keep": _detect_scene_c(True, True),
    "detect_scene_c_teacher": _detect_scene_c(True, False),
    "detect_scene_c_network_keep": _detect_scene_c(False, True),
    "detect_scene_c_network": _detect_scene_c(False, False),
    "detect_scene_separate": _detect_scene_separate,
    "detect_scene_separate_c_network": _detect_scene_separate_c(False, None),
    "detect_scene_separate_c_network_pass2": _detect_scene_separate_c(False, 2),
    "detect_scene_separate_c_teacher": _detect_scene_separate_c(True, None),
    "detect_scene_separate_c_teacher_pass2": _detect_scene_separate_c(True, 2),
    "detect_points_c_teacher": _detect_points_c(True),
    "detect_points_c_network": _detect_points_c(False),
    "detect_points_separate_c_teacher": _detect_points_separate_c(True, None),
    "detect_points_separate_c_network_pass2": _detect_points_separate_c(False, 2),
    "forward_models": _forward_models(None),
    "forward_models_pass2": _forward_models(2),
    "hv_forward": _hv_forward(False),
    "hv_forward_corners": _hv_forward(True),
    "hv_backward": _hv_backward,
    "hv_forward_categories_k1": _hv_forward_categories(1),
    "hv_forward_categories_k3": _hv_forward_categories(3),
    "decode_boxes": _decode_boxes(512),
    "decode_boxes_regrown": _decode_boxes(4),
    "decode_boxes_categories_k1": _decode_boxes_categories(1, 512),
    "decode_boxes_categories_k3": _decode_boxes_categories(3, 512),
    "decode_boxes_categories_k3_regrown": _decode_boxes_categories(3, 4),
}


def _recorded():
    with open(BITS) as f:
        return json.load(f)


def test_every_case_has_recorded_bits():
    assert set(_recorded()) == set(CASES)            # (every case reproduced between the two recording processes)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_recorded_bits(name, cuda, built_lib):
    assert CASES[name](cuda) == _recorded()[name], name + ": not the bits the parent's call layer produced"
