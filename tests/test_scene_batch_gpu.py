"""cv_detect_scenes_f32 / pipeline.detect_scenes_c - B scans in one C call - on three synthetic rooms of 3000, 2000 and 700
points (different seeds, different extents) collated into one batched tensor:

(a) teacher predictions: per scene, grid shape, corner, the three vote grids, candidates, verdicts, boxes, scores, classes
    and detections are the BITS detect_scene_c gives for that scene alone;
(b) network predictions: every output is the bits of the call-by-call pipeline on the same batched tensor (facade forward +
    head_joint, then per scene hv and decode_boxes on row-range views);
(c) a scene's network rows inside the batch against the same scene alone: within 2e-4 (each run meets the project's 1e-4
    network bar against the fp64 oracle, hence twice that between them);
(d) B = 1 equals detect_scene_c in every bit, network output included;  (e) a second call on the grown scratch gives the
    same bits;  (f) a scene without rows and an unsorted batch column are refused with the scene named;
(g) scene_instances(keep[b], ...) equals the one-scene result;  (h) scripts/eval_joint.py --scenes-per-call 3 reports the
    mAP of --scenes-per-call 1."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from canonicalvoting_amd import decode, pipeline
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_scene, synth_predictions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.06
# (seed, points, room): with THRESH every room's teacher decode accepts 3 boxes and rejects 9 candidates or more
ROOMS = ((1, 3000, (2.0, 1.0, 2.0)), (13, 2000, (2.4, 1.0, 1.8)), (25, 700, (1.6, 1.0, 1.6)))
THRESH = 20
RAW_KEYS = ("cand_idx", "verdict", "boxes", "scores", "classes")


def room(seed, n, extent, cuda, batch_index):
    sc = make_scene(seed, n_points=n, res=RES, room=extent, n_boxes=3, margin=0.6, box_scale=0.5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    c4 = torch.cat([torch.full((n, 1), batch_index, dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(cuda)
    feats = (t(sc.feats) * 2 - 1).contiguous()
    xyz, scale, prob, cls = [t(a) for a in synth_predictions(sc)]
    return dict(c4=c4, feats=feats, pts=(c4[:, 1:] * RES).float().contiguous(), teacher=(xyz, scale, prob, cls.int()))


class World:
    """the model, the three rooms, their batched tensor and every result more than one test reads; computed once"""

    def __init__(self, cuda):
        torch.manual_seed(0)
        self.cuda = cuda
        self.model = MinkUNet34C(3, 64).to(cuda).eval()
        self.hv = HoughVoting(RES, 120)
        self.rooms = [room(s, n, e, cuda, b) for b, (s, n, e) in enumerate(ROOMS)]
        cat = lambda f: torch.cat([f(r) for r in self.rooms]).contiguous()
        self.c4, self.feats, self.pts = cat(lambda r: r["c4"]), cat(lambda r: r["feats"]), cat(lambda r: r["pts"])
        self.teacher = tuple(cat(lambda r, i=i: r["teacher"][i]) for i in range(4))
        ends = np.cumsum([n for _, n, _ in ROOMS])
        self.ranges = [(int(e - n), int(e)) for e, (_, n, _) in zip(ends, ROOMS)]
        self._alone, self._batch = {}, {}

    def alone(self, b, teacher):
        """detect_scene_c on room b alone (batch index 0, as a one-scan caller passes it)"""
        if (b, teacher) not in self._alone:
            r = self.rooms[b]
            c4 = r["c4"].clone()
            c4[:, 0] = 0
            keep = {}
            dets, raw, y = pipeline.detect_scene_c(self.model, self.hv, c4, r["feats"], RES, scan_points=r["pts"],
                                                   predictions=r["teacher"] if teacher else None, keep=keep, thresh_high=THRESH)
            self._alone[(b, teacher)] = dict(dets=dets, raw=raw, y=y.clone(), keep=keep)
        return self._alone[(b, teacher)]

    def batch(self, teacher):
        if teacher not in self._batch:
            self._batch[teacher] = self.call(teacher)
        return self._batch[teacher]

    def call(self, teacher):
        keep = []
        out, y = pipeline.detect_scenes_c(self.model, self.hv, self.c4, self.feats, RES, len(ROOMS), scan_points=self.pts,
                                          predictions=self.teacher if teacher else None, keep=keep, thresh_high=THRESH)
        return dict(out=out, y=y.clone(), keep=keep)


@pytest.fixture(scope="module")
def world(cuda, built_lib):
    return World(cuda)


def same_decode(raw_a, dets_a, raw_b, dets_b, tag):
    for k in RAW_KEYS:
        assert raw_a[k].shape == raw_b[k].shape and raw_a[k].tobytes() == raw_b[k].tobytes(), "%s: %s" % (tag, k)
    assert len(dets_a) == len(dets_b), tag + ": detections"
    for (c0, b0, s0), (c1, b1, s1) in zip(dets_a, dets_b):
        assert c0 == c1 and s0 == s1 and np.array_equal(b0, b1), tag + ": detections"


def same_keep(ka, kb, tag, net=True):
    assert tuple(ka["dims"]) == tuple(kb["dims"]), tag + ": dims"
    assert tuple(ka["corner"]) == tuple(kb["corner"]), tag + ": corner"
    for u, v, name in zip(ka["grids"], kb["grids"], ("obj", "rot", "scale")):
        assert u.shape == v.shape and torch.equal(u, v), tag + ": grid_" + name
    if net:
        assert torch.equal(ka["y"], kb["y"]), tag + ": network output"
        for u, v, name in zip(ka["net_pred"], kb["net_pred"], ("xyz", "scale", "prob", "class")):
            assert torch.equal(u, v), tag + ": head " + name


def test_a_teacher_predictions_equal_the_scene_alone(world):
    got = world.batch(True)
    for b in range(len(ROOMS)):
        one = world.alone(b, True)
        tag = "scene %d (teacher)" % b
        same_keep(got["keep"][b], one["keep"], tag, net=False)
        same_decode(got["out"][b][1], got["out"][b][0], one["raw"], one["dets"], tag)
        assert got["keep"][b]["rows"] == world.ranges[b]
        # the comparison saw accepted boxes and rejected candidates
        assert len(one["raw"]["boxes"]) >= 2 and len(one["raw"]["cand_idx"]) > len(one["raw"]["boxes"]), \
            (tag, len(one["raw"]["boxes"]), len(one["raw"]["cand_idx"]))


def test_b_network_predictions_equal_the_call_by_call_pipeline_on_the_batched_tensor(world):
    got = world.batch(False)
    with torch.no_grad():
        y = world.model(ME.SparseTensor(world.feats, world.c4, device=world.cuda)).F
        pred = pipeline.head_joint(y)
    assert torch.equal(y, got["y"]), "network output of the batched tensor"
    for b, (lo, hi) in enumerate(world.ranges):
        tag = "scene %d (network)" % b
        p = [t[lo:hi] for t in pred]
        pts = world.pts[lo:hi]
        g = world.hv(pts, p[0], p[1], p[2])
        raw = decode.decode_boxes(g[0], g[1], g[2], pts, p[0], p[2], p[3], RES, thresh_high=THRESH)
        dets = decode.nms_per_class(raw["boxes"], raw["scores"], raw["classes"])
        kb = got["keep"][b]
        for u, v, name in zip(p, kb["net_pred"], ("xyz", "scale", "prob", "class")):
            assert torch.equal(u, v), tag + ": head " + name
        for u, v, name in zip(g, kb["grids"], ("obj", "rot", "scale")):
            assert u.shape == v.shape and torch.equal(u, v), tag + ": grid_" + name
        same_decode(got["out"][b][1], got["out"][b][0], raw, dets, tag)


def test_c_network_rows_in_the_batch_against_the_scene_alone(world):
    got = world.batch(False)
    worst = 0.0
    for b, (lo, hi) in enumerate(world.ranges):
        worst = max(worst, float((got["y"][lo:hi] - world.alone(b, False)["y"]).abs().max()))
    print("max |y(batch rows) - y(scene alone)| = %.3e" % worst)
    assert worst <= 2e-4, "network rows inside the batch differ from the scene alone by %.3e (bar 2e-4; 3.4e-7 when written)" % worst


def test_d_one_scene_is_detect_scene_c_in_every_bit(world):
    for teacher in (True, False):
        r = world.rooms[0]
        c4 = r["c4"].clone()
        c4[:, 0] = 0
        keep = []
        out, y = pipeline.detect_scenes_c(world.model, world.hv, c4, r["feats"], RES, 1, scan_points=r["pts"],
                                          predictions=r["teacher"] if teacher else None, keep=keep, thresh_high=THRESH)
        one = world.alone(0, teacher)
        tag = "B = 1 (%s)" % ("teacher" if teacher else "network")
        assert torch.equal(y, one["y"]), tag + ": network output"
        same_keep(keep[0], one["keep"], tag)
        same_decode(out[0][1], out[0][0], one["raw"], one["dets"], tag)


def test_e_second_call_on_the_grown_scratch(world):
    first = world.batch(True)
    again = world.call(True)
    assert torch.equal(first["y"], again["y"])
    for b in range(len(ROOMS)):
        same_keep(first["keep"][b], again["keep"][b], "second call, scene %d" % b)
        same_decode(first["out"][b][1], first["out"][b][0], again["out"][b][1], again["out"][b][0], "second call, scene %d" % b)


def test_f_refusals_name_the_scene(world):
    kw = dict(scan_points=world.pts, predictions=world.teacher, thresh_high=THRESH)
    c4 = world.c4.clone()
    lo, hi = world.ranges[1]
    c4[lo:hi, 0] = 2                                    # batch indices 0, 2, 2: scene 1 has no rows
    with pytest.raises(Exception, match="scene 1 has no rows"):
        pipeline.detect_scenes_c(world.model, world.hv, c4, world.feats, RES, 3, **kw)
    c4 = world.c4.clone()
    c4[lo + 5, 0] = 0                                   # a row of scene 0 inside scene 1's range
    with pytest.raises(Exception, match=r"scene \d+.*batch column"):
        pipeline.detect_scenes_c(world.model, world.hv, c4, world.feats, RES, 3, **kw)
    c4 = world.c4.clone()
    c4[-1, 0] = 3                                       # leaves [0, B)
    with pytest.raises(Exception, match=r"scene \d+.*batch column"):
        pipeline.detect_scenes_c(world.model, world.hv, c4, world.feats, RES, 3, **kw)
    with pytest.raises(Exception, match="num_scenes out of range"):
        pipeline.detect_scenes_c(world.model, world.hv, world.c4, world.feats, RES, 17, **kw)
    # ... and the call still works afterwards
    again = world.call(True)
    assert torch.equal(again["y"], world.batch(True)["y"])


def test_g_instance_labels_per_scene(world):
    got = world.call(True)                              # (fresh views: scene_instances reads the scratch of the last call)
    owners = []
    for b, (lo, hi) in enumerate(world.ranges):
        res = pipeline.scene_instances(got["keep"][b], got["out"][b][0], world.pts[lo:hi], counts=True)
        owners.append({k: v.clone() for k, v in res.items()})
    for b in range(len(ROOMS)):
        r = world.rooms[b]
        c4 = r["c4"].clone()
        c4[:, 0] = 0
        keep = {}
        dets = pipeline.detect_scene_c(world.model, world.hv, c4, r["feats"], RES, scan_points=r["pts"], predictions=r["teacher"],
                                       keep=keep, thresh_high=THRESH)[0]
        want = pipeline.scene_instances(keep, dets, r["pts"], counts=True)
        assert len(dets) >= 1 and sorted(want) == sorted(owners[b])
        for k in want:
            assert torch.equal(want[k], owners[b][k]), "scene %d: %s" % (b, k)
        assert int((want["owner"] >= 0).sum()) > 0


def test_h_eval_script_reports_the_same_map():
    def run(per_call):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_joint.py"), "--teacher", "--scenes", "4", "--points",
                            "3000", "--scenes-per-call", str(per_call)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = re.findall(r"IoU (0\.\d+): mAP (\S+)\s+AR (\S+)", r.stdout)
        assert len(lines) == 2, r.stdout
        return lines

    assert run(3) == run(1)
