"""cv_decode_scenes_f32 - the decode over a scene axis - through the C ABI: B = 4 hand-made jobs (tests/decode_scene_cases.py:
four grid shapes, 700 / 50 / 1 / 3000 points, one job without a listed cell, one whose walk is cut at max_iters) against four
calls of cv_decode_f32 on the same data.  Every host output and every mutated grid must be the same BITS, with mutate_grid 0
and 1; tests/decode_ref.py says that the comparison sees accepted boxes, rejected candidates and the cut walk."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from canonicalvoting_amd import decode
from tests import decode_scene_cases as sc

pytestmark = pytest.mark.gpu

KEYS = ("cand_idx", "verdict", "boxes", "scores", "classes")


def t(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def run_batch(cuda, jobs, mutate_grid):
    """returns (the B result dicts, the B grid_obj arrays afterwards)"""
    pts, xyz, prob, cls, ranges = sc.concat(jobs)
    grids = [(t(cuda, c.grid_obj), t(cuda, c.grid_rot), t(cuda, c.grid_scale)) for c in jobs]
    got = decode.decode_boxes_scenes(grids, [c.corner for c in jobs], ranges, t(cuda, pts), t(cuda, xyz), t(cuda, prob),
                                     t(cuda, cls), sc.RES, mutate_grid=mutate_grid, **sc.KW)
    return got, [g[0].cpu().numpy() for g in grids]


def run_alone(cuda, c, mutate_grid):
    g = t(cuda, c.grid_obj)
    got = decode.decode_boxes(g, t(cuda, c.grid_rot), t(cuda, c.grid_scale), t(cuda, c.pts), t(cuda, c.xyz), t(cuda, c.prob),
                              t(cuda, c.cls), c.res, corner=c.corner, mutate_grid=mutate_grid, allow_truncation=True, **c.kw)
    return got, g.cpu().numpy()


def same_bits(a, b, tag):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: %s" % (tag, k)
    assert a["truncated"] == b["truncated"], tag + ": truncated"


def check_batch(cuda, jobs):
    for mutate in (False, True):
        got, after = run_batch(cuda, jobs, mutate)
        assert len(got) == len(jobs)
        for b, c in enumerate(jobs):
            alone, alone_after = run_alone(cuda, c, mutate)
            tag = "scene %d, mutate_grid %d" % (b, mutate)
            same_bits(got[b], alone, tag)
            assert after[b].tobytes() == alone_after.tobytes(), tag + ": grid_obj afterwards"
            if not mutate:
                assert after[b].tobytes() == c.grid_obj.tobytes(), tag + ": the grid was written without mutate_grid"
    return got


def test_four_scenes_equal_four_single_calls(cuda, built_lib):
    jobs = sc.batch()
    want = sc.expected(jobs)
    sc.claims(want)
    got = check_batch(cuda, jobs)
    # ... and what the restatement says about them (exact fields; the boxes are the single call's bits above)
    for b in range(4):
        for k in ("cand_idx", "verdict", "classes", "scores"):
            assert np.array_equal(got[b][k], want[b][k]), "scene %d: %s against tests/decode_ref.py" % (b, k)
    assert [g["truncated"] for g in got] == [False, True, False, False]          # the cut walk's flag is that scene's alone


def test_twins_in_slots_0_and_3(cuda, built_lib):
    got = check_batch(cuda, sc.batch_twins())
    same_bits(got[0], got[3], "slots 0 and 3")


def test_one_scene_is_the_single_call(cuda, built_lib):
    check_batch(cuda, [sc.job_big()])


def test_refusals(cuda, built_lib):
    jobs = sc.batch()
    with pytest.raises(Exception, match="num_scenes out of range"):
        run_batch(cuda, [sc.job_empty()] * 17, False)
    pts, xyz, prob, cls, ranges = sc.concat(jobs)
    grids = [(t(cuda, c.grid_obj), t(cuda, c.grid_rot), t(cuda, c.grid_scale)) for c in jobs]
    ranges[2] = (ranges[2][0], ranges[2][0])                                    # a scene without rows
    with pytest.raises(Exception, match="scene 2"):
        decode.decode_boxes_scenes(grids, [c.corner for c in jobs], ranges, t(cuda, pts), t(cuda, xyz), t(cuda, prob), t(cuda, cls),
                                   sc.RES, **sc.KW)


def test_a_batch_on_both_walkers(cuda, built_lib):
    """CV_DEC_BIG_CELLS=500 (read once per process, hence a fresh interpreter): the grids of 315 and 27 cells stay on the
    512-thread walker, those of 768 and 3456 cells take the 1024-thread one - two walker launches in one batch, and each
    scene still equals the single call, which makes the same choice for its grid"""
    env = dict(os.environ, CV_DEC_BIG_CELLS="500")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_four_scenes_equal_four_single_calls"], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
