"""The decode kernels (csrc/hv_decode.hip: dec_compact, the three greedy walks and their on-device dispatch, dec_backproject,
finalize_block, dec_apply) on the edge cases of tests/decode_ref.py, against its full-grid torch restatement.

Candidate cells, verdicts, classes, scores, `truncated` and the mutated grid must be EXACTLY the restatement's; boxes within
2e-6 of it and within 1e-6 of the oracle's (which shares the kernels' fp conventions).  Every case also runs without
mutate_grid (same result, the grid's bytes untouched) and twice (dec_compact appends in atomic order: the list order differs
between runs and nothing may depend on it).  In this process lists up to 4096 cells take walk_lds and longer ones
walk_global<512>; the last test repeats the cases in a fresh interpreter with CV_DEC_BIG_CELLS=1, where lists up to 24 576
cells take walk_sorted<1024, 24, 64> and longer ones walk_global<1024>."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from canonicalvoting_amd import decode
from tests import decode_ref as dr
from tests.test_decode_ref import BOX_TOL, GOLDEN, check_edge_fixture, oracle_decode

pytestmark = pytest.mark.gpu

EXACT = ("cand_idx", "verdict", "classes", "scores")


def t(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def hip_decode(cuda, c, mutate_grid, **over):
    """decode_boxes on a fresh device copy of the case; returns (result, the grid afterwards, the grid uploaded)"""
    dg = t(cuda, c.grid_obj)
    hip = decode.decode_boxes(dg, t(cuda, c.grid_rot), t(cuda, c.grid_scale), t(cuda, c.pts), t(cuda, c.xyz), t(cuda, c.prob),
                              t(cuda, c.cls), c.res, corner=c.corner, mutate_grid=mutate_grid,
                              allow_truncation=c.allow_truncation, **dict(c.kw, **over))
    return hip, dg.cpu().numpy()


def assert_equals_restatement(hip, want, orc=None, grid_after=None):
    for k in EXACT:
        assert np.array_equal(hip[k], want[k]), k
    assert hip["truncated"] == want["truncated"]
    assert hip["boxes"].shape == want["boxes"].shape
    np.testing.assert_allclose(hip["boxes"], want["boxes"], rtol=0, atol=BOX_TOL)
    if orc is not None:
        np.testing.assert_allclose(hip["boxes"], orc["boxes"], rtol=0, atol=1e-6)
    if grid_after is not None:
        assert np.array_equal(grid_after.view(np.uint32), want["grid_obj_after"].view(np.uint32))


def assert_same_run(a, b):
    for k in EXACT + ("boxes",):
        assert np.array_equal(a[k], b[k]), k
    assert a["truncated"] == b["truncated"]


@pytest.mark.parametrize("name", list(dr.CASES))
def test_edge_case(cuda, built_lib, name):
    c, want = dr.case(name), dr.expected(name)
    orc = oracle_decode(c)
    hip, after = hip_decode(cuda, c, True)
    assert_equals_restatement(hip, want, orc, after)
    again, after2 = hip_decode(cuda, c, True)
    assert_same_run(hip, again)
    assert np.array_equal(after.view(np.uint32), after2.view(np.uint32))
    kept, untouched = hip_decode(cuda, c, False)
    assert_same_run(hip, kept)
    assert np.array_equal(untouched.view(np.uint32), c.grid_obj.view(np.uint32))


def test_lattice_capacity_grows(cuda, built_lib):
    """max_candidates = 9 without allow_truncation: the walk is redone with 72, then 576 slots and returned complete"""
    c, want = dr.LATTICE_GROW(), dr.expected("lattice_291_m512")
    hip, untouched = hip_decode(cuda, c, False)
    assert len(hip["cand_idx"]) == 291 and not hip["truncated"]
    assert_equals_restatement(hip, want)
    assert np.array_equal(untouched.view(np.uint32), c.grid_obj.view(np.uint32))


@pytest.mark.parametrize("name", list(dr.CATEGORY_CASES))
def test_categories_mixed(cuda, built_lib, name):
    """an empty list and two lists that take different walks, side by side in blockIdx.y: category k is the single-category
    decode of its own inputs"""
    cats = dr.CATEGORY_CASES[name]()
    stack = lambda f: t(cuda, np.stack([f(c) for c in cats]))
    pts, kw = cats[0].pts, cats[0].kw

    def run(mutate_grid):
        dg = stack(lambda c: c.grid_obj)
        got = decode.decode_boxes_categories(dg, stack(lambda c: c.grid_rot), stack(lambda c: c.grid_scale), t(cuda, pts),
                                             stack(lambda c: c.xyz), stack(lambda c: c.prob), cats[0].res, class_pred=None,
                                             corner=cats[0].corner, mutate_grid=mutate_grid, **kw)
        return got, dg.cpu().numpy()

    got, after = run(True)
    again, after2 = run(True)
    kept, untouched = run(False)
    assert len(got) == 3 and np.array_equal(after.view(np.uint32), after2.view(np.uint32))
    for k, c in enumerate(cats):
        want = dr.decode(*c.args(), **c.kw)
        assert_equals_restatement(got[k], want, oracle_decode(c), after[k])
        single, _ = hip_decode(cuda, c, True)
        assert_same_run(got[k], single)
        assert_same_run(got[k], again[k])
        assert_same_run(got[k], kept[k])
        assert np.array_equal(untouched[k].view(np.uint32), c.grid_obj.view(np.uint32))
    assert len(got[0]["cand_idx"]) == 0 and len(got[1]["cand_idx"]) > 0 and len(got[2]["cand_idx"]) > 0


@pytest.mark.parametrize("name", list(dr.GOLDEN_CASES))
def test_edge_fixture_from_the_reference_lines(cuda, built_lib, name):
    """the kernels against what eval_joint.py:195-263 itself produced for the exact-arithmetic cases (the fixture alone)"""
    z = np.load(os.path.join(GOLDEN, "decode_edge_ref.npz"))
    c = dr.case(name)
    hip, after = hip_decode(cuda, c, True)
    check_edge_fixture(z, name, c, dict(hip, grid_obj_after=after))


def test_edge_cases_on_the_big_grids_dispatch(cuda, built_lib):
    """CV_DEC_BIG_CELLS=1 sends every grid through dec_greedy_dispatch_big (read once per process, hence a fresh interpreter):
    the len_*, faces_*, corners_* and lattice_291 cases and the second categories_mixed set again - lengths up to 24 576 on
    walk_sorted (63 / 64 / 65 and 1535 / 1536 / 1537 around a thread group's 64 x 24 slots), 24 577 on walk_global<1024>."""
    env = dict(os.environ, CV_DEC_BIG_CELLS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "(test_edge_case and (len_ or faces_ or corners_ or lattice_291)) or categories_mixed_b"],
                       env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
