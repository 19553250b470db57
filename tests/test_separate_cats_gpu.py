"""Category axis of the vote and the decode (separate mode, eval_separate.py:166-264): K categories' grids in ONE vote launch
sequence (cv_hv_forward_cat_f32) and K decodes behind ONE host wait (cv_decode_cat_f32) must be bit for bit the K single
calls (cv_hv_forward_f32, cv_decode_f32) - the vote is fixed point with integer merges, so the category axis cannot change
any sum - and the batched decode must agree with the CPU oracle run per category.  (The single calls the vote is compared with
are the K = 1 case of the same kernels; their own agreement with the CPU oracle is what tests/test_oracle_vote.py and
tests/test_decode_gpu.py check.)"""
import threading

import numpy as np
import pytest
import torch

import oracle
from canonicalvoting_amd import _lib, decode, hv_cuda
from canonicalvoting_amd.synth import make_scene, synth_predictions

pytestmark = pytest.mark.gpu

K = 9
R = 120
SEPARATE = dict(separate_variant=True, err_thresh=float(np.float32(0.3)))     # what detect_scene_separate passes


def t(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def category_teacher(sc, k=K, seed=0):
    """Per-category predictions: category c's points keep the teacher's confident probability, every other point gets a
    background-level, NON-zero one (a trained model's softmax never gives zero) and slightly different offsets."""
    xyz, scale, prob, cls = synth_predictions(sc)
    rng = np.random.default_rng(7 + seed)
    n = xyz.shape[0]
    X = np.empty((k, n, 3), np.float32)
    S = np.empty((k, n, 3), np.float32)
    P = np.empty((k, n), np.float32)
    for c in range(k):
        other = cls != c
        X[c] = xyz + other[:, None] * rng.normal(0, 0.02, (n, 3)).astype(np.float32)
        S[c] = scale
        P[c] = np.where(other, rng.uniform(1e-3, 0.1, n), prob).astype(np.float32)
    return sc.points, X, S, P


_scenes = {}


def scene(n):
    if n not in _scenes:
        if n <= 3000:
            sc = make_scene(11, n_points=n, room=(2.4, 1.6, 2.4), n_boxes=4)
        elif n <= 80000:
            sc = make_scene(12, n_points=n)
        else:
            sc = make_scene(3, n_points=n, room=(9.0, 3.0, 9.0), n_boxes=40)
        _scenes[n] = category_teacher(sc)
    return _scenes[n]


def bits(x):
    return x.contiguous().view(torch.int32)


def scalars(dev, res):
    return torch.tensor(res, dtype=torch.float32, device=dev), torch.tensor(R, dtype=torch.int32, device=dev)


def single_votes(pts, X, S, P, res):
    out = [hv_cuda.forward(pts, X[c], S[c], P[c], *scalars(pts.device, res)) for c in range(X.shape[0])]
    return [torch.stack([o[i] for o in out]) for i in range(3)]


@pytest.mark.parametrize("n", [3000, 80000, 300000])
@pytest.mark.parametrize("part_records", [4096, 12288])
def test_batched_vote_is_k_single_votes_bit_for_bit(cuda, built_lib, n, part_records):
    pts, X, S, P = scene(n)
    res = 0.03
    L = _lib.lib()
    prev = L.cv_hv_set_part_records_thread(part_records)
    try:
        pts_d, X_d, S_d, P_d = t(cuda, pts), t(cuda, X), t(cuda, S), t(cuda, P)
        ref = single_votes(pts_d, X_d, S_d, P_d, res)
        got = hv_cuda.forward_categories(pts_d, X_d, S_d, P_d, *scalars(cuda, res))
        torch.cuda.synchronize()
    finally:
        L.cv_hv_set_part_records_thread(prev)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        assert torch.equal(bits(a), bits(b))
    # every category voted (no culling of low-probability points): background votes reach cells the objects do not
    assert all(float(got[0][c].sum()) > 0 for c in range(K))


def test_batched_vote_k1_is_the_single_call(cuda, built_lib):
    pts, X, S, P = scene(80000)
    pts_d = t(cuda, pts)
    one = hv_cuda.forward(pts_d, t(cuda, X[4]), t(cuda, S[4]), t(cuda, P[4]), *scalars(cuda, 0.03))
    cat = hv_cuda.forward_categories(pts_d, t(cuda, X[4:5]), t(cuda, S[4:5]), t(cuda, P[4:5]), 0.03, R)
    for a, b in zip(cat, one):
        assert torch.equal(bits(a[0]), bits(b))


def same_raw(a, b):
    assert list(a["cand_idx"]) == list(b["cand_idx"])
    assert list(a["verdict"]) == list(b["verdict"])
    assert list(a["classes"]) == list(b["classes"])
    assert a["truncated"] == b["truncated"]
    assert np.array_equal(a["boxes"].view(np.int32), b["boxes"].view(np.int32))
    assert np.array_equal(a["scores"].view(np.int32), b["scores"].view(np.int32))


@pytest.mark.parametrize("n", [3000, 80000, 300000])      # 300k: grids beyond 4 M cells take dec_greedy_dispatch_big
@pytest.mark.parametrize("mutate", [False, True])
def test_batched_decode_is_k_single_decodes(cuda, built_lib, n, mutate):
    pts, X, S, P = scene(n)
    P = P.copy()
    P[2] = np.float32(1e-4)                 # category 2: no cell reaches thresh_high - no candidate at all
    pts_d, X_d, S_d, P_d = t(cuda, pts), t(cuda, X), t(cuda, S), t(cuda, P)
    grids = hv_cuda.forward_categories(pts_d, X_d, S_d, P_d, 0.03, R)
    corner = hv_cuda.recent_corner(grids[0])
    zeros = torch.zeros(pts.shape[0], dtype=torch.int32, device=cuda)
    g_single = grids[0].clone()
    g_batch = grids[0].clone()
    ref = [decode.decode_boxes(g_single[c], grids[1][c], grids[2][c], pts_d, X_d[c], P_d[c], zeros, 0.03, corner=corner,
                               mutate_grid=mutate, **SEPARATE) for c in range(K)]
    got = decode.decode_boxes_categories(g_batch, grids[1], grids[2], pts_d, X_d, P_d, 0.03, corner=corner, mutate_grid=mutate,
                                         **SEPARATE)
    assert len(got) == K
    for a, b in zip(got, ref):
        same_raw(a, b)
    assert len(got[2]["cand_idx"]) == 0
    assert sum(len(g["cand_idx"]) for g in got) > 0
    assert torch.equal(bits(g_batch), bits(g_single))       # the same in-place suppression (or none)
    # an explicit zero class input is the same as none
    again = decode.decode_boxes_categories(grids[0].clone(), grids[1], grids[2], pts_d, X_d, P_d, 0.03, class_pred=zeros,
                                           corner=corner, **SEPARATE)
    for a, b in zip(again, got):
        same_raw(a, b)


def test_batched_decode_truncation_per_category(cuda, built_lib):
    pts, X, S, P = scene(80000)
    pts_d, X_d, S_d, P_d = t(cuda, pts), t(cuda, X), t(cuda, S), t(cuda, P)
    grids = hv_cuda.forward_categories(pts_d, X_d, S_d, P_d, 0.03, R)
    corner = hv_cuda.recent_corner(grids[0])
    zeros = torch.zeros(pts.shape[0], dtype=torch.int32, device=cuda)
    kw = dict(SEPARATE, max_candidates=2, allow_truncation=True)
    ref = [decode.decode_boxes(grids[0][c], grids[1][c], grids[2][c], pts_d, X_d[c], P_d[c], zeros, 0.03, corner=corner, **kw)
           for c in range(K)]
    got = decode.decode_boxes_categories(grids[0], grids[1], grids[2], pts_d, X_d, P_d, 0.03, corner=corner, **kw)
    for a, b in zip(got, ref):
        same_raw(a, b)
    assert any(g["truncated"] for g in got)
    # without allow_truncation the walk is redone with more room: the complete result of every category
    full = decode.decode_boxes_categories(grids[0], grids[1], grids[2], pts_d, X_d, P_d, 0.03, corner=corner, max_candidates=2,
                                          **SEPARATE)
    for c in range(K):
        same_raw(full[c], decode.decode_boxes(grids[0][c], grids[1][c], grids[2][c], pts_d, X_d[c], P_d[c], zeros, 0.03,
                                              corner=corner, **SEPARATE))
        assert not full[c]["truncated"]


def test_batched_decode_matches_cpu_oracle_per_category(cuda, built_lib):
    """oracle grids (hv_oracle.c) of each category decoded in one batched call vs decode_oracle.c run per category"""
    pts, X, S, P = scene(3000)
    res = 0.03
    cats = [2, 4, 7]                        # the categories with objects in this scene
    g = [oracle.hv_forward(pts, X[c], S[c], P[c], res, R) for c in cats]
    corner, _, _ = oracle.grid_geometry(pts, res)
    thr = float(np.sort(g[0][0].ravel())[-200])
    zeros = np.zeros(pts.shape[0], np.int32)
    stack = lambda i: t(cuda, np.stack([gg[i] for gg in g]))
    got = decode.decode_boxes_categories(stack(0), stack(1), stack(2), t(cuda, pts), t(cuda, X[cats]), t(cuda, P[cats]), res,
                                         corner=corner, thresh_high=thr, **SEPARATE)
    n_cand = 0
    for j, c in enumerate(cats):
        ref = oracle.decode(g[j][0], g[j][1], g[j][2], corner, res, pts, X[c], P[c], zeros,
                            oracle.DecodeParams.default(thresh_high=thr, elim_hi_plus1=0, err_thresh=SEPARATE["err_thresh"]))
        assert list(got[j]["cand_idx"]) == list(ref["cand_idx"])
        assert list(got[j]["verdict"]) == list(ref["verdict"])
        np.testing.assert_allclose(got[j]["boxes"], ref["boxes"].reshape(-1, 8, 3), rtol=0, atol=1e-6)
        np.testing.assert_allclose(got[j]["scores"], ref["scores"], rtol=0, atol=0)
        n_cand += len(ref["cand_idx"])
    assert n_cand >= 3


def test_two_host_threads_batched_vote_and_decode(cuda, built_lib):
    """two threads, each on its own stream, running batched vote + decode of separate scenes: the same bits as one at a time"""
    work = [scene(3000), scene(80000)]

    def run(w):
        pts, X, S, P = w
        pts_d, X_d, S_d, P_d = t(cuda, pts), t(cuda, X), t(cuda, S), t(cuda, P)
        grids = hv_cuda.forward_categories(pts_d, X_d, S_d, P_d, 0.03, R)
        raw = decode.decode_boxes_categories(grids[0], grids[1], grids[2], pts_d, X_d, P_d, 0.03, **SEPARATE)
        return grids, raw

    alone = [run(w) for w in work]
    out = [[None] * 4 for _ in work]
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream(cuda)
            with torch.cuda.stream(s):
                for rep in range(4):
                    out[i][rep] = run(work[i])
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
        for rep in range(4):
            grids, raw = out[i][rep]
            for a, b in zip(grids, alone[i][0]):
                assert torch.equal(bits(a), bits(b))
            for a, b in zip(raw, alone[i][1]):
                same_raw(a, b)
