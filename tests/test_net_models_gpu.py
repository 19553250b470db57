"""The model axis of separate mode: K structurally identical network programs as ONE launch sequence
(cv_net_run_models_f32, cv_scene_separate_desc.models_per_pass) against the K programs one after another
(cv_net_run_f32) and against the call-by-call scene - the same bits everywhere: a model's split counts, mask groups,
unit order and summation order do not depend on how many models share its launches.

The scenes have 3000 rows; each kernel family is reached by the thresholds that route to it:
  (a) library defaults: every level below 384 tiles - split-K + conv_finish_small / conv_finish, the matrix-core stem, the
      two-source conv2 of the downsampling blocks, the final conv with 8 columns;
  (b) masked_min_rows = 1024: three mask groups + conv_finish_small on the levels above 1024 rows;
  (c) (b) with hd_min_rows = 2048: the 96-column launches of level 0 on conv_hd<3, 8, 2>;
  (d) split target 1: unsplit conv_hl wherever the 10-offset limit allows."""
import contextlib
import ctypes
import threading

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, pipeline
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from tests.test_separate_scene_gpu import assert_same, by_calls, resident, same_dets, separate_models

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(cuda, built_lib):
    return separate_models(cuda)          # MinkUNet34C(3, 8), seeds 100 + c


@pytest.fixture(scope="module")
def scene(cuda, built_lib):
    return resident(1, 3000, cuda, True)


@contextlib.contextmanager
def routing(name):
    """the calling thread's / process-wide thresholds of one routing, restored on exit"""
    L = _lib.lib()
    prev_m, prev_hd, prev_t = "unset", None, None
    try:
        if name in ("b", "c"):
            prev_m = ME.set_masked_min_rows_thread(1024)
        if name == "c":
            prev_hd = ME.set_option("hd_min_rows", 2048)
        if name == "d":
            prev_t = L.cv_sp_set_split_target_thread(1)
        yield
    finally:
        if prev_t is not None:
            L.cv_sp_set_split_target_thread(prev_t)
        if prev_hd is not None:
            ME.set_option("hd_min_rows", prev_hd)
        if prev_m != "unset":
            ME.set_masked_min_rows_thread(prev_m)


def one_after_another(mods, x):
    """K runs of cv_net_run_f32 on the plan of x (no range check: the flag is not part of this comparison)"""
    return [m.program_forward(x, defer_check=True).F.clone() for m in mods]


@pytest.mark.parametrize("route", ["a", "b", "c", "d"])
def test_executor_over_the_model_axis_equals_k_single_runs(cuda, models, scene, route):
    mods = [models[c] for c in range(3)]
    sc, c4, feats, pts, teacher = scene
    with torch.no_grad(), routing(route):
        x = ME.SparseTensor(feats, c4, device=cuda)
        want = one_after_another(mods, x)
        rows = x.coordinate_manager.fused_fast(mods[0].conv0p1s1.kernel_size).counts
        assert rows[0] == 3000                                   # above both thresholds of (b) and (c)
        assert all(bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0 for w in want)
        assert not torch.equal(want[0], want[1])                 # the models differ: a mixed-up model index would show
        for G in (3, 2, 1):
            got = pipeline.forward_models(mods, x, models_per_pass=G)
            for m in range(3):
                assert torch.equal(want[m], got[m]), "routing %s, %d models per pass: output of model %d" % (route, G, m)


def test_nine_models_in_passes_of_nine_and_four(cuda, models, scene):
    mods = [models[c] for c in range(9)]
    sc, c4, feats, pts, teacher = scene
    with torch.no_grad():
        x = ME.SparseTensor(feats, c4, device=cuda)
        want = one_after_another(mods, x)
        for G in (9, 4):                    # 4: the last pass has one model
            got = pipeline.forward_models(mods, x, models_per_pass=G)
            for m in range(9):
                assert torch.equal(want[m], got[m]), "%d models per pass: output of model %d" % (G, m)


def test_batched_head_equals_k_heads(cuda, built_lib):
    torch.manual_seed(5)
    K, n = 5, 3001
    f = [torch.randn(n, 8, device=cuda) * 3 for _ in range(K)]
    xyz, scale, prob = (torch.empty(K, n, 3, device=cuda), torch.empty(K, n, 3, device=cuda), torch.empty(K, n, device=cuda))
    ptrs = (ctypes.c_void_p * K)(*[t.data_ptr() for t in f])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().cv_head_separate_models_f32(ptrs, K, n, 8, 1, p(xyz), p(scale), p(prob),
                                                      ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), "head")
    for k in range(K):
        w = pipeline.head_separate(f[k])
        assert torch.equal(w[0], xyz[k]) and torch.equal(w[1], scale[k]) and torch.equal(w[2], prob[k])


@pytest.mark.parametrize("in_flight", [None, 7])
def test_batched_scene_equals_the_sequential_call_and_the_stages(cuda, models, scene, in_flight):
    sc, c4, feats, pts, teacher = scene
    hv = HoughVoting(sc.res, 120)
    policy = None if in_flight is None else pipeline.policy_for_scenes_in_flight(in_flight)
    for pred, tag in ((teacher, "teacher predictions"), (None, "network predictions")):
        want = by_calls(models, hv, c4, feats, pts, sc.res, pred, 20, policy)
        seq = {}
        seq_dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, predictions=pred, policy=policy, keep=seq,
                                                    thresh_high=20)
        for rep in range(2):                # the second call runs on the grown scratch
            keep = {}
            dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, predictions=pred, policy=policy, keep=keep,
                                                    thresh_high=20, models_per_pass=9)
            assert_same(want, keep, dets, "%s, batched against the stages (call %d)" % (tag, rep))
            seq_as_want = dict(y=seq["y"], pred=[[seq["net_pred"][j][k] for j in range(3)] for k in range(9)],
                               grids=[[seq["grids"][j][k] for j in range(3)] for k in range(9)], raw=seq["raw"], dets=seq_dets)
            assert_same(seq_as_want, keep, dets, "%s, batched against the sequential call (call %d)" % (tag, rep))
            assert keep["range_flag"] == 0 and keep["needed_ws_bytes"] > seq["needed_ws_bytes"]      # nine arenas, not one
        if pred is not None:
            assert sum(len(r["boxes"]) for r in want["raw"]) >= 2
    # passes of four, four and one
    keep = {}
    dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, policy=policy, keep=keep, thresh_high=20,
                                            models_per_pass=4)
    assert_same(want, keep, dets, "network predictions, four models per pass")


def test_range_flag_per_model(cuda, built_lib, scene):
    """model 1's stem kernel x 1e6: its activations leave the fp16 range, the batched call reports bit 1 and the binding redoes
    the scene call by call"""
    models = separate_models(cuda, 3)
    with torch.no_grad():
        models[1].conv0p1s1.kernel.mul_(1e6)
    sc, c4, feats, pts, teacher = scene
    hv = HoughVoting(sc.res, 120)
    want = pipeline.detect_scene_separate(models, hv, c4, feats, sc.res, thresh_high=20)
    for G in (3, None):
        keep = {}
        dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, keep=keep, thresh_high=20, models_per_pass=G)
        assert keep["range_flag"] == 1 << 1, "models_per_pass=%s" % G
        same_dets(want, dets, "range fallback, models_per_pass=%s" % G)
    # the executor's own flags: one word per model, 16 ints apart
    with torch.no_grad():
        flags = torch.zeros((3, 16), dtype=torch.int32, device=cuda)
        x = ME.SparseTensor(feats, c4, device=cuda)
        pipeline.forward_models([models[c] for c in range(3)], x, models_per_pass=2, range_flags=flags)
        torch.cuda.synchronize()
        assert flags[:, 0].tolist() == [0, 1, 0] and int(flags[:, 1:].abs().sum()) == 0


def test_two_host_threads_run_batched_scenes(cuda, models):
    work = [resident(3, 3000, cuda, True), resident(4, 3000, cuda, True)]
    hv = [HoughVoting(w[0].res, 120) for w in work]
    per_pass = [9, 3]
    alone = [pipeline.detect_scene_separate_c(models, hv[i], w[1], w[2], w[0].res, predictions=w[4], thresh_high=20)
             for i, w in enumerate(work)]
    alone_net = [pipeline.detect_scene_separate_c(models, hv[i], w[1], w[2], w[0].res, thresh_high=20) for i, w in enumerate(work)]
    out = [[None] * 4 for _ in work]
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream(cuda)
            w = work[i]
            with torch.cuda.stream(s):
                for rep in range(4):
                    out[i][rep] = pipeline.detect_scene_separate_c(models, hv[i], w[1], w[2], w[0].res,
                                                                   predictions=w[4] if rep < 2 else None, thresh_high=20,
                                                                   models_per_pass=per_pass[i])
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
        for rep in range(4):
            same_dets(alone[i] if rep < 2 else alone_net[i], out[i][rep], "thread %d call %d" % (i, rep))
