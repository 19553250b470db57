"""Separate mode's vote + decode (eval_separate.py:166-264, nine categories over one scan): the category axis
(hv_cuda.forward_categories + decode.decode_boxes_categories: one vote launch sequence, one decode with one host wait)
against nine single calls (hv_cuda.forward + decode.decode_boxes per category, what detect_scene_separate does).

    python profiles/separate_scene.py [--sizes 80000 300000] [--repeats 3] [--scenes 20] [--out FILE]
                                      [--models-per-pass 3 9] [--whole-only]

and whole scenes (nine 8-channel networks on one coordinate plan, heads, vote, decode, NMS): the call-by-call path of
detect_scene_separate against ONE pipeline.detect_scene_separate_c call (cv_detect_scene_separate_f32), both voting with
the teacher below ("whole" in the output), and against the same call with the nine networks batched over a model axis
(--models-per-pass G ...: "whole_models_G", cv_net_run_models_f32 in passes of G models; with its scratch size,
needed_ws_bytes).  --whole-only measures the one-call paths alone.  Launch counts per scene come from a run of its own under
rocprofv3 --kernel-trace --stats (--scenes 2 --repeats 1) and counting the dispatches per kernel name.

Predictions are a per-category teacher: category c's points keep the synthetic teacher's probability, every other point
gets a background-level, non-zero one (a trained softmax never gives zero), so no category's vote is emptier than a real
one.  One scene in flight.  Per size and repeat, the two paths alternate in one process:
  scenes_per_s      vote + decode of whole scenes, host clock, after a device sync
  vote_ms/decode_ms device time of the stage (events around it; the decode's includes its host wait)
Prints one JSON object and writes it to --out when given."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from canonicalvoting_amd import decode, hv_cuda, pipeline  # noqa: E402
from canonicalvoting_amd import me as ME  # noqa: E402
from canonicalvoting_amd.hough import HoughVoting  # noqa: E402
from canonicalvoting_amd.minkunet import MinkUNet34C  # noqa: E402
from canonicalvoting_amd.synth import make_scene, synth_predictions  # noqa: E402

K, R, RES = 9, 120, 0.03
SEPARATE = dict(separate_variant=True, err_thresh=float(np.float32(0.3)))


def scene_of(n):
    return make_scene(3, n_points=n, room=(9.0, 3.0, 9.0), n_boxes=40) if n > 80000 else make_scene(12, n_points=n)


def whole_inputs(n, pts):
    sc = scene_of(n)
    dev = pts.device
    c4 = torch.cat([torch.zeros((n, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(dev)
    feats = (torch.from_numpy(sc.feats).to(dev) * 2 - 1).float().contiguous()
    models = {}
    for c in range(K):
        torch.manual_seed(100 + c)
        models[c] = MinkUNet34C(3, 8).to(dev).eval()
    return models, HoughVoting(RES, R), c4, feats


def whole_by_calls(models, hv, c4, feats, pts, X, S, P, ev):
    ev[0].record()
    with torch.no_grad():
        x = ME.SparseTensor(feats, c4, device=feats.device)
        for model in models.values():
            pipeline.head_separate(model(x).F)
    dets = pipeline._separate_by_calls(hv, pts, zip(X, S, P), RES, list(models), **SEPARATE)
    ev[1].record()
    ev[2].record()
    return dets


def whole_one_call(models, hv, c4, feats, pts, X, S, P, ev):
    ev[0].record()
    dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, RES, predictions=(X, S, P), scan_points=pts, **SEPARATE)
    ev[1].record()
    ev[2].record()
    return dets


def whole_models(G):
    def run(models, hv, c4, feats, pts, X, S, P, ev, keep=None):
        ev[0].record()
        dets = pipeline.detect_scene_separate_c(models, hv, c4, feats, RES, predictions=(X, S, P), scan_points=pts,
                                                models_per_pass=G, keep=keep, **SEPARATE)
        ev[1].record()
        ev[2].record()
        return dets
    return run


def teacher(n):
    sc = scene_of(n)
    xyz, scale, prob, cls = synth_predictions(sc)
    rng = np.random.default_rng(7)
    X = np.stack([xyz + (cls != c)[:, None] * rng.normal(0, 0.02, xyz.shape).astype(np.float32) for c in range(K)])
    S = np.stack([scale] * K)
    P = np.stack([np.where(cls != c, rng.uniform(1e-3, 0.1, n), prob) for c in range(K)]).astype(np.float32)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    return t(sc.points), t(X), t(S), t(P)


def single(pts, X, S, P, ev):
    res, nr = torch.tensor(RES, device=pts.device), torch.tensor(R, dtype=torch.int32, device=pts.device)
    zeros = torch.zeros(pts.shape[0], dtype=torch.int32, device=pts.device)
    ev[0].record()
    grids = [hv_cuda.forward(pts, X[c], S[c], P[c], res, nr) for c in range(K)]
    ev[1].record()
    raws = [decode.decode_boxes(g[0], g[1], g[2], pts, X[c], P[c], zeros, RES, **SEPARATE) for c, g in enumerate(grids)]
    ev[2].record()
    return raws


def batched(pts, X, S, P, ev):
    ev[0].record()
    g = hv_cuda.forward_categories(pts, X, S, P, RES, R)
    ev[1].record()
    raws = decode.decode_boxes_categories(g[0], g[1], g[2], pts, X, P, RES, **SEPARATE)
    ev[2].record()
    return raws


def measure(fn, args, scenes):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    vote, dec = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(scenes):
        fn(*args, ev)
        ev[2].synchronize()
        vote.append(ev[0].elapsed_time(ev[1]))
        dec.append(ev[1].elapsed_time(ev[2]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(scenes_per_s=scenes / dt, vote_ms=statistics.median(vote), decode_ms=statistics.median(dec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[80000, 300000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--models-per-pass", type=int, nargs="*", default=[], help="also time the one-call path with the networks batched")
    ap.add_argument("--whole-only", action="store_true", help="only the whole-scene one-call paths")
    a = ap.parse_args()
    out = dict(categories=K, num_rots=R, res=RES, sizes={})
    for n in a.sizes:
        args = teacher(n)
        events = lambda: [torch.cuda.Event() for _ in range(3)]
        same_dets = lambda da, db: len(da) == len(db) and all(
            c0 == c1 and s0 == s1 and np.array_equal(b0, b1) for (c0, b0, s0), (c1, b1, s1) in zip(da, db))
        rows = {}
        if not a.whole_only:
            a_raw, b_raw = single(*args, events()), batched(*args, events())
            same = all(list(x["cand_idx"]) == list(y["cand_idx"]) and np.array_equal(x["boxes"], y["boxes"]) for x, y in zip(a_raw, b_raw))
            rows.update(single=[], batched=[])
            for _ in range(a.repeats):
                rows["single"].append(measure(single, args, a.scenes))
                rows["batched"].append(measure(batched, args, a.scenes))
        wargs = whole_inputs(n, args[0]) + args
        whole = {"whole_one_call": whole_one_call}
        if not a.whole_only:
            whole = {"whole_by_calls": whole_by_calls, "whole_one_call": whole_one_call}
        whole.update({"whole_models_%d" % G: whole_models(G) for G in a.models_per_pass})
        first, needed = {}, {}
        for k, fn in whole.items():                  # warm-up (grows the scratch) and the results to compare
            if k.startswith("whole_models_"):
                keep = {}
                first[k] = fn(*wargs, events(), keep=keep)
                needed[k] = keep["needed_ws_bytes"]
            else:
                first[k] = fn(*wargs, events())
            rows[k] = []
        for _ in range(a.repeats):                   # the paths alternate inside a repeat
            for k, fn in whole.items():
                rows[k].append(measure(fn, wargs, a.scenes))
        summ = {k: {m: [round(r[m], 4) for r in v] for m in ("scenes_per_s", "vote_ms", "decode_ms")} for k, v in rows.items()}
        for k in whole:
            summ[k] = {"scenes_per_s": summ[k]["scenes_per_s"], "scene_ms": summ[k]["vote_ms"]}
            if k in needed:
                summ[k]["needed_ws_bytes"] = needed[k]
        summ["whole_same_detections"] = all(same_dets(first["whole_one_call"], d) for d in first.values())
        if not a.whole_only:
            summ["same_results"] = bool(same)
            summ["candidates"] = [len(r["cand_idx"]) for r in b_raw]
        out["sizes"][str(n)] = summ
        print(json.dumps({str(n): summ}), flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
