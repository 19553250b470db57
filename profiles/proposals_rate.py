"""SUN RGB-D proposal sampler: the torch transliteration (HoughVotingModule.forward) against the device path (propose), and
the caller's per-batch loop (brnetcanon.py:213-249 on the call-by-call functions) against proposals.propose_clouds.

    python profiles/proposals_rate.py                  # writes profiles/proposals/propose_rate.txt
    python profiles/proposals_rate.py --one propose    # 20 samples of one path and nothing else: the target of a separate
                                                       #   rocprofv3 --kernel-trace --stats run (launches per sample)

Per sample: P = 512, 60 rotations, a 20 000-point cloud, 1024 seed votes.  Per batch: 8 clouds of 20 000 points through a
MinkUNet34C(3, 8) with random weights.  Wall milliseconds over three alternated repeats; host waits as torch's own
synchronisation check counts them (it sees .item(), masked gathers, blocking copies; the event waits of the library are
added by hand where the text says so).  No speed bar: a few launches on 10^4-cell maps, bound by launch latency."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from canonicalvoting_amd import me as ME, proposals                     # noqa: E402
from canonicalvoting_amd.me import utils as ME_utils                    # noqa: E402
from canonicalvoting_amd.minkunet import MinkUNet34C                    # noqa: E402
from canonicalvoting_amd.pipeline import head_separate                  # noqa: E402
from canonicalvoting_amd.proposals import HoughVotingModule             # noqa: E402
from canonicalvoting_amd.synth import make_scene, synth_predictions     # noqa: E402

DEV = torch.device("cuda:0")
P, ROTS, RES, N_POINTS, N_VOTES = 512, 60, 0.05, 20000, 1024


def sample_inputs(seed):
    sc = make_scene(seed, n_points=N_POINTS, res=RES, room=(4.0, 2.4, 4.0), n_boxes=5)
    xyz, scale, prob, _ = synth_predictions(sc)
    pts = sc.points.astype(np.float32)
    corners = np.stack([pts.min(0), pts.max(0)]).astype(np.float32)
    rng = np.random.default_rng(seed)
    votes = (pts[rng.choice(len(pts), N_VOTES, replace=False)] + rng.normal(0, 0.05, (N_VOTES, 3))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (t(pts), t(xyz), t(scale), t(prob)), torch.from_numpy(corners), t(votes)


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def torch_syncs(fn):
    """host waits torch's synchronisation check reports during one call"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def batch_by_calls(model, hv, clouds, votes, q=0.03):
    """brnetcanon.py:213-249 on the call-by-call functions"""
    with torch.no_grad():
        coords, feats = [], []
        for pc in clouds:
            coord, feat = ME_utils.sparse_quantize(pc, features=pc, quantization_size=q, device="cuda")
            coords.append(coord.float())
            feats.append(feat)
        x = ME.SparseTensor(torch.cat(feats), ME_utils.batched_coordinates(coords), device="cuda")
        cs, fs = model(x).decomposed_coordinates_and_features
        out = []
        for coord, feat, vote in zip(cs, fs, votes):
            xyz, scale, prob = feat[..., :3], torch.exp(feat[..., 3:6]), torch.softmax(feat[..., 6:], dim=-1)[..., 1]
            pc = coord * q
            corner = torch.stack([torch.min(pc, 0)[0], torch.max(pc, 0)[0]])
            out.append(hv.forward(pc, xyz, scale, prob, corner, vote, pow=0.5))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=["forward", "propose"], help="run 20 samples of one path only (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    hv = HoughVotingModule(res=RES, nms_size=0.3, thresh=0, num_proposal=P, num_rots=ROTS)
    args, corners, votes = sample_inputs(5)
    corners_d = corners.to(DEV)
    fwd = lambda: hv.forward(*args, corners_d, votes)
    prop = lambda: hv.propose(*args, corners, votes)
    if a.one:
        fn = fwd if a.one == "forward" else prop
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    lines = ["proposal sampler: P = %d, %d rotations, %d points, %d seed votes, %s" % (P, ROTS, N_POINTS, N_VOTES,
                                                                                        torch.cuda.get_device_name(0))]
    for f in (fwd, prop):
        for _ in range(5):
            f()
    lines.append("per sample, wall ms (mean of %d calls), three alternated repeats" % a.reps)
    for r in range(3):
        lines.append("  repeat %d: forward %.3f   propose %.3f" % (r, wall_ms(fwd, a.reps), wall_ms(prop, a.reps)))
    lines.append("per sample, host waits torch's check reports: forward %d, propose %d (+ 1 event wait of its own)"
                 % (torch_syncs(fwd), torch_syncs(prop)))
    used = []
    g = torch.Generator(device=DEV)
    for seed in range(100):
        g.manual_seed(seed)
        if seed % 25 == 0:
            args_s, corners_s, votes_s = sample_inputs(20 + seed // 25)
        hv.propose(*args_s, corners_s, votes_s, generator=g)
        used += hv.last_rounds_used
    lines.append("rounds_used over 100 samples (4 scenes x 25 generator seeds, budget 4): " +
                 ", ".join("%d x %d" % (used.count(k), k) for k in sorted(set(used))))
    # the batch of 8
    torch.manual_seed(0)
    model = MinkUNet34C(3, 8).to(DEV).eval()
    rng = np.random.default_rng(3)
    clouds, bvotes = [], []
    for b in range(8):
        sc = make_scene(40 + b, n_points=N_POINTS, res=0.03, room=(4.0, 2.4, 4.0), n_boxes=5)
        pts = sc.points.astype(np.float32)
        clouds.append(torch.from_numpy(pts).to(DEV))
        bvotes.append(torch.from_numpy((pts[rng.choice(len(pts), N_VOTES, replace=False)]
                                        + rng.normal(0, 0.05, (N_VOTES, 3))).astype(np.float32)).to(DEV))
    calls = lambda: batch_by_calls(model, hv, clouds, bvotes)
    batch = lambda: proposals.propose_clouds(model, hv, clouds, bvotes)
    for f in (calls, batch):
        for _ in range(3):
            f()
    lines.append("per batch of 8 clouds (voxelise, network, head, sampler), wall ms (mean of 5 calls), three alternated repeats")
    for r in range(3):
        lines.append("  repeat %d: call-by-call loop %.2f   propose_clouds %.2f" % (r, wall_ms(calls, 5), wall_ms(batch, 5)))
    lines.append("per batch, host waits torch's check reports: loop %d, propose_clouds %d (+ its 3 event / C-side waits and the "
                 "network plan's)" % (torch_syncs(calls), torch_syncs(batch)))
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.path.join(ROOT, "profiles", "proposals")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "propose_rate.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
