"""CPU pricing of the peaks vote: how much of hv_fwd_tiles' accumulation lands where the decode can read the rot / scale quotients.

    python profiles/vote_peaks/hot_pricing.py [seed ...]        (default: seeds 0-3, bench.py's scenes, teacher predictions)

Per scene: grid cells, in-bounds votes, cells with objectness >= thresh_high (CPU oracle), (plane, 16 x 32 tile) pairs that hold
such a cell, and the share of the (vote, corner) contributions that land in those pairs / in the bounding box of a pair's hot
cells / in the hot cells themselves."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle                                                      # noqa: E402
from canonicalvoting_amd import decode                             # noqa: E402
from canonicalvoting_amd.synth import make_scene, synth_predictions  # noqa: E402

TX, TZ, R = 16, 32, 120


def price(seed, thresh=float(decode.thresh_high)):
    sc = make_scene(seed)
    xyz, scale, prob, _ = synth_predictions(sc)
    pts = sc.points
    g_obj = oracle.hv_forward(pts, xyz, scale, prob, sc.res, R)[0]
    corner, _, _ = oracle.grid_geometry(pts, sc.res)
    X, Y, Z = g_obj.shape
    hot = g_obj >= thresh
    tx, tz = -(-X // TX), -(-Z // TZ)
    pad = np.zeros((tx * TX, Y, tz * TZ), bool)
    pad[:X, :, :Z] = hot
    pair_hot = pad.reshape(tx, TX, Y, tz, TZ).any((1, 4))                      # [tile x, plane, tile z]
    # bounding box of every pair's hot cells, as a cell mask
    box = np.zeros_like(pad)
    for a, y, b in zip(*np.nonzero(pair_hot)):
        sub = pad[a * TX:(a + 1) * TX, y, b * TZ:(b + 1) * TZ]
        xs, zs = np.nonzero(sub.any(1))[0], np.nonzero(sub.any(0))[0]
        box[a * TX + xs[0]:a * TX + xs[-1] + 1, y, b * TZ + zs[0]:b * TZ + zs[-1] + 1] = True
    in_pair = np.repeat(np.repeat(pair_hot, TX, 0), TZ, 2)
    # the votes, by the reference's fp32 sequence (positions only: the weights do not matter here)
    f = np.float32
    th = (np.arange(R, dtype=f) * f(2 * 3.141592654 / R)).astype(f)
    cs, sn = np.cos(th.astype(np.float64)).astype(f), np.sin(th.astype(np.float64)).astype(f)
    c = (xyz * scale).astype(f)
    res = f(sc.res)
    gx = ((pts[:, None, 0] + ((-cs)[None] * c[:, None, 0] + sn[None] * c[:, None, 2])) - f(corner[0])) / res
    gz = ((pts[:, None, 2] + ((-sn)[None] * c[:, None, 0] - cs[None] * c[:, None, 2])) - f(corner[2])) / res
    gy = np.broadcast_to((((pts[:, 1] - c[:, 1]) - f(corner[1])) / res)[:, None], gx.shape)
    ok = (gx >= 0) & (gy >= 0) & (gz >= 0) & (gx < X - 1) & (gy < Y - 1) & (gz < Z - 1)
    fx, fy, fz = gx[ok].astype(np.int64), gy[ok].astype(np.int64), gz[ok].astype(np.int64)
    n_pair = n_box = n_hot = 0
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                i = (fx + bx, fy + by, fz + bz)
                n_pair += int(in_pair[i].sum()); n_box += int(box[i].sum()); n_hot += int(pad[i].sum())
    tot = 8 * fx.size
    return dict(seed=seed, grid=(X, Y, Z), cells=X * Y * Z, votes=int(fx.size), hot_cells=int(hot.sum()), pairs=tx * tz * Y,
                hot_pairs=int(pair_hot.sum()), in_pairs=n_pair / tot, in_boxes=n_box / tot, in_hot_cells=n_hot / tot)


if __name__ == "__main__":
    oracle.build()
    for s in ([int(a) for a in sys.argv[1:]] or [0, 1, 2, 3]):
        r = price(s)
        print("seed %(seed)d  grid %(grid)s = %(cells)d cells  in-bounds votes %(votes)d  cells >= thresh %(hot_cells)d  "
              "(plane, tile) pairs with one %(hot_pairs)d of %(pairs)d  contributions in those pairs %(in_pairs).3f  "
              "in their hot boxes %(in_boxes).3f  in the hot cells %(in_hot_cells).3f" % r, flush=True)
