"""VERDICT r6 item 1(a), priced on the CPU: mask order INSIDE spatial super-tiles of S rows instead of one global mask order.
Bench scene 0 (make_scene(0, 80000, 0.03)), rows in the plan's order (level 0: stable sort by the Z-order key of the sort's
coarse cubes; a coarse level: first appearance of a child), three groups of nine offsets (group = dz plane, as the network runs
them), rows sorted by (row // S, 9-bit group mask); counted: live (32-row block, offset) units as a share of the 27 per block.
S = inf is today's global order (reproduces the 24.4 % / 42.3 % of profiles/conv_order_stats.py).  CPU only, seconds.
    python profiles/supertile_pricing.py > profiles/r7/supertile_pricing.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd.synth import make_scene  # noqa: E402

SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, None)


def spread3(x):
    r = np.zeros_like(x)
    for b in range(6):
        r |= ((x >> b) & 1) << (3 * b)
    return r


def plan_order(c):
    """cv_sp_sort_rows for one scene: stable sort by the Morton code of ((c - min) >> shift), extents under 64"""
    mn = c.min(0)
    ex = int((c.max(0) - mn).max())
    shift = 0
    while (ex >> shift) >= 64:
        shift += 1
    g = (c - mn) >> shift
    key = spread3(g[:, 0]) | (spread3(g[:, 1]) << 1) | (spread3(g[:, 2]) << 2)
    return c[np.argsort(key, kind="stable")]


def coarser(c, ts):
    """the next level (tensor stride 2 * ts) in first-appearance order of its children"""
    q = c & ~(2 * ts - 1)
    _, first = np.unique(pack(q), return_index=True)
    return q[np.sort(first)]


def pack(c):
    return ((c[:, 0] + 32768) << 40) | ((c[:, 1] + 32768) << 20) | (c[:, 2] + 32768)


def live_table(c, ts):
    """[n, 27] bool: does row i have a neighbour at offset j (first axis fastest, dz slowest)"""
    keys = pack(c)
    order = np.argsort(keys)
    sk = keys[order]
    live = np.zeros((len(c), 27), bool)
    j = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = pack(c + np.array([dx, dy, dz]) * ts)
                pos = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
                live[:, j] = sk[pos] == q
                j += 1
    return live


def units(live, S):
    n = len(live)
    tile = np.arange(n) // S if S else np.zeros(n, np.int64)
    nblk = (n + 31) // 32
    pad = nblk * 32 - n
    tot = 0
    for g in range(3):
        lv = live[:, 9 * g:9 * g + 9]
        mask = (lv * (1 << np.arange(9))).sum(1)
        o = np.lexsort((mask, tile))                       # stable: by tile, then by mask
        l2 = np.concatenate([lv[o], np.zeros((pad, 9), bool)])
        tot += int(l2.reshape(nblk, 32, 9).any(1).sum())
    return tot / (27.0 * nblk)


def main():
    sc = make_scene(0, n_points=80000, res=0.03)
    c = plan_order(np.asarray(sc.coords, np.int64))
    levels = [("ts1", c, 1)]
    c2 = coarser(c, 1)
    levels.append(("ts2", c2, 2))
    levels.append(("ts4", coarser(c2, 2), 4))
    print("live (32-row block, offset) units / (27 per block); three groups of nine offsets; sort key (row // S, group mask)")
    print("%-14s " % "S rows" + " ".join("%7s" % (s if s else "inf") for s in SIZES))
    res = {}
    for name, cc, ts in levels:
        live = live_table(cc, ts)
        res[name] = [units(live, s) for s in SIZES]
        print("%-14s " % ("%s (%d)" % (name, len(cc))) + " ".join("%7.3f" % u for u in res[name]))
    fit = SIZES.index(4096)
    print("\nts1: the partial sums (S x 96 x 4 B) and input rows of a super-tile fit a 4 MB XCD L2 for S <= 4096: %.2f x today's units"
          % (res["ts1"][fit] / res["ts1"][-1]))
    print("(pairs live: " + ", ".join("%s %.1f %%" % (n_, 100 * live_table(c_, t_).mean()) for n_, c_, t_ in levels) + ")")


if __name__ == "__main__":
    main()
