"""The share of a mask-sorted level's partial tiles that are all zeros, priced on the CPU.
bench.py's scenes (make_scene(seed, 80000, 0.03), seeds 0 and 1), rows in the plan's order, the dispatcher's three groups of
nine offsets (the dz planes), each group's rows sorted by the group's 9-bit mask (rows without a neighbour in the group first).
Counted per level: live (32-row block, offset) units as a share of 27 per block (what profiles/supertile_pricing.py prints for
S = inf), and the (group, block) pairs, 32 rows and 128- / 256-row tiles, in which NO row has a neighbour in the group - the
partial tiles that option "zskip" neither writes nor reads.  CPU only, seconds.
    python profiles/zero_tiles/dead_pairs.py > profiles/zero_tiles/dead_pairs.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from canonicalvoting_amd.synth import make_scene  # noqa: E402
from profiles.supertile_pricing import coarser, live_table, plan_order, units  # noqa: E402


def dead_share(live, rows_per_tile):
    """(group, tile) pairs without a live row / all pairs; the rows the pairs hold / 3 n"""
    n = len(live)
    nt = (n + rows_per_tile - 1) // rows_per_tile
    dead_tiles = dead_rows = 0
    for g in range(3):
        lv = live[:, 9 * g:9 * g + 9]
        mask = (lv * (1 << np.arange(9))).sum(1)
        has = np.sort(mask, kind="stable") != 0                    # the group's order: mask 0 first
        pad = np.concatenate([has, np.zeros(nt * rows_per_tile - n, bool)]).reshape(nt, rows_per_tile)
        d = ~pad.any(1)
        dead_tiles += int(d.sum())
        dead_rows += int(np.minimum(rows_per_tile, n - np.nonzero(d)[0] * rows_per_tile).sum()) if d.any() else 0
    return dead_tiles / (3.0 * nt), dead_rows / (3.0 * n)


def main():
    print("level  seed   rows   live units  dead (group, row) pairs  dead (group, tile) pairs of 32 / 128 / 256 rows   rows in dead 128-row tiles")
    for seed in (0, 1):
        sc = make_scene(seed, n_points=80000, res=0.03)
        c = plan_order(np.asarray(sc.coords, np.int64))
        c2 = coarser(c, 1)
        for name, cc, ts in (("ts1", c, 1), ("ts2", c2, 2), ("ts4", coarser(c2, 2), 4)):
            live = live_table(cc, ts)
            rows_dead = 1.0 - np.mean([live[:, 9 * g:9 * g + 9].any(1).mean() for g in range(3)])
            d32, d128, d256 = dead_share(live, 32), dead_share(live, 128), dead_share(live, 256)
            print("%-5s  %4d  %6d   %.3f       %5.1f %%                  %5.1f %% / %5.1f %% / %5.1f %%                             %5.1f %%"
                  % (name, seed, len(cc), units(live, None), 100 * rows_dead, 100 * d32[0], 100 * d128[0], 100 * d256[0], 100 * d128[1]))


if __name__ == "__main__":
    main()
