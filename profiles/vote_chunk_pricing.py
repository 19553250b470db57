"""How often does each block of hv_fwd_tiles (csrc/hv_vote.hip) run on the bench scenes, priced on the CPU: the per-wave
chunk loop of rounds 1-7 (a wave culls 64 records, expands the few it keeps, flushes its vote queue) against the
workgroup-wide survivor list of round 8 (cull everything into a list of 512, one survivor per lane for the arcs, all 512
lanes share the round's items, one flush per wave and round).

    python profiles/vote_chunk_pricing.py [seed ...]        (default: bench.py's scenes 0 and 1, 80 000 points, summed)

Inputs as the kernels form them: points = coords x 0.03, fy as hv_prep_count, (ux, uz, r, a0) as hv_prep_scatter, the
records of a bin in point order, 16 x 32-cell tiles, the streaming launch without the part split.  Every bin s < Y - 1 is
counted twice: planes s and s + 1 both stream it.  Static VALU instruction counts per block (gfx950, the flags of
csrc/build.py, hv_fwd_tiles<0, false> of round 7): ring test of a chunk ~50, arc block 225, compaction + scan + search ~160,
one expansion step ~75, one drain64 on the fast path ~205.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canonicalvoting_amd.synth import make_scene, synth_predictions  # noqa: E402

f32 = np.float32
R, RES, TX, TZ, LQ, TW = 120, f32(0.03), 16, 32, 512, 8
COST = dict(cull=50, arc=225, scan=160, step=75, drain=205)


def arc_atan2(y, x):
    """csrc/hv_vote.hip arc_atan2, in fp32"""
    ax, ay = np.abs(x), np.abs(y)
    a = (np.minimum(ax, ay) / np.maximum(np.maximum(ax, ay), f32(1e-30))).astype(f32)
    q = a * a
    r = ((f32(-0.0464964749) * q + f32(0.15931422)) * q - f32(0.327622764)) * q * a + a
    r = np.where(ay > ax, f32(1.57079637) - r, r)
    r = np.where(x < 0, f32(3.14159274) - r, r)
    return np.where(y < 0, -r, r).astype(f32)


def scene_counts(seed, n_points=80000):
    sc = make_scene(seed, n_points=n_points)
    xyz, scale, prob, _ = synth_predictions(sc)
    pts = sc.points.astype(f32)
    corner = pts.min(0)
    X, Y, Z = (int(v) for v in (np.trunc((pts.max(0) - corner) / RES) + 1))
    c = (xyz * scale).astype(f32)
    gy = ((pts[:, 1] - c[:, 1] - corner[1]) / RES).astype(f32)
    fy = np.where((gy >= 0) & (gy < Y - 1), gy.astype(np.int64), -1)
    ux, uz = ((pts[:, 0] - corner[0]) / RES).astype(f32), ((pts[:, 2] - corner[2]) / RES).astype(f32)
    rad = (np.sqrt(c[:, 0] * c[:, 0] + c[:, 2] * c[:, 2]) / RES).astype(f32)
    a0 = (np.arctan2(c[:, 2], c[:, 0]).astype(f32) + f32(3.14159265)).astype(f32)
    theta = (np.arange(R, dtype=f32) * f32(2 * 3.141592654 / R)).astype(f32)
    cs, sn = np.cos(theta.astype(np.float64)).astype(f32), np.sin(theta.astype(np.float64)).astype(f32)
    tiles_x, tiles_z = -(-X // TX), -(-Z // TZ)
    inv_step = f32(R) * f32(0.159154943)
    # per (bin, tile): kept records (in bin order), their arc lengths and in-tile votes
    per_bin_tile = {}
    for s in range(Y - 1):
        idx = np.flatnonzero(fy == s)
        if not len(idx):
            continue
        bux, buz, br, ba0 = ux[idx], uz[idx], rad[idx], a0[idx]
        ox = ((-cs[None]) * c[idx, 0:1] + sn[None] * c[idx, 2:3]).astype(f32)
        oz = ((-sn[None]) * c[idx, 0:1] - cs[None] * c[idx, 2:3]).astype(f32)
        gx = (((pts[idx, 0:1] + ox) - corner[0]) / RES).astype(f32)
        gz = (((pts[idx, 2:3] + oz) - corner[2]) / RES).astype(f32)
        inb = (gx >= 0) & (gz >= 0) & (gx < X - 1) & (gz < Z - 1)
        lxa, lza = gx.astype(np.int64), gz.astype(np.int64)
        for tx in range(tiles_x):
            for tz in range(tiles_z):
                x0, z0 = tx * TX, tz * TZ
                xlo, xhi, zlo, zhi = f32(x0 - 1), f32(x0 + TX), f32(z0 - 1), f32(z0 + TZ)
                dxn = np.maximum(f32(0), np.maximum(xlo - bux, bux - xhi))
                dzn = np.maximum(f32(0), np.maximum(zlo - buz, buz - zhi))
                dxf = np.maximum(np.abs(bux - xlo), np.abs(bux - xhi))
                dzf = np.maximum(np.abs(buz - zlo), np.abs(buz - zhi))
                dmin, dmax = np.sqrt(dxn * dxn + dzn * dzn), np.sqrt(dxf * dxf + dzf * dzf)
                tol = f32(0.05) + f32(1e-5) * (br + np.abs(bux) + np.abs(buz))
                keep = (br >= dmin - tol) & (br <= dmax + tol)
                k = np.flatnonzero(keep)
                nchunks = -(-len(idx) // 64)
                if not len(k):
                    per_bin_tile[(s, tx, tz)] = (nchunks, k, np.zeros(0, np.int64), np.zeros(0, np.int64))
                    continue
                kx, kz = bux[k], buz[k]
                b0 = arc_atan2(f32(0.5) * (zlo + zhi) - kz, f32(0.5) * (xlo + xhi) - kx)
                lo, hi = np.zeros(len(k), f32), np.zeros(len(k), f32)
                for q in range(4):
                    d = arc_atan2((zhi if q & 2 else zlo) - kz, (xhi if q & 1 else xlo) - kx) - b0
                    d = (d - f32(6.28318531) * np.rint(d * f32(0.159154943))).astype(f32)
                    lo, hi = np.minimum(lo, d), np.maximum(hi, d)
                first = ((b0 + lo - ba0[k]) * inv_step - f32(2)).astype(f32)
                ln = ((hi - lo) * inv_step).astype(np.int64) + 6
                first = (first - f32(R) * np.floor(first / f32(R))).astype(f32)
                a_start = np.clip(first.astype(np.int64), 0, R - 1)
                a_len = np.minimum(ln, R)
                full = ~(dxn[k] + dzn[k] > f32(0.5))
                a_start[full], a_len[full] = 0, R
                # in-tile votes along each arc
                rot = (a_start[:, None] + np.arange(R)[None]) % R
                on = np.arange(R)[None] < a_len[:, None]
                rows = k[:, None]
                lx, lz = lxa[rows, rot] - x0, lza[rows, rot] - z0
                vote = on & inb[rows, rot] & (lx >= -1) & (lx < TX) & (lz >= -1) & (lz < TZ)
                # the tightest single interval of rotations that holds every in-tile vote of the record (+ 2 steps of slack
                # per side; nothing for a record without one): the floor under any conservative one-interval arc
                allv = inb[k] & (lxa[k] - x0 >= -1) & (lxa[k] - x0 < TX) & (lza[k] - z0 >= -1) & (lza[k] - z0 < TZ)
                v2 = np.concatenate([allv, allv], 1)
                pos = np.arange(2 * R)[None]
                gap = (pos - np.maximum.accumulate(np.where(v2, pos, -1), 1)).max(1)          # longest run without a vote
                tight = np.where(allv.any(1), np.minimum(R - np.minimum(gap, R) + 4, R), 0)
                # candidate: the ring leaves the rectangle across an edge line at distance d < r from its centre for the angles
                # within acos(d / r) of the edge's outward normal; the complement of the LARGEST of the four outside arcs is one
                # conservative interval; take it where it is shorter than today's
                kr = np.maximum(br[k], f32(1e-6))
                dist = np.stack([xhi - kx, kx - xlo, zhi - kz, kz - zlo], 1) / kr[:, None]
                h = np.arccos(np.clip(dist, -1, 1)).max(1)
                edge = np.minimum(((2 * np.pi - 2 * h) * inv_step).astype(np.int64) + 6, R)
                cand = np.minimum(a_len, edge)
                # candidate 2: the complement of the longest run of the UNION of the four outside arcs (what merging the four
                # intervals gives), evaluated on 1440 sample angles
                ang = (np.arange(1440) * (2 * np.pi / 1440))[None]
                qx, qz = kx[:, None] + kr[:, None] * np.cos(ang), kz[:, None] + kr[:, None] * np.sin(ang)
                outside = (qx < xlo) | (qx > xhi) | (qz < zlo) | (qz > zhi)
                o2 = np.concatenate([outside, outside], 1)
                p2 = np.arange(2880)[None]
                run = np.minimum((p2 - np.maximum.accumulate(np.where(~o2, p2, -1), 1)).max(1), 1440)
                union = np.minimum(((1440 - run) * (2 * np.pi / 1440) * inv_step).astype(np.int64) + 6, R)
                cand2 = np.minimum(a_len, union)
                per_bin_tile[(s, tx, tz)] = (nchunks, k, a_len, vote.sum(1), vote, on, tight, cand, cand2)
    return Y, tiles_x, tiles_z, per_bin_tile


def price(seeds):
    old = dict(chunks=0, live=0, surv=0, items=0, votes=0, steps=0, full=0, flush=0, flush_lanes=0, tight=0, full_arcs=0,
               full_arc_items=0)
    hist = np.zeros(65, np.int64)
    new = dict(chunks=0, wgs=0, rounds=0, arc_passes=0, surv=0, items=0, votes=0, steps=0, full=0, flush=0, flush_lanes=0)
    for seed in seeds:
        Y, tiles_x, tiles_z, pbt = scene_counts(seed)
        for (s, tx, tz), v in pbt.items():
            nchunks, k = v[0], v[1]
            old["chunks"] += 2 * nchunks
            if not len(k):
                continue
            a_len, votes = v[2], v[3]
            ch = k // 64
            nq = np.bincount(ch, minlength=nchunks)
            items = np.bincount(ch, weights=a_len, minlength=nchunks).astype(np.int64)
            vv = np.bincount(ch, weights=votes, minlength=nchunks).astype(np.int64)
            live = nq > 0
            old["live"] += 2 * int(live.sum())
            old["surv"] += 2 * int(nq.sum())
            hist += 2 * np.bincount(nq[live], minlength=65)
            old["items"] += 2 * int(items.sum())
            old["tight"] += 2 * int(v[6].sum())
            old["cand"] = old.get("cand", 0) + 2 * int(v[7].sum())
            old["cand2"] = old.get("cand2", 0) + 2 * int(v[8].sum())
            old["full_arcs"] += 2 * int((a_len == R).sum())
            old["full_arc_items"] += 2 * int(a_len[a_len == R].sum())
            old["votes"] += 2 * int(vv.sum())
            old["steps"] += 2 * int((-(-items // 64)).sum())
            old["full"] += 2 * int((vv // 64).sum())
            old["flush"] += 2 * int((vv % 64 > 0).sum())
            old["flush_lanes"] += 2 * int((vv % 64).sum())
        # the new loop: survivors of bins y - 1 and y pooled per (tile, plane)
        for y in range(Y):
            for tx in range(tiles_x):
                for tz in range(tiles_z):
                    parts = [pbt[(s, tx, tz)] for s in (y - 1, y) if (s, tx, tz) in pbt]
                    if not parts:
                        continue
                    new["wgs"] += 1
                    new["chunks"] += sum(p[0] for p in parts)
                    parts = [p for p in parts if len(p[1])]
                    if not parts:
                        continue
                    a_len = np.concatenate([p[2] for p in parts])
                    vote = np.concatenate([p[4] for p in parts])
                    on = np.concatenate([p[5] for p in parts])
                    new["surv"] += len(a_len)
                    for r0 in range(0, len(a_len), LQ):
                        al, vo, o = a_len[r0:r0 + LQ], vote[r0:r0 + LQ], on[r0:r0 + LQ]
                        items = int(al.sum())
                        S = -(-items // LQ)
                        new["rounds"] += 1
                        new["arc_passes"] += -(-len(al) // 64)
                        new["items"] += items
                        new["steps"] += TW * S                                  # wave-steps: every wave runs S steps
                        # votes per wave: contiguous slices, item i belongs to lane i // S, wave (i // S) // 64
                        flat = vo[o]                                             # the round's items in list order
                        wave = (np.arange(items) // S) // 64
                        vw = np.bincount(wave, weights=flat, minlength=TW).astype(np.int64)
                        new["votes"] += int(vw.sum())
                        new["full"] += int((vw // 64).sum())
                        new["flush"] += int((vw % 64 > 0).sum())
                        new["flush_lanes"] += int((vw % 64).sum())
    return old, hist, new


if __name__ == "__main__":
    seeds = [int(a) for a in sys.argv[1:]] or [0, 1]
    old, hist, new = price(seeds)
    # per launch: the mean over the scenes
    old = {k: v / len(seeds) for k, v in old.items()}
    new = {k: v / len(seeds) for k, v in new.items()}
    print("seeds %s (every count below is per launch: the mean over these scenes), %d rotations, %d x %d-cell tiles" % (
        seeds, R, TX, TZ))
    print("\n== per-wave chunk loop (rounds 1-7)")
    print("chunk iterations %.0f, with survivors %.0f (%.1f%%), survivors per live chunk %.2f" % (
        old["chunks"], old["live"], 100.0 * old["live"] / old["chunks"], old["surv"] / old["live"]))
    cum = np.cumsum(hist) / hist.sum()
    print("live chunks keeping <= 4: %.0f%%, <= 16: %.0f%%, arc-block lane efficiency %.1f%%" % (
        100 * cum[4], 100 * cum[16], 100.0 * old["surv"] / (64 * old["live"])))
    print("arc items %.0f, in-tile (vote, plane, tile) entries %.0f, items per entry %.2f" % (
        old["items"], old["votes"], old["items"] / old["votes"]))
    print("expansion steps %.0f, full drains %.0f, flush drains %.0f (mean %.1f active lanes)" % (
        old["steps"], old["full"], old["flush"], old["flush_lanes"] / max(1, old["flush"])))
    rows = [("cull test", old["chunks"], COST["cull"]), ("arc block", old["live"], COST["arc"]),
            ("compaction, scan, search", old["live"], COST["scan"]), ("expansion", old["steps"], COST["step"]),
            ("drains", old["full"] + old["flush"], COST["drain"])]
    tot_old = sum(n * c for _, n, c in rows)
    for name, n, c in rows:
        print("  %-26s %9.0f x %3d = %.2e" % (name, n, c, n * c))
    print("  total (without the prologue and epilogue of the waves, ~1e7): %.3e wave-instructions" % tot_old)
    print("\n== workgroup-wide survivor list (round 8): rounds of %d entries, %d lanes per step, %d flushes per round" % (LQ, LQ, TW))
    print("workgroups %.0f, chunk culls %.0f, rounds %.0f (%.2f per workgroup), survivors %.0f" % (
        new["wgs"], new["chunks"], new["rounds"], new["rounds"] / max(1, new["wgs"]), new["surv"]))
    print("arc passes of one wave %.0f, arc items %.0f, in-tile entries %.0f" % (new["arc_passes"], new["items"], new["votes"]))
    print("expansion wave-steps %.0f, full drains %.0f, flush drains %.0f (mean %.1f active lanes)" % (
        new["steps"], new["full"], new["flush"], new["flush_lanes"] / max(1, new["flush"])))
    rows = [("cull test", new["chunks"], COST["cull"]), ("arc block", new["arc_passes"], COST["arc"]),
            ("scan, search (8 waves a round)", TW * new["rounds"], COST["scan"]), ("expansion", new["steps"], COST["step"]),
            ("drains", new["full"] + new["flush"], COST["drain"])]
    tot_new = sum(n * c for _, n, c in rows)
    for name, n, c in rows:
        print("  %-30s %9.0f x %3d = %.2e" % (name, n, c, n * c))
    print("  total: %.3e wave-instructions, %.2f of the chunk loop's (%.2f with 1e7 of prologue and epilogue on both)" % (
        tot_new, tot_new / tot_old, (tot_new + 1e7) / (tot_old + 1e7)))
    print("\n== tighter arcs, priced")
    print("records that get all %d rotations (centre in or within half a cell of the rectangle): %.0f of %.0f survivors, %.1f%% of the arc items" % (
        R, old["full_arcs"], old["surv"], 100.0 * old["full_arc_items"] / old["items"]))
    print("the tightest single interval per record (+ 2 steps of slack per side, none for a record without an in-tile vote): "
          "%.0f items, %.2f per entry (the corner arc %.2f; a tighter arc was to be built at <= 1.8)" % (
              old["tight"], old["tight"] / old["votes"], old["items"] / old["votes"]))
    print("candidate (complement of the largest arc the ring spends beyond one edge line, where shorter than today's arc): "
          "%.0f items, %.2f per entry" % (old["cand"], old["cand"] / old["votes"]))
    print("candidate 2 (complement of the longest run of the union of the four outside arcs): %.0f items, %.2f per entry" % (
        old["cand2"], old["cand2"] / old["votes"]))
