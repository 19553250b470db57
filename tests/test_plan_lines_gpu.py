"""The level-0 maps of cv_sp_scene_plan are built line by line from the occupancy bitmap (sparse_coords.hip: line_job; one
lane reads the five z-bits of a (dx, dy) line and probes the table for the set ones; the 5x5x5 stem map, the 3x3x3 map and the
27 validity bits of every row come out of the same pass) whenever the bitmap exists and may be trusted; otherwise the same job
does the per-entry lookups.  Everything here is integer work and must be EQUAL to the per-entry path:

  * cv_sp_kernel_map (one thread per (row, offset), hash probes only: no bitmap, no lines; pinned against the oracle by
    tests/test_sparse_gpu.py and test_production_size_gpu.py) on the same sorted set and table, and
  * cv_sp_scene_maps on the same levels (the same job without a bitmap: the per-entry fallback, decided on the device).

The mask orders built from the validity words (mp_hist_batch / mp_scatter_batch) are checked for what a consumer relies on:
a permutation, the group key non-decreasing along it, the map rows copied in processing order, the validity bytes."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib
from canonicalvoting_amd.synth import make_scene

BITMAP_BITS = (1 << 20) * 32          # CV_BITMAP_WORDS * 32 (csrc/cv_common.h)
G = 3                                 # mask groups of the fused network (groups of nine offsets = dz planes)
NL = 5
up64 = lambda v: (v + 63) // 64 * 64


def expected_plan_words(n, stem_k, groups, mmr):
    """scene_maps_layout (csrc/net_exec.cpp) with every level at n rows: each item rounded up to 64 words"""
    mp_w = groups * (1 + (27 + groups - 1) // groups) + (groups + 3) // 4 if groups > 1 else 0
    masked = groups > 1 and n >= mmr
    items = [n * stem_k ** 3, n * 28] + ([mp_w * n] if masked else []) + [(5 * max(groups, 1) + 4) * 2048, 1 << 20]
    items += [n * 8] * 4 + [n * 28] * 4 + [n * 8] * 4 + ([mp_w * n] * 4 if masked else []) + [n] * 4
    return sum(up64(w) for w in items)


@pytest.mark.parametrize("n,stem_k,groups,mmr", [(80000, 5, 3, 16384), (80000, 5, 4, 16384), (1000, 5, 3, 16384), (77, 3, 0, 1),
                                                 (300001, 5, 3, 1)])
def test_scene_plan_words_follow_the_layout_with_validity_words(built_lib, n, stem_k, groups, mmr):
    """every 3x3x3 map [rows][27] is followed by rows validity words: 28 words per row and level"""
    L = _lib.lib()
    assert int(L.cv_sp_scene_plan_words(n, stem_k, groups, mmr)) == expected_plan_words(n, stem_k, groups, mmr)
    rows = (ctypes.c_int64 * 5)(n, n // 2 + 1, n // 8 + 1, n // 30 + 1, n // 100 + 1)
    off = _lib.SceneMaps()
    words = int(L.cv_sp_scene_maps_words(rows, n, stem_k, groups, mmr, ctypes.byref(off)))
    starts = sorted([off.stem, off.scratch, off.bitmap] + list(off.down) + list(off.k3) + list(off.up) + list(off.up_perm) +
                    [m for m in off.mask_perm if m >= 0] + [words])
    for i in range(5):
        nxt = starts[starts.index(off.k3[i]) + 1]
        assert off.k3[i] % 64 == 0 and off.k3[i] + 28 * rows[i] <= nxt       # the map and its validity words fit in front
    assert words <= int(L.cv_sp_scene_plan_words(n, stem_k, groups, mmr))


# ---------------------------------------------------------------------------------------------------------------------
def run_plan(coords, dev, mmr):
    """cv_sp_scene_plan on int [N, 4] coordinates -> dict of device tensors (views of the plan's buffers)"""
    L = _lib.lib()
    vp = ctypes.c_void_p
    c = torch.from_numpy(np.ascontiguousarray(coords)).to(dev, torch.int32).contiguous()
    n = c.shape[0]
    cap = int(L.cv_sp_table_capacity(n))
    words = int(L.cv_sp_scene_plan_words(n, 5, G, mmr))
    o_perm, o_inv = 0, up64(n)
    o_coords = [o_inv + up64(n) + i * up64(4 * n) for i in range(NL)]
    o_vals = [o_coords[-1] + up64(4 * n) + i * up64(cap) for i in range(NL)]
    o_counts = o_vals[-1] + up64(cap)
    o_arena = o_counts + 64
    lay = _lib.ScenePlanLayout()          # the library's definition of the same layout (this test keeps its own restatement)
    assert L.cv_sp_scene_plan_layout(n, 5, G, mmr, ctypes.byref(lay)) == 0
    assert (lay.cap, lay.perm, lay.inv, list(lay.coords), list(lay.vals), lay.counts, lay.arena, lay.int_words, lay.key_words) == \
           (cap, o_perm, o_inv, o_coords, o_vals, o_counts, o_arena, o_arena + words, NL * cap)
    ibuf = torch.full((o_arena + words,), -77, dtype=torch.int32, device=dev)
    kbuf = torch.empty(NL * cap, dtype=torch.int64, device=dev)
    sws_b, lws_b = int(L.cv_sp_sort_workspace_bytes(n)), int(L.cv_sp_levels_workspace_bytes(n))
    wbuf = torch.empty(up64(sws_b) + lws_b, dtype=torch.uint8, device=dev)
    ib, kb, wb = ibuf.data_ptr(), kbuf.data_ptr(), wbuf.data_ptr()
    c_coords = (vp * NL)(*[ib + 4 * o for o in o_coords])
    c_keys = (vp * NL)(*[kb + 8 * cap * i for i in range(NL)])
    c_vals = (vp * NL)(*[ib + 4 * o for o in o_vals])
    counts_h = (ctypes.c_int32 * 8)()
    off = _lib.SceneMaps()
    st = vp(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(L.cv_sp_scene_plan(vp(c.data_ptr()), n, vp(ib + 4 * o_perm), vp(ib + 4 * o_inv), c_coords, c_keys, c_vals, cap,
                                      vp(ib + 4 * o_counts), counts_h, 5, G, mmr, vp(ib + 4 * o_arena), words, ctypes.byref(off),
                                      vp(wb), sws_b, vp(wb + up64(sws_b)), lws_b, st), "cv_sp_scene_plan")
        torch.cuda.synchronize()
    counts = [int(counts_h[i]) for i in range(8)]
    rejected = counts[5] != 0 or counts[6] != 0
    if rejected:         # nothing beyond the level-0 maps was built and *offsets was not written: the level-0 offsets depend on n only
        rows = (ctypes.c_int64 * 5)(n, 1, 1, 1, 1)
        L.cv_sp_scene_maps_words(rows, n, 5, G, mmr, ctypes.byref(off))
    arena = ibuf[o_arena:]
    p = dict(input=c, n=n, cap=cap, counts=counts, rejected=rejected, off=off, arena=arena, keep=(ibuf, kbuf, wbuf),
             perm=ibuf[o_perm:o_perm + n], sorted=ibuf[o_coords[0]:o_coords[0] + 4 * n].view(n, 4),
             c_coords=c_coords, c_keys=c_keys, c_vals=c_vals, vals0=ibuf[o_vals[0]:o_vals[0] + cap], keys0=kbuf[:cap],
             words=words, mmr=mmr)
    p["stem"] = arena[off.stem:off.stem + n * 125].view(n, 125)
    rows = [n] + ([1] * 4 if rejected else counts[1:5])
    p["rows"] = rows
    p["k3"] = [arena[off.k3[i]:off.k3[i] + rows[i] * 27].view(rows[i], 27) for i in range(NL)]
    p["mw"] = [arena[off.k3[i] + rows[i] * 27:off.k3[i] + rows[i] * 28] for i in range(NL)]
    return p


def per_entry_maps(p, dev):
    """5x5x5 and 3x3x3 map of the plan's sorted level-0 set by cv_sp_kernel_map: per-entry hash probes against the plan's table"""
    L = _lib.lib()
    n = p["n"]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    srt = p["sorted"].contiguous()
    for k in (5, 3):
        m = torch.empty((n, k ** 3), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.cv_sp_kernel_map(srt.data_ptr(), n, p["keys0"].data_ptr(), p["vals0"].data_ptr(), p["cap"], k, 1,
                                          m.data_ptr(), st), "cv_sp_kernel_map")
        out.append(m)
    torch.cuda.synchronize()
    k5, k3 = out
    stem = torch.where(k5 >= 0, p["perm"][k5.clamp_min(0).long()], k5)       # the sort permutation folded in
    return stem, k3


def step_by_step_maps(p, dev):
    """cv_sp_scene_maps over the plan's own levels: the same jobs WITHOUT a bitmap (per-entry lookups, chosen on the device)"""
    L = _lib.lib()
    vp = ctypes.c_void_p
    rows = (ctypes.c_int64 * 5)(*p["rows"])
    off = _lib.SceneMaps()
    words = int(L.cv_sp_scene_maps_words(rows, p["n"], 5, G, p["mmr"], ctypes.byref(off)))
    arena = torch.full((words,), -77, dtype=torch.int32, device=dev)
    st = vp(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(L.cv_sp_scene_maps(p["c_coords"], p["c_keys"], p["c_vals"], p["cap"], rows, vp(p["perm"].data_ptr()), p["n"], 5, G,
                                      p["mmr"], vp(arena.data_ptr()), words, st), "cv_sp_scene_maps")
        torch.cuda.synchronize()
    return arena, off


def words_from_map(k3):
    """validity word of every row recomputed on the host: bit j = entry j >= 0"""
    return ((k3.cpu().numpy() >= 0).astype(np.int64) << np.arange(27)).sum(1).astype(np.int32)


def check_mask_orders(arena, off, level, rows, k3):
    """orders [G][rows], map rows in processing order [G][rows][9], validity bytes [G][rows] of one level"""
    W = 9
    base = off.mask_perm[level]
    assert base >= 0
    a = arena[base:base + rows * (G * (1 + W)) + (G * rows + 3) // 4].cpu().numpy()
    perm = a[:G * rows].reshape(G, rows)
    nbrp = a[G * rows:G * rows * (1 + W)].reshape(G, rows, W)
    gv = a[G * rows * (1 + W):].view(np.uint8)[:G * rows].reshape(G, rows)
    nbr = k3.cpu().numpy()
    for g in range(G):
        jb, je = 27 * g // G, 27 * (g + 1) // G
        assert np.array_equal(np.sort(perm[g]), np.arange(rows)), (level, g)             # a permutation of the rows
        key = ((nbr[:, jb:je] >= 0) * (1 << np.arange(je - jb))).sum(1)                  # nine offsets: no popcount term
        assert (np.diff(key[perm[g]]) >= 0).all(), (level, g)                            # the group key never decreases
        assert np.array_equal(nbrp[g], nbr[perm[g], jb:je]), (level, g)                  # map rows in processing order
        assert np.array_equal(gv[g], (key != 0).astype(np.uint8)), (level, g)            # "has a neighbour in the group"


def box_cells(coords):
    c = np.asarray(coords, np.int64)
    ext = c[:, 1:].max(0) - c[:, 1:].min(0) + 1
    return int(ext.prod()) * int(c[:, 0].max() + 1), ext


def synth_coords(seeds, n):
    cs = []
    for b, seed in enumerate(seeds):
        sc = make_scene(seed, n_points=n, res=0.03) if n <= 100000 else \
            make_scene(seed, n_points=n, res=0.03, room=(9.0, 3.0, 9.0), n_boxes=40)
        xyz = np.asarray(sc.coords, np.int64)
        if len(seeds) > 1:              # scenes of a batch share one box: bring them together (each scene has its own origin shift)
            xyz = xyz - xyz.min(0) + 3 * b
        cs.append(np.concatenate([np.full((n, 1), b, np.int64), xyz], 1))
    return np.concatenate(cs)


def dense_box_coords(seed, ext, fill, batches=1, shift=(-11, 5, -3)):
    """random voxels of a small box filled to `fill`, its eight corners and the centres of its six faces included: rows on
    every face, so that lines leave the box in x, y and z, with neighbours next to them"""
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(batches):
        occ = rng.random(ext) < fill
        for ix in (0, ext[0] - 1):
            for iy in (0, ext[1] - 1):
                for iz in (0, ext[2] - 1):
                    occ[ix, iy, iz] = True
        for ax in range(3):
            for side in (0, ext[ax] - 1):
                idx = [e // 2 for e in ext]
                idx[ax] = side
                occ[tuple(idx)] = True
        xyz = np.argwhere(occ).astype(np.int64) + np.asarray(shift)
        cs.append(np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], 1))
    c = np.concatenate(cs)
    return c[rng.permutation(len(c))]


def compare_with_per_entry(p, dev, coarse=True):
    stem_ref, k3_ref = per_entry_maps(p, dev)
    assert torch.equal(p["stem"], stem_ref)
    assert torch.equal(p["k3"][0], k3_ref)
    assert np.array_equal(p["mw"][0].cpu().numpy(), words_from_map(k3_ref))
    if p["rejected"]:
        return
    arena2, off2 = step_by_step_maps(p, dev)
    n = p["n"]
    assert torch.equal(arena2[off2.stem:off2.stem + n * 125].view(n, 125), p["stem"])
    for i in range(NL if coarse else 1):
        r = p["rows"][i]
        k3_2 = arena2[off2.k3[i]:off2.k3[i] + r * 27].view(r, 27)
        assert torch.equal(k3_2, p["k3"][i]), i
        if i == 0 or p["off"].mask_perm[i] >= 0:                      # validity words: level 0 and the mask-sorted levels
            host = words_from_map(p["k3"][i])
            assert np.array_equal(p["mw"][i].cpu().numpy(), host), i
            assert np.array_equal(arena2[off2.k3[i] + r * 27:off2.k3[i] + r * 28].cpu().numpy(), host), i
    for arena, off in ((p["arena"], p["off"]), (arena2, off2)):
        for i in range(NL):
            if off.mask_perm[i] >= 0:
                check_mask_orders(arena, off, i, p["rows"][i], p["k3"][i])


@pytest.mark.gpu
@pytest.mark.parametrize("n,seeds", [(8000, (0,)), (80000, (0,)), (300000, (1,)), (20000, (2, 3))])
def test_line_built_level0_maps_equal_the_per_entry_maps(cuda, built_lib, n, seeds):
    """scenes of 8k, 80k and 300k voxels and a two-scene batch: stem map, k3[0], validity words and every mask order"""
    coords = synth_coords(seeds, n)
    coords = coords[np.random.default_rng(n).permutation(len(coords))]
    cells, ext = box_cells(coords)
    assert cells <= BITMAP_BITS, (cells, ext)                # every one of these scenes takes the bitmap-line path
    p = run_plan(coords, cuda, mmr=2000)
    assert not p["rejected"]
    assert any(p["off"].mask_perm[i] >= 0 for i in range(1, NL)) or n < 20000         # coarse levels with validity words too
    compare_with_per_entry(p, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("ext,batches", [((37, 29, 45), 1), ((21, 33, 70), 2), ((5, 4, 3), 1), ((40, 40, 32), 1)])
def test_lines_leaving_the_box_and_straddling_words(cuda, built_lib, ext, batches):
    """small boxes filled to a third: rows on every face and corner of the box (lines leave it in x, y and z; a box thinner than
    the 5-wide kernel), z extents that are no multiple of 32 (a line's five bits straddle two bitmap words) and one that is"""
    coords = dense_box_coords(sum(ext), ext, 0.33, batches)
    cells, e = box_cells(coords)
    assert tuple(e) == tuple(ext) and cells <= BITMAP_BITS
    for ax in range(3):                                       # rows on both faces of every axis
        assert (coords[:, 1 + ax] == coords[:, 1 + ax].min()).any() and (coords[:, 1 + ax] == coords[:, 1 + ax].max()).any()
    if ext[2] >= 5 and ext[2] % 32:                          # (rows of 32 z-cells are whole words: no line straddles)
        u = coords[:, 1:] - coords[:, 1:].min(0)
        bit = (u[:, 0] * ext[1] + u[:, 1]) * ext[2] + u[:, 2]            # the row's own bit (batch 0); its line is bit - 2 .. bit + 2
        whole = (coords[:, 0] == 0) & (u[:, 2] >= 2) & (u[:, 2] <= ext[2] - 3)
        assert (whole & ((bit - 2) // 32 != (bit + 2) // 32)).any()       # some line of five bits lies in two bitmap words
    p = run_plan(coords, cuda, mmr=500)
    assert not p["rejected"]
    compare_with_per_entry(p, cuda)


@pytest.mark.gpu
def test_box_beyond_the_bitmap_takes_the_per_entry_path(cuda, built_lib):
    """clusters spread over a 420^3 box: more cells than the bitmap has bits, the job falls back on the device"""
    rng = np.random.default_rng(5)
    centres = rng.integers(4, 416, (60, 3))
    centres[0], centres[1] = (0, 0, 0), (419, 419, 419)
    pts = (centres[:, None, :] + rng.integers(-3, 4, (60, 120, 3))).reshape(-1, 3)
    pts = np.unique(np.clip(pts, 0, 419), axis=0)
    coords = np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1)
    cells, ext = box_cells(coords)
    assert cells > BITMAP_BITS, (cells, ext)
    p = run_plan(coords, cuda, mmr=500)
    assert not p["rejected"]
    compare_with_per_entry(p, cuda)


@pytest.mark.gpu
def test_untrusted_bitmap_takes_the_per_entry_path(cuda, built_lib):
    """a row with a negative batch index lies outside the bitmap's box (the sort tracks the largest batch index only): the
    insert pass clears mm[7] and the level-0 job must not believe the bits.  Such an input is rejected afterwards (counts[6]),
    but its level-0 maps are built first and must be the per-entry ones"""
    coords = dense_box_coords(9, (30, 20, 41), 0.3)
    coords[::7, 0] = -1
    cells, _ = box_cells(np.concatenate([np.zeros_like(coords[:, :1]), coords[:, 1:]], 1))
    assert cells <= BITMAP_BITS and (coords[:, 0] < 0).any()           # the box fits: only mm[7] == 0 forces the fallback
    p = run_plan(coords, cuda, mmr=500)
    assert p["rejected"] and p["counts"][6] == int((coords[:, 0] < 0).sum())
    compare_with_per_entry(p, cuda)
