"""The coordinate manager on the adversarial sets of tests/coord_ref.py, through the public entry points, against that module's
unpacked dict reference.  Everything is integer work: every comparison is exact equality (coord_ref.same), row order included.

  lazy path   ME.CoordinateManager: cv_sp_build_levels (table_insert_min, insert_all, flag_levels, emit_levels),
              cv_sp_kernel_map (table_find per entry), cv_sp_up_map
  fused path  fused_plan: cv_sp_scene_plan (the row sort, the levels of the sorted rows, line_job with its own probing loop,
              map_rows27, map_job, up_job)
  direct      cv_sp_sort_rows, cv_sp_morton_keys, cv_sp_mask_keys, cv_sp_transpose_map, cv_sp_mask_perms (the lazy launches
              mp_hist / mp_scan / mp_scatter) into sentinel-filled buffers: nothing beyond the documented extent changes

Every input is a valid coordinate set; what the cases are made for is verified on the CPU by tests/test_coord_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME
from tests import coord_ref as cr

SENT, PAD = -77, 64


def dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.int32).contiguous()


def filled(words, dev, dtype=torch.int32):
    return torch.full((words + PAD,), SENT, dtype=dtype, device=dev)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def untouched(buf, words):
    return bool((host(buf)[words:] == SENT).all())


# ----------------------------------------------------------------------------------------------------------- lazy path
@pytest.mark.gpu
@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_lazy_manager_equals_the_reference(cuda, built_lib, name):
    case, ref = cr.case(name), cr.case_reference(name)
    cm = ME.CoordinateManager(dev_i32(case.coords, cuda))
    assert cm.cap == cr.table_capacity(case.n)
    for i in range(cr.NUM_LEVELS):
        assert cm.num_rows(1 << i) == len(ref["levels"][i]), i
        assert cr.same(host(cm.coords[1 << i]), ref["levels"][i]), i                    # order included
    for k, ts, stride in cr.NET_MAPS:
        assert cr.same(host(cm.kernel_map(k, ts, stride)), ref["maps"][(k, ts, stride)]), (k, ts, stride)
    for ts_c in (2, 4, 8, 16):
        assert cr.same(host(cm.up_map(ts_c)), ref["up"][ts_c]), ts_c


# ---------------------------------------------------------------------------------------------------------- fused path
@pytest.mark.gpu
@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_fused_plan_equals_the_reference_on_the_sorted_rows(cuda, built_lib, name):
    case = cr.case(name)
    perm, inv, sref = cr.case_sorted_reference(name)
    if name.startswith("tail_chain") and name != "tail_chain_coarse_4":
        assert cr.box_cells(case.coords) <= cr.BITMAP_BITS                              # the line path is actually taken
    cm = ME.CoordinateManager(dev_i32(case.coords, cuda), num_levels=1, check=False, lazy=True)
    cm_s, stem_map, out_map = cm.fused_plan(5)
    plan, n = cm._fused, case.n
    assert plan.cap == cr.table_capacity(n) and plan.counts == [len(x) for x in sref["levels"]]
    got_perm = host(plan.keep[0][plan.layout.perm:plan.layout.perm + n])
    assert cr.same(got_perm, perm)                                                      # the stable argsort of sort_key
    assert cr.same(host(out_map), inv[:, None])
    for i in range(cr.NUM_LEVELS):
        assert cr.same(host(cm_s.coords[1 << i]), sref["levels"][i]), i
        assert cr.same(host(cm_s.kernel_map(3, 1 << i)), sref["maps"][(3, 1 << i, 1)]), i
    for i in range(4):
        assert cr.same(host(cm_s.kernel_map(2, 1 << i, 2)), sref["maps"][(2, 1 << i, 2)]), i
        assert cr.same(host(cm_s.up_map(2 << i)), sref["up"][2 << i]), i
    # the stem map: rows in sorted order, entries are rows of the caller's order
    assert cr.same(host(stem_map), cr.case_reference(name)["maps"][(5, 1, 1)][perm])


# --------------------------------------------------------------------------------------------------------- direct calls
@pytest.mark.gpu
@pytest.mark.parametrize("name", cr.SORT_CASE_NAMES)
def test_sort_rows_on_the_shift_boundaries_batches_and_sizes(cuda, built_lib, name):
    L = _lib.lib()
    coords = cr.case(name).coords
    n = len(coords)
    perm, inv = cr.sort_perm(coords)
    c = dev_i32(coords, cuda)
    srt, d_perm, d_inv = filled(4 * n, cuda), filled(n, cuda), filled(n, cuda)
    ws = torch.empty(int(L.cv_sp_sort_workspace_bytes(n)), dtype=torch.uint8, device=cuda)
    _lib.check(L.cv_sp_sort_rows(c.data_ptr(), n, srt.data_ptr(), d_perm.data_ptr(), d_inv.data_ptr(), ws.data_ptr(), ws.numel(),
                                 stream()), "cv_sp_sort_rows")
    assert cr.same(host(d_perm)[:n], perm)
    assert cr.same(host(d_inv)[:n], inv)
    assert cr.same(host(srt)[:4 * n].reshape(n, 4), coords[perm])
    assert untouched(srt, 4 * n) and untouched(d_perm, n) and untouched(d_inv, n)
    assert cr.same(host(c), coords)


KEY_CASES = ["batches", "window_edge", "negative_floor", "dense_full", "isolated", "tail_chain_1024", "sizes_1", "sizes_257"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", KEY_CASES)
def test_morton_keys_and_mask_keys(cuda, built_lib, name):
    L = _lib.lib()
    case, ref = cr.case(name), cr.case_reference(name)
    n = case.n
    keys = filled(n, cuda, torch.int64)
    _lib.check(L.cv_sp_morton_keys(dev_i32(case.coords, cuda).data_ptr(), n, keys.data_ptr(), stream()), "cv_sp_morton_keys")
    assert cr.same(host(keys)[:n], cr.morton_key(case.coords)) and untouched(keys, n)
    for k, windows in ((3, ((0, 27), (9, 18))), (5, ((0, 27), (9, 18), (0, 63), (62, 125)))):
        nbr = ref["maps"][(k, 1, 1)]
        d_nbr = dev_i32(nbr, cuda)
        for jb, je in windows:
            keys = filled(n, cuda, torch.int64)
            _lib.check(L.cv_sp_mask_keys(d_nbr.data_ptr(), n, k ** 3, jb, je, keys.data_ptr(), stream()), "cv_sp_mask_keys")
            assert cr.same(host(keys)[:n], cr.mask_key(nbr, jb, je)), (k, jb, je)
            assert untouched(keys, n), (k, jb, je)


def transpose_on_device(nbr, n_in, dev):
    L = _lib.lib()
    n_out, K = nbr.shape
    out = filled(n_in * K, dev)
    _lib.check(L.cv_sp_transpose_map(dev_i32(nbr, dev).data_ptr(), n_out, K, n_in, out.data_ptr(), stream()), "cv_sp_transpose_map")
    assert untouched(out, n_in * K)
    return host(out)[:n_in * K].reshape(n_in, K)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["negative_floor", "batches", "tail_chain_coarse_2", "sizes_257"])
def test_transpose_map(cuda, built_lib, name):
    case, ref = cr.case(name), cr.case_reference(name)
    n = case.n
    for k in (3, 5):
        nbr = ref["maps"][(k, 1, 1)]
        assert cr.same(transpose_on_device(nbr, n, cuda), cr.transposed(nbr, n)), k
    for i in range(4):                                  # k2s2: n_in = the fine row count, n_out = the coarse one
        down, n_fine = ref["maps"][(2, 1 << i, 2)], len(ref["levels"][i])
        got = transpose_on_device(down, n_fine, cuda)
        assert cr.same(got, cr.transposed(down, n_fine)) and cr.same(got, ref["up"][2 << i]), i
        half = down[:max(1, len(down) // 2)]            # half of the coarse rows: fine rows without an entry stay -1 in all columns
        got = transpose_on_device(half, n_fine, cuda)
        assert cr.same(got, cr.transposed(half, n_fine)), i
        if len(down) > 1:
            assert (got == -1).all(1).any(), i
    _, inv = cr.sort_perm(case.coords)                  # the K = 1 out_map of the fused plan: its transposed map is the sort order
    got = transpose_on_device(inv[:, None], n, cuda)
    assert cr.same(got, cr.transposed(inv[:, None], n)) and cr.same(got[:, 0], cr.sort_perm(case.coords)[0])


@functools.lru_cache(maxsize=None)
def perm_maps(n):
    """(3x3x3 map, K = 8 up map) of n rows of a thinned block"""
    ref = cr.case_reference("negative_floor" if n == 2500 else "sizes_%d" % n)
    assert len(ref["levels"][0]) == n
    return ref["maps"][(3, 1, 1)], ref["up"][2]


@pytest.mark.gpu
@pytest.mark.parametrize("with_map", [0, 1])
@pytest.mark.parametrize("groups", [1, 3, 4, 27])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2500])
def test_mask_perms_lazy_launches(cuda, built_lib, n, groups, with_map):
    """cv_sp_mask_perms: orders, and with the map the rows in processing order and the validity bytes.  The padding column
    of a group narrower than W is unspecified and not compared."""
    L = _lib.lib()
    nbr = perm_maps(n)[1 if groups == 1 else 0]
    K = nbr.shape[1]
    W = (K + groups - 1) // groups
    words = groups * n * (1 + W) + (groups * n + 3) // 4 if with_map else groups * n
    flat = filled(words, cuda)
    ws = torch.empty(groups * 4096, dtype=torch.uint8, device=cuda)
    _lib.check(L.cv_sp_mask_perms(dev_i32(nbr, cuda).data_ptr(), n, K, groups, flat.data_ptr(), ws.data_ptr(), ws.numel(),
                                  with_map, stream()), "cv_sp_mask_perms")
    a = host(flat)
    assert (a[words:] == SENT).all()
    perm = a[:groups * n].reshape(groups, n)
    if with_map:
        nbrp = a[groups * n:groups * n * (1 + W)].reshape(groups, n, W)
        gv_all = a[groups * n * (1 + W):].view(np.uint8)
        gv = gv_all[:groups * n].reshape(groups, n)
        sent_bytes = np.full(len(gv_all) // 4, SENT, np.int32).view(np.uint8)
        assert (gv_all[groups * n:] == sent_bytes[groups * n:]).all()                   # the bytes behind the last flag
    for g in range(groups):
        jb, je = K * g // groups, K * (g + 1) // groups
        assert 1 <= je - jb <= W
        key = cr.mask_key(nbr, jb, je)
        assert cr.same(np.sort(perm[g]), np.arange(n)), g                               # a permutation of the rows
        assert (np.diff(key[perm[g]]) >= 0).all(), g                                    # the group key never decreases
        if with_map:
            assert cr.same(nbrp[g][:, :je - jb], nbr[perm[g], jb:je]), g                # map rows in processing order
            assert cr.same(gv[g], (key != 0).astype(np.uint8)), g                       # "has a neighbour in the group"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["negative_floor", "isolated", "sizes_1025"])
def test_wide_group_mask_perms_group_equal_keys(cuda, built_lib, name):
    """CoordinateManager.mask_perms(3, 1, 2): groups of 13 and 14 offsets go through cv_sp_mask_keys and a device argsort"""
    case, ref = cr.case(name), cr.case_reference(name)
    cm = ME.CoordinateManager(dev_i32(case.coords, cuda))
    m = host(cm.mask_perms(3, 1, 2))
    assert m.shape == (2, case.n)
    nbr = ref["maps"][(3, 1, 1)]
    assert cr.same(host(cm.kernel_map(3, 1)), nbr)
    for g in range(2):
        jb, je = 27 * g // 2, 27 * (g + 1) // 2
        key = cr.mask_key(nbr, jb, je)[m[g]]
        assert cr.same(np.sort(m[g]), np.arange(case.n)), g
        change = np.flatnonzero(np.diff(key) != 0)
        assert len(set(key[np.r_[0, change + 1]].tolist())) == len(change) + 1, g       # every key's rows are contiguous
        assert (np.diff(key) >= 0).all(), g
