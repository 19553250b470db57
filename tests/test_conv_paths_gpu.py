"""Every dispatch branch of the sparse convolution (cv_sp_conv_f32 / launch_rows, the weight gradient, the input gradient)
against the float64 oracle with a bound per output element (oracle/sparse_oracle.py ERROR_MODEL), at exact row counts
around the tile and threshold sizes of the dispatcher, with sentinel rows and columns around every output window."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so
from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME

pytestmark = pytest.mark.gpu

SENT = -7.0
PAD = 32                    # sentinel columns left and right of every output window (keeps 128-byte alignment)
PAD_ROWS = 5                # sentinel rows past n_out


# ---- coordinate sets with exact row counts ----------------------------------------------------------------------------
def _grid(n, side_xy, depth):
    g = np.stack(np.meshgrid(np.arange(side_xy), np.arange(side_xy), np.arange(depth), indexing="ij"), -1).reshape(-1, 3)
    return g[:n]


@functools.lru_cache(maxsize=None)
def coords_n(n, kind="box"):
    """[n, 4] int64 (batch 0): "box" a dense cube (a partial last layer: rows with few neighbours), "sheet" one voxel
    thick, "iso" voxels three apart (the centre offset only), "mixed" half box, a quarter sheet, a quarter isolated,
    rows shuffled"""
    if kind == "box":
        s = int(np.ceil(n ** (1 / 3)))
        c = _grid(n, s, s)
    elif kind == "sheet":
        s = int(np.ceil(np.sqrt(n)))
        c = _grid(n, s, 1)
    elif kind == "iso":
        s = int(np.ceil(n ** (1 / 3)))
        c = _grid(n, s, s) * 3
    else:
        a, b = (n + 1) // 2, (n + 3) // 4
        c = np.concatenate([coords_n(a, "box")[:, 1:], coords_n(b, "sheet")[:, 1:] + [0, 0, 200],
                            coords_n(n - a - b, "iso")[:, 1:] + [400, 0, 0]]) if n >= 4 else _grid(n, 2, 2)
        c = c[np.random.default_rng(n).permutation(n)]
    c = np.concatenate([np.zeros((n, 1), np.int64), np.asarray(c, np.int64) - 5], 1)
    assert len(np.unique(c, axis=0)) == n
    return c


@functools.lru_cache(maxsize=None)
def _manager(n, kind):
    return ME.CoordinateManager(torch.from_numpy(coords_n(n, kind)).to(DEV, torch.int32))


@functools.lru_cache(maxsize=None)
def maps(n, kind, k):
    """(GPU map, its CPU copy checked against so.kernel_map, n_in, n_out).  k = 3 / 5 / 2 (stride-1 maps), 1 (no map),
    "down" (k2s2 to ts 2), "up" (the transposed k2s2 map back to ts 1)"""
    cm = _manager(n, kind)
    c1 = coords_n(n, kind)
    if k == 1:
        return None, None, n, n
    if k in ("down", "up"):
        down = cm.kernel_map(2, 1, 2)
        ref = so.kernel_map(c1, so.downsample_coords(c1, 1), 2, 1, 2)
        assert np.array_equal(down.cpu().numpy(), ref)
        if k == "down":
            return down, ref, n, ref.shape[0]
        up = cm.up_map(2)
        ref_up = np.full((n, 8), -1, np.int64)
        cidx, j = np.nonzero(ref >= 0)
        ref_up[ref[cidx, j], j] = cidx
        assert np.array_equal(up.cpu().numpy(), ref_up)
        return up, ref_up, ref.shape[0], n
    g = cm.kernel_map(k, 1)
    ref = so.kernel_map(c1, c1, k, 1, 1)
    assert np.array_equal(g.cpu().numpy(), ref)
    return g, ref, n, n


@functools.lru_cache(maxsize=None)
def operands(n_in, n_out, cin, cout, K, seed=0):
    """x [n_in, cin] with rows of 1e-3 and 30 times the unit scale, w [K, cin, cout], epilogue vectors, residual"""
    rng = np.random.default_rng(seed * 1000003 + n_in * 7 + cin * 131 + cout * 17 + K)
    x = rng.normal(0, 1, (n_in, cin)).astype(np.float32)
    x[::7] *= 1e-3
    x[::11] *= 30.0
    w = (rng.normal(0, 1, (K, cin, cout)) / np.sqrt(cin * min(K, 27))).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(0, 0.2, cout).astype(np.float32)
    res = rng.normal(0, 1, (n_out, cout)).astype(np.float32)
    return x, w, scale, shift, res


@functools.lru_cache(maxsize=None)
def oracle(n, kind, k, cin, cout, bf16=False, j_begin=0, j_end=None):
    """(y64, mag, wabs) of the case, cached for the module"""
    _, ref, n_in, n_out = maps(n, kind, k)
    K = 1 if k == 1 else 8 if k in ("down", "up") else k ** 3
    x, w = operands(n_in, n_out, cin, cout, K)[:2]
    if bf16:
        x, w = so.bf16_round(x), so.bf16_round(w)
    return so.conv64(x, w, ref, j_begin, j_end)


def cuda_t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def path_of(cin, cout, pieces, per_wg=0, stem=False):
    """the product path cv_sp_conv_f32 takes (see launch_rows): cin % 32 != 0 -> conv_rows<NB, false> (fp32 MFMA); more
    than 28 offsets per workgroup -> conv_rows<NB, true> (fp32 MFMA); else the piece kernels"""
    if stem:
        return "h2"
    if cin % 32 or cout % 4 or per_wg > 28:
        return "f32"
    return {1: "bf16", 2: "h2", 3: "x6"}[pieces]


def out_buffer(n_out, cout, hl):
    buf = torch.full((n_out + PAD_ROWS, cout + 2 * PAD), SENT, device=DEV)
    return ME.to_hl(buf) if hl else buf


def read_out(buf, n_out, cout, hl):
    """(window as float64, after checking every sentinel row and column is untouched)"""
    full = (ME.from_hl(buf) if hl else buf).cpu().numpy().astype(np.float64)
    assert (full[:, :PAD] == SENT).all() and (full[:, PAD + cout:] == SENT).all(), "stray column writes"
    assert (full[n_out:] == SENT).all(), "writes past n_out"
    return full[:n_out, PAD:PAD + cout]


def check(got, ref, bound, what):
    ok, i, r = so.within(got, ref, bound)
    assert ok, "%s: element %s off by %.3g x its bound (got %r, fp64 %r, bound %.3g)" % (
        what, i, r, float(got[i]), float(ref[i]), float(bound[i]))


DEV = torch.device("cuda:0")        # the key ME.range_flag files the flag of a cuda:0 launch under


def flag_value():
    torch.cuda.synchronize()
    return int(ME.range_flag(DEV)[0])


def flag_reset():
    torch.cuda.synchronize()
    ME.range_flag(DEV).zero_()


@pytest.fixture(autouse=True)
def _clean_flag(cuda, built_lib):
    flag_reset()
    yield
    flag_reset()


def run_fwd(n, kind, k, cin, cout, pieces=3, flavour=0, epi=True, relu=True, in_hl=False, out_hl=False, res_hl=False,
            j_range=None, stem=False, tickets=False, what="", **kw):
    """one forward launch through ME.conv_forward into a sentinel-padded window, checked element by element"""
    nbr, ref_map, n_in, n_out = maps(n, kind, k)
    K = 1 if k == 1 else 8 if k in ("down", "up") else k ** 3
    x, w, scale, shift, res = operands(n_in, n_out, cin, cout, K)
    jb, je = j_range if j_range else (0, 0)
    nj = (je or K) - jb
    per_wg = nj if flavour == 1 else 0
    path = path_of(cin, cout, pieces, per_wg, stem)
    y64, mag, wabs = oracle(n, kind, k, cin, cout, path == "bf16", jb, je or None)
    b = so.conv_bound(mag, wabs, path, so.conv_units(nj, cin))
    xg = cuda_t(x)
    if in_hl:
        xbuf = torch.zeros((n_in, cin + 64), device=DEV)
        xbuf[:, 32:32 + cin] = xg
        xg = ME.to_hl(xbuf)[:, 32:32 + cin]
    e = {}
    resv = None
    if epi:
        e = dict(scale=cuda_t(scale), shift=cuda_t(shift), relu=relu)
        rbuf = torch.full((n_out + PAD_ROWS, cout + 2 * PAD), SENT, device=DEV)
        rbuf[:n_out, PAD:PAD + cout] = cuda_t(res)
        if res_hl:
            rbuf = ME.to_hl(rbuf)
        e["residual"] = rbuf[:n_out, PAD:PAD + cout]
        resv = res
    obuf = out_buffer(n_out, cout, out_hl)
    if tickets:
        kw["split_tickets"] = torch.zeros(4096, dtype=torch.int32, device=DEV)
    ME.conv_forward(xg, cuda_t(w), nbr, n_out, out=obuf[:n_out, PAD:PAD + cout], flavour=flavour, j_begin=jb,
                    j_end=je, pieces=pieces, in_hl=in_hl, out_hl=out_hl, res_hl=res_hl and epi, stem_mfma=stem,
                    cache_weights=False, **e, **kw)
    got = read_out(obuf, n_out, cout, out_hl)
    if epi:
        z, bz = so.epilogue64(y64, b, scale=scale, shift=shift, res=resv, res_hl=res_hl, relu=relu, hl_out=out_hl)
    else:
        z, bz = so.epilogue64(y64, b, hl_out=out_hl)
    check(got, z, bz, what or "n=%d %s k=%s %d->%d pieces=%d flavour=%d" % (n, kind, k, cin, cout, pieces, flavour))
    if tickets:
        assert int(kw["split_tickets"].abs().sum()) == 0
    assert flag_value() == 0
    return obuf


# ---- 2. the forward dispatch matrix ------------------------------------------------------------------------------------
TAILS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("cout", [32, 64, 96, 128, 256])
def test_tile_tails(cout):
    """n_out around the 128-row tile for every column-block width; the three product modes and the hl output in turn"""
    for i, n in enumerate(TAILS):
        pieces = (3, 2, 1)[i % 3]
        run_fwd(n, "box", 3, 32, cout, pieces=pieces, out_hl=pieces == 2, res_hl=pieces == 2 and i % 2 == 0)
        run_fwd(n, "mixed", 3, 64, cout, pieces=3, epi=i % 2 == 0)


@pytest.mark.parametrize("cout", [32, 64, 96])
@pytest.mark.parametrize("n", [16383, 16384, 16385])
def test_hd_and_auto_mask_thresholds(cout, n):
    """hl input at 16384 rows +- 1: conv_hd on (hd_mask 7: every NB <= 3) or off, the automatic mask groups from 16384 rows"""
    prev = ME.set_option("hd_mask", 7)
    try:
        run_fwd(n, "box", 3, 32, cout, pieces=2, in_hl=True, out_hl=True, res_hl=True)
    finally:
        ME.set_option("hd_mask", prev)
    if cout == 96:          # the default mask (NB = 3 only) and the other two conv_hd shapes, zskip on
        run_fwd(n, "box", 3, 32, cout, pieces=2, in_hl=True)
        for name, val in (("hd_shape", 0), ("hd_shape", 1), ("zskip", 1)):
            prev = ME.set_option(name, val)
            try:
                run_fwd(n, "mixed", 3, 32, cout, pieces=2, in_hl=True, out_hl=True, what="%s=%d n=%d" % (name, val, n))
            finally:
                ME.set_option(name, prev)


# ---- the split count the dispatcher picks, restated so that each test can pin the route it means to take -------------
SPLIT_TARGET = 768          # the library default; pinned for this module by _pinned_split_target


def expected_splits(n_out, cout, K, cin):
    """pick_splits (sparse_conv.hip) for a flavour-0 launch with the default knobs: 64-column workgroups above 96
    columns, 768 target workgroups, <= 24 MB of partial tiles, at most 64 splits.  (The piece kernels raise it to keep
    <= 10 offsets per workgroup; at the sizes asserted here that changes nothing.)"""
    nb = 1 if cout <= 32 else 2 if cout <= 64 else 3 if cout <= 96 else 2
    tiles = -(-n_out // 128) * -(-cout // (nb * 32))
    units = K * (cin // 32) if cin % 32 == 0 and cout % 4 == 0 else -(-K * cin // 32)
    if tiles >= 384 or units <= 1:
        return 1
    s = min(-(-SPLIT_TARGET // tiles), units, max((24 << 20) // (n_out * cout * 4), 2), 64)
    return max(s, 1)


@pytest.fixture(scope="module", autouse=True)
def _pinned_split_target(cuda, built_lib):
    for env in ("CV_SPLIT_TARGET", "CV_SPLIT_TRAFFIC_MB", "CV_NB_MAX", "CV_NB_WIDE"):
        assert env not in os.environ, "%s changes the launch routes these tests pin" % env
    L = _lib.lib()
    prev = ME.set_split_target(SPLIT_TARGET)
    prev_thread = L.cv_sp_set_split_target_thread(0)
    yield
    L.cv_sp_set_split_target_thread(prev_thread)
    ME.set_split_target(prev)


@pytest.mark.parametrize("cin,pieces", [(40, 3), (32, 3), (32, 2)])
@pytest.mark.parametrize("tiles", [383, 384])
def test_pick_splits_tile_threshold(cin, pieces, tiles):
    """383 / 384 tiles of 128 x 32: split or not (j_end = K keeps the automatic mask groups off at these sizes); with
    Cin 40 (conv_rows<1, false>) 3 splits against none"""
    if cin == 40:
        assert expected_splits(tiles * 128, 32, 27, cin) == (3 if tiles == 383 else 1)
    run_fwd(tiles * 128, "box", 3, cin, 32, pieces=pieces, j_range=(0, 27))


@pytest.mark.parametrize("n", [5770, 6144])
@pytest.mark.parametrize("in_hl", [False, True])
def test_split_count_around_finish_small(n, in_hl):
    """46 tiles of 128 x 64 (5770 rows): 17 splits, finished by conv_finish; 48 tiles (6144 rows): 16 splits,
    conv_finish_small"""
    assert expected_splits(n, 64, 27, 32) == (17 if n == 5770 else 16)
    run_fwd(n, "box", 3, 32, 64, pieces=2, in_hl=in_hl, out_hl=True, res_hl=in_hl)
    run_fwd(n, "mixed", 3, 32, 64, pieces=3)


def test_split_cap_64():
    """one or two tiles and 81 units: the 64-split cap, conv_finish"""
    for n in (1, 129):
        assert expected_splits(n, 32, 27, 96) == 64
        run_fwd(n, "box", 3, 96, 32, pieces=3)
        run_fwd(n, "box", 3, 96, 32, pieces=2, in_hl=True, out_hl=True)


@pytest.mark.parametrize("j_end", [10, 11, 28, 29])
def test_offsets_per_workgroup_cross_the_prefetch_sizes(j_end):
    """flavour 1 (no split): 10 offsets -> conv_rows_wp<NB, P, 10>, 11 and 28 -> <NB, P, 28>, 29 -> conv_rows<NB, true>"""
    for pieces in (3, 2) if j_end != 29 else (3,):
        run_fwd(300, "box", 5, 32, 64, pieces=pieces, flavour=1, j_range=(0, j_end))
    if j_end == 28:
        run_fwd(300, "box", 5, 32, 64, pieces=1, flavour=1, j_range=(0, j_end))
    if j_end == 29:
        with pytest.raises(_lib.CvError, match="bf16 compute mode"):
            run_fwd(300, "box", 5, 32, 64, pieces=1, flavour=1, j_range=(0, j_end))


@pytest.mark.parametrize("pieces", [3, 2, 1])
def test_flavour1_whole_kernel(pieces):
    run_fwd(700, "mixed", 3, 64, 96, pieces=pieces, flavour=1)
    run_fwd(129, "box", 3, 32, 256, pieces=pieces, flavour=1)


def _minkunet_shapes():
    sd = so.make_state_dict(3, 64)
    out = set()
    for name, v in sd.items():
        if name.endswith(".kernel"):
            K, cin, cout = (1,) + tuple(v.shape) if v.dim() == 2 else tuple(v.shape)
            k = 1 if K == 1 else 5 if K == 125 else 3 if K == 27 else ("up" if name.startswith("convtr") else "down")
            out.add((k, cin, cout))
    return sorted(out, key=str)


@pytest.mark.parametrize("k,cin,cout", _minkunet_shapes() + [(5, 6, 32)])      # + the 6-channel stem
def test_minkunet34c_shapes(k, cin, cout):
    """every (kernel, Cin, Cout) of MinkUNet34C; the stems also on the matrix-core stem kernel"""
    if cin in (3, 6):
        run_fwd(700, "mixed", 5, cin, cout, pieces=3)
        run_fwd(700, "mixed", 5, cin, cout, pieces=2, stem=True, out_hl=True)
        run_fwd(129, "box", 5, cin, cout, pieces=2, stem=True)
        return
    run_fwd(700, "mixed", k, cin, cout, pieces=3)
    run_fwd(257, "box", k, cin, cout, pieces=2, in_hl=True, out_hl=cout % 32 == 0, res_hl=True)


@pytest.mark.parametrize("cin,cout", [(32, 36), (64, 100), (32, 30), (40, 64), (40, 30), (6, 32)])
def test_odd_channel_counts(cin, cout):
    """Cout % 32 != 0 (36, 100), Cout % 4 != 0 (30: conv_finish_scalar and the word-by-word epilogue), Cin % 32 != 0
    (40: conv_rows<NB, false>), with and without split-K (1x1: no split)"""
    for n, k in ((129, 3), (700, 3), (257, 1)):
        if k == 1 and cin == 6:
            continue
        run_fwd(n, "mixed", k, cin, cout, pieces=3)
        run_fwd(n, "box", k, cin, cout, pieces=2, epi=False)


@pytest.mark.parametrize("groups", [2, 3, 4])
def test_perm_groups(groups):
    """mask-sorted offset groups (one launch, grid.z = group, conv_finish_small); 2 groups are wider than 10 offsets"""
    for n, cout, in_hl in ((700, 64, False), (3000, 96, groups > 2), (129, 256, False)):    # hl: <= 10 offsets a group
        cm = _manager(n, "mixed")
        perms = cm.mask_perms(3, 1, groups)
        run_fwd(n, "mixed", 3, 32, cout, pieces=2 if in_hl else 3, in_hl=in_hl, out_hl=in_hl, row_perm=perms,
                perm_groups=groups, what="groups=%d n=%d" % (groups, n))


def acc_in_halves(pieces, flavour):
    """offsets [0, 13) into an fp32 buffer, [13, 27) on top of it through acc_in with the epilogue, both checked; returns
    the sentinel-padded buffer of the second launch"""
    n, cin, cout = 700, 64, 96
    nbr, ref_map, _, _ = maps(n, "mixed", 3)
    x, w, scale, shift, res = operands(n, n, cin, cout, 27)
    path = path_of(cin, cout, pieces)
    y1, m1, wa1 = oracle(n, "mixed", 3, cin, cout, False, 0, 13)
    y2, m2, wa2 = oracle(n, "mixed", 3, cin, cout, False, 13, 27)
    b1 = so.conv_bound(m1, wa1, path, so.conv_units(13, cin))
    b2 = so.conv_bound(m2, wa2, path, so.conv_units(14, cin))
    part = ME.conv_forward(cuda_t(x), cuda_t(w), nbr, n, flavour=flavour, j_begin=0, j_end=13, pieces=pieces,
                           cache_weights=False)
    check(part.cpu().numpy().astype(np.float64), y1, b1, "first half")
    obuf = out_buffer(n, cout, False)
    ME.conv_forward(cuda_t(x), cuda_t(w), nbr, n, flavour=flavour, j_begin=13, j_end=27, acc_in=part,
                    scale=cuda_t(scale), shift=cuda_t(shift), residual=cuda_t(res), relu=True, pieces=pieces,
                    out=obuf[:n, PAD:PAD + cout], cache_weights=False)
    z, bz = so.epilogue64(y2, b2, acc_in=y1, b_acc=b1, scale=scale, shift=shift, res=res, relu=True)
    check(read_out(obuf, n, cout, False), z, bz, "second half on acc_in, pieces=%d flavour=%d" % (pieces, flavour))
    return obuf


def test_offset_halves_chained_through_acc_in():
    """offsets [0, 13) into an fp32 buffer, [13, 27) on top of it through acc_in with the epilogue"""
    for pieces, flavour in ((3, 1), (2, 0), (3, 0)):
        acc_in_halves(pieces, flavour)


@pytest.mark.parametrize("n,cout", [(700, 64), (3000, 96), (257, 256)])
def test_split_tickets(n, cout):
    """split-K reduced by the last-arriving workgroup of each tile (conv_hl): same bound, counters back at zero"""
    run_fwd(n, "mixed", 3, 32, cout, pieces=2, in_hl=True, out_hl=True, res_hl=True, tickets=True)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("epi", [False, True])
def test_epilogue_switches(relu, epi):
    """scale / shift / residual / ReLU on and off, fp32 and hl operands, on the split and the unsplit routes"""
    for k, n in ((3, 700), (1, 700)):
        run_fwd(n, "mixed", k, 64, 64, pieces=3, epi=epi, relu=relu)
        run_fwd(n, "mixed", k, 64, 64, pieces=2, epi=epi, relu=relu, in_hl=True, out_hl=True, res_hl=epi)
        run_fwd(n, "mixed", k, 64, 64, pieces=2, epi=epi, relu=relu, out_hl=False, res_hl=epi)
    if not epi and not relu:        # ReLU alone
        obuf = out_buffer(700, 64, False)
        nbr, _, _, _ = maps(700, "mixed", 3)
        x, w = operands(700, 700, 64, 64, 27)[:2]
        ME.conv_forward(cuda_t(x), cuda_t(w), nbr, 700, relu=True, out=obuf[:700, PAD:PAD + 64], pieces=3,
                        cache_weights=False)
        y64, mag, wabs = oracle(700, "mixed", 3, 64, 64)
        z, bz = so.epilogue64(y64, so.conv_bound(mag, wabs, "x6", 27 * 2), relu=True)
        check(read_out(obuf, 700, 64, False), z, bz, "relu only")


# the range flag on every epilogue route that writes the hl format: (name, n, k, cin, cout, extra arguments)
RANGE_ROUTES = [
    ("direct wide (1x1, no split)", 700, 1, 32, 64, {}),
    ("conv_finish_small", 6144, 3, 32, 64, {}),       # 16 splits (expected_splits)
    ("conv_finish", 5770, 3, 32, 64, {}),             # 17 splits
    ("conv_hd (1x1, no split)", 16384, 1, 32, 96, {"in_hl": True}),
    ("conv_hd + mask groups", 16384, 3, 32, 96, {"in_hl": True}),
    ("stem", 700, 5, 3, 32, {"stem": True}),
]


@pytest.mark.parametrize("route", RANGE_ROUTES, ids=[r[0] for r in RANGE_ROUTES])
def test_range_flag_per_route(route):
    """0 after in-range outputs (run_fwd checks it), 1 after one output column beyond the fp16 range"""
    name, n, k, cin, cout, extra = route
    if name.startswith("conv_finish"):
        assert expected_splits(n, cout, 27, cin) == (16 if name == "conv_finish_small" else 17)
    if name.startswith("direct"):
        assert expected_splits(n, cout, 1, cin) == 1
    run_fwd(n, "box", k, cin, cout, pieces=2, out_hl=True, what=name, **extra)
    nbr, _, n_in, n_out = maps(n, "box", k)
    K = 1 if k == 1 else k ** 3
    x, w, scale, shift, _ = operands(n_in, n_out, cin, cout, K)
    big = shift.copy()
    big[cout // 2] = 1e5
    xg = ME.to_hl(cuda_t(x)) if extra.get("in_hl") else cuda_t(x)
    obuf = out_buffer(n_out, cout, True)
    ME.conv_forward(xg, cuda_t(w), nbr, n_out, scale=cuda_t(scale), shift=cuda_t(big), out=obuf[:n_out, PAD:PAD + cout],
                    pieces=2, out_hl=True, in_hl=bool(extra.get("in_hl")), stem_mfma=bool(extra.get("stem")),
                    cache_weights=False)
    assert flag_value() == 1, name


# ---- 4. hl operands with the word-by-word epilogue: refused ------------------------------------------------------------
BAD_DESC = ["scale_misaligned_out_hl", "acc_in_misaligned_out_hl", "res_ld_odd_out_hl", "out_ld_odd_res_hl"]


@pytest.mark.parametrize("case", BAD_DESC)
@pytest.mark.parametrize("k", [3, 1])
def test_hl_with_word_epilogue_is_refused(case, k):
    """An hl output or residual with operands that select the word-by-word epilogue (a.wide false) must be refused:
    those epilogues would store fp32 into the hl buffer or read the hl residual as fp32.  Every operand is a real
    device buffer; the misaligned ones are slices of larger allocations, so every access stays in bounds."""
    n, cin, cout = 300, 32, 64
    nbr, ref_map, _, _ = maps(n, "box", k)
    K = 1 if k == 1 else 27
    x, w, scale, shift, res = operands(n, n, cin, cout, K)
    y64, mag, wabs = oracle(n, "box", k, cin, cout)
    b = so.conv_bound(mag, wabs, "h2", so.conv_units(K, cin))
    sc_buf = torch.zeros(cout + 8, device=DEV)
    sc_buf[1:1 + cout] = cuda_t(scale)
    sc = sc_buf[1:1 + cout] if case == "scale_misaligned_out_hl" else cuda_t(scale)
    kw = dict(scale=sc, shift=cuda_t(shift), relu=False, pieces=2, cache_weights=False)
    acc = None
    out_hl = case != "out_ld_odd_res_hl"
    if case == "acc_in_misaligned_out_hl":
        acc_buf = torch.zeros((n, cout + 8), device=DEV)
        acc = acc_buf[:, 1:1 + cout]
        kw["acc_in"] = acc
    if case == "res_ld_odd_out_hl":
        rbuf = torch.zeros((n, cout + 1), device=DEV)
        rbuf[:, :cout] = cuda_t(res)
        kw["residual"] = rbuf[:, :cout]
    if case == "out_ld_odd_res_hl":
        rbuf = torch.zeros((n, cout + 2 * PAD), device=DEV)
        rbuf[:, PAD:PAD + cout] = cuda_t(res)
        kw["residual"] = ME.to_hl(rbuf)[:, PAD:PAD + cout]
        kw["res_hl"] = True
        obuf = torch.full((n + PAD_ROWS, cout + 1), SENT, device=DEV)
        out = obuf[:n, :cout]
    else:
        obuf = out_buffer(n, cout, True)
        out = obuf[:n, PAD:PAD + cout]
    refused = False
    try:
        ME.conv_forward(cuda_t(x), cuda_t(w), nbr, n, out=out, out_hl=out_hl, **kw)
        torch.cuda.synchronize()
    except _lib.CvError as e:
        assert "hl-format" in str(e), e
        refused = True
    if not refused:         # what the launch wrote: fp32 words in an hl buffer / an hl residual read as fp32
        got = (ME.from_hl(obuf)[:n, PAD:PAD + cout] if out_hl else out).cpu().numpy().astype(np.float64)
        r = res if "res" in case else None
        z, bz = so.epilogue64(y64, b, scale=scale, shift=shift, res=r, res_hl="res_hl" in case, hl_out=out_hl)
        check(got, z, bz, "accepted descriptor " + case)
    assert refused, "descriptor accepted"


def word_epilogue_fp32(k, pieces):
    """one launch with fp32 operands that are not 16-byte aligned (scale, acc_in slices) and leading dimensions % 4 != 0
    (residual, output), checked; returns the sentinel-padded buffer"""
    n, cin, cout = 300, 32, 64
    nbr, ref_map, _, _ = maps(n, "box", k)
    K = 1 if k == 1 else 27
    x, w, scale, shift, res = operands(n, n, cin, cout, K)
    y64, mag, wabs = oracle(n, "box", k, cin, cout)
    acc = np.random.default_rng(3).normal(0, 1, (n, cout))
    sc_buf = torch.zeros(cout + 8, device=DEV)
    sc_buf[1:1 + cout] = cuda_t(scale)
    acc_buf = torch.zeros((n, cout + 8), device=DEV)
    acc_buf[:, 1:1 + cout] = cuda_t(acc.astype(np.float32))
    rbuf = torch.zeros((n, cout + 1), device=DEV)
    rbuf[:, :cout] = cuda_t(res)
    obuf = torch.full((n + PAD_ROWS, cout + 2 * PAD + 1), SENT, device=DEV)
    ME.conv_forward(cuda_t(x), cuda_t(w), nbr, n, scale=sc_buf[1:1 + cout], shift=cuda_t(shift),
                    acc_in=acc_buf[:, 1:1 + cout], residual=rbuf[:, :cout], relu=True, pieces=pieces,
                    out=obuf[:n, PAD:PAD + cout], cache_weights=False)
    b = so.conv_bound(mag, wabs, path_of(cin, cout, pieces), so.conv_units(K, cin))
    z, bz = so.epilogue64(y64, b, acc_in=acc.astype(np.float32).astype(np.float64), b_acc=0.0, scale=scale,
                          shift=shift, res=res, relu=True)
    full = obuf.cpu().numpy().astype(np.float64)
    assert (full[:, :PAD] == SENT).all() and (full[:, PAD + cout:] == SENT).all() and (full[n:] == SENT).all()
    check(full[:n, PAD:PAD + cout], z, bz, "word epilogue k=%d pieces=%d" % (k, pieces))
    return obuf


@pytest.mark.parametrize("k", [3, 1])
def test_word_by_word_epilogue_fp32(k):
    """fp32 operands that are not 16-byte aligned (scale, acc_in slices) and leading dimensions % 4 != 0 (residual,
    output): the word-by-word epilogues (epilogue_store, conv_finish's scalar branch) with every operand"""
    for pieces in (3, 2):
        word_epilogue_fp32(k, pieces)


# ---- 3. backward ---------------------------------------------------------------------------------------------------------
WGRAD_PAIRS = [(32, 32), (64, 32), (96, 32), (128, 32), (32, 64), (64, 64), (96, 64), (128, 64), (32, 96), (64, 96),
               (96, 96), (32, 128), (64, 128)]       # conv_wgrad<NA, NB> instances 11 ... 42


def run_wgrad(n, kind, k, cin, cout, pieces, x_pad=0):
    nbr, ref_map, n_in, n_out = maps(n, kind, k)
    K = 1 if k == 1 else 8 if k in ("down", "up") else k ** 3
    x, _, _, _, dy = operands(n_in, n_out, cin, cout, K, seed=1)
    path = {0: "f32", 1: "bf16", 3: "x6"}[pieces]
    xr, dyr = (so.bf16_round(x), so.bf16_round(dy)) if pieces == 1 else (x, dy)
    dw64, mag = so.wgrad64(xr, dyr, ref_map, K)
    L = _lib.lib()
    xbuf = torch.zeros((n_in, cin + x_pad), device=DEV)
    xbuf[:, :cin] = cuda_t(x)
    dyg = cuda_t(dy)
    dw = torch.full((K + 1, cin, cout), SENT, device=DEV)
    # NaN-filled partial tiles: a slot the kernel leaves unwritten cannot pass on stale sums of an earlier launch
    ws = torch.full((int(L.cv_sp_wgrad_workspace_bytes(n_out, cin, cout, K)) // 4,), float("nan"), device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.cv_sp_conv_wgrad_px_f32(xbuf.data_ptr(), xbuf.stride(0), cin, dyg.data_ptr(), dyg.stride(0), cout,
                                         nbr.data_ptr() if nbr is not None else None, K, n_out, dw.data_ptr(),
                                         ws.data_ptr(), 4 * ws.numel(), pieces, st), "cv_sp_conv_wgrad_px_f32")
    got = dw.cpu().numpy().astype(np.float64)
    assert (got[K] == SENT).all(), "writes past dW"
    check(got[:K], dw64, so.wgrad_bound(mag, path, n_out), "wgrad n=%d k=%s %d->%d pieces=%d" % (n, k, cin, cout, pieces))


@pytest.mark.parametrize("pieces", [3, 0, 1])
@pytest.mark.parametrize("cin,cout", WGRAD_PAIRS)
def test_wgrad_every_instance(cin, cout, pieces):
    run_wgrad(700, "mixed", 3, cin, cout, pieces)


@pytest.mark.parametrize("pieces", [3, 0, 1])
def test_wgrad_row_thresholds_and_kernel_sizes(pieces):
    """n_out / 256 (K = 27), n_out / 128 (K <= 8) and below 128 rows; K = 1, 8, 27, 125; an x window with x_ld > Cin"""
    for n in (100, 255, 256, 513):
        run_wgrad(n, "box", 3, 64, 64, pieces)
    for n in (100, 127, 128, 257):
        run_wgrad(n, "box", 1, 32, 96, pieces)
        run_wgrad(n, "box", "down", 32, 32, pieces)
    run_wgrad(300, "mixed", 5, 32, 32, pieces)
    run_wgrad(300, "mixed", 5, 3, 32, pieces)
    run_wgrad(700, "mixed", 3, 96, 64, pieces, x_pad=32)


@pytest.mark.parametrize("pieces", [2, 3])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 96), (128, 64)])
def test_input_gradient_through_transposed_map(cin, cout, pieces):
    """dx = conv(dy, W^T, transposed map) with W packed straight from the forward layout (weight_t)"""
    for n in (1, 127, 128, 129, 257, 700):
        nbr, ref_map, _, _ = maps(n, "mixed", 3)
        nbr_t = ME.transposed_map(nbr, n)
        ref_t = np.full((n, 27), -1, np.int64)
        u, j = np.nonzero(ref_map >= 0)
        ref_t[ref_map[u, j], j] = u
        assert np.array_equal(nbr_t.cpu().numpy(), ref_t)
        _, w, _, _, dy = operands(n, n, cin, cout, 27, seed=2)
        y64, mag, wabs = so.conv64(dy, np.ascontiguousarray(w.transpose(0, 2, 1)), ref_t)
        b = so.conv_bound(mag, wabs, path_of(cout, cin, pieces), so.conv_units(27, cout))
        obuf = out_buffer(n, cin, False)
        ME.conv_forward(cuda_t(dy), cuda_t(w), nbr_t, n, weight_t=True, pieces=pieces, cache_weights=False,
                        out=obuf[:n, PAD:PAD + cin])
        check(read_out(obuf, n, cin, False), y64, b, "dx n=%d %d<-%d pieces=%d" % (n, cin, cout, pieces))
        assert flag_value() == 0
