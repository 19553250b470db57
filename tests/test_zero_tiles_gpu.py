"""Option "zskip" on the rebuilt conv_finish_small: (mask group, row) pairs without a neighbour cost no partial tile - the
product kernels return before their epilogue where no row of a tile has one, and the finish launch reads the row's validity
word (cv_conv_desc.valid_words) first and loads no partial for a dead pair.  Every case runs the same launch with zskip = 0
and zskip = 1 and wants the same bits (torch.equal on the raw output window, hl bytes included); one case per kernel is also
held against the float64 oracle with the per-element bound of oracle/sparse_oracle.py (what tests/conv_two_source.py uses).

Before every zskip = 1 launch the convolution workspace is filled with a NaN pattern: a partial tile that is read without
having been written shows as a NaN in the output.

The mask groups are the dispatcher's: offsets [0, 9), [9, 18), [18, 27) of so.kernel_offsets(3), whose LAST coordinate
is the slowest - group 0 is the layer below a voxel, group 2 the layer above.  The sheets of this file are therefore flat
in the last coordinate (asserted on the host from the kernel map).  A finite set always has a lowest and a highest layer,
so "no dead row in any group" does not exist: the blob case is a dense box whose two faces are its only dead rows.

conv_finish_small keeps no grid cap (its grid covers the items), so there is no case beyond one.
Direct split-K launches (no mask groups) are compared with conv_finish - the same launch into a window whose leading
dimension is odd, which the dispatcher finishes with conv_finish's word-by-word branch - and with recorded hashes
(tests/golden/zero_tiles_bits.json)."""
import contextlib
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so
from canonicalvoting_amd import _lib, pipeline
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.hough import HoughVoting
from tests import conv_two_source as ts
from tests import test_conv_second_source_gpu as second
from tests.test_conv_paths_gpu import (DEV, PAD, PAD_ROWS, SENT, _clean_flag, _pinned_split_target,  # noqa: F401
                                       check, cuda_t, flag_value, out_buffer, read_out)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zero_tiles_bits.json")
NAN_WORD = 0x7FC00000
GROUPS = 3


# ---- coordinate sets ------------------------------------------------------------------------------------------------------
def _sheet(n, z, side=48):
    i = np.arange(n)
    return np.stack([i // side, i % side, np.full(n, z)], 1)


def _iso(n):
    return np.stack([np.arange(n) * 3, np.zeros(n, np.int64), np.full(n, 50)], 1)


@functools.lru_cache(maxsize=None)
def coords(kind, n):
    """[rows, 4] int64, batch 0.  "sheet": n voxels one layer thick; "pair": two equal sheets of n voxels on adjacent layers
    and 40 isolated voxels (rows dead in group 0 = the lower sheet + the isolated = n + 40; the same count for group 2);
    "box": a dense n-voxel box"""
    if kind == "sheet":
        c = _sheet(n, 0)
    elif kind == "pair":
        c = np.concatenate([_sheet(n, 0), _sheet(n, 1), _iso(40)])
    else:
        s = int(np.ceil(n ** (1 / 3)))
        c = np.stack(np.meshgrid(np.arange(s), np.arange(s), np.arange(s), indexing="ij"), -1).reshape(-1, 3)[:n]
    c = c[np.random.default_rng(len(c)).permutation(len(c))]
    return np.concatenate([np.zeros((len(c), 1), np.int64), c.astype(np.int64) - 3], 1)


class Case:
    """kernel map (device and host), mask orders with their map rows, and which (row, group) pairs are live"""


@functools.lru_cache(maxsize=None)
def case(kind, n):
    c = coords(kind, n)
    p = Case()
    p.n = len(c)
    p.cm = ME.CoordinateManager(torch.from_numpy(c).to(DEV, torch.int32))
    p.nbr = p.cm.kernel_map(3, 1)
    p.ref = so.kernel_map(c, c, 3, 1, 1)
    assert np.array_equal(p.nbr.cpu().numpy(), p.ref)
    p.perms = p.cm.mask_perms(3, 1, GROUPS)
    assert getattr(p.perms, "_cv_has_map", False)
    p.live = (p.ref.reshape(p.n, GROUPS, 9) >= 0).any(2)           # [row, group]
    p.dead = [int((~p.live[:, g]).sum()) for g in range(GROUPS)]   # rows at the front of group g's order
    words = ME.map_valid_words(p.nbr).cpu().numpy()
    assert np.array_equal(words, ((p.ref >= 0).astype(np.int64) << np.arange(27)).sum(1).astype(np.int32))
    return p


@functools.lru_cache(maxsize=None)
def operands(n, cin, cout, seed=0):
    rng = np.random.default_rng(seed * 7919 + n * 3 + cin * 131 + cout * 17)
    x = rng.normal(0, 1, (n, cin)).astype(np.float32)
    x[::7] *= 1e-3
    x[::11] *= 30.0
    w = (rng.normal(0, 1, (27, cin, cout)) / np.sqrt(cin * 27)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(0, 0.2, cout).astype(np.float32)
    res = rng.normal(0, 1, (n, cout)).astype(np.float32)
    return x, w, scale, shift, res


@contextlib.contextmanager
def options(**kw):
    prev = []
    try:
        for name, val in kw.items():
            prev.append((name, ME.set_option(name, val)))
        yield
    finally:
        for name, val in reversed(prev):
            ME.set_option(name, val)


def kernel_options(kernel):
    """conv_hd through the option, as tests/test_conv_paths_gpu.py reaches it at small row counts"""
    return dict(hd_mask=7, hd_min_rows=1) if kernel == "hd" else dict(hd_mask=0)


def poison(nbytes):
    """the convolution workspace ME.conv_forward will take, every word a NaN"""
    ws = ME._workspace(DEV, nbytes)
    ws[:ws.numel() // 4 * 4].view(torch.int32).fill_(NAN_WORD)


def poison_all_scratch():
    """every persistent scratch buffer (the scene calls carve their convolution workspace out of one): nothing may rely on what
    a scratch buffer held before the call"""
    torch.cuda.synchronize()
    for buf in list(_lib._scratch_bufs.values()):
        buf[:buf.numel() // 4 * 4].view(torch.int32).fill_(NAN_WORD)


def raw_bytes(buf):
    return buf.contiguous().view(torch.int32)


def run_groups(p, kernel, cin, cout, zskip, res="hl", relu=True, out_hl=True, scale=True, oracle=False):
    """one three-group launch into a sentinel-padded window; returns the whole buffer (raw) after the sentinel check"""
    x, w, sc, sh, r = operands(p.n, cin, cout)
    xbuf = torch.zeros((p.n, cin + 64), device=DEV)
    xbuf[:, 32:32 + cin] = cuda_t(x)
    xg = ME.to_hl(xbuf)[:, 32:32 + cin]
    e = dict(shift=cuda_t(sh), relu=relu)
    if scale:
        e["scale"] = cuda_t(sc)
    if res:
        rbuf = torch.full((p.n + PAD_ROWS, cout + 2 * PAD), SENT, device=DEV)
        rbuf[:p.n, PAD:PAD + cout] = cuda_t(r)
        if res == "hl":
            rbuf = ME.to_hl(rbuf)
        e["residual"] = rbuf[:p.n, PAD:PAD + cout]
    obuf = out_buffer(p.n, cout, out_hl)
    with options(zskip=zskip, **kernel_options(kernel)):
        if zskip:
            poison(4 * GROUPS * p.n * cout + 256)
        ME.conv_forward(xg, cuda_t(w), p.nbr, p.n, out=obuf[:p.n, PAD:PAD + cout], row_perm=p.perms, perm_groups=GROUPS,
                        pieces=2, in_hl=True, out_hl=out_hl, res_hl=res == "hl", cache_weights=False, **e)
    got = read_out(obuf, p.n, cout, out_hl)
    assert np.isfinite(got).all(), "a partial tile was read that nobody wrote (zskip=%d)" % zskip
    assert flag_value() == 0
    if zskip:       # the switch is ON: exactly the partial tiles without a live row still hold the poison
        T = 256 if kernel == "hd" else 128          # rows of a workgroup's tile
        words = ME._workspace(DEV, 4 * GROUPS * p.n * cout + 256)[:4 * GROUPS * p.n * cout].view(torch.int32)
        unwritten = sum(p.n if d == p.n else d // T * T for d in p.dead) * cout
        assert int((words == NAN_WORD).sum()) == unwritten, "partial tiles left unwritten"
    if oracle:
        y, mag, wabs = so.conv64(x, w, p.ref)
        b = so.conv_bound(mag, wabs, "h2", so.conv_units(27, cin))
        z, bz = so.epilogue64(y, b, scale=sc if scale else None, shift=sh, res=r if res else None, res_hl=res == "hl",
                              relu=relu, hl_out=out_hl)
        check(got, z, bz, "%s %d rows %d->%d zskip=%d" % (kernel, p.n, cin, cout, zskip))
    return raw_bytes(obuf)


def same_bits(p, kernel, cin, cout, **kw):
    want = run_groups(p, kernel, cin, cout, 0, **kw)
    got = run_groups(p, kernel, cin, cout, 1, **kw)
    assert torch.equal(want, got), "%s %d rows %d->%d %s: %d words differ" % (kernel, p.n, cin, cout, kw, int((want != got).sum()))


# ---- the cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["hl", "hd"])
@pytest.mark.parametrize("n", [33, 257, 300])
def test_flat_sheet_every_tile_of_two_groups_returns(kernel, n):
    p = case("sheet", n)
    assert p.dead == [n, 0, n]                      # groups 0 and 2 are dead for every row: every one of their tiles returns
    same_bits(p, kernel, 32, 64, oracle=n == 300)


# rows dead in groups 0 and 2 = n + 40: 1285 inside a 32-row block; 1696 on a block edge inside a tile (of 128 and of 256
# rows); 1280 on the edge of a 128-row tile (conv_hl) and of a 256-row workgroup (conv_hd)
BOUNDARIES = {"inside a block": 1245, "block edge inside a tile": 1656, "tile edge": 1240}


@pytest.mark.parametrize("kernel", ["hl", "hd"])
@pytest.mark.parametrize("where", list(BOUNDARIES))
def test_live_dead_boundary(kernel, where):
    p = case("pair", BOUNDARIES[where])
    d = p.dead[0]
    assert p.dead == [d, 0, d] and 2500 <= p.n <= 3400
    if where == "inside a block":
        assert d % 32 != 0
    elif where == "block edge inside a tile":
        assert d % 32 == 0 and d % 128 != 0 and d % 256 != 0
    else:
        assert d % 128 == 0 and d % 256 == 0
    same_bits(p, kernel, 32, 96, oracle=where == "inside a block")


def test_dense_box_only_its_faces_are_dead():
    p = case("box", 2744)                           # 14^3
    assert p.dead == [196, 0, 196]                  # the lowest and the highest layer, nothing else
    for kernel in ("hl", "hd"):
        same_bits(p, kernel, 32, 64)


@pytest.mark.parametrize("cout", [32, 64, 96, 128])
def test_widths(cout):
    """conv_hl with 1 / 2 / 3 column blocks, conv_hd at 96, two 64-column blocks at 128"""
    p = case("pair", BOUNDARIES["inside a block"])
    same_bits(p, "hl", 64, cout)
    if cout == 96:
        same_bits(p, "hd", 64, cout)


def test_four_column_threads():
    """Cout = 36: a width that is no multiple of 8 or 32 (partial column block), fp32 output and residual"""
    p = case("pair", BOUNDARIES["inside a block"])
    same_bits(p, "hl", 32, 36, res="f32", out_hl=False, oracle=True)


@pytest.mark.parametrize("res", [None, "f32", "hl"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("out_hl", [False, True])
def test_epilogues(res, relu, out_hl):
    p = case("pair", BOUNDARIES["block edge inside a tile"])
    same_bits(p, "hl", 32, 64, res=res, relu=relu, out_hl=out_hl, scale=res is not None)


def test_second_source_keeps_validity_off():
    """with a second source every row gets a sum from every group: the dispatcher ignores the validity words (restated from
    tests/test_conv_second_source_gpu.py, which hands none over)"""
    outs = []
    for zskip in (0, 1):
        q = second.prepare("hl", 300, "mixed", 3, 32, 64, 64, groups=3)
        nbr = second.maps(300, "mixed", 3)[0]
        words = ME.map_valid_words(nbr)
        q.d.valid_words = words.data_ptr()
        if zskip:
            q.ws[:q.ws.numel() // 4 * 4].view(torch.int32).fill_(NAN_WORD)
        _lib.check(second.launch(q, options=(("zskip", zskip),)), "cv_sp_conv_f32")
        got = read_out(q.obuf, q.n_out, q.cout, q.out_hl)
        check(got, q.z, q.bz, "second source, zskip=%d" % zskip)
        outs.append(raw_bytes(q.obuf))
    assert torch.equal(outs[0], outs[1])


# ---- the scene calls: the plan's validity words, one model and the model axis -------------------------------------------
def test_scene_calls_same_bits_with_the_plans_words(cuda, built_lib):
    """cv_detect_scene_f32 and cv_detect_scene_separate_f32 (two models with different weights over the model axis) on a
    3000-voxel scene with every level above 1024 rows mask-sorted: the networks' outputs with and without zskip"""
    from canonicalvoting_amd.minkunet import MinkUNet34C
    from tests.test_separate_scene_gpu import resident, separate_models
    sc, c4, feats, pts, teacher = resident(1, 3000, cuda, True)
    hv = HoughVoting(sc.res, 120)
    policy = pipeline.policy_for_scenes_in_flight(7)._replace(masked_min_rows=1024)
    models = separate_models(cuda, 2)
    torch.manual_seed(7)
    joint = MinkUNet34C(3, 64).to(cuda).eval()
    def calls():
        """both scene calls on poisoned scratch; returns the network outputs and how many convolutions of each call were
        dispatched with validity words (the library's counter "zskip_launches")"""
        keep = {}
        poison_all_scratch()
        ME.set_option("zskip_launches", 0)
        pipeline.detect_scene_separate_c(models, hv, c4, feats, sc.res, policy=policy, keep=keep, thresh_high=20,
                                         models_per_pass=2)
        assert keep["range_flag"] == 0 and keep["level_rows"][0] == 3000
        n_sep = ME.set_option("zskip_launches", 0)
        poison_all_scratch()
        y = pipeline.detect_scene_c(joint, hv, c4, feats, sc.res, policy=policy, thresh_high=20)[2]
        torch.cuda.synchronize()
        n_joint = ME.set_option("zskip_launches", 0)
        return [t.clone() for t in keep["y"]] + [y.F.clone() if hasattr(y, "F") else y.clone()], n_sep, n_joint

    outs, engaged = {}, {}
    for zskip in (0, 1, 1):                 # (the second zskip call runs on the grown, poisoned scratch)
        with options(zskip=zskip), torch.no_grad():
            outs[zskip], n_sep, n_joint = calls()
            engaged[zskip] = (n_sep, n_joint)
    # the plan's validity words reached the dispatcher in both calls (over the model axis: one dispatch covers both models);
    # the finest level alone has ten mask-sorted convolutions without a second source
    assert engaged[0] == (0, 0), engaged
    assert engaged[1][0] >= 10 and engaged[1][1] >= 10, engaged
    assert not torch.equal(outs[0][0], outs[0][1])                  # the two models differ
    for a, b in zip(outs[0], outs[1]):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
        assert torch.equal(a, b)


# ---- direct split-K launches on the rebuilt kernel -------------------------------------------------------------------------
SPLIT_TARGETS = {1: {2: 2, 5: 5, 11: 11, 16: 16}, 129: {2: 4, 5: 10, 11: 22, 16: 32}, 700: {2: 12, 5: 30, 11: 66, 16: 96}}
NJ = 16                     # offsets [0, 16): two splits keep 9 offsets per workgroup, sixteen one each


def split_launch(n, splits, in_hl, odd_ld=False):
    """offsets [0, 16) of a 3x3x3 convolution 32 -> 64 split `splits` ways (the calling thread's split target, the count
    restated); returns (window as float64, raw window)"""
    p = case("box", n)
    cin, cout = 32, 64
    x, w, sc, sh, r = operands(p.n, cin, cout, seed=1)
    target = SPLIT_TARGETS[n][splits]
    assert ts.restated_splits(n, cout, NJ, cin, target) == splits
    xg = cuda_t(x)
    if in_hl:
        xbuf = torch.zeros((n, cin + 64), device=DEV)
        xbuf[:, 32:32 + cin] = xg
        xg = ME.to_hl(xbuf)[:, 32:32 + cin]
    obuf = torch.full((n + PAD_ROWS, cout + 2 * PAD + int(odd_ld)), SENT, device=DEV)
    L = _lib.lib()
    prev = L.cv_sp_set_split_target_thread(target)
    try:
        poison(int(L.cv_sp_conv_workspace_bytes(n, cout, 27)))
        ME.conv_forward(xg, cuda_t(w), p.nbr, n, out=obuf[:n, PAD:PAD + cout], j_begin=0, j_end=NJ, pieces=2, in_hl=in_hl,
                        scale=cuda_t(sc), shift=cuda_t(sh), residual=cuda_t(r), relu=True, cache_weights=False)
    finally:
        L.cv_sp_set_split_target_thread(prev)
    full = obuf.cpu().numpy()
    assert (full[:, :PAD] == SENT).all() and (full[:, PAD + cout:] == SENT).all() and (full[n:] == SENT).all()
    win = np.ascontiguousarray(full[:n, PAD:PAD + cout])
    assert np.isfinite(win).all() and flag_value() == 0
    return win, (x, w, sc, sh, r, p)


@pytest.mark.parametrize("n", [1, 129, 700])
@pytest.mark.parametrize("splits", [2, 5, 11, 16])
def test_split_k_against_conv_finish_and_the_oracle(n, splits):
    """fp32 rows (conv_rows_wp, fp16 pairs): the 16-byte aligned window is finished by conv_finish_small, the window with an
    odd leading dimension by conv_finish - the same partial tiles, the same order of additions, the same bits.  hl rows
    (conv_hl): conv_finish_small against the float64 oracle, and against the recorded hash where there is one."""
    small, _ = split_launch(n, splits, in_hl=False)
    big, _ = split_launch(n, splits, in_hl=False, odd_ld=True)
    assert np.array_equal(small.view(np.int32), big.view(np.int32)), "conv_finish_small and conv_finish differ"
    got, (x, w, sc, sh, r, p) = split_launch(n, splits, in_hl=True)
    y, mag, wabs = so.conv64(x, w, p.ref, 0, NJ)
    z, bz = so.epilogue64(y, so.conv_bound(mag, wabs, "h2", so.conv_units(NJ, 32)), scale=sc, shift=sh, res=r, relu=True)
    check(got.astype(np.float64), z, bz, "split-K %d ways, %d rows" % (splits, n))
    golden = json.load(open(GOLDEN))
    key = "splitk_hl_n%d_s%d" % (n, splits)
    digest = hashlib.sha256(got.tobytes()).hexdigest()
    print("%s %s" % (key, digest))
    if key in golden:
        assert digest == golden[key], key
