"""The second source of the sparse convolution (cv_conv_desc.in2 / in2_ld / cin2 / weight2_x6: out += in2 @ W2 on the
output rows, BasicBlock's 1x1 downsample branch inside conv2) on the three kernels that implement it - conv_rows_wp
(fp32 sources; bf16 triples, fp16 pairs, single bf16), conv_hl and conv_hd (hl sources) - against the float64 two-source
oracle with the per-element bound of oracle/sparse_oracle.py (ERROR_MODEL; units = offsets x Cin / 32 + Cin2 / 32).

The descriptor is filled here (ME.conv_forward cannot express a second source); the weights are packed as minkunet.py
packs them (ME.resolve_weights with second=: both BatchNorm scales folded in, one power of two for both fp16-pair sets).
in2 is a column view of a buffer whose other columns hold values a thousand times larger, outputs land in
sentinel-padded windows, and every coordinate set is "mixed": shuffled rows, a quarter of them with the centre offset
only.  tests/test_conv_bound.py shows on the CPU that the bound rejects an absent second source, a dropped last chunk
and a chunk read at the tile position instead of the permuted row on every shape used here."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so
from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME
from tests import conv_two_source as ts
from tests.test_conv_paths_gpu import (DEV, PAD, PAD_ROWS, SENT, _clean_flag, _manager, _pinned_split_target,  # noqa: F401
                                       SPLIT_TARGET, check, cuda_t, flag_value, maps, operands, out_buffer, read_out)

pytestmark = pytest.mark.gpu

KERNELS = ("wp3", "wp2", "wp1", "hl", "hd0", "hd1", "hd2")       # conv_rows_wp<., 3 / 2 / 1>, conv_hl, conv_hd shapes 0 / 1 / 2
FAMILIES = ("wp3", "hl", "hd2")
IN2_PAD = 32                # columns left and right of the in2 view
WORST = {}                  # kernel -> largest error / bound seen (printed by the last test, for orientation only)


class Launch:
    """one filled descriptor with everything it points to"""


def prepare(kernel, n, kind, k, cin, cin2, cout, j_range=None, groups=0, tickets=False, epi="net", flavour=0,
            workspace=True):
    nbr, ref_map, n_in, n_out = maps(n, kind, k)
    K = ts.ksize(k)
    pieces = {"wp3": 3, "wp2": 2, "wp1": 1}.get(kernel, 2)
    hl = kernel[0] == "h"
    folded = epi == "net"
    x, w, scale, shift, res = operands(n_in, n_out, cin, cout, K)
    x2, w2, scale2 = ts.second_operands(n_out, cin2, cout)
    jb, je = j_range if j_range else (0, 0)
    p = Launch()
    p.kernel, p.n_out, p.cout, p.pieces, p.hl, p.K, p.nj = kernel, n_out, cout, pieces, hl, K, (je or K) - jb
    p.case = ts.two_source(n, kind, k, cin, cin2, cout, pieces, jb, je or None, folded)
    p.wt, p.w2t = cuda_t(w), cuda_t(w2)
    p.wp, p.wp2, wpieces, acc_scale, _ = ME.resolve_weights(
        p.wt, p.wt, pieces, col_scale=cuda_t(scale) if folded else None,
        second=(p.w2t, cuda_t(scale2) if folded else None))
    assert wpieces == pieces and p.wp is not None and p.wp2 is not None
    # sources: x between zero columns, x2 between columns a thousand times larger
    xbuf = torch.zeros((n_in, cin + 64), device=DEV)
    xbuf[:, 32:32 + cin] = cuda_t(x)
    big = torch.from_numpy(np.random.default_rng(n_out + cin2).normal(0, 1000, (n_out, cin2 + 2 * IN2_PAD)).astype(np.float32))
    x2buf = big.to(DEV)
    x2buf[:, IN2_PAD:IN2_PAD + cin2] = cuda_t(x2)
    if hl:
        xbuf, x2buf = ME.to_hl(xbuf), ME.to_hl(x2buf)
    p.xbuf, p.x2buf = xbuf, x2buf
    p.xv, p.x2v = xbuf[:, 32:32 + cin], x2buf[:, IN2_PAD:IN2_PAD + cin2]
    p.out_hl = pieces == 2
    p.obuf = out_buffer(n_out, cout, p.out_hl)
    p.out = p.obuf[:n_out, PAD:PAD + cout]
    p.shift = cuda_t(shift)
    d = _lib.ConvDesc(in_=p.xv.data_ptr(), n_in=n_in, in_ld=p.xv.stride(0), cin=cin, weight=p.wt.data_ptr(), K=K, cout=cout,
                      n_out=n_out, shift=p.shift.data_ptr(), relu=1, out=p.out.data_ptr(), out_ld=p.out.stride(0),
                      flavour=flavour, weight_x6=p.wp.data_ptr(), in2=p.x2v.data_ptr(), in2_ld=p.x2v.stride(0), cin2=cin2,
                      weight2_x6=p.wp2.data_ptr(), weight_pieces=pieces, acc_scale=acc_scale, in_hl=int(hl),
                      out_hl=int(p.out_hl), j_begin=jb, j_end=je)
    if nbr is not None:
        d.nbr = nbr.data_ptr()
    if pieces == 2:
        d.range_flag = ME.range_flag(DEV).data_ptr()
    if workspace:
        L = _lib.lib()
        nbytes = max(int(L.cv_sp_conv_workspace_bytes(n_out, cout, K)), 4 * max(groups, 1) * n_out * cout + 256)
        p.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        d.ws, d.ws_bytes = p.ws.data_ptr(), p.ws.numel()
    p.z, p.bz = so.epilogue64(p.case["y"], p.case["bound"], shift=shift, relu=True, hl_out=p.out_hl)
    if not folded:      # an epilogue scale and a residual that is not in2
        p.scale = cuda_t(scale)
        rbuf = torch.full((n_out + PAD_ROWS, cout + 2 * PAD), SENT, device=DEV)
        rbuf[:n_out, PAD:PAD + cout] = cuda_t(res)
        p.rbuf = ME.to_hl(rbuf) if hl else rbuf
        p.res = p.rbuf[:n_out, PAD:PAD + cout]
        d.scale, d.residual, d.res_ld, d.res_hl = p.scale.data_ptr(), p.res.data_ptr(), p.res.stride(0), int(hl)
        p.z, p.bz = so.epilogue64(p.case["y"], p.case["bound"], scale=scale, shift=shift, res=res, res_hl=hl, relu=True,
                                  hl_out=p.out_hl)
    if groups > 1:
        if -(-K // groups) <= ts.WP_NPRE:
            p.perms = ME._perms_with_map(nbr, groups)
            d.perm_has_map = 1
        else:               # groups wider than 10 offsets: the orders without their map rows (conv_rows_wp's 28-offset instance)
            p.perms = _manager(n, kind).mask_perms(k, 1, groups)
        d.row_perm, d.perm_groups = p.perms.data_ptr(), groups
    if tickets:
        p.tickets = torch.zeros(4096, dtype=torch.int32, device=DEV)
        d.split_tickets = p.tickets.data_ptr()
    p.d = d
    return p


def launch(p, target=None, options=()):
    """cv_sp_conv_f32 on the prepared descriptor under the kernel's options and a split target of the calling thread;
    returns the return code (the options and the target are restored)"""
    L = _lib.lib()
    opts = list(options)
    if p.kernel.startswith("hd"):
        opts += [("hd_mask", 7), ("hd_min_rows", 1), ("hd_shape", int(p.kernel[2]))]
    prev = []
    prev_t = L.cv_sp_set_split_target_thread(target) if target is not None else None
    try:
        for name, val in opts:
            prev.append((name, ME.set_option(name, val)))
        with torch.cuda.device(DEV):
            rc = L.cv_sp_conv_f32(ctypes.byref(p.d), _lib.stream(DEV))
        torch.cuda.synchronize()
    finally:
        for name, val in reversed(prev):
            ME.set_option(name, val)
        if prev_t is not None:
            L.cv_sp_set_split_target_thread(prev_t)
    return rc


def run_two(kernel, *shape, target=None, options=(), what="", **kw):
    """one two-source launch, checked element by element; returns the output window (float64)"""
    p = prepare(kernel, *shape, **kw)
    rc = launch(p, target, options)
    _lib.check(rc, "cv_sp_conv_f32")
    got = read_out(p.obuf, p.n_out, p.cout, p.out_hl)
    what = what or "%s %s %s" % (kernel, shape, kw)
    ok, i, r = so.within(got, p.z, p.bz)
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    check(got, p.z, p.bz, what)
    if kw.get("tickets"):
        assert int(p.tickets.abs().sum()) == 0
    assert flag_value() == 0, what
    return got


# ---- tile tails ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_tile_tails(kernel):
    """n_out around the 128-row tile; conv_hd's workgroups hold 256 (shapes 0, 2) or 128 rows (shape 1): at 257 rows seven
    waves of the last workgroup see no live row of the second source"""
    for n in (ts.HD_TAIL_ROWS if kernel.startswith("hd") else ts.TAIL_ROWS):
        run_two(kernel, n, "mixed", 3, 32, 64, 64)


# ---- how the chunks of in2 are dealt to the split-K slices -------------------------------------------------------------
@pytest.mark.parametrize("kernel", FAMILIES)
@pytest.mark.parametrize("deal", ts.DEAL_CASES, ids=["%dx%d_%s" % (d[0] + (d[1][2] if d[1][6] is None else "j10",)) for d in ts.DEAL_CASES])
def test_chunks_dealt_to_splits(kernel, deal):
    """(splits, Cin2 / 32): one slice with every chunk, three slices with a chunk for one / for two / two for one of
    them, 27 slices of which 25 get none; the split count pinned by the calling thread's target and asserted by the
    restated dispatcher"""
    (splits, chunks), shape, target = deal
    n, kind, k, cin, cin2, cout, jr = shape
    n_out = maps(n, kind, k)[3]
    nj = jr[1] - jr[0] if jr else ts.ksize(k)
    assert chunks == cin2 // 32
    assert ts.restated_splits(n_out, cout, nj, cin, target or SPLIT_TARGET) == splits
    if k == "down":
        assert n_out != n
    run_two(kernel, n, kind, k, cin, cin2, cout, j_range=jr, target=target)


def test_chunks_dealt_with_split_tickets():
    """conv_hl reducing its partial tiles in the last-arriving workgroup: three slices, four chunks"""
    (splits, chunks), shape, target = ts.DEAL_CASES[6]
    assert (splits, chunks) == (3, 4)
    n, kind, k, cin, cin2, cout, jr = shape
    a = run_two("hl", n, kind, k, cin, cin2, cout, target=target, tickets=True)
    b = run_two("hl", n, kind, k, cin, cin2, cout, target=target)
    assert np.array_equal(a, b), "tickets and the finish launch sum in the same order"


# ---- mask groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", FAMILIES)
@pytest.mark.parametrize("chunks", ts.GROUP_CHUNKS)
def test_three_mask_groups(kernel, chunks):
    """three offset groups in their own row orders (map rows in processing order behind the orders): the second source's
    row is the OUTPUT row taken through the group's order, its chunks are dealt to the groups"""
    got = run_two(kernel, 300, "mixed", 3, 32, 32 * chunks, 64, groups=3)
    if kernel == "hl":          # zskip: the dispatcher keeps the validity bytes off with a second source - same values
        again = run_two(kernel, 300, "mixed", 3, 32, 32 * chunks, 64, groups=3, options=(("zskip", 1),))
        assert np.array_equal(got, again)


@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("pieces", [3, 2])
def test_two_and_four_mask_groups_on_conv_rows_wp(groups, pieces):
    """two groups are 13 and 14 offsets wide (the 28-offset instance, orders without map rows), four are 6 and 7"""
    run_two("wp%d" % pieces, 300, "mixed", 3, 32, 64, 64, groups=groups)


# ---- widths and the epilogue ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cout", ts.WIDTHS)
def test_widths(kernel, cout):
    """one to four 32-column blocks per workgroup, 64-column workgroups above 96 columns (conv_hd: NB <= 3 on every one)"""
    run_two(kernel, 129, "mixed", 3, 64, 64, cout)


@pytest.mark.parametrize("kernel", KERNELS)
def test_unfolded_scale_and_a_residual_that_is_not_in2(kernel):
    """(conv + in2 @ W2) * scale + shift + residual, ReLU: the scale in the epilogue, the residual its own buffer"""
    run_two(kernel, 300, "mixed", 3, 32, 64, 96, epi="unfolded")
    run_two(kernel, 257, "mixed", "down", 64, 32, 64, epi="unfolded")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def assert_refused(p, rc, match):
    msg = (_lib.lib().cv_last_error() or b"").decode()
    full = (ME.from_hl(p.obuf) if p.out_hl else p.obuf).cpu().numpy()
    touched = not (full == SENT).all()
    if rc == 0:         # accepted: say what it computed
        got = full[:p.n_out, PAD:PAD + p.cout].astype(np.float64)
        ok, i, r = so.within(got, p.z, p.bz)
        pytest.fail("descriptor accepted; element %s is off by %.3g x its bound (got %r, fp64 %r)" %
                    (i, r, float(got[i]), float(p.z[i])))
    assert rc == -22, (rc, msg)                 # CV_EINVAL
    assert match in msg, msg
    assert not touched, "a refused launch wrote to the output window"


@pytest.mark.parametrize("kernel", ["wp3", "hl"])
@pytest.mark.parametrize("case", ["weight2_null", "cin2_40", "in2_ld_odd", "in2_misaligned"])
def test_bad_second_source_descriptors_are_refused(kernel, case):
    """every operand is a real device buffer and the misaligned in2 is a slice of a larger allocation: an accepted
    descriptor would still stay in bounds"""
    p = prepare(kernel, 300, "mixed", 3, 32, 64, 64)
    if case == "weight2_null":
        p.d.weight2_x6 = None
    elif case == "cin2_40":
        p.d.cin2 = 40
    elif case == "in2_ld_odd":
        p.d.in2_ld = p.d.in2_ld - 1
    else:
        p.d.in2 = p.x2v.data_ptr() + 4
    assert_refused(p, launch(p), "hl-format input" if kernel == "hl" and case != "weight2_null" else "second source")


def test_more_live_units_than_conv_hl_lists_is_refused():
    """one row, ten offsets in one workgroup: 10 x 1632 / 32 + 96 / 32 = 513 units > HL_MAX_UNITS = 512"""
    p = prepare("hl", 1, "mixed", 3, 1632, 96, 32, j_range=(0, 10))
    assert ts.restated_splits(1, 32, 10, 1632, 1) == 1
    assert_refused(p, launch(p, target=1), "units per workgroup")


def test_sources_of_different_formats_are_refused_by_the_executor():
    """cv_net_run_f32: an fp32 first source with an hl second source"""
    L = _lib.lib()
    n, cin, cout = 129, 32, 32
    nbr = maps(n, "mixed", 3)[0]
    p = prepare("wp2", n, "mixed", 3, cin, 32, cout)
    bufs = (_lib.NetBuf * 3)(_lib.NetBuf(-1, cin, 0, 0), _lib.NetBuf(0, 32, 0, 1), _lib.NetBuf(0, cout, 0, 0))
    op = _lib.NetOp(in_buf=0, in_col=0, cin=cin, out_buf=2, out_col=0, cout=cout, res_buf=-1, map=0, K=27, perm=-1, relu=1,
                    weight=p.wt.data_ptr(), shift=p.shift.data_ptr(), weight_x6=p.wp.data_ptr(), in2_buf=1, in2_col=0, cin2=32,
                    weight2_x6=p.wp2.data_ptr(), weight_pieces=2, acc_scale=p.d.acc_scale)
    rows = (ctypes.c_int64 * 1)(n)
    nbytes = int(L.cv_net_arena_bytes(bufs, 3, rows, 1))
    arena = torch.full((nbytes // 4,), SENT, device=DEV)
    xin = cuda_t(operands(n, n, cin, cout, 27)[0])
    ext = (ctypes.c_void_p * 1)(xin.data_ptr())
    ext_ld = (ctypes.c_int * 1)(cin)
    c_maps = (ctypes.c_void_p * 1)(nbr.data_ptr())
    with torch.cuda.device(DEV):
        rc = L.cv_net_run_f32(ctypes.byref(op), 1, bufs, 3, rows, 1, _lib.ptr(arena), nbytes, ext, ext_ld, c_maps, 1, None, 0,
                              _lib.ptr(p.ws), p.ws.numel(), None, _lib.stream(DEV))
    torch.cuda.synchronize()
    assert rc == -22 and b"share a format" in L.cv_last_error()
    assert bool((arena == SENT).all())


@pytest.mark.parametrize("route", ["flavour1", "flavour0_no_workspace"])
def test_second_source_beyond_28_offsets_per_workgroup_is_refused(route):
    """A 5x5x5 kernel in one workgroup (flavour 1, or flavour 0 without a workspace to split through) is more than
    conv_rows_wp prefetches; the fp32 kernel that takes such launches (conv_rows) has no second source.  The launch must
    be refused, not run with the second source dropped."""
    p = prepare("wp3", 300, "mixed", 5, 32, 32, 32, flavour=1 if route == "flavour1" else 0, workspace=False)
    assert_refused(p, launch(p), "second source")


def test_largest_error_over_bound_is_reported():
    """orientation only (LABNOTES): the largest error / bound each kernel reached in this module's runs"""
    print("\nsecond source, largest error / bound per kernel:", {k: round(v, 4) for k, v in sorted(WORST.items())})
