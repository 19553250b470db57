"""The network executor (cv_net_run_f32) and its model axis (cv_net_run_models_f32), op by op.

Hand-built programs of three or four ops on "mixed" coordinate sets of 300 and 129 rows run as one program and as K
models in one launch sequence.  The arena and the workspace are this module's own sentinel-filled tensors; after a run
EVERY op's output of EVERY model is read back from the arena (layout restated: buffers in order at 256-byte boundaries,
model m one cv_net_arena_bytes further) and checked per element against the float64 reference of that model's parameters
applied to that model's own decoded device input, with the per-element bounds of oracle/sparse_oracle.py - every op in
isolation, no chained error budget.  Beside it the claim of tests/test_net_models_gpu.py, per op: model m's buffers equal
the single run of program m bit for bit.  Every model has its own weights, scale and shift; the weight magnitudes differ
by powers of four, so acc_scale differs per model.

Programs: a block with the fused shortcut (second source, the caller's output per model), a plain block (residual from
the arena, a final 1x1 to 8 columns), a concat program (matrix-core stem into columns [32, 64) of a 64-channel buffer, a
down conv reading that view, an up conv writing columns [0, 32), a 1x1 over all 64).  Routes: library defaults (split-K,
conv_finish), 8 splits (conv_finish_small), three mask groups through the perms table, conv_hd, split target 1."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so
from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME
from tests import conv_two_source as ts
from tests.test_conv_paths_gpu import (DEV, PAD, PAD_ROWS, SENT, _manager, _pinned_split_target,  # noqa: F401
                                       SPLIT_TARGET, check, cuda_t, maps, operands)

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
MAP_STEM, MAP_K3, MAP_DOWN, MAP_UP = 0, 1, 2, 3
PERM_K3, PERM_UP = 0, 1
GROUPS = 3
WORST = {}


def align256(v):
    return (v + 255) // 256 * 256


def op(tag, src, dst, K, map_slot, cin, cout, in_col=0, out_col=0, res=None, relu=True, second=None, scale=True,
       perm=-1, groups=0, fold=False):
    """src / dst / res / second[0]: buffer indices; second = (buffer, column, channels); fold: the scale goes into the
    packed weights (the stem and every two-source op)"""
    return dict(tag=tag, src=src, dst=dst, K=K, map=map_slot, cin=cin, cout=cout, in_col=in_col, out_col=out_col, res=res,
                relu=relu, second=second, scale=scale, perm=perm, groups=groups, fold=fold or second is not None)


def k3(tag, src, dst, c, cout, **kw):
    return op(tag, src, dst, 27, MAP_K3, c, cout, perm=PERM_K3, groups=GROUPS, **kw)


# buffers: (level, channels, rows_level, hl); level -1: the caller's tensor, in the order "in", "out"
def shortcut_program(planes):
    bufs = [(-1, 32, 0, 1), (0, planes, 0, 1), (0, planes, 0, 1), (-1, planes, 0, 0)]
    ops = [op("conv0", 0, 1, 1, -1, 32, planes, relu=False),
           k3("conv1", 1, 2, planes, planes),
           k3("conv2", 2, 3, planes, planes, second=(1, 0, planes))]
    return "shortcut%d" % planes, bufs, ops, dict(cin=32, in_hl=True, cout=planes)


def plain_program():
    bufs = [(-1, 32, 0, 1), (0, 64, 0, 1), (0, 64, 0, 1), (0, 64, 0, 1), (-1, 8, 0, 0)]
    ops = [op("conv0", 0, 1, 1, -1, 32, 64, relu=False),
           k3("conv1", 1, 2, 64, 64),
           k3("conv2", 2, 3, 64, 64, res=1),
           op("final", 3, 4, 1, -1, 64, 8, relu=False, scale=False)]
    return "plain", bufs, ops, dict(cin=32, in_hl=True, cout=8)


def concat_program(cin):
    bufs = [(-1, cin, 0, 0), (0, 64, 0, 1), (1, 64, 1, 1), (-1, 32, 0, 0)]
    ops = [op("stem", 0, 1, 125, MAP_STEM, cin, 32, out_col=32, fold=True),
           op("down", 1, 2, 8, MAP_DOWN, 32, 64, in_col=32),
           op("up", 2, 1, 8, MAP_UP, 64, 32, perm=PERM_UP),
           op("final", 1, 3, 1, -1, 64, 32, relu=False)]
    return "concat%d" % cin, bufs, ops, dict(cin=cin, in_hl=False, cout=32)


@functools.lru_cache(maxsize=None)
def tables(n):
    """(device maps, device orders, CPU maps, level rows) of the n-row "mixed" set"""
    m5, r5, _, _ = maps(n, "mixed", 5)
    m3, r3, _, _ = maps(n, "mixed", 3)
    md, rd, _, n1 = maps(n, "mixed", "down")
    mu, ru, _, _ = maps(n, "mixed", "up")
    perms = [ME._perms_with_map(m3, GROUPS), _manager(n, "mixed").up_perm(2)]
    return [m5, m3, md, mu], perms, [r5, r3, rd, ru], [n, n1]


class Model:
    """program m with its packed weights: the cv_net_op array and what it points to"""

    def __init__(self, name, ops, m):
        self.keep, self.prm = [], []
        arr = (_lib.NetOp * len(ops))()
        for i, o in enumerate(ops):
            cin2 = o["second"][2] if o["second"] else 0
            p = ts.model_params(m, name + "/" + o["tag"], o["K"], o["cin"], o["cout"], cin2)
            self.prm.append(p)
            w = cuda_t(p["w"])
            scale = cuda_t(p["scale"]) if o["scale"] else None
            second = (cuda_t(p["w2"]), cuda_t(p["scale2"])) if cin2 else None
            wp, wp2, pieces, acc_scale, folded = ME.resolve_weights(w, w, 2, stem=o["map"] == MAP_STEM, col_scale=scale,
                                                                    second=second)
            assert pieces == 2 and folded == o["fold"]
            shift = cuda_t(p["shift"])
            self.keep += [w, scale, second, wp, wp2, shift]
            a = arr[i]
            a.in_buf, a.in_col, a.cin = o["src"], o["in_col"], o["cin"]
            a.out_buf, a.out_col, a.cout = o["dst"], o["out_col"], o["cout"]
            a.res_buf, a.res_col = (o["res"], 0) if o["res"] is not None else (-1, 0)
            a.map, a.K, a.perm, a.perm_groups, a.relu = o["map"], o["K"], o["perm"], o["groups"], int(o["relu"])
            a.weight, a.shift, a.weight_x6 = w.data_ptr(), shift.data_ptr(), wp.data_ptr()
            if scale is not None and not folded:
                a.scale = scale.data_ptr()
            a.in2_buf, a.in2_col, a.cin2 = (o["second"][0], o["second"][1], cin2) if cin2 else (-1, 0, 0)
            if cin2:
                a.weight2_x6 = wp2.data_ptr()
            a.weight_pieces, a.acc_scale = 2, acc_scale
        self.ops = arr


@functools.lru_cache(maxsize=None)
def model(name, m):
    return Model(name, PROGRAMS[name][2], m)


PROGRAMS = {p[0]: p for p in (shortcut_program(64), shortcut_program(256), plain_program(), concat_program(3),
                              concat_program(6))}


@contextlib.contextmanager
def routing(route):
    """(split target, perms table on, options) of a route, restored on exit"""
    L = _lib.lib()
    target = {"small": 24, "unsplit": 1}.get(route)
    prev_t = L.cv_sp_set_split_target_thread(target) if target else None
    prev = []
    try:
        if route == "hd":
            for name, val in (("hd_mask", 7), ("hd_min_rows", 1)):
                prev.append((name, ME.set_option(name, val)))
        yield target or SPLIT_TARGET
    finally:
        for name, val in reversed(prev):
            ME.set_option(name, val)
        if prev_t is not None:
            L.cv_sp_set_split_target_thread(prev_t)


class Run:
    """the memory of one executor call over `count` models and what came back"""


def layout(bufs, rows):
    """restated arena layout: (byte offset of every arena buffer, bytes of one arena)"""
    off, at = 0, {}
    for i, (level, ch, _, _) in enumerate(bufs):
        if level < 0:
            continue
        off = align256(off)
        at[i] = off
        off += 4 * rows[level] * ch
    one = 256 + sum(align256(4 * rows[b[0]] * b[1]) for b in bufs if b[0] >= 0)
    assert off <= one
    return at, one


def need_bytes(ops, bufs, rows, route, target):
    """largest partial-tile area an op of the program takes on this route (the restated dispatcher)"""
    need = 0
    for o in ops:
        n_out = rows[bufs[o["dst"]][2]]
        if o["map"] == MAP_STEM:
            continue
        if route == "groups" and o["groups"] > 1:
            sp = o["groups"]
        else:
            sp = ts.restated_splits(n_out, o["cout"], o["K"], o["cin"], target)
        if sp > 1:
            need = max(need, 4 * sp * n_out * o["cout"])
    return need


def execute(name, n, route, models, first=0, table=None, table_ld=None, single=False, flags=None):
    """cv_net_run_f32 (single: models = [m]) or cv_net_run_models_f32 over `models`; returns a Run"""
    L = _lib.lib()
    _, bufs, ops, io = PROGRAMS[name]
    gmaps, gperms, _, rows = tables(n)
    count = len(models)
    mods = [model(name, m) for m in models]
    r = Run()
    r.at, r.one = layout(bufs, rows)
    c_bufs = (_lib.NetBuf * len(bufs))(*[_lib.NetBuf(*b) for b in bufs])
    c_rows = (ctypes.c_int64 * 2)(*rows)
    assert r.one == int(L.cv_net_arena_bytes(c_bufs, len(bufs), c_rows, 2))
    assert count * r.one == int(L.cv_net_models_arena_bytes(c_bufs, len(bufs), c_rows, 2, count))
    r.arena = torch.full((count * r.one // 4,), SENT, device=DEV)
    # the caller's input (shared) and one sentinel-padded output per model
    x = operands(n, n, io["cin"], 32, 1, seed=5)[0]
    if io["in_hl"]:
        xbuf = torch.zeros((n, io["cin"] + 64), device=DEV)
        xbuf[:, 32:32 + io["cin"]] = cuda_t(x)
        r.xin = ME.to_hl(xbuf)[:, 32:32 + io["cin"]]
    else:
        r.xin = cuda_t(x)
    r.x = r.xin if not io["in_hl"] else ME.from_hl(r.xin)
    r.obufs = [torch.full((n + PAD_ROWS, io["cout"] + 2 * PAD), SENT, device=DEV) for _ in models]
    outs = [b[:n, PAD:PAD + io["cout"]] for b in r.obufs]
    ext_ld = (ctypes.c_int * 2)(r.xin.stride(0), outs[0].stride(0))
    exts = [(vp * 2)(r.xin.data_ptr(), o.data_ptr()) for o in outs]
    c_maps = (vp * 4)(*[g.data_ptr() for g in gmaps])
    c_perms = (vp * 2)(gperms[0].data_ptr() if route == "groups" else None, gperms[1].data_ptr() if route == "groups" else None)
    r.flags = torch.zeros((count, 16), dtype=torch.int32, device=DEV) if flags is None else flags[first:first + count]
    with routing(route) as target:
        need = need_bytes(ops, bufs, rows, route, target)
        r.need, r.ws_one = need, align256(need) + 256
        ws_bytes = int(L.cv_net_models_workspace_bytes(r.ws_one, count))
        assert ws_bytes == count * r.ws_one
        r.ws = torch.full((ws_bytes // 4,), SENT, device=DEV)
        with torch.cuda.device(DEV):
            if single:
                rc = L.cv_net_run_f32(mods[0].ops, len(ops), c_bufs, len(bufs), c_rows, 2, _lib.ptr(r.arena), r.one, exts[0],
                                      ext_ld, c_maps, 4, c_perms, 2, _lib.ptr(r.ws), ws_bytes, _lib.ptr(r.flags), _lib.stream(DEV))
            else:
                c_ops = (vp * count)(*[ctypes.cast(m.ops, vp) for m in mods])
                c_bufs_k = (vp * count)(*[ctypes.cast(c_bufs, vp)] * count)
                c_ext = (vp * count)(*[ctypes.cast(e, vp) for e in exts])
                if table is None:
                    table, table_ld = params_table([m.ops for m in mods], len(ops)), count
                entry = ctypes.sizeof(_lib.NetModelParams)
                rc = L.cv_net_run_models_f32(c_ops, c_bufs_k, len(ops), len(bufs), count, c_rows, 2, _lib.ptr(r.arena),
                                             count * r.one, c_ext, ext_ld, c_maps, 4, c_perms, 2, _lib.ptr(r.ws), ws_bytes,
                                             _lib.ptr(r.flags), vp(table.data_ptr() + entry * first), table_ld, _lib.stream(DEV))
        torch.cuda.synchronize()
    _lib.check(rc, "cv_net_run%s_f32" % ("" if single else "_models"))
    r.outs, r.models, r.bufs, r.ops, r.rows, r.n = outs, list(models), bufs, ops, rows, n
    return r


def params_table(op_arrays, n_ops):
    """cv_net_models_params_fill's host image [n_ops][K] on the device"""
    L = _lib.lib()
    K = len(op_arrays)
    nbytes = int(L.cv_net_models_params_bytes(n_ops, K))
    assert nbytes == ctypes.sizeof(_lib.NetModelParams) * n_ops * K
    host = torch.zeros(nbytes, dtype=torch.uint8)
    c_ops = (vp * K)(*[ctypes.cast(a, vp) for a in op_arrays])
    _lib.check(L.cv_net_models_params_fill(c_ops, n_ops, K, vp(host.data_ptr()), nbytes), "cv_net_models_params_fill")
    return host.to(DEV)


def raw(r, i, b):
    """buffer b of the run's i-th model as it lies in memory: [rows, channels] fp32 words"""
    level, ch, rows_level, _ = r.bufs[b]
    if level < 0:
        return r.xin if b == 0 else r.outs[i]
    start = (i * r.one + r.at[b]) // 4
    return r.arena[start:start + r.rows[level] * ch].view(r.rows[level], ch)


def decoded(r, i, b):
    v = raw(r, i, b)
    if b == 0:
        return r.x
    return ME.from_hl(v) if r.bufs[b][3] else v


def check_memory(r):
    """the caller's windows, the arena bytes between and behind the buffers and the workspace guards are untouched"""
    for i, ob in enumerate(r.obufs):
        full = ob.cpu().numpy()
        c = full.shape[1] - 2 * PAD
        assert (full[:, :PAD] == SENT).all() and (full[:, PAD + c:] == SENT).all() and (full[r.n:] == SENT).all(), \
            "model %d wrote around its output window" % r.models[i]
    mask = torch.ones(r.arena.numel(), dtype=torch.bool, device=DEV)
    for i in range(len(r.models)):
        for b, at in r.at.items():
            start = (i * r.one + at) // 4
            mask[start:start + r.rows[r.bufs[b][0]] * r.bufs[b][1]] = False
    assert bool((r.arena[mask] == SENT).all()), "arena bytes outside the buffers were written"
    for i in range(len(r.models)):
        guard = r.ws[(i * r.ws_one + r.need) // 4:(i + 1) * r.ws_one // 4]
        assert guard.numel() >= 64 and bool((guard == SENT).all()), "model %d's workspace share ran into the next" % r.models[i]
    assert int(r.flags.abs().sum()) == 0, "range flags of an in-range run"


def check_ops(r, name, route):
    """every op of every model against the float64 reference of its own decoded input"""
    cpu_maps = tables(r.n)[2]
    for i, m in enumerate(r.models):
        prm = model(name, m).prm
        for o, p in zip(r.ops, prm):
            cin, cout, K = o["cin"], o["cout"], o["K"]
            x = decoded(r, i, o["src"])[:, o["in_col"]:o["in_col"] + cin].cpu().numpy()
            got = decoded(r, i, o["dst"])[:, o["out_col"]:o["out_col"] + cout].cpu().numpy().astype(np.float64)
            nbr = cpu_maps[o["map"]] if o["map"] >= 0 else None
            hl_out = bool(r.bufs[o["dst"]][3])
            scale = p["scale"] if o["scale"] else None
            we = so.folded_weights(p["w"], scale if o["fold"] else None)
            cin2 = 0
            if o["second"]:
                sb, sc, cin2 = o["second"]
                x2 = decoded(r, i, sb)[:, sc:sc + cin2].cpu().numpy()
                y, mag, wabs = so.conv64_two(x, we, nbr, x2, so.folded_weights(p["w2"], p["scale2"]))
            else:
                y, mag, wabs = so.conv64(x, we, nbr)
            b = so.conv_bound(mag, wabs, "h2", so.conv_units_two(K, cin, cin2))
            res = decoded(r, i, o["res"])[:, :cout].cpu().numpy() if o["res"] is not None else None
            z, bz = so.epilogue64(y, b, scale=None if o["fold"] else scale, shift=p["shift"], res=res,
                                  res_hl=res is not None and bool(r.bufs[o["res"]][3]), relu=o["relu"], hl_out=hl_out)
            what = "%s n=%d route %s, model %d, op %s" % (name, r.n, route, m, o["tag"])
            assert np.abs(z).max() > 0.05, what + ": a reference of zeros checks nothing"
            key = name.rstrip("0123456789") + "/" + o["tag"]
            WORST[key] = max(WORST.get(key, 0.0), so.within(got, z, bz)[2])
            check(got, z, bz, what)


def same_bits(r, i, s, what):
    """every buffer of the run's i-th model equals the single run s"""
    for b in range(1, len(r.bufs)):
        assert torch.equal(raw(r, i, b).view(torch.int32), raw(s, 0, b).view(torch.int32)), "%s: buffer %d" % (what, b)


def run_case(name, n, route, counts):
    singles = {}
    for K in counts:
        models = list(range(K))
        r = execute(name, n, route, models)
        check_memory(r)
        check_ops(r, name, route)
        for i, m in enumerate(models):
            if m not in singles:
                singles[m] = execute(name, n, route, [m], single=True)
                check_memory(singles[m])
                if m == 0:
                    check_ops(singles[m], name, route)
            same_bits(r, i, singles[m], "%s n=%d route %s, %d models, model %d" % (name, n, route, K, m))


ROUTES = ("default", "small", "groups", "hd", "unsplit")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["shortcut64", "plain", "concat3"])
def test_programs_per_op_on_every_route(name, route):
    """300 rows, K = 1, 2, 3 on the default route, 3 on the others"""
    run_case(name, 300, route, (1, 2, 3) if route == "default" else (3,))


@pytest.mark.parametrize("name", ["shortcut64", "plain", "concat6"])
def test_programs_on_129_rows(name):
    """two tiles, one of a single row; the 6-channel stem"""
    run_case(name, 129, "default", (2,))
    run_case(name, 129, "groups", (3,))


@pytest.mark.parametrize("name", ["shortcut64", "shortcut256", "concat3"])
def test_sixteen_models(name):
    """K = 16 (CV_MAX_CATEGORIES); with 256 columns grid.y = 16 x 4"""
    run_case(name, 300, "default", (16,))


@pytest.mark.parametrize("name", ["shortcut64", "plain", "concat3"])
def test_five_models_in_passes_of_two(name):
    """passes of 2, 2 and 1 over one table of five models: the table pointer advances by the pass's first model,
    params_ld stays 5 (pipeline.forward_models); the range flags move 64 bytes per model"""
    _, bufs, ops, _ = PROGRAMS[name]
    table = params_table([model(name, m).ops for m in range(5)], len(ops))
    flags = torch.zeros((5, 16), dtype=torch.int32, device=DEV)
    for first in (0, 2, 4):
        models = list(range(first, min(first + 2, 5)))
        r = execute(name, 300, "default", models, first=first, table=table, table_ld=5, flags=flags)
        assert r.flags.data_ptr() == flags.data_ptr() + 64 * first
        check_memory(r)
        check_ops(r, name, "default, pass from model %d" % first)
        for i, m in enumerate(models):
            same_bits(r, i, execute(name, 300, "default", [m], single=True), "%s pass from %d, model %d" % (name, first, m))


def test_largest_error_over_bound_is_reported():
    """orientation only (LABNOTES): the largest error / bound per op kind over this module's runs"""
    print("\nnetwork programs, largest error / bound per op:", {k: round(v, 4) for k, v in sorted(WORST.items())})
