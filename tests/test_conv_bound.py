"""CPU checks of the float64 convolution oracle and its per-element bound (oracle/sparse_oracle.py ERROR_MODEL) that
tests/test_conv_paths_gpu.py holds the HIP kernels to, and of the host-only weight-gradient plan knobs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(seed=0):
    """a dense 9 x 9 x 5 box, a sheet and isolated voxels: rows with 27 down to 1 neighbour"""
    box = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    sheet = np.stack(np.meshgrid(np.arange(6), np.arange(6), [0], indexing="ij"), -1).reshape(-1, 3) + [20, 0, 0]
    iso = np.stack([np.arange(12) * 3, np.full(12, 40), np.full(12, 40)], -1)
    pair = np.array([[60, 60, 60], [61, 60, 60]])
    c = np.concatenate([box, sheet, iso, pair])
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)


def _fp16_high(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def _case(cin=32, cout=32, seed=0):
    coords = _scene(seed)
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (len(coords), cin)).astype(np.float32)
    w = (rng.normal(0, 1, (27, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    nbr = so.kernel_map(coords, coords, 3, 1, 1)
    return x, w, nbr


def test_fp64_oracle_matches_the_fp32_oracle_and_bounds_it():
    """y64 agrees with the torch fp32 oracle within the fp32-MFMA bound (a correct fp32 evaluation passes)"""
    x, w, nbr = _case(64, 96)
    y64, mag, wabs = so.conv64(x, w, nbr)
    y32 = so.conv(torch.from_numpy(x), torch.from_numpy(w), nbr).numpy()
    ok, i, r = so.within(y32, y64, so.conv_bound(mag, wabs, "f32", so.conv_units(27, 64)))
    assert ok, (i, r)
    assert r < 0.05                         # fp32 summation sits far inside the worst-case bound
    # mag is the sum of |terms|: never below |y|, equal for a single-term row of same-sign products
    assert (mag + 1e-12 >= np.abs(y64)).all()


@pytest.mark.parametrize("path", ["f32", "x6", "h2"])
def test_bound_rejects_one_dropped_contribution(path):
    """(a) the oracle output with the contribution of one (row, offset) removed, on the valid row of smallest mag that
    has at least two neighbours, is outside the bound of every path"""
    x, w, nbr = _case()
    y64, mag, wabs = so.conv64(x, w, nbr)
    nn = (nbr >= 0).sum(1)
    rows = np.nonzero(nn >= 2)[0]
    u = rows[np.argmin(mag[rows].sum(1))]
    j = [jj for jj in range(27) if nbr[u, jj] >= 0 and jj != 13][0]
    bad = y64.copy()
    bad[u] -= x[nbr[u, j]].astype(np.float64) @ w[j].astype(np.float64)
    b = so.conv_bound(mag, wabs, path, so.conv_units(27, 32))
    assert so.within(y64, y64, b)[0]
    ok, i, r = so.within(bad, y64, b)
    assert not ok and i[0] == u, (i, r)
    # the same through the epilogue (scale, shift, residual) and an hl-format output
    rng = np.random.default_rng(1)
    sc, sh = rng.uniform(0.5, 1.5, 32), rng.normal(0, 0.2, 32)
    res = rng.normal(0, 1, y64.shape)
    z, bz = so.epilogue64(y64, b, scale=sc, shift=sh, res=res, hl_out=True)
    assert so.within(z, z, bz)[0] and not so.within(bad * sc + sh + res, z, bz)[0]


def test_bound_rejects_fp16_high_pieces_only():
    """(b) products of the fp16 high pieces alone (the fp16-pair path without its low pieces) are outside the h2 bound"""
    x, w, nbr = _case()
    y64, mag, wabs = so.conv64(x, w, nbr)
    yh, _, _ = so.conv64(_fp16_high(x), _fp16_high(w), nbr)
    assert not so.within(yh, y64, so.conv_bound(mag, wabs, "h2", so.conv_units(27, 32)))[0]
    # ... while the pair (h + l, ll dropped) is inside it
    xh, wh = _fp16_high(x), _fp16_high(w)
    xl, wl = _fp16_high(x - xh), _fp16_high(w - wh)
    yp = so.conv64(xh, wh, nbr)[0] + so.conv64(xh, wl, nbr)[0] + so.conv64(xl, wh, nbr)[0]
    assert so.within(yp, y64, so.conv_bound(mag, wabs, "h2", so.conv_units(27, 32)))[0]


def test_bf16_mode_oracle_is_independent_of_the_fp32_result():
    """the bf16 mode's yardstick is y64 of the RNE-rounded operands: the unrounded y64 is outside its bound"""
    x, w, nbr = _case()
    xr, wr = so.bf16_round(x), so.bf16_round(w)
    assert np.abs(xr - x).max() > 0 and (np.abs(xr - x) <= np.abs(x) * 2.0 ** -8).all()
    y64, mag, wabs = so.conv64(xr, wr, nbr)
    yfull = so.conv64(x, w, nbr)[0]
    assert not so.within(yfull, y64, so.conv_bound(mag, wabs, "bf16", so.conv_units(27, 32)))[0]


def test_wgrad_oracle_and_bound():
    x, w, nbr = _case(32, 64)
    rng = np.random.default_rng(5)
    dy = rng.normal(0, 1, (nbr.shape[0], 64))
    dw, mag = so.wgrad64(x, dy, nbr, 27)
    xt = torch.from_numpy(x).double().requires_grad_(False)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    so.conv(xt, wt, nbr).mul(torch.from_numpy(dy)).sum().backward()
    assert np.allclose(wt.grad.numpy(), dw, rtol=0, atol=1e-12)
    b = so.wgrad_bound(mag, "x6", nbr.shape[0])
    bad = dw.copy()
    u = int(np.nonzero((nbr >= 0).sum(1) >= 2)[0][0])
    bad[13] -= np.outer(x[nbr[u, 13]], dy[u])          # one row's contribution to the centre offset dropped
    assert so.within(dw, dw, b)[0] and not so.within(bad, dw, b)[0]


# ---- the two-source bound separates the defects the second-source and network-program tests exist for ----------------
def _worst(bad, case):
    return float((np.abs(bad - case["y"]) / case["bound"]).max())


def test_two_source_reference_adds_both_sources():
    from tests import conv_two_source as ts
    c = ts.two_source(129, "mixed", 3, 32, 64, 32, 3)
    x, w, scale = ts.operands(129, 129, 32, 32, 27)[:3]
    x2, w2, scale2 = ts.second_operands(129, 64, 32)
    y1, m1, a1 = so.conv64(x, so.folded_weights(w, scale), c["ref"])
    w2e = so.folded_weights(w2, scale2)[0]
    assert np.array_equal(c["y"], y1 + x2.astype(np.float64) @ w2e)
    assert np.array_equal(c["mag"], m1 + np.abs(x2).astype(np.float64) @ np.abs(w2e))
    assert np.array_equal(c["wabs"], a1 + np.abs(w2e).sum(0)[None])
    assert so.conv_units_two(27, 32, 64) == 29 and so.conv_units_two(10, 40, 128) == 24
    # the fold is one fp32 rounding of the product; the bf16 packer rounds that once more
    assert np.array_equal(so.folded_weights(w, scale), (w * scale).astype(np.float32).astype(np.float64))
    assert np.array_equal(so.folded_weights(w, scale, bf16=True), so.bf16_round((w * scale).astype(np.float32)))


@pytest.mark.parametrize("pieces", [3, 2, 1])
def test_two_source_bound_rejects_a_lost_or_misplaced_second_source(pieces):
    """(i) the second source absent, (ii) its last chunk dropped, (iii) x2 read at the tile position for one mask group:
    each more than twice the bound on some element of every shape tests/test_conv_second_source_gpu.py runs"""
    from tests import conv_two_source as ts
    seen = set()
    for n, kind, k, cin, cin2, cout, jr, groups in ts.section1_shapes():
        jb, je = jr if jr else (0, None)
        c = ts.two_source(n, kind, k, cin, cin2, cout, pieces, jb, je)
        assert so.within(c["y"], c["y"], c["bound"])[0]
        for name, bad in ts.defects(c, groups):
            if name.startswith("tile") and n == 1:
                continue
            r = _worst(bad, c)
            assert r > 2, "%s at %s: only %.3g x the bound" % (name, (n, kind, k, cin, cin2, cout, jr, groups), r)
            seen.add(name)
    assert len(seen) == 3


@pytest.mark.parametrize("cout", [64, 256])
def test_two_source_bound_rejects_the_neighbour_models_parameters(cout):
    """(iv) model m's two-source conv with model m - 1's shift, and separately with its w2, on the parameters of
    tests/test_net_program_gpu.py (stand-in activations of the same scale)"""
    from tests import conv_two_source as ts
    ref = ts.ref_map(300, "mixed", 3)[0]
    x = ts.operands(300, 300, 64, cout, 27)[0]
    x2 = ts.second_operands(300, 64, cout)[0]
    for m in range(1, 16):
        p, q = (ts.model_params(mm, "shortcut/conv2", 27, 64, cout, 64) for mm in (m, m - 1))
        we, w2e = so.folded_weights(p["w"], p["scale"]), so.folded_weights(p["w2"], p["scale2"])
        y, mag, wabs = so.conv64_two(x, we, ref, x2, w2e)
        b = so.conv_bound(mag, wabs, "h2", so.conv_units_two(27, 64, 64))
        z, bz = so.epilogue64(y, b, shift=p["shift"], relu=True, hl_out=True)
        z_shift = so.epilogue64(y, b, shift=q["shift"], relu=True)[0]
        y_w2 = so.conv64_two(x, we, ref, x2, so.folded_weights(q["w2"], q["scale2"]))[0]
        z_w2 = so.epilogue64(y_w2, b, shift=p["shift"], relu=True)[0]
        for name, bad in (("shift", z_shift), ("w2", z_w2)):
            r = float((np.abs(bad - z) / bz).max())
            assert r > 2, "model %d with model %d's %s: only %.3g x the bound" % (m, m - 1, name, r)


WS_CODE = ("import sys; sys.path.insert(0, sys.argv[1]); from canonicalvoting_amd import _lib; "
           "print(int(_lib.lib().cv_sp_wgrad_workspace_bytes(20000, 64, 64, 27)), "
           "int(_lib.lib().cv_sp_wgrad_workspace_bytes(20000, 32, 32, 8)))")


def _ws_bytes(**env):
    e = dict(os.environ)
    for k in ("CV_WGRAD_MULT", "CV_WGRAD_TASKS", "CV_WGRAD_CAP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", WS_CODE, ROOT], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (env, r.returncode, r.stderr[-2000:])
    return tuple(int(v) for v in r.stdout.split())


def test_wgrad_plan_knobs_are_clamped(built_lib):
    """CV_WGRAD_MULT / CV_WGRAD_TASKS / CV_WGRAD_CAP are read once per process: every setting in a fresh child.  Zero or
    negative values act as 1 (0,0,0 made the per-offset split sum zero and the plan divided by it)."""
    ones = _ws_bytes(CV_WGRAD_MULT="1,1,1")
    assert min(ones) > 256
    assert _ws_bytes(CV_WGRAD_MULT="0,0,0") == ones
    assert _ws_bytes(CV_WGRAD_MULT="-3,-1,-2") == ones
    assert _ws_bytes(CV_WGRAD_TASKS="1") == _ws_bytes(CV_WGRAD_TASKS="0") == _ws_bytes(CV_WGRAD_TASKS="-5")
    assert _ws_bytes(CV_WGRAD_CAP="1") == _ws_bytes(CV_WGRAD_CAP="0") == _ws_bytes(CV_WGRAD_CAP="-1")
    assert min(_ws_bytes(CV_WGRAD_CAP="-1")) > 256
