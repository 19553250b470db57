"""The row kernels and the heads, each entry point as a pure function of its own inputs through the C ABI, against the
float64 oracle with a bound per output element (oracle/sparse_oracle.py ROW_ERROR_MODEL, pinned on the CPU by
tests/test_row_bound.py).  Every output lives in a sentinel-filled allocation (PAD words in front and behind, the columns
[c, ld) of every row, PAD_ROWS rows below); misaligned and odd-ld operands are slices of larger allocations; workspaces are
NaN-filled before every call.

kernel (all of them in csrc/row_ops.hip) -> test (every dispatch branch of the entry points):
  affine_rows4            test_affine_sizes (c % 4 == 0), test_affine_switches, test_affine_in_place,
                          test_affine_grid_caps[rows4] (second grid-stride trip past 16384 blocks)
  affine_rows             test_affine_sizes (c = 3, 30), test_affine_scalar_reasons (c % 4, x_ld, y_ld, res_ld, base,
                          scale vector), test_affine_grid_caps[rows] (past 8192 blocks)
  affine_rows4 + hl twin  test_affine_hl (hl bits, ReLU bit words, range flag), test_backward[bits] reads the words back
  to_hl / from_hl         test_hl_format, test_hl_format_grid_cap (past 8192 blocks), test_hl_format_refusals
  bn_fold                 test_bn_fold
  col_sum                 test_col_sums (cv_sp_col_sum_f32), chunks 1, 2 and the 256 cap
  col_sum_partial/_chunks test_col_sums (cv_sp_col_sum_det_f32); both block sums are one body, col_block_sum, and the chunk
                          sum is sum_in_order4 of sparse_conv_common.h (shared with wgrad_reduce, sparse_train.hip)
  bn_col_reduce4<0>       test_bn_stats (c = 4 ... 1024: rl = 256 ... 1, idle threads at c = 96 and 384; n around the
                          four-rows-in-flight loop and the chunk thresholds), test_bn_stats_chunk_cap
  bn_col_reduce<0>        test_bn_stats_scalar (c % 4, c > 1024, odd ld, misaligned base)
  bn_col_finish<0/1>      every statistics / backward test (chunks 1 ... 1024)
  bn_col_reduce4<1>       test_backward (mask: none, y rows, bit words)
  bn_col_reduce<1>        test_backward[scalar cases]
  bn_backward_apply4      test_backward, test_backward_grid_caps[apply4] (past 16384 blocks)
  bn_backward_apply       test_backward[scalar cases], test_backward_grid_caps[apply] (past 8192 blocks)
  bn_backward_apply4 twin test_backward_twin (slot maxima, scale exponent and its escapes, inverse word, range flag; grids
                          below and past the 4096-block cap), test_backward_refusals
  head_joint              test_head_joint
  head_separate(_models)  test_head_separate (one row body, head_separate_row, under both)
"""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so
from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME
from tests.test_row_bound import bn_chunks, col_chunks, head_rows

pytestmark = pytest.mark.gpu

SENT = -7.0
SENT_I = 0x5A5A5A5A
PAD = 32                    # sentinel words in front of and behind every output (keeps 128-byte alignment)
PAD_ROWS = 5                # sentinel rows below
EPS = 1e-5
MOM = 0.1
DEV = torch.device("cuda:0")
f32 = np.float32
RATIOS = {}                 # quantity -> worst error-to-bound ratio of this run (test_zz_report prints the table)
T0 = time.time()


def cuda_t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


HL_SENT = so.hl_bits(np.full((1, 32), SENT, f32))[0]          # the 32 words of a chunk of sentinels in the hl format


class Win:
    """one real allocation filled with sentinels and the [n, c] window of leading dimension ld inside it, `mis` words off
    the 128-byte alignment, starting at column col0.  hl: the allocation is sentinel-filled, then converted as out_buffer of
    test_conv_paths_gpu does; read() compares the raw words"""

    def __init__(self, n, c, ld=None, data=None, mis=0, col0=0, hl=False, dtype=torch.float32):
        ld = c if ld is None else ld
        assert ld >= col0 + c and (not hl or (mis == 0 and ld % 32 == 0 and col0 % 32 == 0 and c % 32 == 0))
        self.n, self.c, self.ld, self.mis, self.col0, self.hl = n, c, ld, mis, col0, hl
        self.sent = SENT_I if dtype == torch.int32 else SENT
        total = PAD + mis + (n + PAD_ROWS) * ld + PAD
        self.flat = torch.full((total,), self.sent, dtype=dtype, device=DEV)
        if hl:
            self.flat = ME.to_hl(self.flat.view(-1, 32)).view(-1)
        a = PAD + mis
        self.t = self.flat[a:a + n * ld].view(n, ld)[:, col0:col0 + c]
        if data is not None:
            self.t.copy_(cuda_t(data))

    def read(self):
        """the window (fp32 values, int32 words, or the uint32 words of an hl window) after checking that every word
        outside it still holds the sentinel"""
        full = self.flat.view(torch.int32).cpu().numpy().view(np.uint32) if self.hl else self.flat.cpu().numpy()
        idx = (PAD + self.mis + np.arange(self.n)[:, None] * self.ld + self.col0 + np.arange(self.c)[None, :]).ravel()
        outside = np.ones(full.shape[0], bool)
        outside[idx] = False
        want = np.tile(HL_SENT, full.shape[0] // 32) if self.hl else self.sent
        assert (full[outside] == (want[outside] if self.hl else want)).all(), "writes outside the window"
        return full[idx].reshape(self.n, self.c)


def vec(c, data=None):
    return Win(1, c, ld=(c + 3) // 4 * 4, data=None if data is None else np.asarray(data).reshape(1, c))


def misaligned_vec(data):
    buf = torch.zeros(len(data) + 8, device=DEV)
    buf[1:1 + len(data)] = cuda_t(data)
    return buf[1:1 + len(data)]


@functools.lru_cache(maxsize=8)
def case(n, c):
    return so.row_case(n, c)


def check(got, ref, bound, what, key):
    ok, i, r = so.within(got, ref, bound)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert ok, "%s %s: element %s off by %.3g x its bound (got %r, fp64 %r, bound %.3g)" % (
        key, what, i, r, float(np.asarray(got)[i]), float(ref[i]), float(bound[i]))


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


def hl_pieces(words):
    """uint16 (h, l) per element [n, c] of hl words [n, c]"""
    n, c = words.shape
    p = np.ascontiguousarray(words, np.uint32).view(np.uint16).reshape(n, c // 32, 2, 32)
    return p[:, :, 0].reshape(n, c), p[:, :, 1].reshape(n, c)


def check_hl_bits(words, values, what):
    """the hl words against hl_bits(values): the same bits for 2^-14 <= |v| <= 65000, within 2^-25 below"""
    values = np.ascontiguousarray(values, f32)
    h, l = hl_pieces(words)
    hr, lr = hl_pieces(so.hl_bits(values))
    a = np.abs(values)
    exact = (a >= 2.0 ** -14) & (a <= 65000.0)
    bad = exact & ((h != hr) | (l != lr))
    assert not bad.any(), "%s: %d of %d hl elements differ, first at %s" % (what, bad.sum(), exact.sum(), np.argwhere(bad)[0])
    small = a < 2.0 ** -14
    dec = so.hl_decode(words).astype(np.float64)
    assert (np.abs(dec - values)[small] <= 2.0 ** -25).all(), what


def pack_bits(open_):
    n, c = open_.shape
    return (open_.reshape(n, c // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ---- affine -----------------------------------------------------------------------------------------------------------
def run_affine(n, c, scale=True, shift=True, res=True, relu=True, x_ld=None, y_ld=None, res_ld=None, mis=0,
               in_place=False, scale_mis=False, what=""):
    d = case(n, c)
    x_ld = c + 32 if x_ld is None else x_ld
    y_ld = c + 64 if y_ld is None else y_ld
    res_ld = c + 32 if res_ld is None else res_ld
    xw = Win(n, c, x_ld, d["x"], mis=mis)
    yw = xw if in_place else Win(n, c, y_ld)
    rw = Win(n, c, res_ld, d["res"]) if res else None
    sc = (misaligned_vec(d["gamma"]) if scale_mis else cuda_t(d["gamma"])) if scale else None
    sh = cuda_t(d["beta"]) if shift else None
    ME.affine_forward(xw.t, sc, sh, relu, out=yw.t, residual=rw.t if res else None)
    got = yw.read()
    z, b = so.affine64(d["x"], d["gamma"] if scale else None, d["beta"] if shift else None, d["res"] if res else None, relu)
    check(got, z, b, "n=%d c=%d %s" % (n, c, what), "affine")
    if res:
        assert np.array_equal(rw.read(), d["res"])
    if not in_place:
        assert np.array_equal(xw.read(), d["x"])


@pytest.mark.parametrize("c", [3, 4, 30, 32, 96, 1028])
def test_affine_sizes(c):
    for n in (1, 63, 64, 65, 257):
        run_affine(n, c)


@pytest.mark.parametrize("c", [30, 96])
def test_affine_switches(c):
    """scale / shift / residual / relu one by one: ReLU only, a scale without a shift, ..."""
    for scale, shift, res, relu in ((False, False, False, True), (True, False, False, False), (True, True, False, False),
                                    (False, False, True, False), (True, False, True, True), (False, False, True, True)):
        run_affine(65, c, scale, shift, res, relu, what="scale=%d shift=%d res=%d relu=%d" % (scale, shift, res, relu))


@pytest.mark.parametrize("reason", ["c", "x_ld", "y_ld", "res_ld", "base", "scale"])
def test_affine_scalar_reasons(reason):
    """each reason for the scalar kernel in turn, every other operand fit for float4"""
    for n, c in ((65, 96), (257, 32)):
        kw = {"c": dict(), "x_ld": dict(x_ld=c + 33), "y_ld": dict(y_ld=c + 33), "res_ld": dict(res_ld=c + 35),
              "base": dict(mis=1), "scale": dict(scale_mis=True)}[reason]
        run_affine(n, c - 2 if reason == "c" else c, what=reason, **kw)


def test_affine_in_place():
    for n, c in ((65, 96), (257, 30)):
        run_affine(n, c, in_place=True, what="in place")
        run_affine(n, c, scale=False, shift=False, res=False, in_place=True, what="ReLU in place")


@pytest.mark.parametrize("kernel", ["rows4", "rows"])
def test_affine_grid_caps(kernel):
    """one case past each grid cap: the grid-stride loop takes a second trip"""
    if kernel == "rows4":
        assert (131073 * 32 + 255) // 256 > 16384
        run_affine(131073, 128, x_ld=128, y_ld=128, res_ld=128, what="past 16384 blocks")
    else:
        assert (70001 * 37 + 255) // 256 > 8192
        run_affine(70001, 37, x_ld=48, y_ld=48, res_ld=48, what="past 8192 blocks")


def test_affine_shift_without_scale_is_refused():
    """the kernels apply the (scale, shift) pair or neither: a lone shift must not be dropped silently"""
    d = case(65, 96)
    xw, yw = Win(65, 96, data=d["x"]), Win(65, 96)
    with pytest.raises(_lib.CvError, match=r"\(-22\)"):
        ME.affine_forward(xw.t, None, cuda_t(d["beta"]), False, out=yw.t)
    hw, bw = Win(65, 96, hl=True), Win(65, 3, dtype=torch.int32)
    with pytest.raises(_lib.CvError, match=r"\(-22\)"):
        ME.affine_forward(xw.t, None, cuda_t(d["beta"]), False, out=yw.t, out_hl=hw.t, relu_bits=bw.t)
    yw.read(), hw.read(), bw.read()


@pytest.mark.parametrize("c", [32, 96, 384])
def test_affine_hl(c):
    """the hl twin and the ReLU bit words of cv_sp_affine_hl_f32"""
    for n in (1, 7, 8, 9, 257):
        d = case(n, c)
        for relu in (True, False) if n == 257 else (True,):
            xw, rw = Win(n, c, c + 32, d["x"]), Win(n, c, c + 4, d["res"])
            yw, hw, bw = Win(n, c, c + 64), Win(n, c, c + 64, col0=32, hl=True), Win(n, c // 32, dtype=torch.int32)
            ME.affine_forward(xw.t, cuda_t(d["gamma"]), cuda_t(d["beta"]), relu, out=yw.t, residual=rw.t, out_hl=hw.t,
                              relu_bits=bw.t)
            y, words, bits = yw.read(), hw.read(), bw.read().view(np.uint32)
            what = "n=%d c=%d relu=%d" % (n, c, relu)
            z, b = so.affine64(d["x"], d["gamma"], d["beta"], d["res"], relu)
            check(y, z, b, what, "affine")
            check_hl_bits(words, y, what)
            zh, bh = so.affine64(d["x"], d["gamma"], d["beta"], d["res"], relu, hl_out=True)
            check(so.hl_decode(words), zh, bh, what, "affine hl twin")
            assert np.array_equal(bits, pack_bits(y > 0)), what
            sure = np.abs(z) > b
            got_open = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, c).astype(bool)
            assert np.array_equal(got_open[sure], (z > 0)[sure]), what
            assert flag_value() == 0


def test_affine_hl_range_flag():
    n, c = 9, 96
    x = case(n, c)["x"].copy()
    for plant in (False, True):
        if plant:
            x[5, 70] = 7e4
        xw, yw, hw = Win(n, c, data=x), Win(n, c), Win(n, c, hl=True)
        ME.affine_forward(xw.t, None, None, True, out=yw.t, out_hl=hw.t)
        assert np.array_equal(yw.read(), np.maximum(x, 0))
        hw.read()
        assert flag_value() == int(plant)


# ---- hl format -----------------------------------------------------------------------------------------------------------
def to_hl(xw, hw, flag=None):
    f = ME.range_flag(DEV) if flag is None else flag
    return _lib.lib().cv_sp_to_hl_f32(P(xw.t), xw.n, xw.c, xw.t.stride(0), P(hw.t), hw.t.stride(0), f.data_ptr(), stream())


def from_hl(hw, yw):
    return _lib.lib().cv_sp_from_hl_f32(P(hw.t), hw.n, hw.c, hw.t.stride(0), P(yw.t), yw.t.stride(0), stream())


def run_format(n, c, x_ld, h_ld, col0, y_ld, mis=0):
    x = case(n, c)["x"].copy()
    x.ravel()[:6] = [0.0, 2.0 ** -14, 3e-6, -2.0 ** -24, 65000.0, -1e-7][:min(6, x.size)]
    xw, hw, yw = Win(n, c, x_ld, x, mis=mis), Win(n, c, h_ld, col0=col0, hl=True), Win(n, c, y_ld, mis=mis)
    _lib.check(to_hl(xw, hw), "cv_sp_to_hl_f32")
    words = hw.read()
    check_hl_bits(words, x, "to_hl n=%d c=%d" % (n, c))
    _lib.check(from_hl(hw, yw), "cv_sp_from_hl_f32")
    assert np.array_equal(yw.read(), so.hl_decode(words)), "from_hl n=%d c=%d" % (n, c)
    assert np.array_equal(hw.read(), words) and flag_value() == 0


@pytest.mark.parametrize("c", [32, 96, 128])
def test_hl_format(c):
    """bits against hl_bits, the round trip against float32(h) + float32(l); windows that start at column 32 of a wider
    buffer; an fp32 side whose leading dimension is no multiple of 4 and whose base is not 16-byte aligned"""
    for n in (1, 9, 257):
        run_format(n, c, c, c, 0, c)
        run_format(n, c, c + 33, c + 64, 32, c + 1, mis=1)


def test_hl_format_grid_cap():
    assert (65537 * 32 + 255) // 256 > 8192
    run_format(65537, 128, 128, 128, 0, 128)


def test_hl_format_refusals():
    """c % 32 != 0 and an hl base that is not 128-byte aligned: CV_EINVAL, nothing written"""
    x = case(9, 96)["x"]
    xw, hw, yw = Win(9, 48, 96, x[:, :48]), Win(9, 96, 128, hl=True), Win(9, 48, 96)
    L = _lib.lib()
    f = ME.range_flag(DEV).data_ptr()
    assert L.cv_sp_to_hl_f32(P(xw.t), 9, 48, 96, P(hw.t), 128, f, stream()) == -22
    assert L.cv_sp_from_hl_f32(P(hw.t), 9, 48, 128, P(yw.t), 96, stream()) == -22
    off = hw.flat[PAD + 4:]                          # 16 bytes past a row start: inside the allocation, not 128-byte aligned
    assert off.data_ptr() % 128 == 16
    xw = Win(9, 96, data=x)
    yw2 = Win(9, 96)
    assert L.cv_sp_to_hl_f32(P(xw.t), 9, 96, 96, P(off), 128, f, stream()) == -22
    assert L.cv_sp_from_hl_f32(P(off), 9, 96, 128, P(yw2.t), 96, stream()) == -22
    hw.read(), yw.read(), yw2.read()


# ---- bn_fold --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 127, 128, 129])
@pytest.mark.parametrize("bias", [False, True])
def test_bn_fold(c, bias):
    d = case(7, c)
    var = np.abs(d["running_var"])
    if c >= 3:
        var[c - 1] = 0.0                                 # eps decides
        var[c // 2] = 1e-7
    sw, hw = vec(c), vec(c)
    ins = [cuda_t(a) for a in (d["gamma"], d["beta"], d["running_mean"], var)]
    bt = cuda_t(d["bias"]) if bias else None
    _lib.check(_lib.lib().cv_sp_bn_fold_f32(*[P(t) for t in ins], P(bt), EPS, c, P(sw.t), P(hw.t), stream()), "cv_sp_bn_fold_f32")
    (s, bs), (h, bh) = so.bn_fold64(d["gamma"], d["beta"], d["running_mean"], var, d["bias"] if bias else None, EPS)
    check(sw.read()[0], s, bs, "c=%d" % c, "fold scale")
    check(hw.read()[0], h, bh, "c=%d" % c, "fold shift")


# ---- column sums ---------------------------------------------------------------------------------------------------------
COL_LD = 67


@functools.lru_cache(maxsize=1)
def col_data():
    x = so.row_case(262145, 64)["x"]
    buf = torch.full((262145, COL_LD), SENT, device=DEV)          # (the gap columns hold sentinels: a wrong column shows)
    buf[:, :64] = cuda_t(x)
    return x, buf


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1024, 1025, 262144, 262145])
def test_col_sums(n):
    """both entry points, ld > c; the chunk count restated from row_ops.hip (1, 2 and the 256 cap)"""
    x, buf = col_data()
    L = _lib.lib()
    chunks = col_chunks(n)
    s64, b64 = so.col_sum64(x[:n], chunks)
    for c in (1, 3, 31, 32, 33, 64):
        assert int(L.cv_sp_col_sum_workspace_bytes(n, c)) == 4 * chunks * c
        ws = torch.full((chunks * c + PAD,), float("nan"), device=DEV)
        for det in (True, False):
            ow = vec(c)
            if det:
                rc = L.cv_sp_col_sum_det_f32(P(buf), n, c, COL_LD, P(ow.t), P(ws), 4 * chunks * c, stream())
            else:
                rc = L.cv_sp_col_sum_f32(P(buf), n, c, COL_LD, P(ow.t), stream())
            _lib.check(rc, "cv_sp_col_sum")
            check(ow.read()[0], s64[:c], b64[:c], "n=%d c=%d det=%d" % (n, c, det), "col_sum")
        assert bool(torch.isnan(ws[chunks * c:]).all()), "writes past the workspace"


# ---- BatchNorm statistics --------------------------------------------------------------------------------------------------
def nan_ws(c):
    nbytes = int(_lib.lib().cv_sp_bn_workspace_bytes(c))
    return torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV), nbytes


def run_stats(n, c, ld, running, mis=0):
    d = case(n, c)
    xw = Win(n, c, ld, d["x"], mis=mis)
    outs = {k: vec(c) for k in ("mean", "var", "scale", "shift")}
    if running:
        outs["running_mean"], outs["running_var"] = vec(c, d["running_mean"]), vec(c, d["running_var"])
    ws, nbytes = nan_ws(c)
    gamma, beta = cuda_t(d["gamma"]), cuda_t(d["beta"])              # (held: a temporary's block could be handed out again)
    rc = _lib.lib().cv_sp_bn_stats_f32(P(xw.t), n, c, ld, P(gamma), P(beta), EPS, MOM,
                                       P(outs["running_mean"].t if running else None),
                                       P(outs["running_var"].t if running else None), P(outs["mean"].t), P(outs["var"].t),
                                       P(outs["scale"].t), P(outs["shift"].t), P(ws), nbytes, stream())
    _lib.check(rc, "cv_sp_bn_stats_f32")
    ref = so.bn_stats64(d["x"], n, d["gamma"], d["beta"], EPS, MOM, d["running_mean"] if running else None,
                        d["running_var"] if running else None)
    what = "n=%d c=%d ld=%d running=%d mis=%d" % (n, c, ld, running, mis)
    for k, (v, b) in ref.items():
        check(outs[k].read()[0], v, b, what, k)
    assert np.array_equal(xw.read(), d["x"])
    return {k: w.read()[0] for k, w in outs.items()}


@pytest.mark.parametrize("c", [4, 8, 32, 96, 384, 1024])
def test_bn_stats(c):
    """bn_col_reduce4<0>: rl = 256 / (c / 4) row lanes from 256 to 1, n around the chunk count n / 256 and the
    four-rows-in-flight loop; ld = c and c + 32; running statistics from non-trivial values and absent"""
    for i, n in enumerate((1, 2, 255, 256, 511, 512, 513, 4099)):
        run_stats(n, c, c + 32 * (i % 2), running=i % 3 != 2)
    run_stats(4099, c, c, running=False)
    run_stats(513, c, c + 32, running=True)


@pytest.mark.parametrize("c,ld,mis", [(3, 3, 0), (37, 37, 0), (1028, 1028, 0), (96, 97, 0), (96, 96, 1), (32, 35, 1)])
def test_bn_stats_scalar(c, ld, mis):
    """bn_col_reduce<0>: c % 4 != 0, c > 1024, an odd leading dimension, a base that is not 16-byte aligned"""
    for i, n in enumerate((1, 2, 255, 256, 513, 4099)):
        run_stats(n, c, ld, running=i % 2 == 0, mis=mis)


@pytest.mark.parametrize("n", [262143, 262144, 262400])
def test_bn_stats_chunk_cap(n):
    """1023 chunks, 1024, and the cap"""
    assert bn_chunks(n) == (1023 if n == 262143 else 1024)
    run_stats(n, 4, 4, running=True)
    run_stats(n, 3, 3, running=False)


# ---- BatchNorm backward ----------------------------------------------------------------------------------------------------
def stats_inputs(d, n):
    """fp32 mean / biased variance handed to the backward call (exact inputs of the oracle), and the forward's y"""
    x64 = d["x"].astype(np.float64)
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    mean32, var32 = mean.astype(f32), var.astype(f32)
    scale = (d["gamma"] / np.sqrt(var32 + f32(EPS))).astype(f32)
    shift = (d["beta"] - mean32 * scale).astype(f32)
    return mean32, var32, scale, shift


def run_backward(n, c, ld, mask, dres, mis=0, twin=None, dy_scale=1.0, verify=True):
    """one cv_sp_bn_backward_f32 / _hl_f32 call; mask: None, "y" (the ReLU output's rows) or "bits" (the words of the affine
    call).  twin: (slot tensor, flag tensor) -> also dx_hl.  Returns (dx_gpu, dx_hl words or None)"""
    d = case(n, c)
    L = _lib.lib()
    mean32, var32, scale, shift = stats_inputs(d, n)
    dy = (d["dy"] * f32(dy_scale)).astype(f32)
    yw = bw = open_ = None
    if mask == "y":
        y = np.maximum(d["x"] * scale + shift + d["res"], f32(0)).astype(f32)
        yw, open_ = Win(n, c, ld, y, mis=mis), y > 0
    elif mask == "bits":
        xa, ya, ha, bw = Win(n, c, data=d["x"]), Win(n, c), Win(n, c, hl=True), Win(n, c // 32, dtype=torch.int32)
        ME.affine_forward(xa.t, cuda_t(scale), cuda_t(shift), True, out=ya.t, residual=cuda_t(d["res"]), out_hl=ha.t,
                          relu_bits=bw.t)
        open_ = ya.read() > 0
        assert np.array_equal(bw.read().view(np.uint32), pack_bits(open_))
    xw, dyw = Win(n, c, ld, d["x"], mis=mis), Win(n, c, ld, dy, mis=mis)
    dxw = Win(n, c, ld, mis=mis)
    drw = Win(n, c, ld, mis=mis) if dres else None
    dgw, dbw = vec(c), vec(c)
    ws, nbytes = nan_ws(c)
    mean_t, var_t, gamma_t = cuda_t(mean32), cuda_t(var32), cuda_t(d["gamma"])     # (held until the results are read)
    common = (P(xw.t), P(dyw.t), P(yw.t if yw else None), n, c, ld, P(mean_t), P(var_t), EPS,
              P(gamma_t), P(dgw.t), P(dbw.t), P(dxw.t), P(drw.t if dres else None), P(ws), nbytes)
    hw = None
    if twin is not None or mask == "bits":
        if twin is not None:
            hw = Win(n, c, ld, hl=True)
        rc = L.cv_sp_bn_backward_hl_f32(*common, P(hw.t if hw else None), P(twin[0] if twin else None),
                                        P(twin[1] if twin else None), P(bw.t if bw else None), stream())
    else:
        rc = L.cv_sp_bn_backward_f32(*common, stream())
    _lib.check(rc, "cv_sp_bn_backward")
    dx = dxw.read()
    if verify:
        ref = so.bn_backward64(d["x"], dy, open_, mean32, var32, d["gamma"], n, EPS)
        what = "n=%d c=%d ld=%d mask=%s dres=%d mis=%d" % (n, c, ld, mask, dres, mis)
        check(dbw.read()[0], *ref["dbeta"], what, "dbeta")
        check(dgw.read()[0], *ref["dgamma"], what, "dgamma")
        check(dx, *ref["dx"], what, "dx")
        if dres:
            assert np.array_equal(drw.read(), ref["dres"][0].astype(f32)), what
    assert np.array_equal(xw.read(), d["x"]) and np.array_equal(dyw.read(), dy)
    return dx, (hw.read() if hw else None)


BWD = [(1, 32), (2, 4), (255, 8), (256, 96), (511, 384), (512, 1024), (513, 32), (4099, 96), (4099, 4), (513, 1024)]


@pytest.mark.parametrize("mask", [None, "y", "bits"])
def test_backward(mask):
    """bn_col_reduce4<1> + bn_backward_apply4 over the (n, c) grid of the statistics, thinned; dres on and off; ld = c and
    c + 32 with sentinels in the gap of dx and dres"""
    for i, (n, c) in enumerate(BWD):
        if mask == "bits" and c % 32:
            continue
        run_backward(n, c, c + 32 * (i % 2), mask, dres=(i + (mask is None)) % 2 == 0)
    run_backward(4099, 96, 128, mask, dres=True)


@pytest.mark.parametrize("n,c,ld,mis", [(257, 3, 3, 0), (1000, 37, 40, 0), (65, 1028, 1028, 0), (257, 96, 97, 0),
                                        (257, 96, 96, 1), (4099, 30, 32, 0)])
def test_backward_scalar(n, c, ld, mis):
    """bn_col_reduce<1> + bn_backward_apply: c % 4 != 0, c > 1024, an odd leading dimension, a misaligned base"""
    run_backward(n, c, ld, "y", dres=True, mis=mis)
    run_backward(n, c, ld, None, dres=n % 2 == 0, mis=mis)


@pytest.mark.parametrize("kernel", ["apply4", "apply"])
def test_backward_grid_caps(kernel):
    if kernel == "apply4":
        assert (131073 * 32 + 255) // 256 > 16384
        run_backward(131073, 128, 128, "y", dres=True)
    else:
        assert (70001 * 37 + 255) // 256 > 8192
        run_backward(70001, 37, 37, "y", dres=True)


def new_slot(prev=None):
    """8193 words of a layer's slot (this call's maxima, the previous call's, the inverse factor) and sentinels behind"""
    s = torch.zeros(8193 + PAD, dtype=torch.int32, device=DEV)
    s[8193:] = SENT_I
    if prev is not None:
        s[4096:8192] = cuda_t(np.asarray(prev, np.uint32).view(np.int32))
    return s


def read_slot(s):
    w = s.cpu().numpy().view(np.uint32)
    assert (w[8193:] == SENT_I).all(), "writes behind the slot"
    return w[:4096], w[4096:8192], w[8192:8193].view(f32)[0]


@pytest.mark.parametrize("n,c", [(257, 32), (4099, 96), (40000, 32), (40000, 96), (44000, 96)])
def test_backward_twin(n, c):
    """the scaled hl twin of dx (cv_sp_bn_backward_hl_f32): per-workgroup maxima, the power of two taken from the previous
    call's maxima with its escapes, the inverse factor, the range flag.  (44000 x 96: 4125 workgroups' worth of work on
    the 4096-block grid)"""
    grid = min((n * (c // 4) + 255) // 256, 4096)
    assert (grid == 4096) == (n == 44000)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(prev, dy_scale=1.0, verify=False):
        flag.zero_()
        slot = new_slot(prev)
        dx, words = run_backward(n, c, c + 32, "y", dres=False, twin=(slot, flag), dy_scale=dy_scale, verify=verify)
        cur, old, inv = read_slot(slot)
        assert np.array_equal(old, np.zeros(4096, np.uint32) if prev is None else prev), "the previous maxima were overwritten"
        assert cur[:grid].max() == np.abs(dx).max().astype(f32).view(np.uint32), "largest |dx| of the call"
        assert (cur[grid:] == 0).all(), "maxima beyond the grid"
        return dx, words, cur, inv, int(flag.cpu()[0])

    # an all-zero slot: no scale
    dx, words, cur, inv, fl = call(None, verify=True)       # (the later calls are compared with their own dx)
    assert inv == 1.0 and fl == 0
    check_hl_bits(words, dx, "hs = 1")
    m0 = float(np.abs(dx).max())
    # the previous call's maxima decide the factor: largest |dx| near 2^-20, 1, 2^20
    for target in (2.0 ** -20, 1.0, 2.0 ** 20):
        s = 2.0 ** np.round(np.log2(target / m0))
        dx1, words1, cur1, inv1, fl1 = call(None, s)
        assert fl1 == int(np.abs(dx1).max() > 65000.0)            # (unscaled, 2^20 is beyond the fp16 range)
        E = int(cur1.max() >> 23) & 255
        assert abs(E - 127 - np.log2(target)) <= 1
        dx2, words2, cur2, inv2, fl2 = call(cur1, s)
        assert np.array_equal(dx2, dx1)
        assert inv2 == f32(2.0 ** (E - 136)) and fl2 == 0
        scaled = dx2 * f32(2.0 ** (136 - E))
        assert 2.0 ** 9 <= np.abs(scaled).max() < 2.0 ** 10
        check_hl_bits(words2, scaled, "target %g" % target)
    # the escapes: exponents below 10 and above 250 leave the factor at 1
    for e_bits, name in ((9, "2^-118"), (251, "2^124")):
        prev = np.zeros(4096, np.uint32)
        prev[(7 * e_bits) % grid] = (e_bits << 23) | 0x400000
        dx3, words3, cur3, inv3, fl3 = call(prev)
        assert inv3 == 1.0 and fl3 == 0 and np.array_equal(dx3, dx)
        check_hl_bits(words3, dx3, "escape " + name)
    for e_bits in (10, 250):                                        # ... and the last exponents inside
        prev = np.zeros(4096, np.uint32)
        prev[0] = e_bits << 23
        inv4 = call(prev)[3]
        assert inv4 == f32(2.0 ** (e_bits - 136))


def test_backward_refusals():
    """dx_hl without a slot (and the reverse), bit words with c = 48"""
    L = _lib.lib()
    n, c = 65, 96
    d = case(n, c)
    mean32, var32, _, _ = stats_inputs(d, n)
    xw, dyw, dxw, hw = Win(n, c, data=d["x"]), Win(n, c, data=d["dy"]), Win(n, c), Win(n, c, hl=True)
    dgw, dbw = vec(c), vec(c)
    ws, nbytes = nan_ws(c)
    slot, flag = new_slot(), torch.zeros(1, dtype=torch.int32, device=DEV)
    bits = Win(n, 3, dtype=torch.int32)
    mean_t, var_t, gamma_t = cuda_t(mean32), cuda_t(var32), cuda_t(d["gamma"])

    def call(cc, ld, hl, sl, bt):
        return L.cv_sp_bn_backward_hl_f32(P(xw.t), P(dyw.t), P(None), n, cc, ld, P(mean_t), P(var_t), EPS,
                                          P(gamma_t), P(dgw.t), P(dbw.t), P(dxw.t), P(None), P(ws), nbytes,
                                          P(hl), P(sl), P(flag), P(bt), stream())

    assert call(c, c, hw.t, None, None) == -22
    assert call(c, c, None, slot, None) == -22
    assert call(48, c, None, None, bits.t) == -22
    torch.cuda.synchronize()
    dxw.read(), hw.read(), dgw.read(), dbw.read(), read_slot(slot)
    assert int(flag.cpu()[0]) == 0


# ---- heads -----------------------------------------------------------------------------------------------------------------
def prob_tol(p):
    return np.where(p >= 1e-3, 2e-6 * p, 2e-6 * p + 1e-7)


@pytest.mark.parametrize("ncls", [1, 9, 20])
@pytest.mark.parametrize("log_scale", [0, 1])
def test_head_joint(ncls, log_scale):
    """tied logits, a background arg-max (head 0), log_scale off, nclasses != 9, ld wider than the row, n % 256 != 0"""
    L = _lib.lib()
    for n in (1, 255, 256, 257, 1000):
        for ld in (7 * ncls + 1, 64, 96):
            if ld < 7 * ncls + 1:
                continue
            f, planted = head_rows(n, ncls, ld)
            fw = Win(n, ld, data=f)
            xw, sw, pw, cw = Win(n, 3), Win(n, 3), Win(n, 1), Win(n, 1, dtype=torch.int32)
            _lib.check(L.cv_head_joint_f32(P(fw.t), n, ld, ncls, log_scale, P(xw.t), P(sw.t), P(pw.t), P(cw.t), stream()),
                       "cv_head_joint_f32")
            xyz, scale, prob, cls = so.head_joint64(f, ncls, log_scale)
            what = "n=%d ncls=%d ld=%d" % (n, ncls, ld)
            assert np.array_equal(xw.read(), xyz.astype(f32)), what
            assert np.array_equal(cw.read()[:, 0], cls), what
            if log_scale:
                check(sw.read(), scale, 2e-6 * np.abs(scale), what, "head scale")
            else:
                assert np.array_equal(sw.read(), scale.astype(f32)), what
            check(pw.read()[:, 0], prob, prob_tol(prob), what, "head prob")
    f, _ = head_rows(9, ncls, 7 * ncls + 1)
    fw, xw, sw, pw, cw = Win(9, 7 * ncls + 1, data=f), Win(9, 3), Win(9, 3), Win(9, 1), Win(9, 1, dtype=torch.int32)
    assert L.cv_head_joint_f32(P(fw.t), 9, 7 * ncls, ncls, log_scale, P(xw.t), P(sw.t), P(pw.t), P(cw.t), stream()) == -22
    xw.read(), sw.read(), pw.read(), cw.read()


@pytest.mark.parametrize("K", [1, 2, _lib.MAX_CATEGORIES])
@pytest.mark.parametrize("ld", [8, 64])
def test_head_separate(K, ld):
    """cv_head_separate_f32 against the oracle; cv_head_separate_models_f32: outputs [K][n][3], [K][n][3], [K][n] with a
    sentinel block behind each, every model's slice equal to its single-model call bit for bit"""
    L = _lib.lib()
    for n in (1, 257, 1000):
        for log_scale in (0, 1):
            fs = [head_rows(n, 1, ld, seed=100 + k)[0] for k in range(K)]
            for f in fs:
                f[:, 3:6] = np.clip(f[:, 3:6], -10, 10)
                f[1::64, 7] = f[1::64, 6]                             # a tie: prob = 0.5
            fws = [Win(n, ld, data=f) for f in fs]
            single = []
            for k in range(K):
                xw, sw, pw = Win(n, 3), Win(n, 3), Win(n, 1)
                _lib.check(L.cv_head_separate_f32(P(fws[k].t), n, ld, log_scale, P(xw.t), P(sw.t), P(pw.t), stream()),
                           "cv_head_separate_f32")
                single.append((xw.read(), sw.read(), pw.read()[:, 0]))
                xyz, scale, prob = so.head_separate64(fs[k], log_scale)
                what = "n=%d ld=%d model %d" % (n, ld, k)
                assert np.array_equal(single[k][0], xyz.astype(f32)), what
                if log_scale:
                    check(single[k][1], scale, 2e-6 * np.abs(scale), what, "head scale")
                else:
                    assert np.array_equal(single[k][1], scale.astype(f32)), what
                check(single[k][2], prob, prob_tol(prob), what, "head prob")
            xw, sw, pw = Win(K * n, 3), Win(K * n, 3), Win(K * n, 1)
            ptrs = (ctypes.c_void_p * K)(*[fw.t.data_ptr() for fw in fws])
            _lib.check(L.cv_head_separate_models_f32(ptrs, K, n, ld, log_scale, P(xw.t), P(sw.t), P(pw.t), stream()),
                       "cv_head_separate_models_f32")
            gx, gs, gp = xw.read().reshape(K, n, 3), sw.read().reshape(K, n, 3), pw.read().reshape(K, n)
            for k in range(K):
                assert np.array_equal(gx[k], single[k][0]) and np.array_equal(gs[k].view(np.uint32), single[k][1].view(np.uint32))
                assert np.array_equal(gp[k].view(np.uint32), single[k][2].view(np.uint32))


def test_zz_report():
    """not a check of its own: the worst error-to-bound ratio per quantity of this run and the module's wall time"""
    for k in sorted(RATIOS):
        print("ratio %-22s %.3f" % (k, RATIOS[k]))
    print("module wall time %.1f s" % (time.time() - T0))
