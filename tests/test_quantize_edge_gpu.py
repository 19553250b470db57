"""The voxeliser (section 6 of csrc/sparse_coords.hip) on the adversarial clouds of tests/quantize_ref.py, straight through
cv_sp_quantize_f32 / _f64 on torch's current stream, against that module's dict reference.  Everything compared is an integer:
every comparison is exact equality, row order included.

Outputs go into sentinel-filled int32 allocations with 64 guard words on either side and three spare rows behind m; the
workspace has exactly the size the library asks for, is filled with a byte pattern first and has guard bytes behind it; counts
holds garbage before the call.  Every case is called five times (fresh workspace; the same workspace again; with h_counts;
without d_inverse; offsets [0] instead of NULL) and the same bytes are asked of every call.

Every input is a valid call with a 16-byte aligned coords4; what the cases are made for is verified on the CPU by
tests/test_quantize_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib
from canonicalvoting_amd import me as ME
from canonicalvoting_amd.me import utils as me_utils
from tests import coord_ref as cr
from tests import quantize_ref as qr

pytestmark = pytest.mark.gpu

SENT, GUARD, SPARE = -77, 64, 3
WS_BYTE, WS_GUARD = 0xA5, 256
GARBAGE = (123456789, -9)


class Out:
    """the four output allocations of one call as host arrays, guards included"""

    def __init__(self, m, coords4, index, inverse, counts, ws, need, h_counts):
        self.m = m
        self.coords4, self.index, self.inverse, self.counts = (t.cpu().numpy() for t in (coords4, index, inverse, counts))
        self.ws_guard = ws[need:].cpu().numpy()
        self.h_counts = None if h_counts is None else tuple(h_counts)

    def inner(self, a, width=1):
        return a[GUARD:GUARD + (self.m + SPARE) * width]

    def bytes(self, names=("coords4", "index", "inverse", "counts")):
        return tuple(getattr(self, k).tobytes() for k in names)


def upload(c, dev):
    """the case's rows on the device as its layout asks: (flat tensor, first element, [m, 3] view)"""
    flat, first = c.laid_out()
    d = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    assert d.data_ptr() % 16 == 0
    return d, first, torch.as_strided(d, (c.m, 3), (c.ld, 1), first)


def call(c, d, first, offsets, want_inverse=True, host_counts=False, ws=None):
    """one cv_sp_quantize_* call on torch's current stream; returns (Out, the workspace)"""
    L, m, dev = _lib.lib(), c.m, d.device
    words = lambda n: torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device=dev)
    coords4, index, inverse, counts = words((m + SPARE) * 4), words(m + SPARE), words(m + SPARE), words(2)
    counts[GUARD:GUARD + 2] = torch.tensor(GARBAGE, dtype=torch.int32)
    need = int(L.cv_sp_quantize_workspace_bytes(m))
    if ws is None:
        ws = torch.full((need + WS_GUARD,), WS_BYTE, dtype=torch.uint8, device=dev)
    at = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    assert at(coords4).value % 16 == 0 and ws.numel() == need + WS_GUARD
    h = (ctypes.c_int32 * 2)(*GARBAGE) if host_counts else None
    off = None if offsets is None else (ctypes.c_int64 * len(offsets))(*offsets)
    f64 = c.dtype == np.float64
    fn = L.cv_sp_quantize_f64 if f64 else L.cv_sp_quantize_f32
    rc = fn(ctypes.c_void_p(d.data_ptr() + first * d.element_size()), m, c.ld, c.q, c.floor_only, off,
            0 if offsets is None else len(offsets), at(coords4), at(index), at(inverse) if want_inverse else None, at(counts), h,
            ctypes.c_void_p(ws.data_ptr()), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "cv_sp_quantize_f64" if f64 else "cv_sp_quantize_f32")
    torch.cuda.current_stream().synchronize()
    return Out(m, coords4, index, inverse, counts, ws, need, h), ws


def check(out, ref, want_inverse=True):
    """the documented extent holds the reference's values, everything else what it held before the call"""
    m, n = out.m, ref["n"]
    assert out.counts[GUARD:GUARD + 2].tolist() == [n, ref["rejected"]]
    c4 = out.inner(out.coords4, 4).reshape(m + SPARE, 4)
    assert cr.same(c4[:n], ref["coords4"]) and (c4[n:] == SENT).all()
    idx = out.inner(out.index)
    assert cr.same(idx[:n], ref["index"]) and (idx[n:] == SENT).all()
    inv = out.inner(out.inverse)
    if want_inverse:
        assert cr.same(inv[:m], ref["inverse"]) and (inv[m:] == SENT).all()
    else:
        assert (inv == SENT).all()
    for a, width in ((out.coords4, 4), (out.index, 1), (out.inverse, 1)):
        assert (a[:GUARD] == SENT).all() and (a[GUARD + (m + SPARE) * width:] == SENT).all()
    assert (out.counts[:GUARD] == SENT).all() and (out.counts[GUARD + 2:] == SENT).all()
    assert (out.ws_guard == WS_BYTE).all() and out.ws_guard.size == WS_GUARD


@pytest.mark.parametrize("name", qr.CASE_NAMES)
def test_c_abi_equals_the_reference(cuda, built_lib, name):
    c, ref = qr.case(name), qr.case_reference(name)
    d, first, view = upload(c, cuda)
    a, ws = call(c, d, first, c.offsets)                                   # a workspace of pattern bytes
    check(a, ref)
    b, _ = call(c, d, first, c.offsets, ws=ws)                             # the same workspace, now holding the previous table
    check(b, ref)
    assert b.bytes() == a.bytes()
    h, _ = call(c, d, first, c.offsets, host_counts=True, ws=ws)           # the host's two ints are d_counts
    check(h, ref)
    assert h.bytes() == a.bytes() and h.h_counts == (ref["n"], ref["rejected"]) and a.h_counts is None
    x, _ = call(c, d, first, c.offsets, want_inverse=False, ws=ws)         # d_inverse == NULL changes nothing else
    check(x, ref, want_inverse=False)
    assert x.bytes(("coords4", "index", "counts")) == a.bytes(("coords4", "index", "counts"))
    if c.offsets is None:                                                  # one cloud given as offsets [0]
        o, _ = call(c, d, first, [0], ws=ws)
        check(o, ref)
        assert o.bytes() == a.bytes()

    # the wrapper adds nothing, and its set goes into a coordinate manager as it is
    q = None if c.floor_only else c.q
    if ref["rejected"]:
        with pytest.raises(RuntimeError, match=r"\b%d points rejected" % ref["rejected"]):
            me_utils.quantize_device(view, q, c.offsets, return_inverse=True)
        return
    coords4, index, inverse = me_utils.quantize_device(view, q, c.offsets, return_inverse=True)
    n, m = ref["n"], c.m
    assert coords4.dtype == index.dtype == inverse.dtype == torch.int32
    assert coords4.cpu().numpy().tobytes() == a.inner(a.coords4, 4)[:4 * n].tobytes()
    assert index.cpu().numpy().tobytes() == a.inner(a.index)[:n].tobytes()
    assert inverse.cpu().numpy().tobytes() == a.inner(a.inverse)[:m].tobytes()
    dev_set = torch.from_numpy(a.inner(a.coords4, 4)[:4 * n].reshape(n, 4).copy()).to(cuda)
    cm = ME.CoordinateManager(dev_set, num_levels=1, check=True)          # raises on duplicates and rows outside the key window
    assert cm.counts[0] == n


@pytest.mark.parametrize("name", ["runs_rejected_f32", "runs_rejected_f64"])
def test_side_stream_and_repeat_give_the_same_bytes(cuda, built_lib, name):
    c, ref = qr.case(name), qr.case_reference(name)
    d, first, _ = upload(c, cuda)
    a, _ = call(c, d, first, c.offsets)
    check(a, ref)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        s1, ws = call(c, d, first, c.offsets)
        s2, _ = call(c, d, first, c.offsets, ws=ws)
    torch.cuda.current_stream(cuda).wait_stream(side)
    check(s1, ref)
    check(s2, ref)
    assert s1.bytes() == a.bytes() and s2.bytes() == a.bytes()
