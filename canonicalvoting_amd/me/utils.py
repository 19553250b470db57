"""``ME.utils`` subset: batched_coordinates (train_joint.py:82), sparse_quantize
(utils/dataloader.py:197, sunrgbd/brnetcanon.py:218; on the device: quantize_device / quantize_batch, voxel_rows for
what a scene gathers behind it, scan_rows for what a training batch computes behind it, and quantize_nowait + sym_rows for
the per-category trainer's batch with one host wait behind both), kaiming_normal_
(utils/resnet.py:112); sym_loss, the per-category trainer's coordinate loss over packed symmetry labels
(train_separate.py:265-280); row_loss, the per-row losses of both trainers and the joint trainer's validation form
(train_joint.py:253-283, :311-340)."""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .._lib import ptr as _ptr, stream as _stream


def _ptr_if_any(t):
    """_ptr(t), NULL also for a tensor without elements (torch gives those an address of its own)"""
    return _ptr(t) if t is not None and t.numel() else None


def batched_coordinates(coords, dtype=torch.int32, device=None):
    """list of [Ni, 3] coordinates -> [sum Ni, 4] with the batch index in column 0; floats are floored."""
    out = []
    for b, c in enumerate(coords):
        c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c)
        if c.is_floating_point():
            c = torch.floor(c)
        c = c.to(dtype)
        out.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=dtype, device=c.device), c], 1))
    r = torch.cat(out, 0)
    return r.to(device) if device is not None else r


def _quantize_host(c, quantization_size, return_inverse=False):
    """(voxels [M,3] int32, first point of every voxel ascending, inverse or None) - numpy, the reference path"""
    if quantization_size is not None:
        c = np.floor(c / quantization_size)
    c = c.astype(np.int32)
    if not return_inverse:
        _, idx = np.unique(c, axis=0, return_index=True)
        return c, np.sort(idx), None
    _, idx, inv = np.unique(c, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(idx)                      # np.unique's (lexicographic) row -> its place in first-occurrence order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return c, idx[order], rank[np.asarray(inv).reshape(-1)]


def quantize_device(points, quantization_size=None, offsets=None, return_inverse=False):
    """Voxelisation on the GPU (cv_sp_quantize_f32 / _f64, on torch's current stream, one host wait for the voxel count).

    points [M, 3] on the device, fp32 or fp64 (other dtypes are computed in fp64, as numpy promotes them), rows may be
    strided; ``offsets``: first rows of the clouds when the rows are several clouds one after the other (batch index =
    cloud).  Voxel = floor(p / quantization_size) in the input's precision, floor(p) when quantization_size is None.
    Returns (coords4 [N, 4] int32 = (batch, x, y, z), index [N] int32 = first point of every voxel, ascending,
    inverse [M] int32 or None).  Raises RuntimeError when points are non-finite or outside the coordinate window."""
    assert points.is_cuda and points.dim() == 2 and points.shape[1] == 3, "points: a [M, 3] device tensor"
    if points.dtype not in (torch.float32, torch.float64):
        points = points.to(torch.float64)
    if points.stride(1) != 1 or points.stride(0) < 3:
        points = points.contiguous()
    coords4, index, inverse, _, (n, rejected) = _quantize_call(points, quantization_size, offsets, return_inverse, True)
    if rejected != 0:
        raise_rejected(rejected)
    return coords4[:n], index[:n], inverse


def quantize_nowait(points, quantization_size, offsets):
    """quantize_device's sibling WITHOUT the host wait (cv_sp_quantize_f32 with h_counts == NULL): float32 ``points`` [M, 3]
    of the clouds whose first rows are ``offsets``, on torch's current stream.  Returns the full-size buffers
    (coords4 [M, 4], index [M], inverse [M], counts [2] = (N, rejected points)), all int32 on the device: only the first N rows
    of coords4 / index are written, and nothing has been checked - the caller reads ``counts`` behind its own wait and treats
    rejected points as quantize_device does."""
    assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3 \
        and points.stride(1) == 1 and points.stride(0) >= 3, "points: a float32 [M, 3] device tensor"
    return _quantize_call(points, quantization_size, offsets, True, False)[:4]


def raise_rejected(count):
    """the error of a voxelisation that rejected ``count`` points, worded the same wherever the count is read"""
    raise RuntimeError("sparse_quantize: %d points rejected (a non-finite component, or a voxel outside the supported "
                       "window: spatial coordinates in [-32704, 32703])" % count) from None


def _quantize_call(points, quantization_size, offsets, return_inverse, host_counts):
    """The one call into cv_sp_quantize_f32 / _f64, on torch's current stream: ``points`` [M, 3] fp32 or fp64 device rows
    (unit column stride), ``offsets`` None or the first rows of the clouds.  Returns the full-size int32 device buffers
    (coords4 [M, 4], index [M], inverse [M] or None, counts [2] = (N, rejected points)) and, with ``host_counts``, the two
    counts as host ints - the call then waits for them; without, h_counts is NULL, nothing waits and the fifth entry is None."""
    L = _lib.lib()
    dev, m = points.device, points.shape[0]
    if m == 0:
        raise RuntimeError("sparse_quantize: empty point cloud")
    f64 = points.dtype == torch.float64
    h_off, n_clouds = None, 0
    if offsets is not None:
        offsets = [int(o) for o in (offsets.tolist() if hasattr(offsets, "tolist") else offsets)]
        h_off, n_clouds = (ctypes.c_int64 * len(offsets))(*offsets), len(offsets)
    coords4 = torch.empty((m, 4), dtype=torch.int32, device=dev)
    index = torch.empty(m, dtype=torch.int32, device=dev)
    inverse = torch.empty(m, dtype=torch.int32, device=dev) if return_inverse else None
    counts_d = torch.empty(2, dtype=torch.int32, device=dev)
    counts_h = (ctypes.c_int32 * 2)() if host_counts else None
    ws = _lib.scratch(dev, "quantize", int(L.cv_sp_quantize_workspace_bytes(m)))
    fn = L.cv_sp_quantize_f64 if f64 else L.cv_sp_quantize_f32
    q = 0.0 if quantization_size is None else float(np.float64(quantization_size) if f64 else np.float32(quantization_size))
    with torch.cuda.device(dev):
        _lib.check(fn(_ptr(points), m, points.stride(0), q, 1 if quantization_size is None else 0, h_off, n_clouds,
                      _ptr(coords4), _ptr(index), _ptr(inverse) if return_inverse else None,
                      _ptr(counts_d), counts_h, _ptr(ws), ws.numel(), _stream(dev)),
                   "cv_sp_quantize_f64" if f64 else "cv_sp_quantize_f32")
    return coords4, index, inverse, counts_d, (tuple(int(c) for c in counts_h) if host_counts else None)


def quantize_batch(clouds, quantization_size, return_inverse=False, offsets=None):
    """Several clouds voxelised by ONE pass: ``clouds`` is a list of [Mi, 3] device tensors, or one [M, 3] tensor with
    ``offsets`` (first row of every cloud).  Returns coords4 [N, 4] (batch, x, y, z), index [N] (rows of the concatenated
    clouds) and, with return_inverse, inverse [M] - what sparse_quantize per cloud followed by batched_coordinates gives;
    equal points of different clouds stay separate voxels."""
    if torch.is_tensor(clouds):
        if offsets is None:
            offsets = [0]
        pts = clouds
    else:
        assert offsets is None, "offsets come with ONE tensor of concatenated clouds"
        offsets = [0]
        for c in clouds[:-1]:
            offsets.append(offsets[-1] + c.shape[0])
        dt = torch.float64 if any(c.dtype != torch.float32 for c in clouds) else torch.float32
        pts = torch.cat([c.to(dt) for c in clouds], 0)
    coords4, index, inverse = quantize_device(pts, quantization_size, offsets, return_inverse)
    return (coords4, index, inverse) if return_inverse else (coords4, index)


def voxel_rows(coords4, index, res, *columns, recentre_from=None, out=None, points=True):
    """What a scene reads of a voxelised cloud, in ONE launch on torch's current stream (cv_sp_voxel_rows_f32): the world
    points ``float(coords4[:, 1:]) * float32(res)`` - the bits of ``(coords4[:, 1:] * res).float()`` - and
    ``column[index]`` for up to eight raw-point-aligned ``columns`` ([M, w] or [M], float32 or int32, unit column stride;
    the row stride may exceed w: a column block of a wider tensor).  Rows move as 32-bit words, payloads untouched.

    recentre_from: None, one int for every column or a sequence with one entry (int or None) per column: columns >= it are
    written as ``x * 2 - 1`` (float32).  out: optional destinations, one per column ([N, w] windows, row stride >= w; the
    words beyond w are left alone).  points=False: no world points (coords4 and res are not read).
    Returns (points [N, 3] float32 or None, list of the gathered columns)."""
    L = _lib.lib()
    n, dev = index.shape[0], index.device
    assert index.dtype == torch.int32 and index.is_contiguous(), "index: a contiguous int32 device tensor"
    if len(columns) > _lib.GATHER_MAX_JOBS:
        raise ValueError("voxel_rows: at most %d columns per call (got %d)" % (_lib.GATHER_MAX_JOBS, len(columns)))
    if recentre_from is None or isinstance(recentre_from, int):
        recentre_from = [recentre_from] * len(columns)
    pts = None
    if points:
        assert coords4.dtype == torch.int32 and coords4.is_contiguous() and coords4.shape == (n, 4), "coords4: contiguous int32 [N, 4]"
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    jobs = (_lib.GatherJob * max(len(columns), 1))()
    outs = []
    for i, col in enumerate(columns):
        if col.dtype not in (torch.float32, torch.int32):
            raise TypeError("voxel_rows: columns are float32 or int32 (got %s)" % col.dtype)
        c2 = col if col.dim() == 2 else col.unsqueeze(1)
        w = c2.shape[1]
        if c2.stride(1) != 1 or c2.stride(0) < w:
            c2 = c2.contiguous()
        if out is not None and out[i] is not None:
            dst = out[i]
            d2 = dst if dst.dim() == 2 else dst.unsqueeze(1)
            assert d2.dtype == col.dtype and d2.shape == (n, w) and d2.stride(1) == 1 and d2.stride(0) >= w, "out: [N, w] windows"
        else:
            dst = torch.empty((n, w) if col.dim() == 2 else (n,), dtype=col.dtype, device=dev)
            d2 = dst if dst.dim() == 2 else dst.unsqueeze(1)
        rf = recentre_from[i]
        if rf is not None and col.dtype != torch.float32:
            raise TypeError("voxel_rows: only float32 columns are recentred")
        jobs[i] = _lib.GatherJob(c2.data_ptr(), c2.stride(0), d2.data_ptr(), d2.stride(0), w, -1 if rf is None else int(rf))
        outs.append(dst)
    with torch.cuda.device(dev):
        _lib.check(L.cv_sp_voxel_rows_f32(_ptr(coords4) if points else None, _ptr(index), n,
                                          float(res) if points else 0.0, _ptr(pts) if points else None, jobs,
                                          len(columns), _stream(dev)), "cv_sp_voxel_rows_f32")
    return pts, outs


def _check_vertex_arrays(who, points, rgb, owner, scale, cls, colour, jitter, n_clouds):
    """what scan_rows and sym_rows both require of the per-vertex arrays, the model table and the colour operands; returns the
    number of models"""
    m, k = points.shape[0], cls.shape[0]
    assert points.dtype == torch.float32 and points.shape == (m, 3) and points.stride(1) == 1, "points: float32 [M, 3]"
    assert rgb.dtype == torch.uint8 and rgb.shape == (m, 3) and rgb.is_contiguous(), "rgb: contiguous uint8 [M, 3]"
    assert owner.dtype == torch.int32 and owner.shape == (m,) and owner.is_contiguous(), "owner: contiguous int32 [M]"
    assert scale.dtype == torch.float32 and scale.shape == (k, 3) and scale.is_contiguous(), "scale: contiguous float32 [m, 3]"
    assert cls.dtype == torch.int32 and cls.shape == (k,) and cls.is_contiguous(), "cls: contiguous int32 [m]"
    if (colour is None) != (jitter is None):
        raise ValueError("%s: the colour table and the jitter come together" % who)
    if colour is not None:
        assert colour.dtype == torch.float64 and colour.shape == (n_clouds, 6) and colour.is_contiguous(), "colour: float64 [B, 6]"
        assert jitter.dtype == torch.float64 and jitter.shape == (m,) and jitter.is_contiguous(), "jitter: contiguous float64 [M]"
    return k


def scan_rows(coords4, index, points, rgb, owner, minv, scale, cls, colour=None, jitter=None, use_xyz=False, recentre=False,
              out=None):
    """The training batch of voxelised raw scans, in ONE launch on torch's current stream (cv_sp_scan_rows_f32): features and
    labels of the kept rows from the raw per-vertex arrays, the bits ScanNetXYZProbMultiDataset.__getitem__ computes on the host.

    coords4 [N, 4] / index [N] int32 as quantize_batch returns them; per raw vertex: points [M, 3] float32 (the row stride may
    exceed 3), rgb [M, 3] uint8, owner [M] int32 (row of the model table, -1 = background); model table: minv [m, 3, 4]
    float64, scale [m, 3] float32, cls [m] int32 (m may be 0); colour [B, 6] float64 (gain, shift per cloud) with jitter [M]
    float64, both or neither.  use_xyz: the points in front of the colours; recentre: colours as c * 2 - 1.
    out: optional (feats, xyz, scale, cls) destinations ([N, w] windows, row stride >= w; cls [N] int64, any stride).
    Returns (feats [N, 3|6] float32, xyz [N, 3] float32, scale [N, 3] float32, cls [N] int64)."""
    L = _lib.lib()
    n, m, dev = index.shape[0], points.shape[0], index.device
    assert index.dtype == torch.int32 and index.is_contiguous(), "index: a contiguous int32 device tensor"
    assert coords4.dtype == torch.int32 and coords4.is_contiguous() and coords4.shape == (n, 4), "coords4: contiguous int32 [N, 4]"
    n_clouds = 1 if colour is None else colour.shape[0]
    k = _check_vertex_arrays("scan_rows", points, rgb, owner, scale, cls, colour, jitter, n_clouds)
    assert minv.dtype == torch.float64 and minv.shape == (k, 3, 4) and minv.is_contiguous(), "minv: contiguous float64 [m, 3, 4]"
    fw = 6 if use_xyz else 3
    widths, dtypes = (fw, 3, 3, 1), (torch.float32, torch.float32, torch.float32, torch.int64)
    dst = list(out) if out is not None else [None] * 4
    for i, (w, dt) in enumerate(zip(widths, dtypes)):
        if dst[i] is None:
            dst[i] = torch.empty((n, w) if i < 3 else (n,), dtype=dt, device=dev)
        else:
            d2 = dst[i] if i < 3 else dst[i].unsqueeze(1)
            assert d2.dtype == dt and d2.shape == (n, w) and (d2.stride(1) == 1 or w == 1) and d2.stride(0) >= w, "out: [N, w] windows"
    ptr = _ptr_if_any
    d = _lib.ScanRowsDesc(ptr(coords4), ptr(index), n, m, ptr(points), points.stride(0), ptr(rgb), ptr(owner),
                          ptr(minv), ptr(scale), ptr(cls), k, ptr(colour), ptr(jitter), n_clouds, int(bool(use_xyz)),
                          int(bool(recentre)), ptr(dst[0]), dst[0].stride(0), ptr(dst[1]), dst[1].stride(0),
                          ptr(dst[2]), dst[2].stride(0), ptr(dst[3]), dst[3].stride(0))
    with torch.cuda.device(dev):
        _lib.check(L.cv_sp_scan_rows_f32(ctypes.byref(d), _stream(dev)), "cv_sp_scan_rows_f32")
    return tuple(dst)


def sym_rows(coords4, index, inverse, quant_counts, points, rgb, owner, scale, cls, colour, jitter, offsets, seg_vertex, seg_vptr,
             pose_ptr, minv, n_targets, reference_indexing=True, use_xyz=False, recentre=False, h_counts=None):
    """The per-category trainer's batch behind quantize_nowait, on torch's current stream and without a host wait
    (cv_sp_sym_rows_f32): packed symmetry labels and the row arrays into buffers of the host's upper bounds.

    coords4 / index / inverse / quant_counts as quantize_nowait returns them; per raw vertex points [M, 3] float32 (row stride
    >= 3), rgb [M, 3] uint8, owner [M] int32; model table scale [m, 3] float32, cls [m] int32; colour [B, 6] float64 with
    jitter [M] float64, both or neither; offsets [B] int64 (device); the segments' vertex lists seg_vertex [Q] int32 with
    seg_vptr / pose_ptr [S0 + 1] int32 and minv [J0, 3, 4] float64; n_targets: the bound T0 = sum of list length * poses.
    h_counts: a pinned int32 [8] tensor that receives the counts by a copy on the stream, or None.
    Returns a dict of the upper-bound buffers: rows, pseg, urow, upoint [Q], uptr [Q + 1], seg_ptr, pose_ptr, tgt_ptr
    [S0 + 1], targets [T0, 3], feats [M, 3|6], scale [M, 3], obj, cls [M] int64, counts int32 [8] (_lib.SYM_ROWS_COUNTS)."""
    L = _lib.lib()
    dev, m, q, s0, j0 = index.device, points.shape[0], seg_vertex.shape[0], seg_vptr.shape[0] - 1, minv.shape[0]
    i32c = lambda t, shape: t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev
    assert i32c(coords4, (m, 4)) and i32c(index, (m,)) and i32c(inverse, (m,)) and i32c(quant_counts, (2,)), \
        "coords4 / index / inverse / counts: quantize_nowait's full-size int32 buffers"
    n_clouds = offsets.shape[0]
    k = _check_vertex_arrays("sym_rows", points, rgb, owner, scale, cls, colour, jitter, n_clouds)
    assert owner.device == dev and cls.device == dev, "owner / cls: on the device of index"
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.device == dev, "offsets: int64 [B] on the device"
    assert i32c(seg_vertex, (q,)) and i32c(seg_vptr, (s0 + 1,)) and i32c(pose_ptr, (s0 + 1,)), "segment lists: int32"
    assert minv.dtype == torch.float64 and minv.shape == (j0, 3, 4) and minv.is_contiguous(), "minv: contiguous float64 [J0, 3, 4]"
    if h_counts is not None:
        assert h_counts.dtype == torch.int32 and h_counts.numel() == 8 and h_counts.is_pinned(), "h_counts: pinned int32 [8]"
    t0 = int(n_targets)
    new = lambda shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=dev)
    o = dict(rows=new(q), pseg=new(q), seg_ptr=new(s0 + 1), pose_ptr=new(s0 + 1), tgt_ptr=new(s0 + 1),
             targets=new((t0, 3), torch.float32), urow=new(q), uptr=new(q + 1), upoint=new(q),
             feats=new((m, 6 if use_xyz else 3), torch.float32), scale=new((m, 3), torch.float32), obj=new(m, torch.int64),
             cls=new(m, torch.int64), counts=new(8))
    ws = _lib.scratch(dev, "sym_rows", int(L.cv_sp_sym_rows_workspace_bytes(m, q, s0, n_clouds)))
    ptr = _ptr_if_any
    d = _lib.SymRowsDesc(ptr(coords4), ptr(index), ptr(inverse), ptr(quant_counts), m, ptr(points), points.stride(0), ptr(rgb),
                         ptr(owner), ptr(scale), ptr(cls), k, ptr(colour), ptr(jitter), ptr(offsets), n_clouds,
                         ptr(seg_vertex), q, ptr(seg_vptr), ptr(pose_ptr), s0, ptr(minv), j0, t0,
                         int(bool(reference_indexing)), int(bool(use_xyz)), int(bool(recentre)),
                         ptr(o["rows"]), ptr(o["pseg"]), ptr(o["seg_ptr"]), ptr(o["pose_ptr"]), ptr(o["tgt_ptr"]), ptr(o["targets"]),
                         ptr(o["urow"]), ptr(o["uptr"]), ptr(o["upoint"]), ptr(o["feats"]), o["feats"].stride(0),
                         ptr(o["scale"]), 3, ptr(o["obj"]), ptr(o["cls"]), ptr(o["counts"]), ptr(h_counts),
                         _ptr(ws), ws.numel())
    with torch.cuda.device(dev):
        _lib.check(L.cv_sp_sym_rows_f32(ctypes.byref(d), _stream(dev)), "cv_sp_sym_rows_f32")
    return o


def _sym_desc(out_feats, sym, weights, xyz_factor):
    """cv_sym_loss_desc of predictions ``out_feats`` [N, C >= 3] and a device SymBatch, outputs and workspace still unset"""
    dev = out_feats.device
    assert out_feats.is_cuda and out_feats.dtype == torch.float32 and out_feats.dim() == 2 and out_feats.stride(1) == 1 \
        and out_feats.stride(0) >= 3 and out_feats.shape[1] >= 3, "out_feats: float32 [N, C >= 3] device rows"
    ints = (sym.rows, sym.pseg, sym.seg_ptr, sym.pose_ptr, sym.tgt_ptr, sym.urow, sym.uptr, sym.upoint)
    assert all(t.device == dev and t.dtype == torch.int32 and t.is_contiguous() for t in ints), "sym: int32 tensors on the output's device"
    assert sym.targets.device == dev and sym.targets.dtype == torch.float32 and sym.targets.is_contiguous(), "sym.targets: float32 [T, 3]"
    S, P = sym.n_segments, sym.rows.shape[0]
    assert sym.seg_ptr.shape[0] == S + 1 and sym.pose_ptr.shape[0] == S + 1 and sym.tgt_ptr.shape[0] == S + 1 \
        and sym.pseg.shape[0] == P and sym.upoint.shape[0] == P and sym.uptr.shape[0] == sym.urow.shape[0] + 1, "sym: inconsistent sizes"
    if sym.max_row >= out_feats.shape[0]:
        raise ValueError("sym_loss: label row %d outside the %d output rows" % (sym.max_row, out_feats.shape[0]))
    ptr = _ptr_if_any
    d = _lib.SymLossDesc()
    d.d_out, d.n_rows, d.ld = ptr(out_feats), out_feats.shape[0], out_feats.stride(0)
    d.d_rows, d.d_pseg, d.n_points = ptr(sym.rows), ptr(sym.pseg), P
    d.d_seg_ptr, d.d_pose_ptr, d.d_tgt_ptr, d.n_segments, d.n_jobs = ptr(sym.seg_ptr), ptr(sym.pose_ptr), ptr(sym.tgt_ptr), S, sym.n_jobs
    d.d_targets, d.n_targets = ptr(sym.targets), sym.targets.shape[0]
    d.d_urow, d.d_uptr, d.d_upoint, d.n_urows = ptr(sym.urow), ptr(sym.uptr), ptr(sym.upoint), sym.urow.shape[0]
    d.w = (ctypes.c_float * 3)(*[float(v) for v in weights])
    d.xyz_factor = float(xyz_factor)
    return d


class _SymLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_feats, sym, weights, xyz_factor):
        L = _lib.lib()
        dev = out_feats.device
        out_feats = out_feats if out_feats.stride(1) == 1 else out_feats.contiguous()
        d = _sym_desc(out_feats, sym, weights, xyz_factor)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        pose_loss = torch.empty(max(sym.n_jobs, 1), dtype=torch.float32, device=dev)
        best = torch.empty(max(sym.n_segments, 1), dtype=torch.int32, device=dev)
        seg_loss = torch.empty(max(sym.n_segments, 1), dtype=torch.float32, device=dev)
        ws = _lib.scratch(dev, "sym_loss", int(L.cv_sym_loss_workspace_bytes(d.n_targets, d.n_jobs)))
        d.d_loss, d.d_pose_loss, d.d_best, d.d_seg_loss = (_ptr(t) for t in (loss, pose_loss, best, seg_loss))
        d.d_ws, d.ws_bytes = _ptr(ws), ws.numel()
        with torch.cuda.device(dev):
            _lib.check(L.cv_sym_loss_fwd_f32(ctypes.byref(d), _stream(dev)), "cv_sym_loss_fwd_f32")
        ctx.save_for_backward(out_feats, best)
        ctx.sym, ctx.weights, ctx.xyz_factor = sym, weights, xyz_factor
        ctx.mark_non_differentiable(pose_loss, best)
        return loss.reshape(()), pose_loss[:sym.n_jobs], best[:sym.n_segments]

    @staticmethod
    def backward(ctx, grad_loss, _grad_pose, _grad_best):
        out_feats, best = ctx.saved_tensors
        dev = out_feats.device
        grad = torch.zeros(out_feats.shape, dtype=torch.float32, device=dev)
        gl = grad_loss.to(torch.float32).reshape(1).contiguous()
        d = _sym_desc(out_feats, ctx.sym, ctx.weights, ctx.xyz_factor)
        d.d_best, d.d_grad_loss, d.d_grad, d.grad_ld = _ptr(best), _ptr(gl), _ptr(grad), grad.stride(0)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cv_sym_loss_bwd_f32(ctypes.byref(d), _stream(dev)), "cv_sym_loss_bwd_f32")
        return grad, None, None, None


def sym_loss(out_feats, sym, weights=(1.0, 1.0, 1.0), xyz_factor=1.0, return_poses=False):
    """The per-category model's coordinate loss over packed symmetry labels (cv_sym_loss_fwd_f32 / cv_sym_loss_bwd_f32, two
    launches forward and one backward on torch's current stream, no host wait): per segment the weighted mean square distance
    of columns 0..2 of ``out_feats`` [N, C] to the targets of every symmetry-equivalent pose, the minimum over the poses (the
    lowest pose on ties, NaN as torch.min), the mean over the segments times ``xyz_factor`` - a scalar.  ``sym``: a
    data.SymBatch whose tensors are on the output's device (data.sym_to_device); its ``max_row`` is checked against N here,
    on the host, before anything is launched.  The backward gives an [N, C] gradient that is zero outside columns 0..2 of
    labelled rows, through the winning pose only: torch's full-reduction ``min()`` splits the gradient evenly over exact ties,
    which distinct poses do not produce (tests/test_sym_loss.py requires a decidable minimum of every case it runs).
    Bit-reproducible: no atomics, every sum in an order the labels fix.  return_poses: also (pose losses [J], best pose [S])."""
    loss, pose_loss, best = _SymLossFn.apply(out_feats, sym, tuple(float(v) for v in weights), float(xyz_factor))
    return (loss, pose_loss, best) if return_poses else loss


def row_loss_layout(layout, nclasses=9):
    """(heads, n_logits, xyz_col, scale_col, logit_col, obj_lo, obj_hi, with_xyz) of cv_row_loss_desc: 'joint' = the
    [N, 7 nclasses + 1] output (objects 0 .. nclasses - 1), 'separate' = the per-category [N, 8] output (object = label 1; its
    coordinate term stays with sym_loss)"""
    if layout == "joint":
        return (nclasses, nclasses + 1, 0, 3 * nclasses, 6 * nclasses, 0, nclasses - 1, 1)
    if layout == "separate":
        return _lib.ROW_LOSS_LAYOUTS["separate"]
    raise ValueError("row_loss: layout %r is neither 'joint' nor 'separate'" % (layout,))


def _row_loss_desc(out_feats, labels, xyz_labels, scale_labels, cfg):
    """cv_row_loss_desc of the network output and its per-row labels, outputs and workspace still unset"""
    layout, gather, empty, log_scale, weights, xyz_factor, scale_factor = cfg
    dev, n = out_feats.device, out_feats.shape[0]
    assert out_feats.is_cuda and out_feats.dtype == torch.float32 and out_feats.dim() == 2 and out_feats.stride(1) == 1, \
        "out_feats: float32 [N, C] device rows"
    assert labels.device == dev and labels.dtype == torch.int64 and labels.shape == (n,) and labels.is_contiguous(), \
        "labels: int64 [N] on the output's device"
    for name, t in (("xyz_labels", xyz_labels), ("scale_labels", scale_labels)):
        assert t is None or (t.device == dev and t.dtype == torch.float32 and t.shape == (n, 3) and t.is_contiguous()), \
            "%s: float32 [N, 3] on the output's device" % name
    d = _lib.RowLossDesc()
    d.d_out, d.n_rows, d.ld = _ptr_if_any(out_feats), n, out_feats.stride(0) if n > 1 else out_feats.shape[1]
    d.d_labels, d.d_xyz_labels, d.d_scale_labels = _ptr_if_any(labels), _ptr_if_any(xyz_labels), _ptr_if_any(scale_labels)
    d.heads, d.n_logits, d.xyz_col, d.scale_col, d.logit_col, d.obj_lo, d.obj_hi, d.with_xyz = layout
    d.log_scale, d.gather, d.empty = int(bool(log_scale)), _lib.ROW_LOSS_GATHER[gather], _lib.ROW_LOSS_EMPTY[empty]
    d.w = (ctypes.c_float * 3)(*weights)
    d.xyz_factor, d.scale_factor = xyz_factor, scale_factor
    return d


class _RowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_feats, labels, xyz_labels, scale_labels, cfg):
        L = _lib.lib()
        dev = out_feats.device
        out_feats = out_feats if out_feats.stride(1) == 1 else out_feats.contiguous()
        d = _row_loss_desc(out_feats, labels, xyz_labels, scale_labels, cfg)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        info = torch.empty(2, dtype=torch.int32, device=dev)
        ws = _lib.scratch(dev, "row_loss", int(L.cv_row_loss_workspace_bytes(d.n_rows)))
        d.d_losses, d.d_info, d.d_ws, d.ws_bytes = _ptr(losses), _ptr(info), _ptr(ws), ws.numel()
        with torch.cuda.device(dev):
            _lib.check(L.cv_row_loss_fwd_f32(ctypes.byref(d), _stream(dev)), "cv_row_loss_fwd_f32")
        ctx.save_for_backward(out_feats, labels, xyz_labels, scale_labels, info)
        ctx.cfg = cfg
        parts = losses[:3].clone()                 # (the parts are reported, the gradient flows through the total)
        ctx.mark_non_differentiable(parts, info)
        return losses[3], parts, info

    @staticmethod
    def backward(ctx, grad_total, _grad_parts, _grad_info):
        out_feats, labels, xyz_labels, scale_labels, info = ctx.saved_tensors
        dev = out_feats.device
        grad = torch.empty(out_feats.shape, dtype=torch.float32, device=dev)        # every element is written by the launch
        gl = grad_total.to(torch.float32).reshape(1).contiguous()
        d = _row_loss_desc(out_feats, labels, xyz_labels, scale_labels, ctx.cfg)
        d.d_info, d.d_grad_loss, d.d_grad = _ptr(info), _ptr(gl), _ptr_if_any(grad)
        d.grad_ld, d.n_cols = grad.stride(0) if grad.shape[0] > 1 else grad.shape[1], grad.shape[1]
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cv_row_loss_bwd_f32(ctypes.byref(d), _stream(dev)), "cv_row_loss_bwd_f32")
        return grad, None, None, None, None


def row_loss(out_feats, labels, xyz_labels, scale_labels, *, layout="joint", gather="label", empty="zero", nclasses=9,
             log_scale=True, weights=(1.0, 1.0, 1.0), xyz_factor=1.0, scale_factor=1.0, return_info=False):
    """The per-row losses of a trainer on the device (cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32: two launches forward, one
    backward, on torch's current stream, no host wait): the masked squared errors of the chosen head's coordinate and scale
    columns and the cross entropy of the logits, as include/cv_hip.h defines them.  ``out_feats`` [N, C] float32,
    ``labels`` [N] (any integer dtype), ``xyz_labels`` / ``scale_labels`` [N, 3]; layout 'joint' ([N, 7 nclasses + 1]) or
    'separate' ([N, 8]; no coordinate term, ``xyz_labels`` may be None).  gather 'label' (training) or 'argmax' (the
    validation form, no gradient); empty 'zero' (no object row: zero terms) or 'nan' (the reference's mean over nothing).
    Returns the device scalars (loss_xyz, loss_scale, loss_class, total); the gradient flows through ``total`` (the three
    parts are reported values).  return_info: also the int32 pair (object rows, labels above the last logit)."""
    if gather not in _lib.ROW_LOSS_GATHER or empty not in _lib.ROW_LOSS_EMPTY:
        raise ValueError("row_loss: gather %r / empty %r" % (gather, empty))
    lay = row_loss_layout(layout, nclasses)
    if gather == "argmax" and out_feats.requires_grad and torch.is_grad_enabled():
        out_feats = out_feats.detach()
    dev = out_feats.device
    prep = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
    cfg = (lay, gather, empty, bool(log_scale), tuple(float(v) for v in weights), float(xyz_factor), float(scale_factor))
    total, parts, info = _RowLossFn.apply(out_feats, labels.to(device=dev, dtype=torch.int64).contiguous(),
                                          prep(xyz_labels) if lay[7] else None, prep(scale_labels), cfg)
    res = (parts[0], parts[1], parts[2], total)
    return res + (info,) if return_info else res


def sparse_quantize(coordinates, features=None, labels=None, quantization_size=None, return_index=False,
                    return_inverse=False, device=None, **_):
    """floor(coords / quantization_size), one (the first) point per voxel, voxels in the order of their first points.

    numpy in and ``device=None``: numpy out, on the host.  A torch tensor in, or ``device=`` given (sunrgbd/brnetcanon.py:218):
    torch tensors out - int32 coords [N, 3], features / labels gathered by the first-point index - on ``device``, else on the
    input's device; a device result is computed by the HIP kernels (quantize_device), a CPU result by the host path.
    ``return_inverse=True`` appends the map point -> output row as the last element.
    (quantization_size=None: the host path converts with astype - it truncates towards zero - while the device floors, as
    MinkowskiEngine does; the two agree on non-negative and on integer-valued coordinates.)"""
    as_torch = torch.is_tensor(coordinates) or device is not None
    if as_torch:
        dev = torch.device(device) if device is not None else coordinates.device
        if dev.type == "cuda":
            pts = coordinates if torch.is_tensor(coordinates) else torch.from_numpy(np.ascontiguousarray(coordinates))
            c4, idx, inv = quantize_device(pts.to(dev), quantization_size, None, return_inverse)
            c, gi = c4[:, 1:].contiguous(), idx.long()
            take = lambda a: torch.as_tensor(a).to(dev)[gi]
        else:
            c, idx, inv = _quantize_host(coordinates.numpy() if torch.is_tensor(coordinates) else np.asarray(coordinates),
                                         quantization_size, return_inverse)
            c, idx = torch.from_numpy(c[idx]), torch.from_numpy(idx.astype(np.int32))
            inv = torch.from_numpy(inv.astype(np.int32)) if inv is not None else None
            gi = idx.long()
            take = lambda a: torch.as_tensor(a)[gi]
    else:
        c, idx, inv = _quantize_host(np.asarray(coordinates), quantization_size, return_inverse)
        c = c[idx]
        take = lambda a: np.asarray(a)[idx]
    if return_index:
        out = (c, idx)
    elif features is None:
        out = (c,)
    elif labels is None:
        out = (c, take(features))
    else:
        out = (c, take(features), take(labels))
    if return_inverse:
        out = out + (inv,)
    return out[0] if len(out) == 1 else out


def kaiming_normal_(tensor, a=0, mode="fan_in", nonlinearity="leaky_relu"):
    """ME.utils.kaiming_normal_ on a conv ``kernel`` [K, Cin, Cout] / [Cin, Cout]:
    fan_in = Cin * K, fan_out = Cout * K."""
    if tensor.dim() == 3:
        K, cin, cout = tensor.shape
    else:
        (cin, cout), K = tensor.shape, 1
    fan = cin * K if mode == "fan_in" else cout * K
    gain = torch.nn.init.calculate_gain(nonlinearity, a)
    std = gain / math.sqrt(fan)
    with torch.no_grad():
        return tensor.normal_(0, std)
