"""Drop-in for the reference's pybind module ``hv_cuda`` (houghvoting/src/hv_cuda.cpp:74-77).

    forward(points, xyz_labels, scale_labels, obj_labels, res, num_rots[, corners])
        -> [grid_obj[X,Y,Z], grid_rot[X,Y,Z,2], grid_scale[X,Y,Z,3]]      (hv_cuda.cpp:30-45)
    backward(grad_grid, points, xyz_labels, scale_labels, obj_labels, res, num_rots)
        -> [d_xyz_labels, d_scale_labels, d_obj_labels]                    (hv_cuda.cpp:47-71)
    forward_categories(points, xyz[K,N,3], scale[K,N,3], obj[K,N], res, num_rots)
        -> [K,...] grids: K separate-mode categories in one launch sequence (no reference counterpart)
    forward_scenes(points, xyz_labels, scale_labels, obj_labels, row_ranges, res, num_rots[, corners][, thresh])
        -> B grid triples: B scenes' row ranges of shared arrays in one launch sequence (no reference counterpart)

Same argument meaning, same input checks and messages (``"<name> must be a CUDA tensor"``,
``"<name> must be contiguous"``, hv_cuda.cpp:26-28), same fresh writable outputs on the inputs'
device.  The optional 7th ``corners[2,3]`` is the SUN RGB-D caller's variant
(sunrgbd/brnetcanon.py:99).  Under PyTorch-ROCm "cuda" tensors are HIP device memory; the
work is done by the hand-written gfx950 kernels in libcvhip.so on torch's current stream.

Differences that are improvements, not behaviour changes: kernels run on the current stream
instead of the legacy default stream, one host sync per forward (the grid shape has to reach
the host) instead of twelve, zero when ``corners`` is given.
"""
import ctypes
import threading

import torch

from . import _lib

ALGO_AUTO, ALGO_DIRECT, ALGO_TILES = 0, 1, 2
_algo = ALGO_AUTO


def set_algorithm(algo):
    """0 auto, 1 direct global atomics, 2 LDS tiles (for A/B measurements)."""
    global _algo
    _algo = int(algo)


def _remember_corner(grid_obj, mn):
    # kept on the tensor OBJECT (like _scalar's host value): a cache keyed by address would hand a grid that was
    # not produced by forward() (a loaded / golden grid on a recycled allocation of the same shape) a stale origin
    grid_obj._cv_corner = [float(v) for v in mn]


def recent_corner(grid_obj):
    """grid origin of a grid_obj returned by forward() (None for any other tensor)"""
    return getattr(grid_obj, "_cv_corner", None)


def _check_input(x, name):
    if not x.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not x.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _scalar(t, kind):
    """Host value of a 0-dim device tensor (res / num_rots).  The reference dereferences these
    on the device (hv_cuda_kernel.cu:22-23); we need them on the host for the launch geometry,
    so the value is read once per tensor OBJECT and version and kept on the object itself
    (a cache keyed by address would hand a recycled allocation the previous tensor's value)."""
    hit = getattr(t, "_cv_host_value", None)
    if hit is None or hit[0] != t._version:
        hit = (t._version, float(t.item()) if kind == "f" else int(t.item()))
        try:
            t._cv_host_value = hit
        except AttributeError:      # exotic tensor subclass without a __dict__: just re-read every call
            pass
    return hit[1]


def prime_scalar(t, value):
    """Record ``value`` as the host value of the 0-dim device tensor ``t`` that was just created from it, so that the first
    vote through ``t`` does not read it back (``_scalar`` still re-reads after any in-place change of ``t``)."""
    t._cv_host_value = (t._version, value)


_ptr, _stream = _lib.ptr, _lib.stream


def _f3(vals):
    return (ctypes.c_float * 3)(*[float(v) for v in vals])


_prefetched = {}
_pinned_pool = []
_prefetch_lock = threading.Lock()      # scene threads share the two containers (bench.py, pipeline.detect_scene)


def _pinned6():
    # pinned landing buffers are recycled: allocating page-locked memory costs about a millisecond per call
    with _prefetch_lock:
        if _pinned_pool:
            return _pinned_pool.pop()
    return torch.empty(6, dtype=torch.float32).pin_memory()


def _recycle(host):
    with _prefetch_lock:
        if len(_pinned_pool) < 64:
            _pinned_pool.append(host)


def reserve_pinned(count):
    """create `count` pinned landing buffers now (bench.py does it before the clock starts)"""
    bufs = [torch.empty(6, dtype=torch.float32).pin_memory() for _ in range(count)]
    for b in bufs:
        _recycle(b)


def prefetch_geometry(points):
    """Start the bounds reduction of `points` now, without waiting for it: a later forward()/grid_geometry() on
    the same (unmodified) tensor picks the result up instead of reducing and stalling in front of the vote.
    Call it before the network forward of the scene (pipeline.detect_scene does)."""
    L = _lib.lib()
    dev = points.device
    ws = _lib.scratch(dev, "hv_minmax", L.cv_hv_minmax_workspace_bytes())
    host = _pinned6()
    with torch.cuda.device(dev):
        _lib.check(L.cv_hv_minmax_async_f32(_ptr(points), points.shape[0], _ptr(host),
                                            _ptr(ws), ws.numel(), _stream(dev)), "cv_hv_minmax_async_f32")
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    stale = []
    with _prefetch_lock:
        # the entry keeps `points` alive, so the address cannot be recycled while it is cached
        # (keyed per host thread: two scene threads may work on the same resident scene at the same time)
        key = (threading.get_ident(), points.data_ptr())
        old = _prefetched.pop(key, None)
        _prefetched[key] = (points, points._version, host, ev)
        if old is not None:
            stale.append(old)
        if len(_prefetched) > 64:
            # entries nobody came back for (a prefetch without a vote): drop the oldest ones whose copy has landed -
            # torch's pinned allocator does not know about the raw hipMemcpyAsync, so a buffer released earlier could
            # be reissued and overwritten by a copy still in flight; entries of other threads still in flight stay
            for k in list(_prefetched)[:-32]:
                if _prefetched[k][3].query():
                    stale.append(_prefetched.pop(k))
    for ent in stale:
        ent[3].synchronize()
        _recycle(ent[2])


def _take_prefetched(points):
    with _prefetch_lock:
        hit = _prefetched.pop((threading.get_ident(), points.data_ptr()), None)
    if hit is None:
        return None
    hit[3].synchronize()
    if hit[0] is not points or hit[1] != points._version:
        _recycle(hit[2])
        return None
    h = hit[2].tolist()
    _recycle(hit[2])
    return h[:3], h[3:]


def _grid_dims(mn, mx, res):
    dims = (ctypes.c_int * 3)()
    _lib.check(_lib.lib().cv_hv_grid_dims_f32(mn, mx, ctypes.c_float(res), dims), "cv_hv_grid_dims_f32")
    return [int(d) for d in dims]


def grid_geometry(points, res):
    """(corner[3], max[3], dims[3]) as hv_cuda_kernel.cu:129-134 computes them (one host sync, or none when
    prefetch_geometry(points) ran earlier)."""
    pre = _take_prefetched(points)
    if pre is not None:
        mn, mx = _f3(pre[0]), _f3(pre[1])
    else:
        L = _lib.lib()
        ws = _lib.scratch(points.device, "hv_minmax", L.cv_hv_minmax_workspace_bytes())
        mn = (ctypes.c_float * 3)()
        mx = (ctypes.c_float * 3)()
        with torch.cuda.device(points.device):
            _lib.check(L.cv_hv_minmax_f32(_ptr(points), points.shape[0], mn, mx, _ptr(ws), ws.numel(),
                                          _stream(points.device)), "cv_hv_minmax_f32")
    return list(mn), list(mx), _grid_dims(mn, mx, res)


def _checked_inputs(points, xyz_labels, scale_labels, obj_labels, res, num_rots, categories=False):
    """The input checks of forward / backward and, with ``categories``, of forward_categories (labels with a leading K axis;
    ``res`` / ``num_rots`` may then be numbers).  Returns (N, res, num_rots, K or None), the two scalars as host values."""
    named = ((points, "points"), (xyz_labels, "xyz_labels"), (scale_labels, "scale_labels"), (obj_labels, "obj_labels"))
    for t, name in named + (() if categories else ((res, "res"), (num_rots, "num_rots"))):
        _check_input(t, name)
    for t, name in named:
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32 (got %s)" % (name, t.dtype))
    n, K = points.shape[0], None
    if categories:
        if xyz_labels.dim() != 3:
            raise RuntimeError("expected xyz_labels / scale_labels [K,N,3] and obj_labels [K,N]")
        K = xyz_labels.shape[0]
    lead = () if K is None else (K,)
    if points.dim() != 2 or points.shape[1] != 3 or xyz_labels.shape != lead + (n, 3) \
            or scale_labels.shape != lead + (n, 3) or obj_labels.shape != lead + (n,):
        raise RuntimeError("expected points [N,3], xyz_labels / scale_labels [K,N,3] and obj_labels [K,N]" if categories else
                           "expected points/xyz_labels/scale_labels [N,3] and obj_labels [N]")
    if n == 0:
        # the reference fails inside torch::min on an empty tensor (hv_cuda_kernel.cu:129)
        raise RuntimeError("hv_cuda: cannot vote with zero points")
    return (n, _scalar(res, "f") if torch.is_tensor(res) else float(res),
            _scalar(num_rots, "i") if torch.is_tensor(num_rots) else int(num_rots), K)


def _vote(points, xyz_labels, scale_labels, obj_labels, res_v, nrot, mn, dims, K=None):
    """The vote onto the grid (origin ``mn``, ``dims``): cv_hv_forward_f32, or with K cv_hv_forward_cat_f32 over the labels'
    category axis (grids [K,X,Y,Z,...]); the grid origin is remembered on grid_obj for the decode that follows."""
    L = _lib.lib()
    n, dev = points.shape[0], points.device
    shape = (() if K is None else (K,)) + tuple(dims)
    grid_obj = torch.empty(shape, dtype=torch.float32, device=dev)
    grid_rot = torch.empty(shape + (2,), dtype=torch.float32, device=dev)
    grid_scale = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    cdims = (ctypes.c_int * 3)(*dims)
    if K is None:
        fn, name, cat, wsb = L.cv_hv_forward_f32, "cv_hv_forward_f32", (), L.cv_hv_forward_workspace_bytes(n, nrot, cdims, _algo)
    else:
        fn, name, cat = L.cv_hv_forward_cat_f32, "cv_hv_forward_cat_f32", (K,)
        wsb = L.cv_hv_forward_cat_workspace_bytes(n, nrot, cdims, _algo, K)
    ws = _lib.scratch(dev, "hv_forward", wsb)
    with torch.cuda.device(dev):
        _lib.check(fn(_ptr(points), _ptr(xyz_labels), _ptr(scale_labels), _ptr(obj_labels), n, ctypes.c_float(res_v), nrot,
                      _f3(mn), cdims, *cat, _ptr(grid_obj), _ptr(grid_rot), _ptr(grid_scale), _ptr(ws), ws.numel(), _algo,
                      _stream(dev)), name)
    # remember the grid origin of this grid so the decode that follows does not reduce the points again
    _remember_corner(grid_obj, mn)
    return [grid_obj, grid_rot, grid_scale]


def forward(points, xyz_labels, scale_labels, obj_labels, res, num_rots, corners=None):
    n, res_v, nrot, _ = _checked_inputs(points, xyz_labels, scale_labels, obj_labels, res, num_rots)
    if corners is None:
        mn, _, dims = grid_geometry(points, res_v)
    else:
        c = corners.detach().to("cpu", torch.float32)
        mn = [float(v) for v in c[0]]
        dims = _grid_dims(_f3(mn), _f3(c[1]), res_v)
    return _vote(points, xyz_labels, scale_labels, obj_labels, res_v, nrot, mn, dims)


def forward_categories(points, xyz_labels, scale_labels, obj_labels, res, num_rots):
    """K categories' votes over the same scan points in ONE launch sequence (cv_hv_forward_cat_f32; separate mode,
    eval_separate.py:166-186): xyz_labels / scale_labels [K,N,3], obj_labels [K,N] -> [grid_obj[K,X,Y,Z],
    grid_rot[K,X,Y,Z,2], grid_scale[K,X,Y,Z,3]].  Category k is bit for bit forward(points, xyz_labels[k], ...).
    ``res`` / ``num_rots`` are 0-dim tensors (as forward takes them) or numbers."""
    n, res_v, nrot, K = _checked_inputs(points, xyz_labels, scale_labels, obj_labels, res, num_rots, categories=True)
    mn, _, dims = grid_geometry(points, res_v)
    return _vote(points, xyz_labels, scale_labels, obj_labels, res_v, nrot, mn, dims, K)


def _scene_bounds(points, row_ranges):
    """(min[3], max[3]) of every row range with ONE host wait: B reductions enqueued on the stream (the kernels grid_geometry
    runs, so the values are forward's), each landing in its own pinned buffer, then one wait for all of them."""
    L = _lib.lib()
    dev = points.device
    ws = _lib.scratch(dev, "hv_minmax", L.cv_hv_minmax_workspace_bytes())
    hosts = [_pinned6() for _ in row_ranges]
    with torch.cuda.device(dev):
        for (a, b), host in zip(row_ranges, hosts):
            # (byte offset of the first row: a slice of a slice keeps the storage offset)
            first = points.data_ptr() + a * 3 * 4
            _lib.check(L.cv_hv_minmax_async_f32(first, b - a, _ptr(host), _ptr(ws), ws.numel(), _stream(dev)),
                       "cv_hv_minmax_async_f32")
        torch.cuda.current_stream(dev).synchronize()
    out = []
    for host in hosts:
        h = host.tolist()
        _recycle(host)
        out.append((h[:3], h[3:]))
    return out


def forward_scenes(points, xyz_labels, scale_labels, obj_labels, row_ranges, res, num_rots, corners=None, thresh=None):
    """B scenes' votes in ONE launch sequence (cv_hv_forward_scenes_f32): scene i votes the rows ``row_ranges[i] = (a, b)`` of the
    shared points [N,3], xyz_labels / scale_labels [N,3] and obj_labels [N] onto its own grid.  Returns a list of B
    ``[grid_obj, grid_rot, grid_scale]``, each bit for bit ``forward(points[a:b], xyz_labels[a:b], ...)`` - with ``corners``
    (a sequence of B [2,3] boxes) the 7-argument form.  Ranges may come in any order and leave gaps; 1 <= B <= 16.  Without
    ``corners`` the B bounds cost one host wait for the whole batch.  ``thresh``: the peaks entry point
    (cv_hv_forward_peaks_scenes_f32) - grid_rot / grid_scale hold values only where grid_obj >= thresh.  Every grid's origin
    is remembered for the decode, so ``decode.decode_boxes_scenes`` takes the result directly.  ``res`` / ``num_rots`` are
    0-dim tensors (as forward takes them) or numbers."""
    named = ((points, "points"), (xyz_labels, "xyz_labels"), (scale_labels, "scale_labels"), (obj_labels, "obj_labels"))
    for t, name in named + tuple((t, nm) for t, nm in ((res, "res"), (num_rots, "num_rots")) if torch.is_tensor(t)):
        _check_input(t, name)
    for t, name in named:
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32 (got %s)" % (name, t.dtype))
    n = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or xyz_labels.shape != (n, 3) or scale_labels.shape != (n, 3) \
            or obj_labels.shape != (n,):
        raise RuntimeError("expected points/xyz_labels/scale_labels [N,3] and obj_labels [N]")
    ranges = [(int(a), int(b)) for a, b in row_ranges]
    B = len(ranges)
    if not 1 <= B <= _lib.MAX_SCENES:
        raise RuntimeError("hv_cuda: expected 1 to %d row ranges (got %d)" % (_lib.MAX_SCENES, B))
    for i, (a, b) in enumerate(ranges):
        if not 0 <= a <= b <= n:
            raise RuntimeError("hv_cuda: row range %d (%d, %d) lies outside the %d rows" % (i, a, b, n))
        if a == b:
            raise RuntimeError("hv_cuda: cannot vote with zero points (row range %d)" % i)
    if corners is not None and len(corners) != B:
        raise RuntimeError("hv_cuda: expected one corners[2,3] box per row range")
    res_v = _scalar(res, "f") if torch.is_tensor(res) else float(res)
    nrot = _scalar(num_rots, "i") if torch.is_tensor(num_rots) else int(num_rots)
    if corners is None:
        geo = [(mn, _grid_dims(_f3(mn), _f3(mx), res_v)) for mn, mx in _scene_bounds(points, ranges)]
    else:
        geo = []
        for c in corners:
            c = c.detach().to("cpu", torch.float32)
            mn = [float(v) for v in c[0]]
            geo.append((mn, _grid_dims(_f3(mn), _f3(c[1]), res_v)))
    L = _lib.lib()
    dev = points.device
    jobs = (_lib.DecodeSceneJob * B)()
    out = []
    for i, ((a, b), (mn, dims)) in enumerate(zip(ranges, geo)):
        shape = tuple(dims)
        grids = [torch.empty(shape + tail, dtype=torch.float32, device=dev) for tail in ((), (2,), (3,))]
        j = jobs[i]
        j.d_grid_obj, j.d_grid_rot, j.d_grid_scale = (g.data_ptr() for g in grids)
        j.dims[:] = dims
        j.corner[:] = mn
        j.row0, j.n = a, b - a
        out.append(grids)
    wsb = L.cv_hv_forward_scenes_workspace_bytes(jobs, B, nrot, _algo)
    ws = _lib.scratch(dev, "hv_forward", max(wsb, 256))
    head = [jobs, B, _ptr(points), _ptr(xyz_labels), _ptr(scale_labels), _ptr(obj_labels), ctypes.c_float(res_v), nrot, _ptr(ws),
            ws.numel(), _algo]
    with torch.cuda.device(dev):
        if thresh is None:
            _lib.check(L.cv_hv_forward_scenes_f32(*head, _stream(dev)), "cv_hv_forward_scenes_f32")
        else:
            _lib.check(L.cv_hv_forward_peaks_scenes_f32(*head, ctypes.c_float(thresh), _stream(dev)),
                       "cv_hv_forward_peaks_scenes_f32")
    for grids, (mn, _) in zip(out, geo):
        _remember_corner(grids[0], mn)
    return out


def backward(grad_grid, points, xyz_labels, scale_labels, obj_labels, res, num_rots, corners=None):
    """``corners`` (optional, not in the reference's 7-positional signature): the [2,3] box the forward was
    given; the grid origin is then corners[0] as in forward() instead of the minimum of the points."""
    _check_input(grad_grid, "grad_grid")
    n, res_v, nrot, _ = _checked_inputs(points, xyz_labels, scale_labels, obj_labels, res, num_rots)
    if grad_grid.dtype != torch.float32 or grad_grid.dim() != 3:
        raise RuntimeError("grad_grid must be a float32 [X,Y,Z] tensor")
    L = _lib.lib()
    dev = points.device
    if corners is None:
        mn, _, _ = grid_geometry(points, res_v)      # hv_cuda_kernel.cu:274-276
    else:
        mn = [float(v) for v in corners.detach().to("cpu", torch.float32)[0]]
    cdims = (ctypes.c_int * 3)(*grad_grid.shape)     # :200 sizes come from grad_grid
    d_xyz = torch.empty_like(xyz_labels)
    d_scale = torch.empty_like(scale_labels)
    d_obj = torch.empty_like(obj_labels)
    with torch.cuda.device(dev):
        _lib.check(L.cv_hv_backward_f32(_ptr(grad_grid), _ptr(points), _ptr(xyz_labels),
                                        _ptr(scale_labels), _ptr(obj_labels), n,
                                        ctypes.c_float(res_v), nrot, _f3(mn), cdims, _ptr(d_xyz),
                                        _ptr(d_scale), _ptr(d_obj), _stream(dev)),
                   "cv_hv_backward_f32")
    return [d_xyz, d_scale, d_obj]


def count_votes(points, xyz_labels, scale_labels, res, num_rots, corner, dims):
    """Number of in-bounds (point, rotation) votes: V_in of the algorithmic byte count."""
    L = _lib.lib()
    dev = points.device
    ws = _lib.scratch(dev, "hv_count", 256)
    out = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        _lib.check(L.cv_hv_count_votes_f32(_ptr(points), _ptr(xyz_labels), _ptr(scale_labels),
                                           points.shape[0], ctypes.c_float(res), int(num_rots),
                                           _f3(corner), (ctypes.c_int * 3)(*dims), ctypes.byref(out),
                                           _ptr(ws), ws.numel(), _stream(dev)),
                   "cv_hv_count_votes_f32")
    return int(out.value)
