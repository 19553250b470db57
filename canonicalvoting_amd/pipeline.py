"""The eval_joint.py / eval_separate.py per-scene path as functions: network -> head split -> vote -> decode -> NMS
(eval_joint.py:163-280), everything on the device, three host syncs per scene (coordinate-set
sizes, vote-grid shape, decode results).

Three ways to run a scene, the same kernels in the same order and the same bits from each:
  call by call      detect_scene (one joint model), detect_scene_separate (one model per category)
  one C call        detect_scene_c, detect_scene_separate_c (cv_detect_scene_f32 / cv_detect_scene_separate_f32)
  from a raw cloud  detect_points_c, detect_points_separate_c (voxelise + gather + the scene in one C call; detect_points is
                    their call-by-call reference)
The joint and the separate calls share everything but their mode's fields: one host-scratch type (_SceneHost, one per
device, stream and mode), one fill of the descriptor fields both modes have (_fill_scene_desc, _fill_landing), one growing
call (_call_growing), one finish step per mode (_finish_joint, _finish_separate) that the voxel-array and the raw-cloud call
both end in, one model-set prologue (_model_set) and one vote + decode + NMS loop per category (_separate_by_calls)."""
import collections
import contextlib
import ctypes
import threading

import numpy as np
import torch

from . import _lib, decode, hv_cuda
from . import me as ME
from ._lib import ptr, stream, vp

SCRATCH_FLOOR = 64 << 20      # bytes of device scratch a scene call starts from


class ScenePolicy(collections.namedtuple("ScenePolicy", "conv_split_target vote_part_records masked_min_rows")):
    """Launch sizing of ONE scene call - the three choices that depend on how many scenes the host keeps in flight:
    conv_split_target  workgroups a split coarse-level convolution aims at (0: the library's value, 768)
    vote_part_records  records one workgroup of a hot (tile, plane) of the vote takes (0: the library's value, 4096)
    masked_min_rows    rows from which a level's 3x3x3 convolutions run mask-sorted (library: 16384)
    Every integer output is the same under every policy; the network output moves in fp32 summation order only
    (tests/test_production_size_gpu.py runs the parity cases under both policies).  A policy travels WITH the call -
    cv_scene_desc.conv_split_target / vote_part_records / masked_min_rows for detect_scene_c, the calling thread's values inside
    scene_policy(...) for the call-by-call path - so two hosts with different policies in one process do not see each other."""
    __slots__ = ()

    def as_config(self):
        return {"conv_split_target": self.conv_split_target, "vote_part_records": self.vote_part_records,
                "masked_min_rows": self.masked_min_rows}


def policy_for_scenes_in_flight(n):
    """The launch sizing for a host that keeps `n` scenes in flight on separate streams (one thread + stream per scene, as
    bench.py does).  The library's defaults are the best for ONE scene at a time; from four scenes in flight the other scenes
    fill the chip and three choices turn (measured on MI355X, LABNOTES rounds 3 and 5): the split convolutions aim at 256
    workgroups instead of 768, a hot (tile, plane) of the vote takes 12288 records per workgroup instead of 4096, and the
    3x3x3 convolutions run mask-sorted from 8192 rows instead of 16384."""
    lib_rows = ME.CoordinateManager.LIB_MASKED_MIN_ROWS
    if int(n) >= 4:
        return ScenePolicy(256, 12288, min(8192, lib_rows))
    return ScenePolicy(0, 0, lib_rows)


@contextlib.contextmanager
def scene_policy(policy):
    """The calling thread's launches inside the block run under `policy` (None: no change): what detect_scene and the module
    paths read (cv_sp_set_split_target_thread, cv_hv_set_part_records_thread, ME.masked_min_rows()); restored on exit."""
    if policy is None:
        yield
        return
    L = _lib.lib()
    prev_t = L.cv_sp_set_split_target_thread(int(policy.conv_split_target))
    prev_r = L.cv_hv_set_part_records_thread(int(policy.vote_part_records))
    prev_m = ME.set_masked_min_rows_thread(policy.masked_min_rows)
    try:
        yield
    finally:
        L.cv_sp_set_split_target_thread(prev_t)
        L.cv_hv_set_part_records_thread(prev_r)
        ME.set_masked_min_rows_thread(prev_m)


def configure_for_scenes_in_flight(n, model=None):
    """policy_for_scenes_in_flight(n) installed PROCESS-WIDE (the default of every thread that runs without a policy of its
    own): for a process with one host loop.  Call it before the scene threads start; hosts that share a process pass
    `policy=` per call instead.  `model` is not needed any more (the models follow ME.masked_min_rows()).  Returns the
    settings as a dict."""
    pol = policy_for_scenes_in_flight(n)
    ME.set_split_target(pol.conv_split_target)
    _lib.lib().cv_hv_set_part_records(pol.vote_part_records)
    ME.CoordinateManager.MASKED_MIN_ROWS = pol.masked_min_rows
    return pol.as_config()


# ---- the call-by-call paths -------------------------------------------------------------------------------------------------------

def _head(out_feats, log_scale, nclasses=None):
    """the head split in one kernel: xyz[N,3], scale[N,3], prob[N] and, for the joint model (``nclasses``), class[N] (int32)"""
    L = _lib.lib()
    F = out_feats.contiguous()
    n, dev = F.shape[0], F.device
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((n, 3), dtype=torch.float32, device=dev)
    prob = torch.empty((n,), dtype=torch.float32, device=dev)
    cls = torch.empty((n,), dtype=torch.int32, device=dev) if nclasses is not None else None
    log_scale = 1 if log_scale else 0
    with torch.cuda.device(dev):
        if nclasses is None:
            _lib.check(L.cv_head_separate_f32(ptr(F), n, F.stride(0), log_scale, ptr(xyz), ptr(scale), ptr(prob), stream(dev)),
                       "cv_head_separate_f32")
            return xyz, scale, prob
        _lib.check(L.cv_head_joint_f32(ptr(F), n, F.stride(0), nclasses, log_scale, ptr(xyz), ptr(scale), ptr(prob), ptr(cls),
                                       stream(dev)), "cv_head_joint_f32")
    return xyz, scale, prob, cls


def head_joint(out_feats, nclasses=9, log_scale=True):
    """eval_joint.py:173-190 in one kernel: -> xyz[N,3], scale[N,3], prob[N], class[N] (int32)."""
    return _head(out_feats, log_scale, nclasses)


def head_separate(out_feats, log_scale=True):
    """eval_separate.py:170-181 in one kernel: -> xyz[N,3], scale[N,3], prob[N]."""
    return _head(out_feats, log_scale)


def detect_scene(model, hv, coords4, feats, res, nclasses=9, log_scale=True, policy=None, **decode_kw):
    """coords4 [N,4] int (batch 0), feats [N,C] already recentred (eval_joint.py:167-168).  policy: ScenePolicy of this call.
    Returns (detections [(class, box[8,3], score)], raw decode dict, network output)."""
    with torch.no_grad(), scene_policy(policy):
        # eval_joint.py:193 scan points; their bounds reduction (the vote grid shape) runs under the network
        scan_points = (coords4[:, 1:].to(feats.device) * res).float().contiguous()
        hv_cuda.prefetch_geometry(scan_points)
        x = ME.SparseTensor(feats, coords4, device=feats.device)
        deferred = hasattr(model, "check_range")
        y = model(x, defer_check=True) if deferred else model(x)
        for attempt in range(2):
            xyz, scale, prob, cls = head_joint(y.F, nclasses, log_scale)
            dets, raw = decode.detect(hv, coords4[:, 1:], xyz, scale, prob, cls, res, nclasses,
                                      scan_points=scan_points, **decode_kw)
            # decode has waited for the stream: the fp16-range flag of the network's convolutions is final now
            y2 = model.check_range(x, y) if (deferred and attempt == 0) else y
            if y2 is y:
                break
            y = y2
    return dets, raw, y


def _separate_defaults(decode_kw):
    """the decode of eval_separate.py: its elimination slice (:209) and a float32 error threshold (tensor > 0.3, :252)"""
    decode_kw.setdefault("separate_variant", True)
    decode_kw.setdefault("err_thresh", float(np.float32(0.3)))


def _separate_by_calls(hv, scan_points, predictions, res, categories, overlap_threshold=0.3, **decode_kw):
    """vote + decode + NMS per category (eval_separate.py:186-264).  ``predictions`` yields one (xyz [N,3], scale [N,3],
    prob [N]) per category and is read category by category: a generator runs its network between two categories' decodes, as
    detect_scene_separate's does.  Returns [(category, box[8,3], score)]."""
    zeros_cls = torch.zeros(scan_points.shape[0], dtype=torch.int32, device=scan_points.device)
    out = []
    for category, pred in zip(categories, predictions):
        xyz, scale, prob = [p.contiguous() for p in pred]
        with torch.no_grad():
            g = hv(scan_points, xyz, scale, prob)
        raw = decode.decode_boxes(g[0], g[1], g[2], scan_points, xyz, prob, zeros_cls, res, **decode_kw)
        for i in decode.nms(raw["boxes"], raw["scores"], overlap_threshold):
            out.append((category, raw["boxes"][i], float(raw["scores"][i])))
    return out


def detect_scene_separate(models, hv, coords4, feats, res, log_scale=True, overlap_threshold=0.3, **decode_kw):
    """eval_separate.py:162-264: one 8-channel model per category on the SAME SparseTensor (the
    coordinate sets, kernel maps and mask orders are built once and shared by all models - the
    reference rebuilds nothing either, but here it is one hash/map build per scene, not per model),
    vote + decode (eval_separate.py:209 elimination slice, float32 error threshold) and NMS per category.
    models: dict category -> MinkUNet34C(in, 8).  Returns [(category, box[8,3], score)]."""
    _separate_defaults(decode_kw)
    with torch.no_grad():
        x = ME.SparseTensor(feats, coords4, device=feats.device)
        scan_points = (coords4[:, 1:].to(feats.device) * res).float().contiguous()
        heads = (head_separate(model(x).F, log_scale) for model in models.values())
        return _separate_by_calls(hv, scan_points, heads, res, list(models.keys()), overlap_threshold, **decode_kw)


# ---- what the one-call paths share ------------------------------------------------------------------------------------------------

class _SceneHost:
    """Host-side scratch of the scene calls of one (device, stream, mode): the pinned landing words, the result arrays -
    [M] candidates, [K, M] with a category axis - the device scratch size the last calls needed (``ws_hint``) and where the
    last call's host time went (``last_host_us``)."""

    def __init__(self, M, K=None, B=None):
        self.M, self.K, self.B = M, K, B
        rows = (M,) if K is None else (K, M)
        if B is not None:   # joint over a scene axis (detect_scenes_c): [B, M]
            rows = (B, M)
        pinned = 256 + 64 * _lib.MAX_SCENES if B is not None else 256 if K is None else 64 + 64 * _lib.MAX_CATEGORIES
        self.pinned = torch.empty(pinned, dtype=torch.uint8).pin_memory()
        self.cand = np.zeros(rows, np.int64)
        self.verdict = np.zeros(rows, np.int32)
        self.boxes = np.zeros(rows + (8, 3), np.float32)
        self.scores = np.zeros(rows, np.float32)
        if K is None:       # joint: the boxes' classes and the NMS picks
            self.classes, self.pick = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
        else:               # separate: (category, box) of every detection
            self.det_cat, self.det_box = np.zeros(K * M, np.int32), np.zeros(K * M, np.int32)
        self.ws_hint = 0
        self.last_host_us = (0.0, 0.0, 0.0, 0.0)


_hosts = {}
_model_tables = {}
_scene_lock = threading.Lock()


def _host(dev, max_candidates, K=None, B=None):
    """the _SceneHost of the calling thread's current stream and of the mode (K None: joint; B: joint over a scene axis of
    up to B scenes); regrown for more candidates, categories or scenes"""
    key = (dev.index, _lib.stream_handle(dev), K is not None) + (() if B is None else ("scenes",))
    with _scene_lock:
        host = _hosts.get(key)
        if host is None or host.M < max_candidates or (K is not None and host.K < K) or (B is not None and host.B < B):
            host = _hosts[key] = _SceneHost(max_candidates, K, B)
    return host


def last_scene_host_us(dev=None):
    """(plan + wait, network enqueue, head + vote enqueue, decode + wait) host microseconds of the calling thread's last
    detect_scene_c call on its current stream"""
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    host = _hosts.get((dev.index, _lib.stream_handle(dev), False))
    return host.last_host_us if host is not None else None


def _fill_scene_desc(d, model, hv, coords4, feats, scan_points, res, policy, pieces, max_channels, log_scale):
    """the scene and launch-sizing fields cv_scene_desc and cv_scene_separate_desc share (model: the one, or the first of the K,
    that the plan follows)"""
    if coords4 is not None:          # (None: a raw-cloud call, which makes the scene's arrays itself)
        d.d_coords4, d.n, d.d_feats, d.feats_ld = ptr(coords4), coords4.shape[0], ptr(feats), feats.stride(0)
        d.d_points = ptr(scan_points)
    d.res, d.num_rots = float(res), hv_cuda._scalar(hv.num_rots, "i")
    d.stem_k, d.mask_groups = model.conv0p1s1.kernel_size, ME.CoordinateManager.plan_mask_groups()
    d.masked_min_rows = policy.masked_min_rows if policy is not None else model.masked_min_rows()
    if policy is not None:
        d.conv_split_target, d.vote_part_records = int(policy.conv_split_target), int(policy.vote_part_records)
    d.max_channels, d.use_range_flag = max_channels, 1 if pieces == 2 else 0
    d.log_scale = 1 if log_scale else 0
    d.vote_algo = hv_cuda._algo


def _fill_landing(d, host, decode_kw, separate_variant, nms_threshold, events):
    """the decode and landing fields both descriptors share: cv_decode_params from the keyword arguments of
    decode.decode_boxes (``separate_variant``: the mode's default), candidate capacity, NMS threshold, the stage events
    (five recorded torch.cuda.Event - their handles exist: scene start, after the network, the head split, the vote, the
    decode), the host's pinned words and its cand / verdict / boxes / scores arrays"""
    p = d.decode
    p.thresh_high = float(decode_kw.get("thresh_high", decode.thresh_high))
    p.thresh_low = float(decode_kw.get("thresh_low", decode.thresh_low))
    p.valid_ratio = float(decode_kw.get("valid_ratio", decode.valid_ratio))
    p.elimination = int(decode_kw.get("elimination", decode.elimination))
    p.prob_thresh = float(decode_kw.get("prob_thresh", 0.3))
    p.elim_hi_plus1 = 0 if decode_kw.get("separate_variant", separate_variant) else 1
    p.err_thresh = float(decode_kw.get("err_thresh", 0.3))
    d.max_candidates, d.nms_threshold = host.M, float(nms_threshold)
    if events is not None:
        for i in range(5):
            d.events[i] = events[i].cuda_event
    d.h_pinned, d.pinned_bytes = ptr(host.pinned), host.pinned.numel()
    d.h_cand_idx, d.h_verdict = vp(host.cand.ctypes.data), vp(host.verdict.ctypes.data)
    d.h_boxes, d.h_scores = vp(host.boxes.ctypes.data), vp(host.scores.ctypes.data)


def _call_growing(fn, name, d, r, dev, scratch_name, ws_hint):
    """fn(d, r, stream) on a device scratch of at least ws_hint bytes; CV_ENOMEM: grow the scratch to result.needed_ws_bytes and
    run the scene again (four attempts).  Returns the scratch the results' device views point into."""
    need = max(ws_hint, SCRATCH_FLOOR)
    for attempt in range(4):
        ws = _lib.scratch(dev, scratch_name, need)
        d.d_ws, d.ws_bytes = ptr(ws), ws.numel()
        with torch.cuda.device(dev):
            rc = fn(ctypes.byref(d), ctypes.byref(r), stream(dev))
        if rc != -12 or r.needed_ws_bytes <= ws.numel():
            break
        torch.cuda.current_stream(dev).synchronize()
        need = int(r.needed_ws_bytes)
    _lib.check(rc, name)          # (still CV_ENOMEM after four growing attempts: not an empty scene)
    return ws


def _device_view(address, shape, dtype, dev, owner):
    """tensor view of a region of the scene scratch (valid until the next scene call on the same stream)"""
    count = int(np.prod(shape))
    off = int(address) - owner.data_ptr()
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    assert 0 <= off and off + nbytes <= owner.numel()
    return owner[off:off + nbytes].view(dtype).view(*shape).clone()


def _points_front(front, points, feats, res, recentre_from, predictions, return_inverse, with_class):
    """cv_points_front of a raw cloud; returns (coords4 [M, 4], index [M], inverse [M] or None, the tensors to keep alive)"""
    dev = points.device
    assert points.is_cuda and points.dim() == 2 and points.shape[1] == 3, "points: a [M, 3] device tensor"
    if points.dtype not in (torch.float32, torch.float64):      # (as ME.utils.quantize_device: computed in fp64, as numpy promotes them)
        points = points.to(torch.float64)
    if points.stride(1) != 1 or points.stride(0) < 3:
        points = points.contiguous()
    m, in_channels = points.shape[0], feats.shape[1]
    if m == 0:
        raise RuntimeError("sparse_quantize: empty point cloud")
    feats = feats.to(device=dev, dtype=torch.float32)
    if feats.stride(1) != 1 or feats.stride(0) < feats.shape[1]:
        feats = feats.contiguous()
    if feats.shape != (m, in_channels):
        raise ValueError("raw cloud: feats must be [%d, %d] (got %s)" % (m, in_channels, tuple(feats.shape)))
    coords4 = torch.empty((m, 4), dtype=torch.int32, device=dev)
    index = torch.empty(m, dtype=torch.int32, device=dev)
    inverse = torch.empty(m, dtype=torch.int32, device=dev) if return_inverse else None
    front.d_raw_points, front.m, front.points_ld = ptr(points), m, points.stride(0)
    front.points_f64 = 1 if points.dtype == torch.float64 else 0
    front.quantization_size = float(res)
    front.d_raw_feats, front.raw_feats_ld, front.in_channels = ptr(feats), feats.stride(0), in_channels
    front.recentre_from = -1 if recentre_from is None else int(recentre_from)
    front.d_coords4, front.d_index = ptr(coords4), ptr(index)
    front.d_inverse = ptr(inverse) if return_inverse else None
    alive = [points, feats]
    if predictions is not None:
        pred = [p.to(dev).contiguous() for p in predictions]
        if with_class:
            pred[3] = pred[3].to(torch.int32).contiguous()
            front.d_raw_class = ptr(pred[3])
        front.d_raw_xyz, front.d_raw_scale, front.d_raw_prob = ptr(pred[0]), ptr(pred[1]), ptr(pred[2])
        alive += pred
    return coords4, index, inverse, alive


def _call_points(fn, name, d, r, dev, scratch_name, ws_hint):
    """_call_growing for a raw-cloud descriptor (the scratch and its size live in the embedded scene descriptor / result); a
    rejected cloud raises RuntimeError with the count, as ME.utils.quantize_device does"""
    call = lambda _d, _r, s: fn(ctypes.byref(d), ctypes.byref(r), s)
    try:
        return _call_growing(call, name, d.scene, r.scene, dev, scratch_name, ws_hint)
    except _lib.CvError:
        if r.rejected:
            ME.utils.raise_rejected(r.rejected)
        raise


# ---- joint mode -------------------------------------------------------------------------------------------------------------------

def _fill_joint_desc(d, host, program, y, nclasses, decode_kw, adaptive_split, events, keep):
    """cv_scene_desc beyond the shared fields: the program, the output, the classes and picks"""
    c_ops, c_bufs = program[:2]
    d.ops, d.n_ops, d.bufs, d.n_bufs = ctypes.cast(c_ops, vp), len(c_ops), ctypes.cast(c_bufs, vp), len(c_bufs)
    d.d_out_feats, d.out_ld, d.out_channels = ptr(y), y.stride(0), y.shape[1]
    d.nclasses, d.adaptive_split = nclasses, 1 if adaptive_split else 0
    d.peak_quotients = 1 if keep is None else 0      # nobody sees the grids without ``keep``: rot / scale only where the decode reads them
    d.h_classes, d.h_pick = vp(host.classes.ctypes.data), vp(host.pick.ctypes.data)
    _fill_landing(d, host, decode_kw, False, 0.3, events)


def _finish_joint(host, r, keep, y, n, dev, ws, more_keep=None):
    """After cv_detect_scene_f32 / cv_detect_points_f32 (``r``: the cv_scene_result): raise the host's scratch hint, note
    where the host time went, and - unless the scene has to be redone (a convolution input beyond the fp16 range, or more
    candidate cells than the result arrays hold: returns None) - copy the results out: (detections, raw decode dict, y).
    ``keep`` (optional) receives ``more_keep()`` and the device views."""
    host.ws_hint = max(host.ws_hint, int(r.needed_ws_bytes))
    host.last_host_us = tuple(r.host_us)            # (plan + wait, network enqueue, head + vote, decode + wait)
    if r.range_flag or r.truncated:
        return None
    k, m = r.n_boxes, r.n_cand
    raw = dict(boxes=host.boxes[:k].copy(), scores=host.scores[:k].copy(), classes=host.classes[:k].copy(),
               cand_idx=host.cand[:m].copy(), verdict=host.verdict[:m].copy(), truncated=False)
    dets = [(int(raw["classes"][i]), raw["boxes"][i], float(raw["scores"][i])) for i in host.pick[:r.n_det]]
    if keep is not None:
        if more_keep is not None:
            keep.update(more_keep())
        view = lambda p, shape, dt=torch.float32: _device_view(p, shape, dt, dev, ws)
        X, Y, Z = r.dims
        keep.update(y=y, dims=(X, Y, Z), corner=tuple(r.corner), level_rows=list(r.level_rows),
                    grids=(view(r.d_grid_obj, (X, Y, Z)), view(r.d_grid_rot, (X, Y, Z, 2)), view(r.d_grid_scale, (X, Y, Z, 3))),
                    net_pred=(view(r.d_xyz, (n, 3)), view(r.d_scale, (n, 3)), view(r.d_prob, (n,)),
                              view(r.d_class, (n,), torch.int32)), raw=raw)
    return dets, raw, y


def detect_scene_c(model, hv, coords4, feats, res, nclasses=9, log_scale=True, scan_points=None, predictions=None,
                   max_candidates=512, keep=None, events=None, adaptive_split=False, policy=None, **decode_kw):
    """detect_scene through ONE C call (cv_detect_scene_f32: coordinate plan -> network program -> head -> vote -> decode
    -> per-class NMS; two host waits inside it, the GIL released for its whole duration).  Same kernels in the same order
    as detect_scene: bit-identical results (tests/test_scene_call_gpu.py).  ``predictions`` = (xyz, scale, prob, class)
    fed to vote + decode instead of the network's (bench.py --predictions teacher).  A scene that needs what the call
    does not do - a range fallback onto the bf16 triples, a decode walk beyond ``max_candidates`` - is redone by the
    call-by-call path.  ``events``: five recorded torch.cuda.Event that the call re-records at the stage boundaries.
    ``policy``: ScenePolicy of THIS call (None: the thread's / process-wide values).
    Returns (detections, raw decode dict, network output [N, C])."""
    dev = feats.device
    _keep_begin(keep, res)
    n = coords4.shape[0]
    if scan_points is None:
        scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
    pieces = model.eval_pieces()
    program = model._program(dev, pieces)
    coords4 = coords4.to(device=dev, dtype=torch.int32).contiguous()
    feats = feats.contiguous()
    y = torch.empty((n, model.final.out_channels), dtype=torch.float32, device=dev)
    host = _host(dev, max_candidates)
    d, r = _lib.SceneDesc(), _lib.SceneResult()
    _fill_scene_desc(d, model, hv, coords4, feats, scan_points, res, policy, pieces, max(model.PLANES), log_scale)
    if predictions is not None:
        px, ps, pp, pc = predictions
        pc = pc.to(torch.int32).contiguous()
        d.d_xyz_in, d.d_scale_in, d.d_prob_in, d.d_class_in = ptr(px), ptr(ps), ptr(pp), ptr(pc)
        if keep is not None:
            keep["decode_prob"] = pp
    _fill_joint_desc(d, host, program, y, nclasses, decode_kw, adaptive_split, events, keep)
    ws = _call_growing(_lib.lib().cv_detect_scene_f32, "cv_detect_scene_f32", d, r, dev, "scene_call", host.ws_hint)
    out = _finish_joint(host, r, keep, y, n, dev, ws)
    if out is not None:
        return out
    # rare: a convolution input beyond the fp16 range, or more candidate cells than the result arrays hold
    if r.range_flag:
        model.range_fallbacks = getattr(model, "range_fallbacks", 0) + 1
    with torch.no_grad(), scene_policy(policy):
        x = ME.SparseTensor(feats, coords4, device=dev)
        yy = model.program_forward(x, pieces=3) if r.range_flag else x._like(y, 1)
        pred = head_joint(yy.F, nclasses, log_scale) if predictions is None else predictions
        dets, raw = decode.detect(hv, coords4[:, 1:], pred[0], pred[1], pred[2], pred[3], res, nclasses,
                                  scan_points=scan_points, **decode_kw)
    return dets, raw, yy.F


def detect_scenes_c(model, hv, coords4, feats, res, num_scenes, scan_points=None, predictions=None, keep=None, policy=None,
                    events=None, nclasses=9, log_scale=True, max_candidates=512, adaptive_split=False, **decode_kw):
    """detect_scene_c for ``num_scenes`` scans in ONE C call (cv_detect_scenes_f32): ``coords4`` / ``feats`` are the scans
    collated one after another with batch indices 0..B-1 (non-decreasing), ``scan_points`` and ``predictions`` cover all rows.
    One coordinate plan, one network program and one head launch over all rows, one vote and one decode over the scene
    axis: two host waits per batch.  Scene b's vote grids, decode and detections are the bits detect_scene_c gives for that
    scan alone when ``predictions`` are given; on the network's own predictions they follow the batched network output,
    which agrees with the scan-alone output within the network's tolerance.  A raised fp16-range flag redoes the whole batch
    call by call on the bf16 triples, a decode walk beyond ``max_candidates`` that scene's decode, as detect_scene_c does.
    ``keep``: a list that receives B dicts, each what detect_scene_c's ``keep`` holds for that scene (scene_instances takes
    them unchanged).  Returns ([(detections, raw decode dict)] per scene, network output [N, C])."""
    dev = feats.device
    B = int(num_scenes)
    n = coords4.shape[0]
    if scan_points is None:
        scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
    pieces = model.eval_pieces()
    program = model._program(dev, pieces)
    coords4 = coords4.to(device=dev, dtype=torch.int32).contiguous()
    feats = feats.contiguous()
    y = torch.empty((n, model.final.out_channels), dtype=torch.float32, device=dev)
    host = _host(dev, max_candidates, B=max(B, 1))
    d, r = _lib.ScenesDesc(), _lib.ScenesResult()
    d.num_scenes = B
    _fill_scene_desc(d.scene, model, hv, coords4, feats, scan_points, res, policy, pieces, max(model.PLANES), log_scale)
    if predictions is not None:
        px, ps, pp, pc = predictions
        pc = pc.to(torch.int32).contiguous()
        d.scene.d_xyz_in, d.scene.d_scale_in, d.scene.d_prob_in, d.scene.d_class_in = ptr(px), ptr(ps), ptr(pp), ptr(pc)
    _fill_joint_desc(d.scene, host, program, y, nclasses, decode_kw, adaptive_split, events, keep)
    call = lambda _d, _r, s: _lib.lib().cv_detect_scenes_f32(ctypes.byref(d), ctypes.byref(r), s)
    ws = _call_growing(call, "cv_detect_scenes_f32", d.scene, r, dev, "scene_call", host.ws_hint)
    host.ws_hint = max(host.ws_hint, int(r.needed_ws_bytes))
    host.last_host_us = tuple(r.host_us)
    yy = y
    if r.range_flag:        # rare: a convolution input beyond the fp16 range - the whole batch again on the bf16 triples
        model.range_fallbacks = getattr(model, "range_fallbacks", 0) + 1
        with torch.no_grad(), scene_policy(policy):
            yy = model.program_forward(ME.SparseTensor(feats, coords4, device=dev), pieces=3).F
    net_pred = head_joint(yy, nclasses, log_scale) if r.range_flag and predictions is None else None
    view = lambda p, shape, dt=torch.float32: _device_view(p, shape, dt, dev, ws)
    out, head = [], None
    if keep is not None:
        del keep[:]
    for b in range(B):
        lo, hi = int(r.row0[b]), int(r.row0[b] + r.rows[b])
        kb = None
        if keep is not None:
            kb = {}
            _keep_begin(kb, res)
            keep.append(kb)
            if predictions is not None:
                kb["decode_prob"] = pp[lo:hi]
        if r.range_flag or r.truncated[b]:
            # this scene's vote and decode call by call, on its rows
            pred = [t[lo:hi] for t in (predictions if predictions is not None else net_pred or head_joint(yy, nclasses, log_scale))]
            with torch.no_grad(), scene_policy(policy):
                dets, raw = decode.detect(hv, coords4[lo:hi, 1:], pred[0], pred[1], pred[2], pred[3], res, nclasses,
                                          scan_points=scan_points[lo:hi], **decode_kw)
            out.append((dets, raw))
            continue
        k, m = r.n_boxes[b], r.n_cand[b]
        raw = dict(boxes=host.boxes[b, :k].copy(), scores=host.scores[b, :k].copy(), classes=host.classes[b, :k].copy(),
                   cand_idx=host.cand[b, :m].copy(), verdict=host.verdict[b, :m].copy(), truncated=False)
        dets = [(int(raw["classes"][i]), raw["boxes"][i], float(raw["scores"][i])) for i in host.pick[b, :r.n_det[b]]]
        if kb is not None:
            X, Y, Z = r.dims[b]
            if head is None:
                head = [view(r.d_xyz, (n, 3)), view(r.d_scale, (n, 3)), view(r.d_prob, (n,)), view(r.d_class, (n,), torch.int32)]
            kb.update(y=y[lo:hi], rows=(lo, hi), dims=(X, Y, Z), corner=tuple(r.corner[b]), level_rows=list(r.level_rows),
                      grids=(view(r.d_grid_obj[b], (X, Y, Z)), view(r.d_grid_rot[b], (X, Y, Z, 2)),
                             view(r.d_grid_scale[b], (X, Y, Z, 3))),
                      net_pred=tuple(t[lo:hi] for t in head), raw=raw)
        out.append((dets, raw))
    return out, yy


def detect_points(model, hv, points, feats, res, predictions=None, return_inverse=False, **kw):
    """detect_scene_c from a RAW device cloud: ``points`` [M, 3] (fp32 or fp64) are voxelised on the device at ``res``
    (ME.utils.quantize_device: one point - the first - per voxel), ``feats`` [M, C] and, if given, the raw-point-aligned
    ``predictions`` (xyz, scale, prob, class) are gathered by the first-point index, and the scene runs as detect_scene_c
    runs it - world points formed from the integer coordinates - so the results are bit for bit those of quantising on
    the host and calling detect_scene_c.  Returns detect_scene_c's (detections, raw, network output) plus ``index`` [N]
    (and ``inverse`` [M] with return_inverse).  The call-by-call reference of detect_points_c, which does all of it in ONE
    C call."""
    coords4, index, inverse = ME.utils.quantize_device(points, res, None, return_inverse)
    gi = index.long()
    dev = coords4.device
    f = feats.to(dev)[gi]
    if predictions is not None:
        predictions = tuple(p.to(dev)[gi].contiguous() for p in predictions)
    out = detect_scene_c(model, hv, coords4, f, res, predictions=predictions, **kw)
    return out + ((index, inverse) if return_inverse else (index,))


def detect_points_c(model, hv, points, feats, res, predictions=None, return_inverse=False, recentre_from=None, nclasses=9,
                    log_scale=True, max_candidates=512, keep=None, events=None, adaptive_split=False, policy=None, **decode_kw):
    """detect_points through ONE C call (cv_detect_points_f32: voxelise -> one gather launch for the features, world points
    and predictions of the voxels' first points -> the scene of detect_scene_c), the GIL released for all of it: a host
    that keeps several raw scenes in flight from several threads makes one foreign call per scene.  Same kernels in the same
    order as detect_points: the same bits.  Three host waits inside the call: the voxel count, the level counts, the decode.

    points [M, 3] device tensor (fp64 clouds are voxelised in fp64, other dtypes than fp32 converted to it; rows may be
    strided), feats [M, C] and the optional ``predictions`` (xyz, scale, prob, class) aligned with the RAW points.
    ``recentre_from`` = c: feature columns >= c are fed to the network as ``x * 2 - 1`` (eval_joint.py:167-168, in the
    gather).  ``keep`` / ``events`` / ``policy`` / ``max_candidates`` as detect_scene_c; keep also receives ``scan_points``,
    ``feats`` (the gathered ones) and the call's ``host_us`` / ``host_us_front``.  The network output buffer has M rows (the
    voxel count N is not known before the call): the returned y is its first N.  A scene that needs what the call does not
    do (range fallback, a decode walk beyond ``max_candidates``) is rerun through detect_scene_c from the voxel arrays the call
    filled.  A cloud with rejected points raises RuntimeError with their count.
    Returns (detections, raw, y [N, C'], index [N][, inverse [M]])."""
    dev = points.device
    _keep_begin(keep, res)
    pieces = model.eval_pieces()
    program = model._program(dev, pieces)
    d, r = _lib.PointsDesc(), _lib.PointsResult()
    coords4, index, inverse, alive = _points_front(d.front, points, feats, res, recentre_from, predictions, return_inverse, True)
    y = torch.empty((coords4.shape[0], model.final.out_channels), dtype=torch.float32, device=dev)
    host = _host(dev, max_candidates)
    _fill_scene_desc(d.scene, model, hv, None, None, None, res, policy, pieces, max(model.PLANES), log_scale)
    _fill_joint_desc(d.scene, host, program, y, nclasses, decode_kw, adaptive_split, events, keep)
    ws = _call_points(_lib.lib().cv_detect_points_f32, "cv_detect_points_f32", d, r, dev, "scene_call", host.ws_hint)
    del alive
    n = int(r.n)
    coords4, index, y = coords4[:n], index[:n], y[:n]
    tail = (index, inverse) if return_inverse else (index,)
    view = lambda p, shape, dt=torch.float32: _device_view(p, shape, dt, dev, ws)
    gathered = lambda: dict(scan_points=view(r.d_points, (n, 3)), feats=view(r.d_feats, (n, d.front.in_channels)),
                            host_us=tuple(r.scene.host_us), host_us_front=float(r.host_us_front),
                            front_ws_bytes=int(r.front_ws_bytes),
                            **({} if predictions is None else dict(decode_prob=view(r.d_prob_in, (n,)))))
    out = _finish_joint(host, r.scene, keep, y, n, dev, ws, gathered)
    if out is not None:
        return out + tail
    pred = None
    if predictions is not None:
        pred = (view(r.d_xyz_in, (n, 3)), view(r.d_scale_in, (n, 3)), view(r.d_prob_in, (n,)), view(r.d_class_in, (n,), torch.int32))
    return detect_scene_c(model, hv, coords4, view(r.d_feats, (n, d.front.in_channels)), res, nclasses=nclasses,
                          log_scale=log_scale, predictions=pred, max_candidates=max_candidates, keep=keep, events=events,
                          adaptive_split=adaptive_split, policy=policy, **decode_kw) + tail


# ---- separate mode ----------------------------------------------------------------------------------------------------------------

def model_params_table(mods, dev, pieces):
    """Device table of cv_net_model_params [n_ops][K] for the model set ``mods`` (cv_net_run_models_f32: what differs between
    the K programs without a constant stride - packed weights, folded affine, acc_scale).  Cached per model set next to
    the programs it was filled from: a program that ``_program`` rebuilt (another parameter version) rebuilds the table.
    Returns (programs, table tensor)."""
    progs = [m._program(dev, pieces) for m in mods]
    key = (str(dev), pieces, tuple(id(m) for m in mods))
    with _scene_lock:
        hit = _model_tables.get(key)
    if hit is not None and len(hit[0]) == len(progs) and all(a is b for a, b in zip(hit[0], progs)):
        return progs, hit[1]
    L = _lib.lib()
    K, n_ops = len(progs), len(progs[0][0])
    if any(len(p[0]) != n_ops for p in progs):
        raise ValueError("model_params_table: the models' programs differ in length")
    nbytes = L.cv_net_models_params_bytes(n_ops, K)
    host = np.zeros(nbytes, np.uint8)
    ops = (vp * K)(*[ctypes.cast(p[0], vp) for p in progs])
    _lib.check(L.cv_net_models_params_fill(ops, n_ops, K, vp(host.ctypes.data), nbytes), "cv_net_models_params_fill")
    table = torch.from_numpy(host).to(dev)
    with _scene_lock:
        _model_tables[key] = (progs, table)
    return progs, table


def _model_set(who, mods, dev, models_per_pass, scene_call=True):
    """The prologue of every call on K structurally identical models (``who``: the caller's name in the error text):
    -> (K, pieces, G, programs, parameter table).  A scene call takes 1..MAX_CATEGORIES models, and G = 0 (``models_per_pass``
    None or 0) runs one network after another, without a table; forward_models (scene_call False) always runs over the
    model axis, all K in one pass unless told otherwise."""
    K = len(mods)
    if scene_call and not 1 <= K <= _lib.MAX_CATEGORIES:
        raise ValueError("%s: 1..%d models (got %d)" % (who, _lib.MAX_CATEGORIES, K))
    pieces = mods[0].eval_pieces()
    G = int(models_per_pass or 0)
    if scene_call and G < 0:
        raise ValueError("%s: models_per_pass must be >= 0 (got %d)" % (who, G))
    if not scene_call:
        G = min(G, K) if G else K
    if G > 0 or not scene_call:
        return (K, pieces, G) + model_params_table(mods, dev, pieces)
    return K, pieces, G, [m._program(dev, pieces) for m in mods], None


def forward_models(mods, x, models_per_pass=None, range_flags=None):
    """The eval forward of K structurally identical models on ONE SparseTensor through cv_net_run_models_f32: passes of up
    to ``models_per_pass`` models (None: all K), every launch covering the pass's models.  Returns the K outputs [N, C] -
    bit for bit what ``m.program_forward(x)`` gives for each model.  ``range_flags``: optional zeroed int32 device tensor
    [K, 16]; word [k, 0] is set when model k saw an input beyond the fp16 range (nothing is redone here)."""
    L = _lib.lib()
    dev = x.F.device
    mods = list(mods)
    K, pieces, G, progs, table = _model_set("forward_models", mods, dev, models_per_pass, scene_call=False)
    m0 = mods[0]
    plan = x.coordinate_manager.fused_fast(m0.conv0p1s1.kernel_size)
    args = m0.launch_args(plan, max_planes=max(max(m.PLANES) for m in mods))
    if args is None:
        raise ValueError("forward_models: the plan has no mask orders for a level that runs mask-sorted")
    rows, ws_one, c_maps, c_perms = args
    feats = x.F.contiguous()
    ys = [torch.empty((plan.counts[0], m.final.out_channels), dtype=torch.float32, device=dev) for m in mods]
    c_bufs0 = progs[0][1]
    arena = _lib.scratch(dev, "net_arena_models", L.cv_net_models_arena_bytes(c_bufs0, len(c_bufs0), rows, 5, G))
    ws = _lib.scratch(dev, "conv_ws_models", L.cv_net_models_workspace_bytes(ws_one, G))
    ext_ld = (ctypes.c_int * 2)(feats.stride(0), ys[0].stride(0))
    n_ops = len(progs[0][0])
    entry = ctypes.sizeof(_lib.NetModelParams)
    with torch.cuda.device(dev):
        for k0 in range(0, K, G):
            g = min(G, K - k0)
            ops = (vp * g)(*[ctypes.cast(p[0], vp) for p in progs[k0:k0 + g]])
            bufs = (vp * g)(*[ctypes.cast(p[1], vp) for p in progs[k0:k0 + g]])
            ext = [(vp * 2)(feats.data_ptr(), y.data_ptr()) for y in ys[k0:k0 + g]]
            c_ext = (vp * g)(*[ctypes.cast(e, vp) for e in ext])
            flag = vp(range_flags.data_ptr() + 64 * k0) if range_flags is not None else None
            _lib.check(L.cv_net_run_models_f32(ops, bufs, n_ops, len(c_bufs0), g, rows, 5, ptr(arena), arena.numel(), c_ext,
                                               ext_ld, c_maps, len(c_maps), c_perms, len(c_perms), ptr(ws), ws.numel(), flag,
                                               vp(table.data_ptr() + entry * k0), K, stream(dev)), "cv_net_run_models_f32")
    return ys


def _fill_separate_desc(d, host, progs, table, G, ys, decode_kw, overlap_threshold, events):
    """cv_scene_separate_desc beyond the shared fields: the K programs and outputs as arrays, the pass size, the detections'
    (category, box).  Returns the pointer tables the descriptor refers to (keep them alive over the call)."""
    K = len(progs)
    d.num_models = K
    if G > 0:
        d.models_per_pass, d.d_model_params = G, ptr(table)
    ops = (vp * K)(*[ctypes.cast(p[0], vp) for p in progs])
    n_ops = (ctypes.c_int * K)(*[len(p[0]) for p in progs])
    bufs = (vp * K)(*[ctypes.cast(p[1], vp) for p in progs])
    n_bufs = (ctypes.c_int * K)(*[len(p[1]) for p in progs])
    outs = (vp * K)(*[y.data_ptr() for y in ys])
    d.ops, d.n_ops, d.bufs, d.n_bufs = ctypes.cast(ops, vp), ctypes.cast(n_ops, vp), ctypes.cast(bufs, vp), ctypes.cast(n_bufs, vp)
    d.d_out_feats, d.out_ld, d.out_channels = ctypes.cast(outs, vp), ys[0].stride(0), ys[0].shape[1]
    d.h_det_cat, d.h_det_box = vp(host.det_cat.ctypes.data), vp(host.det_box.ctypes.data)
    _fill_landing(d, host, decode_kw, True, overlap_threshold, events)
    return ops, n_ops, bufs, n_bufs, outs


def _finish_separate(host, r, keep, categories, ys, n, dev, ws, **more_keep):
    """After cv_detect_scene_separate_f32 / cv_detect_points_separate_f32 (``r``: the cv_scene_separate_result): raise the
    host's scratch hint, hand ``keep`` (optional) the call's ``range_flag`` bits, ``needed_ws_bytes`` and ``more_keep``, and -
    unless the scene has to be redone (a model's input beyond the fp16 range, or a category whose walk filled the result
    arrays: returns None) - copy the detections out; ``keep`` then also receives the per-category raw decode and the device
    views."""
    K = len(categories)
    host.ws_hint = max(host.ws_hint, int(r.needed_ws_bytes))
    host.last_host_us = tuple(r.host_us)
    if keep is not None:
        keep.update(range_flag=int(r.range_flag), needed_ws_bytes=int(r.needed_ws_bytes), **more_keep)
    if r.range_flag or any(r.truncated[k] for k in range(K)):
        return None
    dets = [(categories[int(c)], host.boxes[int(c), int(b)].copy(), float(host.scores[int(c), int(b)]))
            for c, b in zip(host.det_cat[:r.n_det], host.det_box[:r.n_det])]
    if keep is not None:
        X, Y, Z = r.dims
        view = lambda p, shape: _device_view(p, shape, torch.float32, dev, ws)
        raw = [dict(boxes=host.boxes[k, :r.n_boxes[k]].copy(), scores=host.scores[k, :r.n_boxes[k]].copy(),
                    cand_idx=host.cand[k, :r.n_cand[k]].copy(), verdict=host.verdict[k, :r.n_cand[k]].copy())
               for k in range(K)]
        keep.update(y=ys, dims=(X, Y, Z), corner=tuple(r.corner), level_rows=list(r.level_rows), raw=raw,
                    grids=(view(r.d_grid_obj, (K, X, Y, Z)), view(r.d_grid_rot, (K, X, Y, Z, 2)),
                           view(r.d_grid_scale, (K, X, Y, Z, 3))),
                    net_pred=(view(r.d_xyz, (K, n, 3)), view(r.d_scale, (K, n, 3)), view(r.d_prob, (K, n))),
                    host_us=tuple(r.host_us))
    return dets


def detect_scene_separate_c(models, hv, coords4, feats, res, predictions=None, policy=None, keep=None, events=None,
                            log_scale=True, overlap_threshold=0.3, max_candidates=512, scan_points=None,
                            models_per_pass=None, **decode_kw):
    """detect_scene_separate through ONE C call (cv_detect_scene_separate_f32: the coordinate plan once, the K models'
    programs, K heads, ONE vote and ONE decode over the category axis - one host wait for the decode - and NMS per category;
    the GIL released for the whole call).  Returns what detect_scene_separate returns, [(category, box[8,3], score)], in the
    same order and the same bits.  ``predictions`` = (xyz [K,N,3], scale [K,N,3], prob [K,N]) fed to vote + decode instead of
    the networks'.  A scene with a model's input beyond the fp16 range, or a category whose walk fills ``max_candidates``,
    is redone by the call-by-call path.  ``keep`` receives the per-model outputs (``y``), the head outputs (``net_pred``),
    the [K,...] grids, the per-category raw decode (``raw``), dims and corner, and - also for a scene that is redone - the call's
    ``range_flag`` bits and ``needed_ws_bytes``.  ``events``: five recorded torch.cuda.Event
    re-recorded at the stage boundaries.  ``policy``: ScenePolicy of this call.  ``models_per_pass`` = G >= 1: the K networks
    run as passes of up to G models over a model axis (cv_net_run_models_f32: every convolution launch covers G models) and
    the K heads as one launch - the same bits with about K times fewer network launches, G arenas and convolution workspaces
    of scratch; None or 0: one network after another."""
    _separate_defaults(decode_kw)
    dev = feats.device
    n = coords4.shape[0]
    categories, mods = list(models.keys()), list(models.values())
    _keep_begin(keep, res, categories)
    if scan_points is None:
        scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
    K, pieces, G, progs, table = _model_set("detect_scene_separate_c", mods, dev, models_per_pass)
    coords4 = coords4.to(device=dev, dtype=torch.int32).contiguous()
    feats = feats.contiguous()
    ys = [torch.empty((n, m.final.out_channels), dtype=torch.float32, device=dev) for m in mods]
    M = int(max_candidates)
    host = _host(dev, M, K)
    d, r = _lib.SceneSeparateDesc(), _lib.SceneSeparateResult()
    _fill_scene_desc(d, mods[0], hv, coords4, feats, scan_points, res, policy, pieces, max(max(m.PLANES) for m in mods), log_scale)
    if predictions is not None:
        px, ps, pp = [a.contiguous() for a in predictions]
        d.d_xyz_in, d.d_scale_in, d.d_prob_in = ptr(px), ptr(ps), ptr(pp)
        if keep is not None:
            keep["decode_prob"] = pp
    alive = _fill_separate_desc(d, host, progs, table, G, ys, decode_kw, overlap_threshold, events)
    ws = _call_growing(_lib.lib().cv_detect_scene_separate_f32, "cv_detect_scene_separate_f32", d, r, dev,
                       "scene_call_separate", host.ws_hint)
    del alive
    dets = _finish_separate(host, r, keep, categories, ys, n, dev, ws)
    if dets is not None:
        return dets
    # rare: a convolution input beyond the fp16 range, or more candidate cells than the result arrays hold
    kw = dict(decode_kw, max_candidates=M)
    if predictions is None:
        return detect_scene_separate(models, hv, coords4, feats, res, log_scale=log_scale, overlap_threshold=overlap_threshold, **kw)
    return _separate_by_calls(hv, scan_points, zip(*predictions), res, categories, overlap_threshold, **kw)


def detect_points_separate_c(models, hv, points, feats, res, predictions=None, models_per_pass=None, return_inverse=False,
                             recentre_from=None, policy=None, keep=None, events=None, log_scale=True, overlap_threshold=0.3,
                             max_candidates=512, **decode_kw):
    """detect_scene_separate_c from a RAW device cloud through ONE C call (cv_detect_points_separate_f32): voxelise, gather,
    then the K models' scene.  ``predictions`` = (xyz [K, M, 3], scale [K, M, 3], prob [K, M]) aligned with the raw points; the
    other arguments as detect_points_c / detect_scene_separate_c.  The same bits as ME.utils.quantize_device + torch gathers
    + detect_scene_separate_c.  Returns (detections [(category, box[8,3], score)], index [N][, inverse [M]]); ``keep``
    receives what detect_scene_separate_c's does (``y``: the K outputs' first N rows) plus ``coords4`` and ``world_points``
    [N, 3], the scan points the scene ran on."""
    _separate_defaults(decode_kw)
    dev = points.device
    categories, mods = list(models.keys()), list(models.values())
    _keep_begin(keep, res, categories)
    K, pieces, G, progs, table = _model_set("detect_points_separate_c", mods, dev, models_per_pass)
    d, r = _lib.PointsSeparateDesc(), _lib.PointsSeparateResult()
    coords4, index, inverse, alive = _points_front(d.front, points, feats, res, recentre_from, predictions, return_inverse, False)
    ys = [torch.empty((coords4.shape[0], m.final.out_channels), dtype=torch.float32, device=dev) for m in mods]
    M = int(max_candidates)
    host = _host(dev, M, K)
    _fill_scene_desc(d.scene, mods[0], hv, None, None, None, res, policy, pieces, max(max(m.PLANES) for m in mods), log_scale)
    alive.append(_fill_separate_desc(d.scene, host, progs, table, G, ys, decode_kw, overlap_threshold, events))
    ws = _call_points(_lib.lib().cv_detect_points_separate_f32, "cv_detect_points_separate_f32", d, r, dev,
                      "scene_call_separate", host.ws_hint)
    del alive
    n = int(r.n)
    coords4, index, ys = coords4[:n], index[:n], [y[:n] for y in ys]
    tail = (index, inverse) if return_inverse else (index,)
    view = lambda p, shape: _device_view(p, shape, torch.float32, dev, ws)
    fed = {} if predictions is None else dict(decode_prob=view(r.d_prob_in, (K, n)))
    dets = _finish_separate(host, r.scene, keep, categories, ys, n, dev, ws, coords4=coords4,
                            world_points=view(r.d_points, (n, 3)), **fed)
    if dets is not None:
        return (dets,) + tail
    pred = None
    if predictions is not None:
        pred = (view(r.d_xyz_in, (K, n, 3)), view(r.d_scale_in, (K, n, 3)), view(r.d_prob_in, (K, n)))
    return (detect_scene_separate_c(models, hv, coords4, view(r.d_feats, (n, d.front.in_channels)), res, predictions=pred,
                                    policy=policy, keep=keep, events=events, log_scale=log_scale,
                                    overlap_threshold=overlap_threshold, max_candidates=M, models_per_pass=models_per_pass,
                                    **decode_kw),) + tail


# ---- instance labels --------------------------------------------------------------------------------------------------------------

def _keep_begin(keep, res, categories=None):
    """What scene_instances needs beyond the call's results: the voxel size and, in separate mode, the category order.  The
    device views of an earlier call on the same dict are dropped: a scene that is redone call by call hands out none."""
    if keep is None:
        return
    for stale in ("grids", "net_pred", "decode_prob", "world_points"):
        keep.pop(stale, None)
    keep["res"] = float(res)
    if categories is not None:
        keep["categories"] = list(categories)


def _match_accepted(raw, box, used):
    """position among ``raw``'s accepted boxes of the first unused one whose corner array equals ``box`` exactly"""
    for i in range(len(raw["boxes"])):
        if i not in used and np.array_equal(raw["boxes"][i], box):
            used.add(i)
            return i
    raise ValueError("scene_instances: a detection's box is not among the accepted boxes of this scene's decode")


def scene_instances(keep, detections, scan_points=None, support="confident", prob_thresh=0.3, counts=False, inverse=None):
    """Which scan points each detection of a scene owns (decode.instance_labels on what ``keep`` holds).

    ``keep`` is the dict a one-call entry point filled (detect_scene_c, detect_scene_separate_c, detect_points_c,
    detect_points_separate_c), ``detections`` the list that call returned - or any list of its (class or category, box,
    score) entries.  ``scan_points`` [N,3]: the scene's world points; None takes the ones a raw-cloud call kept
    (``keep["scan_points"]``, ``keep["world_points"]`` from detect_points_separate_c).  Each detection is matched to the
    accepted box of the decode (``cand_idx[verdict == 0]``, acceptance order) whose corner array equals its own exactly -
    in separate mode among its category's - the first unused match taken; the box is then rebuilt from that grid cell as
    the decode built it, so membership is the decode's own in-box test (eval_joint.py:231-234) and, with
    ``support="confident"``, ``prob > prob_thresh`` (:245) on the prob the decode was fed (the call's ``predictions`` if it
    had any, else ``net_pred``); ``support="inside"`` takes every point inside.  Where boxes overlap, the point goes to the
    detection with the higher score, ties to the earlier one in ``detections``.  Labels are positions in ``detections``,
    -1 = no owner.

    Returns a dict: ``owner`` int32 [N] (joint mode) or [K,N] (separate mode, row k = category k's detections only, plus
    ``merged`` [N]: over all categories the best-scoring detection that has the point); with ``counts`` also ``count_in``
    / ``count_owned`` int32 [len(detections)] - points inside each detection's box under ``support``, owned or not, and
    points it owns within its category; with ``inverse`` [M] (``return_inverse`` of a raw-cloud call) also ``raw_owner``
    [M], the labels of the raw points: ``owner[inverse]`` (``merged[inverse]`` in separate mode).

    Everything is enqueued on the current stream, without a host wait.  ``keep``'s grids and predictions are VIEWS of the
    stream's scene scratch, which the next scene call on that stream overwrites: enqueue this call before it.  A scene
    that was redone call by call (a convolution input beyond the fp16 range, a decode walk beyond ``max_candidates``) has
    no grids in ``keep``: RuntimeError."""
    if keep is None or "grids" not in keep or "net_pred" not in keep or "raw" not in keep:
        raise RuntimeError("scene_instances: keep holds no grids - pass keep= to a one-call scene entry point; a scene that "
                           "was redone call by call (range fallback, truncated decode walk) hands none out")
    if "res" not in keep:
        raise RuntimeError("scene_instances: keep holds no res (it was not filled by a one-call scene entry point)")
    if scan_points is None:
        scan_points = keep.get("scan_points", keep.get("world_points"))
        if scan_points is None:
            raise RuntimeError("scene_instances: scan_points is needed (keep holds none: only the raw-cloud calls keep them)")
    separate = isinstance(keep["raw"], list)
    dets = list(detections)
    D = len(dets)
    # priority: score descending, ties to the earlier detection
    order = sorted(range(D), key=lambda p: (-float(dets[p][2]), p))
    rank = {p: i for i, p in enumerate(order)}
    raws = keep["raw"] if separate else [keep["raw"]]
    K = len(raws)
    accepted = [np.asarray(r["cand_idx"])[np.asarray(r["verdict"]) == 0] for r in raws]
    used = [set() for _ in range(K)]
    cat_of = [keep["categories"].index(d[0]) if separate else 0 for d in dets]
    cell_of = [int(accepted[cat_of[p]][_match_accepted(raws[cat_of[p]], np.asarray(dets[p][1], np.float32), used[cat_of[p]])])
               for p in range(D)]
    lists = [[p for p in order if cat_of[p] == k] for k in range(K)]
    cells = [[cell_of[p] for p in lst] for lst in lists]
    _, g_rot, g_scale = keep["grids"]
    prob = keep.get("decode_prob", keep["net_pred"][2])          # what the decode was fed: ``predictions=`` or the heads' own
    scan_points = scan_points.contiguous()
    args = (keep["corner"], keep["res"], scan_points)
    kw = dict(support=support, prob_thresh=prob_thresh, counts=counts)
    if separate:
        res_ = decode.instance_labels(g_rot, g_scale, *args, prob, cells, lists, **kw)
    else:
        res_ = decode.instance_labels(g_rot, g_scale, *args, prob, cells[0], lists[0], **kw)
    owner = res_[0] if counts else res_
    out = dict(owner=owner)
    dev = owner.device
    labels = owner
    if separate:
        # the best-ranked of a point's K owners (rank D: none)
        rank_of = torch.tensor([rank[p] for p in range(D)] + [D], dtype=torch.int64, device=dev)      # [-1] -> D
        best = rank_of[owner.long()].argmin(0, keepdim=True)
        out["merged"] = labels = owner.gather(0, best)[0]
    if counts:
        # list positions -> detection positions
        pos = torch.tensor([(cat_of[p], lists[cat_of[p]].index(p)) for p in range(D)], dtype=torch.int64, device=dev).reshape(D, 2)
        for name, c in (("count_in", res_[1]), ("count_owned", res_[2])):
            c = c if separate else c[None]
            out[name] = c[pos[:, 0], pos[:, 1]] if D else c.new_zeros(0)
    if inverse is not None:
        out["raw_owner"] = labels[inverse.long()]
    return out


def instances_report(detections, out):
    """One line per detection from scene_instances(..., counts=True): the scan points it owns and the ones inside its box
    (under the call's support), with ``inverse`` also the raw points it owns.  One host copy."""
    D = len(detections)
    cols = [out["count_owned"].cpu().numpy(), out["count_in"].cpu().numpy()]
    if "raw_owner" in out:
        r = out["raw_owner"]
        cols.append(torch.bincount(r[r >= 0].long(), minlength=D)[:D].cpu().numpy() if D else np.zeros(0, np.int64))
    lines = []
    for p, (c, _, score) in enumerate(detections):
        tail = "  raw points owned %7d" % cols[2][p] if len(cols) == 3 else ""
        lines.append("  det %3d  class %-10s score %.4f  owned %6d  members %6d%s" % (p, c, score, cols[0][p], cols[1][p], tail))
    return lines
