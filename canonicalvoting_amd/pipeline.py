"""The eval_joint.py per-scene path as functions: network -> head split -> vote -> decode -> NMS
(eval_joint.py:163-280), everything on the device, three host syncs per scene (coordinate-set
sizes, vote-grid shape, decode results)."""
import collections
import contextlib
import ctypes
import os

import torch

from . import _lib, decode, hv_cuda
from . import me as ME

vp = ctypes.c_void_p


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


def head_joint(out_feats, nclasses=9, log_scale=True):
    """eval_joint.py:173-190 in one kernel: -> xyz[N,3], scale[N,3], prob[N], class[N] (int32)."""
    L = _lib.lib()
    F = out_feats.contiguous()
    n, dev = F.shape[0], F.device
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((n, 3), dtype=torch.float32, device=dev)
    prob = torch.empty((n,), dtype=torch.float32, device=dev)
    cls = torch.empty((n,), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.cv_head_joint_f32(p(F), n, F.stride(0), nclasses, 1 if log_scale else 0, p(xyz), p(scale),
                                       p(prob), p(cls), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "cv_head_joint_f32")
    return xyz, scale, prob, cls


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


def head_separate(out_feats, log_scale=True):
    """eval_separate.py:170-181 in one kernel: -> xyz[N,3], scale[N,3], prob[N]."""
    L = _lib.lib()
    F = out_feats.contiguous()
    n, dev = F.shape[0], F.device
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((n, 3), dtype=torch.float32, device=dev)
    prob = torch.empty((n,), dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.cv_head_separate_f32(p(F), n, F.stride(0), 1 if log_scale else 0, p(xyz), p(scale), p(prob),
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "cv_head_separate_f32")
    return xyz, scale, prob


def detect_scene_separate(models, hv, coords4, feats, res, log_scale=True, overlap_threshold=0.3, **decode_kw):
    """eval_separate.py:162-264: one 8-channel model per category on the SAME SparseTensor (the
    coordinate sets, kernel maps and mask orders are built once and shared by all models - the
    reference rebuilds nothing either, but here it is one hash/map build per scene, not per model),
    vote + decode (eval_separate.py:209 elimination slice, float32 error threshold) and NMS per category.
    models: dict category -> MinkUNet34C(in, 8).  Returns [(category, box[8,3], score)]."""
    import numpy as np
    decode_kw.setdefault("separate_variant", True)
    decode_kw.setdefault("err_thresh", float(np.float32(0.3)))     # tensor > 0.3 compares in float32 (:252)
    out = []
    with torch.no_grad():
        x = ME.SparseTensor(feats, coords4, device=feats.device)
        scan_points = (coords4[:, 1:].to(feats.device) * res).float().contiguous()
        zeros_cls = torch.zeros(coords4.shape[0], dtype=torch.int32, device=feats.device)
        for category, model in models.items():
            xyz, scale, prob = head_separate(model(x).F, log_scale)
            grid_obj, grid_rot, grid_scale = hv(scan_points, xyz, scale, prob)
            raw = decode.decode_boxes(grid_obj, grid_rot, grid_scale, scan_points, xyz, prob, zeros_cls, res,
                                      **decode_kw)
            for i in decode.nms(raw["boxes"], raw["scores"], overlap_threshold):
                out.append((category, raw["boxes"][i], float(raw["scores"][i])))
    return out


def _separate_by_calls(hv, scan_points, xyz, scale, prob, res, categories, overlap_threshold=0.3, **decode_kw):
    """vote + decode + NMS of detect_scene_separate on given per-category predictions ([K,N,3], [K,N,3], [K,N])"""
    zeros_cls = torch.zeros(scan_points.shape[0], dtype=torch.int32, device=scan_points.device)
    out = []
    for k, category in enumerate(categories):
        with torch.no_grad():
            g = hv(scan_points, xyz[k].contiguous(), scale[k].contiguous(), prob[k].contiguous())
        raw = decode.decode_boxes(g[0], g[1], g[2], scan_points, xyz[k].contiguous(), prob[k].contiguous(), zeros_cls, res,
                                  **decode_kw)
        for i in decode.nms(raw["boxes"], raw["scores"], overlap_threshold):
            out.append((category, raw["boxes"][i], float(raw["scores"][i])))
    return out


def _fill_decode_params(p, decode_kw, separate_variant):
    """cv_decode_params from the keyword arguments of decode.decode_boxes (separate_variant: the caller's default)"""
    p.thresh_high = float(decode_kw.get("thresh_high", decode.thresh_high))
    p.thresh_low = float(decode_kw.get("thresh_low", decode.thresh_low))
    p.valid_ratio = float(decode_kw.get("valid_ratio", decode.valid_ratio))
    p.elimination = int(decode_kw.get("elimination", decode.elimination))
    p.prob_thresh = float(decode_kw.get("prob_thresh", 0.3))
    p.elim_hi_plus1 = 0 if decode_kw.get("separate_variant", separate_variant) else 1
    p.err_thresh = float(decode_kw.get("err_thresh", 0.3))


def _set_events(d, events):
    """five recorded torch.cuda.Event (their handles exist): scene start, after the network, the head split, the vote, the decode"""
    if events is not None:
        for i in range(5):
            d.events[i] = events[i].cuda_event


def _fill_scene_desc(d, model, hv, coords4, feats, scan_points, res, policy, pieces, max_channels, log_scale):
    """the fields cv_scene_desc and cv_scene_separate_desc share (model: the one, or the first of the K, that the plan follows)"""
    if coords4 is not None:          # (None: a raw-cloud call, which makes the scene's arrays itself)
        d.d_coords4, d.n, d.d_feats, d.feats_ld = vp(coords4.data_ptr()), coords4.shape[0], vp(feats.data_ptr()), feats.stride(0)
        d.d_points = vp(scan_points.data_ptr())
    d.res, d.num_rots = float(res), hv_cuda._scalar(hv.num_rots, "i")
    d.stem_k, d.mask_groups = model.conv0p1s1.kernel_size, ME.CoordinateManager.plan_mask_groups()
    d.masked_min_rows = policy.masked_min_rows if policy is not None else model.masked_min_rows()
    if policy is not None:
        d.conv_split_target, d.vote_part_records = int(policy.conv_split_target), int(policy.vote_part_records)
    d.max_channels, d.use_range_flag = max_channels, 1 if pieces == 2 else 0
    d.log_scale = 1 if log_scale else 0
    d.vote_algo = hv_cuda._algo


def _call_growing(fn, name, d, r, dev, scratch_name, ws_hint):
    """fn(d, r, stream) on a device scratch of at least ws_hint bytes; CV_ENOMEM: grow the scratch to result.needed_ws_bytes and
    run the scene again (four attempts).  Returns the scratch the results' device views point into."""
    need = max(ws_hint, 64 << 20)
    for attempt in range(4):
        ws = _lib.scratch(dev, scratch_name, need)
        d.d_ws, d.ws_bytes = vp(ws.data_ptr()), ws.numel()
        with torch.cuda.device(dev):
            rc = fn(ctypes.byref(d), ctypes.byref(r), vp(torch.cuda.current_stream(dev).cuda_stream))
        if rc != -12 or r.needed_ws_bytes <= ws.numel():
            break
        torch.cuda.current_stream(dev).synchronize()
        need = int(r.needed_ws_bytes)
    _lib.check(rc, name)          # (still CV_ENOMEM after four growing attempts: not an empty scene)
    return ws


_sep_hosts = {}
_model_tables = {}


def model_params_table(mods, dev, pieces):
    """Device table of cv_net_model_params [n_ops][K] for the model set ``mods`` (cv_net_run_models_f32: what differs between
    the K programs without a constant stride - packed weights, folded affine, acc_scale).  Cached per model set next to
    the programs it was filled from: a program that ``_program`` rebuilt (another parameter version) rebuilds the table.
    Returns (programs, table tensor)."""
    import numpy as np
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


def forward_models(mods, x, models_per_pass=None, range_flags=None):
    """The eval forward of K structurally identical models on ONE SparseTensor through cv_net_run_models_f32: passes of up
    to ``models_per_pass`` models (None: all K), every launch covering the pass's models.  Returns the K outputs [N, C] -
    bit for bit what ``m.program_forward(x)`` gives for each model.  ``range_flags``: optional zeroed int32 device tensor
    [K, 16]; word [k, 0] is set when model k saw an input beyond the fp16 range (nothing is redone here)."""
    L = _lib.lib()
    dev = x.F.device
    mods = list(mods)
    K = len(mods)
    G = K if not models_per_pass else min(int(models_per_pass), K)
    pieces = 1 if ME.COMPUTE_DTYPE == "bf16" else mods[0].PIECES
    progs, table = model_params_table(mods, dev, pieces)
    m0 = mods[0]
    plan = x.coordinate_manager.fused_fast(m0.conv0p1s1.kernel_size)
    n = plan.counts
    masked = [n[i] >= m0.masked_min_rows() for i in range(5)]
    if any(m and plan.perm_ptrs[i] is None for i, m in enumerate(masked)):
        raise ValueError("forward_models: the plan has no mask orders for a level that runs mask-sorted")
    perm_ptrs = [p if masked[i] else None for i, p in enumerate(plan.perm_ptrs[:5])] + plan.perm_ptrs[5:]
    map_ptrs = plan.map_ptrs
    feats = x.F.contiguous()
    ys = [torch.empty((n[0], m.final.out_channels), dtype=torch.float32, device=dev) for m in mods]
    rows = (ctypes.c_int64 * 5)(*n)
    c_bufs0 = progs[0][1]
    arena = _lib.scratch(dev, "net_arena_models", L.cv_net_models_arena_bytes(c_bufs0, len(c_bufs0), rows, 5, G))
    sorted_levels = (ctypes.c_int * 5)(*[p is not None for p in perm_ptrs[:5]])
    ws_one = L.cv_sp_scene_conv_workspace_bytes(rows, sorted_levels, m0.MASK_GROUPS, max(max(m.PLANES) for m in mods))
    ws = _lib.scratch(dev, "conv_ws_models", L.cv_net_models_workspace_bytes(ws_one, G))
    ext_ld = (ctypes.c_int * 2)(feats.stride(0), ys[0].stride(0))
    c_maps = (vp * len(map_ptrs))(*map_ptrs)
    c_perms = (vp * len(perm_ptrs))(*perm_ptrs)
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
            _lib.check(L.cv_net_run_models_f32(ops, bufs, n_ops, len(c_bufs0), g, rows, 5, vp(arena.data_ptr()), arena.numel(),
                                               c_ext, ext_ld, c_maps, len(map_ptrs), c_perms, len(perm_ptrs), vp(ws.data_ptr()),
                                               ws.numel(), flag, vp(table.data_ptr() + entry * k0), K,
                                               vp(torch.cuda.current_stream(dev).cuda_stream)), "cv_net_run_models_f32")
    return ys


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
    import numpy as np
    decode_kw.setdefault("separate_variant", True)
    decode_kw.setdefault("err_thresh", float(np.float32(0.3)))
    L = _lib.lib()
    dev = feats.device
    n = coords4.shape[0]
    categories = list(models.keys())
    mods = [models[c] for c in categories]
    K = len(mods)
    if not 1 <= K <= _lib.MAX_CATEGORIES:
        raise ValueError("detect_scene_separate_c: 1..%d models (got %d)" % (_lib.MAX_CATEGORIES, K))
    if scan_points is None:
        scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
    pieces = 1 if ME.COMPUTE_DTYPE == "bf16" else mods[0].PIECES
    G = int(models_per_pass or 0)
    if G < 0:
        raise ValueError("detect_scene_separate_c: models_per_pass must be >= 0 (got %d)" % G)
    if G > 0:
        progs, table = model_params_table(mods, dev, pieces)
    else:
        progs, table = [m._program(dev, pieces) for m in mods], None
    coords4 = coords4.to(device=dev, dtype=torch.int32).contiguous()
    feats = feats.contiguous()
    ys = [torch.empty((n, m.final.out_channels), dtype=torch.float32, device=dev) for m in mods]
    M = int(max_candidates)
    host = _sep_host(dev, K, M)
    d = _lib.SceneSeparateDesc()
    _fill_scene_desc(d, mods[0], hv, coords4, feats, scan_points, res, policy, pieces, max(max(m.PLANES) for m in mods), log_scale)
    if predictions is not None:
        px, ps, pp = [a.contiguous() for a in predictions]
        d.d_xyz_in, d.d_scale_in, d.d_prob_in = vp(px.data_ptr()), vp(ps.data_ptr()), vp(pp.data_ptr())
    alive = _fill_separate_desc(d, host, progs, table, G, ys, decode_kw, overlap_threshold, events)
    r = _lib.SceneSeparateResult()
    ws = _call_growing(L.cv_detect_scene_separate_f32, "cv_detect_scene_separate_f32", d, r, dev, "scene_call_separate",
                       host["ws_hint"])
    del alive
    host["ws_hint"] = max(host["ws_hint"], int(r.needed_ws_bytes))
    if keep is not None:
        keep.update(range_flag=int(r.range_flag), needed_ws_bytes=int(r.needed_ws_bytes))
    if r.range_flag or any(r.truncated[k] for k in range(K)):
        # rare: a convolution input beyond the fp16 range, or more candidate cells than the result arrays hold
        kw = dict(decode_kw, max_candidates=M)
        if predictions is None:
            return detect_scene_separate(models, hv, coords4, feats, res, log_scale=log_scale,
                                         overlap_threshold=overlap_threshold, **kw)
        return _separate_by_calls(hv, scan_points, predictions[0], predictions[1], predictions[2], res, categories,
                                  overlap_threshold, **kw)
    return _separate_results(host, r, keep, categories, ys, n, dev, ws)


def _sep_host(dev, K, M):
    """host-side scratch of the separate scene calls on the calling thread's current stream: pinned landing words, result arrays"""
    import numpy as np
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    with _scene_lock:
        host = _sep_hosts.get(key)
        if host is None or host["M"] < M or host["K"] < K:
            host = _sep_hosts[key] = dict(
                M=M, K=K, ws_hint=0, pinned=torch.empty(64 + 64 * _lib.MAX_CATEGORIES, dtype=torch.uint8).pin_memory(),
                cand=np.zeros((K, M), np.int64), verdict=np.zeros((K, M), np.int32), boxes=np.zeros((K, M, 8, 3), np.float32),
                scores=np.zeros((K, M), np.float32), det_cat=np.zeros(K * M, np.int32), det_box=np.zeros(K * M, np.int32))
    return host


def _fill_separate_desc(d, host, progs, table, G, ys, decode_kw, overlap_threshold, events):
    """cv_scene_separate_desc beyond _fill_scene_desc: the K programs and outputs, decode parameters, the host's landing arrays.
    Returns the pointer tables the descriptor refers to (keep them alive over the call)."""
    K = len(progs)
    d.num_models = K
    if G > 0:
        d.models_per_pass, d.d_model_params = G, vp(table.data_ptr())
    ops = (vp * K)(*[ctypes.cast(p[0], vp) for p in progs])
    n_ops = (ctypes.c_int * K)(*[len(p[0]) for p in progs])
    bufs = (vp * K)(*[ctypes.cast(p[1], vp) for p in progs])
    n_bufs = (ctypes.c_int * K)(*[len(p[1]) for p in progs])
    outs = (vp * K)(*[y.data_ptr() for y in ys])
    d.ops, d.n_ops, d.bufs, d.n_bufs = ctypes.cast(ops, vp), ctypes.cast(n_ops, vp), ctypes.cast(bufs, vp), ctypes.cast(n_bufs, vp)
    d.d_out_feats, d.out_ld, d.out_channels = ctypes.cast(outs, vp), ys[0].stride(0), ys[0].shape[1]
    _fill_decode_params(d.decode, decode_kw, True)
    d.max_candidates, d.nms_threshold = host["M"], float(overlap_threshold)
    _set_events(d, events)
    d.h_pinned, d.pinned_bytes = vp(host["pinned"].data_ptr()), host["pinned"].numel()
    d.h_cand_idx, d.h_verdict = vp(host["cand"].ctypes.data), vp(host["verdict"].ctypes.data)
    d.h_boxes, d.h_scores = vp(host["boxes"].ctypes.data), vp(host["scores"].ctypes.data)
    d.h_det_cat, d.h_det_box = vp(host["det_cat"].ctypes.data), vp(host["det_box"].ctypes.data)
    return ops, n_ops, bufs, n_bufs, outs


def _separate_results(host, r, keep, categories, ys, n, dev, ws):
    """detections of a finished cv_scene_separate_result; ``keep`` (optional) receives the per-category raw decode and the device views"""
    K = len(categories)
    dets = [(categories[int(c)], host["boxes"][int(c), int(b)].copy(), float(host["scores"][int(c), int(b)]))
            for c, b in zip(host["det_cat"][:r.n_det], host["det_box"][:r.n_det])]
    if keep is not None:
        X, Y, Z = r.dims
        view = lambda ptr, shape: _device_view(ptr, shape, torch.float32, dev, ws)
        raw = [dict(boxes=host["boxes"][k, :r.n_boxes[k]].copy(), scores=host["scores"][k, :r.n_boxes[k]].copy(),
                    cand_idx=host["cand"][k, :r.n_cand[k]].copy(), verdict=host["verdict"][k, :r.n_cand[k]].copy())
               for k in range(K)]
        keep.update(y=ys, dims=(X, Y, Z), corner=tuple(r.corner), level_rows=list(r.level_rows), raw=raw,
                    grids=(view(r.d_grid_obj, (K, X, Y, Z)), view(r.d_grid_rot, (K, X, Y, Z, 2)),
                           view(r.d_grid_scale, (K, X, Y, Z, 3))),
                    net_pred=(view(r.d_xyz, (K, n, 3)), view(r.d_scale, (K, n, 3)), view(r.d_prob, (K, n))),
                    host_us=tuple(r.host_us))
    return dets


class _SceneHost:
    """per-(device, stream) host-side scratch of detect_scene_c: pinned landing words and the result arrays"""

    def __init__(self, max_candidates):
        import numpy as np
        self.M = max_candidates
        self.pinned = torch.empty(256, dtype=torch.uint8).pin_memory()
        self.cand = np.zeros(max_candidates, np.int64)
        self.verdict = np.zeros(max_candidates, np.int32)
        self.boxes = np.zeros((max_candidates, 8, 3), np.float32)
        self.scores = np.zeros(max_candidates, np.float32)
        self.classes = np.zeros(max_candidates, np.int32)
        self.pick = np.zeros(max_candidates, np.int32)
        self.ws_hint = 0
        self.last_host_us = (0.0, 0.0, 0.0, 0.0)


_scene_hosts = {}
_scene_lock = __import__("threading").Lock()


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
    import numpy as np
    L = _lib.lib()
    dev = feats.device
    n = coords4.shape[0]
    if scan_points is None:
        scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
    pieces = 1 if ME.COMPUTE_DTYPE == "bf16" else model.PIECES
    c_ops, c_bufs, _ = model._program(dev, pieces)
    coords4 = coords4.to(device=dev, dtype=torch.int32).contiguous()
    feats = feats.contiguous()
    y = torch.empty((n, model.final.out_channels), dtype=torch.float32, device=dev)
    host = _scene_host(dev, max_candidates)
    d = _lib.SceneDesc()
    _fill_scene_desc(d, model, hv, coords4, feats, scan_points, res, policy, pieces, max(model.PLANES), log_scale)
    if predictions is not None:
        px, ps, pp, pc = predictions
        pc = pc.to(torch.int32).contiguous()
        d.d_xyz_in, d.d_scale_in, d.d_prob_in, d.d_class_in = (vp(px.data_ptr()), vp(ps.data_ptr()), vp(pp.data_ptr()),
                                                                 vp(pc.data_ptr()))
    _fill_joint_desc(d, host, c_ops, c_bufs, y, nclasses, decode_kw, adaptive_split, events)
    d.peak_quotients = 1 if keep is None else 0      # nobody sees the grids without ``keep``: rot / scale only where the decode reads them
    r = _lib.SceneResult()
    ws = _call_growing(L.cv_detect_scene_f32, "cv_detect_scene_f32", d, r, dev, "scene_call", host.ws_hint)
    host.ws_hint = max(host.ws_hint, int(r.needed_ws_bytes))
    host.last_host_us = tuple(r.host_us)            # where the call's host time went (plan + wait, network enqueue, head + vote, decode + wait)
    if r.range_flag or r.truncated:
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
    dets, raw = _joint_results(host, r, keep, y, n, dev, ws)
    return dets, raw, y


def _scene_host(dev, max_candidates):
    """the _SceneHost of the calling thread's current stream (one per (device, stream); regrown for more candidates)"""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    with _scene_lock:
        host = _scene_hosts.get(key)
        if host is None or host.M < max_candidates:
            host = _scene_hosts[key] = _SceneHost(max_candidates)
    return host


def _fill_joint_desc(d, host, c_ops, c_bufs, y, nclasses, decode_kw, adaptive_split, events):
    """cv_scene_desc beyond _fill_scene_desc: program, output, decode parameters, the host's landing arrays"""
    d.ops, d.n_ops, d.bufs, d.n_bufs = ctypes.cast(c_ops, vp), len(c_ops), ctypes.cast(c_bufs, vp), len(c_bufs)
    d.d_out_feats, d.out_ld, d.out_channels = vp(y.data_ptr()), y.stride(0), y.shape[1]
    d.nclasses = nclasses
    _fill_decode_params(d.decode, decode_kw, False)
    d.max_candidates, d.nms_threshold = host.M, 0.3
    d.adaptive_split = 1 if adaptive_split else 0
    _set_events(d, events)
    d.h_pinned, d.pinned_bytes = vp(host.pinned.data_ptr()), host.pinned.numel()
    d.h_cand_idx, d.h_verdict = vp(host.cand.ctypes.data), vp(host.verdict.ctypes.data)
    d.h_boxes, d.h_scores, d.h_classes, d.h_pick = (vp(host.boxes.ctypes.data), vp(host.scores.ctypes.data),
                                                    vp(host.classes.ctypes.data), vp(host.pick.ctypes.data))


def _joint_results(host, r, keep, y, n, dev, ws):
    """(detections, raw decode dict) of a finished cv_scene_result; ``keep`` (optional) receives the device views"""
    k, m = r.n_boxes, r.n_cand
    raw = dict(boxes=host.boxes[:k].copy(), scores=host.scores[:k].copy(), classes=host.classes[:k].copy(),
               cand_idx=host.cand[:m].copy(), verdict=host.verdict[:m].copy(), truncated=False)
    dets = [(int(raw["classes"][i]), raw["boxes"][i], float(raw["scores"][i])) for i in host.pick[:r.n_det]]
    if keep is not None:
        view = lambda ptr, shape, dt=torch.float32: _device_view(ptr, shape, dt, dev, ws)
        X, Y, Z = r.dims
        keep.update(y=y, dims=(X, Y, Z), corner=tuple(r.corner), level_rows=list(r.level_rows),
                    grids=(view(r.d_grid_obj, (X, Y, Z)), view(r.d_grid_rot, (X, Y, Z, 2)), view(r.d_grid_scale, (X, Y, Z, 3))),
                    net_pred=(view(r.d_xyz, (n, 3)), view(r.d_scale, (n, 3)), view(r.d_prob, (n,)),
                              view(r.d_class, (n,), torch.int32)), raw=raw)
    return dets, raw


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


def _points_front(front, points, feats, in_channels, recentre_from, predictions, return_inverse, with_class):
    """cv_points_front of a raw cloud; returns (coords4 [M, 4], index [M], inverse [M] or None, the tensors to keep alive)"""
    dev = points.device
    assert points.is_cuda and points.dim() == 2 and points.shape[1] == 3, "points: a [M, 3] device tensor"
    if points.dtype not in (torch.float32, torch.float64):      # (as ME.utils.quantize_device: computed in fp64, as numpy promotes them)
        points = points.to(torch.float64)
    if points.stride(1) != 1 or points.stride(0) < 3:
        points = points.contiguous()
    m = points.shape[0]
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
    front.d_raw_points, front.m, front.points_ld = vp(points.data_ptr()), m, points.stride(0)
    front.points_f64 = 1 if points.dtype == torch.float64 else 0
    front.d_raw_feats, front.raw_feats_ld, front.in_channels = vp(feats.data_ptr()), feats.stride(0), in_channels
    front.recentre_from = -1 if recentre_from is None else int(recentre_from)
    front.d_coords4, front.d_index = vp(coords4.data_ptr()), vp(index.data_ptr())
    front.d_inverse = vp(inverse.data_ptr()) if return_inverse else None
    alive = [points, feats]
    if predictions is not None:
        pred = [p.to(dev).contiguous() for p in predictions]
        if with_class:
            pred[3] = pred[3].to(torch.int32).contiguous()
            front.d_raw_class = vp(pred[3].data_ptr())
        front.d_raw_xyz, front.d_raw_scale, front.d_raw_prob = vp(pred[0].data_ptr()), vp(pred[1].data_ptr()), vp(pred[2].data_ptr())
        alive += pred
    return coords4, index, inverse, alive


def _call_points(fn, name, d, r, dev, scratch_name, ws_hint):
    """_call_growing for a raw-cloud descriptor (the scratch and its size live in the embedded scene descriptor / result); a
    rejected cloud raises RuntimeError with the count, as ME.utils.quantize_device does"""
    call = lambda _d, _r, stream: fn(ctypes.byref(d), ctypes.byref(r), stream)
    try:
        return _call_growing(call, name, d.scene, r.scene, dev, scratch_name, ws_hint)
    except _lib.CvError:
        if r.rejected:
            ME.utils.raise_rejected(r.rejected)
        raise


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
    L = _lib.lib()
    dev = points.device
    pieces = 1 if ME.COMPUTE_DTYPE == "bf16" else model.PIECES
    c_ops, c_bufs, _ = model._program(dev, pieces)
    d, r = _lib.PointsDesc(), _lib.PointsResult()
    coords4, index, inverse, alive = _points_front(d.front, points, feats, feats.shape[1], recentre_from, predictions,
                                                   return_inverse, True)
    d.front.quantization_size = float(res)
    y = torch.empty((coords4.shape[0], model.final.out_channels), dtype=torch.float32, device=dev)
    host = _scene_host(dev, max_candidates)
    _fill_scene_desc(d.scene, model, hv, None, None, None, res, policy, pieces, max(model.PLANES), log_scale)
    _fill_joint_desc(d.scene, host, c_ops, c_bufs, y, nclasses, decode_kw, adaptive_split, events)
    d.scene.peak_quotients = 1 if keep is None else 0      # (as detect_scene_c)
    ws = _call_points(L.cv_detect_points_f32, "cv_detect_points_f32", d, r, dev, "scene_call", host.ws_hint)
    del alive
    n = int(r.n)
    host.ws_hint = max(host.ws_hint, int(r.scene.needed_ws_bytes))
    host.last_host_us = tuple(r.scene.host_us)
    coords4, index, y = coords4[:n], index[:n], y[:n]
    tail = (index, inverse) if return_inverse else (index,)
    view = lambda ptr, shape, dt=torch.float32: _device_view(ptr, shape, dt, dev, ws)
    if r.scene.range_flag or r.scene.truncated:
        pred = None
        if predictions is not None:
            pred = (view(r.d_xyz_in, (n, 3)), view(r.d_scale_in, (n, 3)), view(r.d_prob_in, (n,)), view(r.d_class_in, (n,), torch.int32))
        return detect_scene_c(model, hv, coords4, view(r.d_feats, (n, d.front.in_channels)), res, nclasses=nclasses,
                              log_scale=log_scale, predictions=pred, max_candidates=max_candidates, keep=keep, events=events,
                              adaptive_split=adaptive_split, policy=policy, **decode_kw) + tail
    if keep is not None:
        keep.update(scan_points=view(r.d_points, (n, 3)), feats=view(r.d_feats, (n, d.front.in_channels)),
                    host_us=tuple(r.scene.host_us), host_us_front=float(r.host_us_front), front_ws_bytes=int(r.front_ws_bytes))
    dets, raw = _joint_results(host, r.scene, keep, y, n, dev, ws)
    return (dets, raw, y) + tail


def detect_points_separate_c(models, hv, points, feats, res, predictions=None, models_per_pass=None, return_inverse=False,
                             recentre_from=None, policy=None, keep=None, events=None, log_scale=True, overlap_threshold=0.3,
                             max_candidates=512, **decode_kw):
    """detect_scene_separate_c from a RAW device cloud through ONE C call (cv_detect_points_separate_f32): voxelise, gather,
    then the K models' scene.  ``predictions`` = (xyz [K, M, 3], scale [K, M, 3], prob [K, M]) aligned with the raw points; the
    other arguments as detect_points_c / detect_scene_separate_c.  The same bits as ME.utils.quantize_device + torch gathers
    + detect_scene_separate_c.  Returns (detections [(category, box[8,3], score)], index [N][, inverse [M]]); ``keep``
    receives what detect_scene_separate_c's does (``y``: the K outputs' first N rows) plus ``coords4``."""
    import numpy as np
    decode_kw.setdefault("separate_variant", True)
    decode_kw.setdefault("err_thresh", float(np.float32(0.3)))
    L = _lib.lib()
    dev = points.device
    categories = list(models.keys())
    mods = [models[c] for c in categories]
    K = len(mods)
    if not 1 <= K <= _lib.MAX_CATEGORIES:
        raise ValueError("detect_points_separate_c: 1..%d models (got %d)" % (_lib.MAX_CATEGORIES, K))
    pieces = 1 if ME.COMPUTE_DTYPE == "bf16" else mods[0].PIECES
    G = int(models_per_pass or 0)
    if G < 0:
        raise ValueError("detect_points_separate_c: models_per_pass must be >= 0 (got %d)" % G)
    if G > 0:
        progs, table = model_params_table(mods, dev, pieces)
    else:
        progs, table = [m._program(dev, pieces) for m in mods], None
    d, r = _lib.PointsSeparateDesc(), _lib.PointsSeparateResult()
    coords4, index, inverse, alive = _points_front(d.front, points, feats, feats.shape[1], recentre_from, predictions,
                                                   return_inverse, False)
    d.front.quantization_size = float(res)
    m = coords4.shape[0]
    ys = [torch.empty((m, mod.final.out_channels), dtype=torch.float32, device=dev) for mod in mods]
    M = int(max_candidates)
    host = _sep_host(dev, K, M)
    _fill_scene_desc(d.scene, mods[0], hv, None, None, None, res, policy, pieces, max(max(mod.PLANES) for mod in mods), log_scale)
    alive.append(_fill_separate_desc(d.scene, host, progs, table, G, ys, decode_kw, overlap_threshold, events))
    ws = _call_points(L.cv_detect_points_separate_f32, "cv_detect_points_separate_f32", d, r, dev, "scene_call_separate",
                      host["ws_hint"])
    del alive
    n = int(r.n)
    host["ws_hint"] = max(host["ws_hint"], int(r.scene.needed_ws_bytes))
    coords4, index, ys = coords4[:n], index[:n], [y[:n] for y in ys]
    tail = (index, inverse) if return_inverse else (index,)
    if keep is not None:
        keep.update(range_flag=int(r.scene.range_flag), needed_ws_bytes=int(r.scene.needed_ws_bytes), coords4=coords4)
    if r.scene.range_flag or any(r.scene.truncated[k] for k in range(K)):
        view = lambda ptr, shape: _device_view(ptr, shape, torch.float32, dev, ws)
        pred = None
        if predictions is not None:
            pred = (view(r.d_xyz_in, (K, n, 3)), view(r.d_scale_in, (K, n, 3)), view(r.d_prob_in, (K, n)))
        return (detect_scene_separate_c(models, hv, coords4, view(r.d_feats, (n, d.front.in_channels)), res, predictions=pred,
                                        policy=policy, keep=keep, events=events, log_scale=log_scale,
                                        overlap_threshold=overlap_threshold, max_candidates=M, models_per_pass=models_per_pass,
                                        **decode_kw),) + tail
    return (_separate_results(host, r.scene, keep, categories, ys, n, dev, ws),) + tail


def last_scene_host_us(dev=None):
    """(plan + wait, network enqueue, head + vote enqueue, decode + wait) host microseconds of the calling thread's last
    detect_scene_c call on its current stream"""
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    host = _scene_hosts.get((dev.index, torch.cuda.current_stream(dev).cuda_stream))
    return host.last_host_us if host is not None else None


def _device_view(ptr, shape, dtype, dev, owner):
    """tensor view of a region of the scene scratch (valid until the next scene call on the same stream)"""
    import numpy as np
    count = int(np.prod(shape))
    off = int(ptr) - owner.data_ptr()
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    assert 0 <= off and off + nbytes <= owner.numel()
    return owner[off:off + nbytes].view(dtype).view(*shape).clone()
