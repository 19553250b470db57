"""Detection decode: the reference's inline loop as one function.

``decode_boxes`` is eval_joint.py:195-263 (greedy peak picking, grid suppression,
back-projection check, class vote) and ``decode_boxes_categories`` the same over K separate-mode
categories with one host sync: two thin wrappers, each through its own C entry point, around one
walk (``_walk``); ``nms`` / ``get_iou_obb`` are eval_joint.py:75-89 and
utils/calc_map.py:6-21; ``detect`` chains vote -> decode -> per-class NMS the way
eval_joint.py:193-280 does.  Module-level constants keep the reference's names and values
(eval_joint.py:18-21).
"""
import ctypes

import numpy as np
import torch

from . import _lib, hv_cuda
from ._lib import ptr, stream

thresh_high = 60
thresh_low = 10
valid_ratio = 0.2
elimination = 2


def _walk(K, grid_obj, grid_rot, grid_scale, scan_points, xyz_pred, prob_pred, class_pred, res, corner, params, mutate_grid,
          allow_truncation):
    """The decode behind decode_boxes (K None: cv_decode_f32) and decode_boxes_categories (cv_decode_cat_f32 over K
    categories): operand checks, grid origin, the walk - redone with eight times the room while it stops early with a cell
    >= thresh_high still live - and the results, one dict per category.  ``params``: cv_decode_params, max_iters = the first
    capacity."""
    who = "decode_boxes" if K is None else "decode_boxes_categories"
    L = _lib.lib()
    dev = grid_obj.device
    for t, name in ((grid_obj, "grid_obj"), (grid_rot, "grid_rot"), (grid_scale, "grid_scale"),
                    (scan_points, "scan_points"), (xyz_pred, "xyz_pred"), (prob_pred, "prob_pred")):
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
            raise RuntimeError("%s must be a contiguous float32 CUDA tensor" % name)
    n = scan_points.shape[0]
    if K is not None and (grid_obj.dim() != 4 or tuple(xyz_pred.shape) != (K, n, 3) or tuple(prob_pred.shape) != (K, n)):
        raise RuntimeError("expected grid_obj [K,X,Y,Z], xyz_pred [K,N,3] and prob_pred [K,N]")
    # (class_pred None - class 0 everywhere - is the category call's alone)
    cls = None if (class_pred is None and K is not None) else class_pred.to(torch.int32).contiguous()
    if corner is None:
        corner = hv_cuda.recent_corner(grid_obj)            # set by hv_cuda.forward / forward_categories (same points)
    if corner is None:
        corner, _, _ = hv_cuda.grid_geometry(scan_points, float(res))
    dims = (ctypes.c_int * 3)(*(grid_obj.shape if K is None else grid_obj.shape[1:]))
    rows = 1 if K is None else K
    if K is None:
        fn, name, cat, ws_bytes = L.cv_decode_f32, "cv_decode_f32", (), lambda M: L.cv_decode_workspace_bytes(dims, n, M)
    else:
        fn, name, cat, ws_bytes = L.cv_decode_cat_f32, "cv_decode_cat_f32", (K,), lambda M: L.cv_decode_cat_workspace_bytes(dims, n, M, K)
    M = params.max_iters
    while True:
        params.max_iters = M
        ws = _lib.scratch(dev, "decode", ws_bytes(M))
        n_cand, n_boxes, truncated = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.int32)
        cand = np.zeros((rows, M), np.int64)
        verdict = np.zeros((rows, M), np.int32)
        boxes = np.zeros((rows, M, 8, 3), np.float32)
        scores = np.zeros((rows, M), np.float32)
        classes = np.zeros((rows, M), np.int32)
        with torch.cuda.device(dev):
            rc = fn(ptr(grid_obj), ptr(grid_rot), ptr(grid_scale), dims,
                    (ctypes.c_float * 3)(*[float(v) for v in corner]), ctypes.c_float(float(res)),
                    ptr(scan_points), ptr(xyz_pred), ptr(prob_pred), ptr(cls), n, *cat, ctypes.byref(params),
                    1 if mutate_grid else 0, ptr(ws), ws.numel(), n_cand.ctypes.data_as(_lib.c_int_p),
                    cand.ctypes.data_as(_lib.c_i64_p), verdict.ctypes.data_as(_lib.c_i32_p),
                    n_boxes.ctypes.data_as(_lib.c_int_p), boxes.ctypes.data_as(_lib.c_float_p),
                    scores.ctypes.data_as(_lib.c_float_p), classes.ctypes.data_as(_lib.c_i32_p),
                    truncated.ctypes.data_as(_lib.c_int_p), stream(dev))
        _lib.check(rc, name)
        if not truncated.any() or allow_truncation:
            break
        # the reference's `while True` (eval_joint.py:204-209) runs until the grid maximum drops below thresh_high:
        # a capped walk that stopped early is redone with more room, never returned as if it were complete
        if M >= 65536 or mutate_grid:
            raise RuntimeError("%s: more than %d candidate cells >= thresh_high (max_candidates)" % (who, M))
        M = min(M * 8, 65536)
    out = []
    for k in range(rows):
        b, m = int(n_boxes[k]), int(n_cand[k])
        out.append(dict(boxes=boxes[k, :b].copy(), scores=scores[k, :b].copy(), classes=classes[k, :b].copy(),
                        cand_idx=cand[k, :m].copy(), verdict=verdict[k, :m].copy(), truncated=bool(truncated[k])))
    return out


def _params(thresh_high, thresh_low, valid_ratio, elimination, prob_thresh, separate_variant, max_candidates, err_thresh):
    return _lib.DecodeParams(float(thresh_high), float(thresh_low), float(valid_ratio), int(elimination), float(prob_thresh),
                             0 if separate_variant else 1, int(max_candidates), float(err_thresh))


def decode_boxes(grid_obj, grid_rot, grid_scale, scan_points, xyz_pred, prob_pred, class_pred, res,
                 corner=None, thresh_high=thresh_high, thresh_low=thresh_low,
                 valid_ratio=valid_ratio, elimination=elimination, prob_thresh=0.3, err_thresh=0.3,
                 separate_variant=False, max_candidates=512, mutate_grid=False, allow_truncation=False):
    """Greedy decode on the device, one host sync (cv_decode_f32).

    scan_points [N,3] f32 world points (``curr_points * res``, eval_joint.py:200), ``corner``
    defaults to their minimum (``corners[0]``, :201).  Returns a dict with ``boxes`` [K,8,3],
    ``scores`` [K], ``classes`` [K] (numpy, acceptance order) plus the examined candidate cells
    and verdicts (0 accepted, 1 too few confident points :246-247, 2 LCC error :252-253).
    ``separate_variant`` selects eval_separate.py:209's elimination slice (no ``+1``).
    ``max_candidates`` is the first capacity of the walk, not a limit on the result: the reference's ``while True``
    (:204-209) runs until the grid maximum drops below ``thresh_high``, so a walk that fills its capacity with a cell
    >= thresh_high still live is redone with eight times the room (up to 65536, then RuntimeError).
    ``allow_truncation=True`` returns the capped walk instead, marked ``truncated=True`` in the dict."""
    p = _params(thresh_high, thresh_low, valid_ratio, elimination, prob_thresh, separate_variant, max_candidates, err_thresh)
    return _walk(None, grid_obj, grid_rot, grid_scale, scan_points, xyz_pred, prob_pred, class_pred, res, corner, p,
                 mutate_grid, allow_truncation)[0]


def decode_boxes_categories(grid_obj, grid_rot, grid_scale, scan_points, xyz_pred, prob_pred, res, class_pred=None,
                            corner=None, thresh_high=thresh_high, thresh_low=thresh_low, valid_ratio=valid_ratio,
                            elimination=elimination, prob_thresh=0.3, err_thresh=0.3, separate_variant=False,
                            max_candidates=512, mutate_grid=False, allow_truncation=False):
    """decode_boxes over K categories with ONE host sync (cv_decode_cat_f32): grids [K,X,Y,Z] (+[2], [3]) as
    hv_cuda.forward_categories returns them, xyz_pred [K,N,3], prob_pred [K,N], scan_points [N,3]; ``class_pred`` [N]
    shared by the categories, None = class 0 everywhere (separate mode, eval_separate.py:195-264).  Returns a list of K
    dicts, entry k exactly what decode_boxes returns for category k alone (same keys, same truncation rule: a walk that
    fills ``max_candidates`` with a live cell >= thresh_high is redone with eight times the room)."""
    p = _params(thresh_high, thresh_low, valid_ratio, elimination, prob_thresh, separate_variant, max_candidates, err_thresh)
    return _walk(grid_obj.shape[0], grid_obj, grid_rot, grid_scale, scan_points, xyz_pred, prob_pred, class_pred, res, corner,
                 p, mutate_grid, allow_truncation)


def decode_boxes_scenes(grids, corners, row_ranges, scan_points, xyz_pred, prob_pred, class_pred, res,
                        thresh_high=thresh_high, thresh_low=thresh_low, valid_ratio=valid_ratio, elimination=elimination,
                        prob_thresh=0.3, err_thresh=0.3, separate_variant=False, max_candidates=512, mutate_grid=False):
    """decode_boxes over B scenes with ONE host sync (cv_decode_scenes_f32).  ``grids``: B triples (grid_obj [X,Y,Z],
    grid_rot [X,Y,Z,2], grid_scale [X,Y,Z,3]) of any shapes, ``corners``: B grid origins, ``row_ranges``: B (first, end) row
    ranges of the shared scan_points / xyz_pred [N,3], prob_pred / class_pred [N].  ``corners`` None: the origins that
    hv_cuda.forward_scenes (or forward) remembered on the grids it returned.  Returns a list of B dicts, entry b exactly
    what ``decode_boxes(..., allow_truncation=True)`` returns for scene b's grids and rows alone: a walk that fills
    ``max_candidates`` comes back capped and marked ``truncated`` (the caller redoes that scene)."""
    L = _lib.lib()
    B = len(grids)
    dev = scan_points.device
    for t, name in [(scan_points, "scan_points"), (xyz_pred, "xyz_pred"), (prob_pred, "prob_pred")] + [
            (g, "grids[%d][%d]" % (b, i)) for b, tri in enumerate(grids) for i, g in enumerate(tri)]:
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32:
            raise RuntimeError("%s must be a contiguous float32 CUDA tensor" % name)
    if corners is None:
        corners = [hv_cuda.recent_corner(tri[0]) for tri in grids]
        if any(c is None for c in corners):
            raise RuntimeError("decode_boxes_scenes: corners=None needs grids returned by hv_cuda.forward_scenes / forward")
    if not (len(corners) == B and len(row_ranges) == B):
        raise RuntimeError("decode_boxes_scenes: one corner and one row range per grid triple")
    cls = class_pred.to(torch.int32).contiguous()
    p = _params(thresh_high, thresh_low, valid_ratio, elimination, prob_thresh, separate_variant, max_candidates, err_thresh)
    M = p.max_iters
    jobs = (_lib.DecodeSceneJob * max(B, 1))()
    for b in range(B):
        j = jobs[b]
        j.d_grid_obj, j.d_grid_rot, j.d_grid_scale = (ptr(g) for g in grids[b])
        j.dims = (ctypes.c_int * 3)(*grids[b][0].shape)
        j.corner = (ctypes.c_float * 3)(*[float(v) for v in corners[b]])
        j.row0, j.n = int(row_ranges[b][0]), int(row_ranges[b][1]) - int(row_ranges[b][0])
        if not 0 <= j.row0 <= j.row0 + j.n <= scan_points.shape[0]:
            raise RuntimeError("decode_boxes_scenes: row range %d leaves the shared arrays" % b)
    rows = max(B, 1)
    ws = _lib.scratch(dev, "decode", max(L.cv_decode_scenes_workspace_bytes(jobs, B, M), 256))
    n_cand, n_boxes, truncated = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    cand = np.zeros((rows, M), np.int64)
    verdict = np.zeros((rows, M), np.int32)
    boxes = np.zeros((rows, M, 8, 3), np.float32)
    scores = np.zeros((rows, M), np.float32)
    classes = np.zeros((rows, M), np.int32)
    with torch.cuda.device(dev):
        rc = L.cv_decode_scenes_f32(jobs, B, ctypes.c_float(float(res)), ptr(scan_points), ptr(xyz_pred), ptr(prob_pred), ptr(cls),
                                    ctypes.byref(p), 1 if mutate_grid else 0, ptr(ws), ws.numel(),
                                    n_cand.ctypes.data_as(_lib.c_int_p), cand.ctypes.data_as(_lib.c_i64_p),
                                    verdict.ctypes.data_as(_lib.c_i32_p), n_boxes.ctypes.data_as(_lib.c_int_p),
                                    boxes.ctypes.data_as(_lib.c_float_p), scores.ctypes.data_as(_lib.c_float_p),
                                    classes.ctypes.data_as(_lib.c_i32_p), truncated.ctypes.data_as(_lib.c_int_p), stream(dev))
    _lib.check(rc, "cv_decode_scenes_f32")
    return [dict(boxes=boxes[b, :n_boxes[b]].copy(), scores=scores[b, :n_boxes[b]].copy(), classes=classes[b, :n_boxes[b]].copy(),
                 cand_idx=cand[b, :n_cand[b]].copy(), verdict=verdict[b, :n_cand[b]].copy(), truncated=bool(truncated[b]))
            for b in range(B)]


SUPPORT = {"confident": 1, "inside": 0}      # instance_labels' ``support`` -> cv_decode_instances_f32's confident_only


def instance_labels(grid_rot, grid_scale, corner, res, scan_points, prob, cells, label_of=None, support="confident",
                    prob_thresh=0.3, counts=False):
    """Which scan points each of a list of boxes owns (cv_decode_instances_f32; two launches, no host wait).

    A box is the grid cell the decode examined as a candidate (``raw["cand_idx"]``); its geometry is formed from
    ``grid_rot`` / ``grid_scale`` / ``corner`` / ``res`` exactly as the decode formed it, so membership is the decode's
    own in-box test (eval_joint.py:231-234), with ``support="confident"`` also ``prob > prob_thresh`` (:245);
    ``support="inside"`` takes every point inside the box (``prob`` may then be None).  A point's owner is the FIRST box of
    ``cells`` that has it as a member: order the list by priority.

    Single form: grids [X,Y,Z,2] / [X,Y,Z,3], prob [N], ``cells`` a sequence of B cells -> owner [N] int32.
    Category form: grids [K,X,Y,Z,2|3], prob [K,N], ``cells`` a list of K sequences -> owner [K,N].  scan_points [N,3] is
    shared.  ``label_of`` (same shape as ``cells``; default: the box's position in its list) is what ``owner`` holds for an
    owned point, -1 for a point no box has.  ``counts=True`` also returns (count_in, count_owned), int32 [B] or [K,max B]:
    members of each box, owned or not, and points it owns."""
    L = _lib.lib()
    if support not in SUPPORT:
        raise ValueError("instance_labels: support must be 'confident' or 'inside' (got %r)" % (support,))
    confident = SUPPORT[support]
    single = grid_rot.dim() == 4
    if prob is None and confident:
        raise ValueError("instance_labels: support='confident' needs prob")
    for t, name in ((grid_rot, "grid_rot"), (grid_scale, "grid_scale"), (scan_points, "scan_points"), (prob, "prob")):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32):
            raise RuntimeError("%s must be a contiguous float32 CUDA tensor" % name)
    dev = scan_points.device
    n = scan_points.shape[0]
    cells = [cells] if single else list(cells)
    label_of = None if label_of is None else ([label_of] if single else list(label_of))
    K = len(cells)
    shape = tuple(grid_rot.shape[:-1] if single else grid_rot.shape[1:-1])
    if (len(shape) != 3 or tuple(grid_rot.shape) != (() if single else (K,)) + shape + (2,)
            or tuple(grid_scale.shape) != (() if single else (K,)) + shape + (3,)
            or (prob is not None and tuple(prob.shape) != ((n,) if single else (K, n)))):
        raise RuntimeError("instance_labels: expected grid_rot [K,X,Y,Z,2], grid_scale [K,X,Y,Z,3] and prob [K,N] for the K "
                           "cell lists (without K for one list)")
    n_boxes = np.array([len(c) for c in cells], np.int32)
    B = int(n_boxes.max()) if K else 0
    h_cells = np.zeros((K, max(B, 1)), np.int64)
    h_label = np.zeros((K, max(B, 1)), np.int32)
    for k in range(K):
        h_cells[k, :n_boxes[k]] = np.asarray(cells[k], np.int64).reshape(-1)
        h_label[k, :n_boxes[k]] = np.arange(n_boxes[k]) if label_of is None else np.asarray(label_of[k], np.int32).reshape(-1)
    M = h_cells.shape[1]
    owner = torch.empty((K, n), dtype=torch.int32, device=dev)
    cin = torch.zeros((K, M), dtype=torch.int32, device=dev) if counts else None
    cown = torch.zeros((K, M), dtype=torch.int32, device=dev) if counts else None
    ws = _lib.scratch(dev, "instances", L.cv_decode_instances_workspace_bytes(K, M))
    with torch.cuda.device(dev):
        rc = L.cv_decode_instances_f32(ptr(grid_rot), ptr(grid_scale), (ctypes.c_int * 3)(*shape),
                                       (ctypes.c_float * 3)(*[float(v) for v in corner]), ctypes.c_float(float(res)),
                                       ptr(scan_points), ptr(prob), n, K, h_cells.ctypes.data_as(_lib.c_i64_p),
                                       h_label.ctypes.data_as(_lib.c_i32_p), n_boxes.ctypes.data_as(_lib.c_int_p), M,
                                       ctypes.c_float(float(prob_thresh)), confident, ptr(owner), ptr(cin), ptr(cown), ptr(ws),
                                       ws.numel(), stream(dev))
    _lib.check(rc, "cv_decode_instances_f32")
    if single:
        return (owner[0], cin[0, :B], cown[0, :B]) if counts else owner[0]
    return (owner, cin[:, :B], cown[:, :B]) if counts else owner


def get_iou_obb(bbox1, bbox2):
    """utils/calc_map.py:6-21 on two [8,3] corner arrays."""
    a = np.ascontiguousarray(bbox1, np.float32)
    b = np.ascontiguousarray(bbox2, np.float32)
    return float(_lib.lib().cv_iou_obb(a.ctypes.data_as(_lib.c_float_p), b.ctypes.data_as(_lib.c_float_p)))


def nms(boxes, scores, overlap_threshold):
    """eval_joint.py:75-89: indices kept, highest score first."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8, 3)
    s = np.ascontiguousarray(scores, np.float32)
    n = int(s.shape[0])
    pick = np.zeros(max(n, 1), np.int32)
    k = _lib.lib().cv_nms_obb(b.ctypes.data_as(_lib.c_float_p), s.ctypes.data_as(_lib.c_float_p), n,
                              float(overlap_threshold), pick.ctypes.data_as(_lib.c_i32_p))
    if k < 0:
        _lib.check(k, "cv_nms_obb")
    return [int(v) for v in pick[:k]]


def nms_per_class(boxes, scores, classes, nclasses=9, overlap_threshold=0.3):
    """eval_joint.py:270-280 -> [(class, box[8,3], score)] in the reference's order."""
    out = []
    if len(classes) == 0:
        return out
    for i in range(nclasses):
        sel = classes == i
        if sel.sum() > 0:
            bc, sc = boxes[sel], scores[sel]
            for j in nms(bc, sc, overlap_threshold):
                out.append((i, bc[j], float(sc[j])))
    return out


def detect(hv, coords_int, xyz_pred, scale_pred, prob_pred, class_pred, res, nclasses=9, scan_points=None, **kw):
    """eval_joint.py:193-280 after the network: vote, decode, per-class NMS.

    ``hv`` is a HoughVoting module, ``coords_int`` the [N,3] integer voxel coordinates
    (``scan_points[:, 1:]``).  Returns (detections, raw) where detections is the
    ``map_scene`` list of (class, box, score)."""
    if scan_points is None:
        scan_points = (coords_int.to(xyz_pred.device) * res).float().contiguous()    # :193,:200
    with torch.no_grad():
        grid_obj, grid_rot, grid_scale = hv(scan_points, xyz_pred.contiguous(),
                                            scale_pred.contiguous(), prob_pred.contiguous())
    raw = decode_boxes(grid_obj, grid_rot, grid_scale, scan_points, xyz_pred.contiguous(),
                       prob_pred.contiguous(), class_pred, res, **kw)
    dets = nms_per_class(raw["boxes"], raw["scores"], raw["classes"], nclasses)
    return dets, raw
