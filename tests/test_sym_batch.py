"""The per-category trainer's batch built on the device from raw scans, the parts that need no GPU:
``ScanNetXYZProbSymDataset.raw_item`` / ``collate_raw_sym`` and ``restate``, a numpy restatement of cv_sp_sym_rows_f32's
contract as include/cv_hip.h words it, against ``collate_sym([ds[i] ...])`` bit for bit - on the reference class's goldens
(tests/golden/data_ref.npz: sym0, symaug1) and on every generated case of tests/test_sym_batch_gpu.py - the random-stream
contract, the host-side argument checks of the C entry, and named wrong results the comparison has to reject.

Expected values come from ``__getitem__`` + ``collate_sym``, the goldens and the restatement - never from the code under test."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data
from tests.golden.make_data_golden import mini_cfg
from tests.test_train_batch import _model, _quat_y, write_dataset

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "data_ref.npz"))
RES = 0.03
SYM_FIELDS = ("rows", "pseg", "seg_ptr", "pose_ptr", "tgt_ptr", "targets", "urow", "uptr", "upoint")
NONE, UP2, UP4, INF = "__SYM_NONE", "__SYM_ROTATE_UP_2", "__SYM_ROTATE_UP_4", "__SYM_ROTATE_UP_INF"
BLOCK, SPAN = 256, 256 * 1024            # cv_sp_sym_rows_block(), cv_sp_sym_rows_scan_span(): checked against the library below


# ---- the contract of cv_sp_sym_rows_f32 in numpy ---------------------------------------------------------------------

def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def target_sum(m, p, fused=False):
    """[len, 3] fp64: ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3]; fused: the same with fused multiply-adds"""
    x, y, z = (p[:, k].astype(np.float64)[:, None] for k in range(3))
    if not fused:
        return ((m[None, :, 0] * x + m[None, :, 1] * y) + m[None, :, 2] * z) + m[None, :, 3]
    out = np.empty((p.shape[0], 3))
    for i in range(p.shape[0]):
        for r in range(3):
            t = _fma(m[r, 1], p[i, 1], m[r, 0] * np.float64(p[i, 0]))
            out[i, r] = _fma(m[r, 2], p[i, 2], t) + m[r, 3]
    return out


def restate(b, res, use_xyz=False, recentre=False, reference_indexing=True, wrong=None, with_sums=False):
    """a RawSymBatch -> dict of everything ``collate_sym`` gives (coords4, feats, scale, obj, cls, the SymBatch's tensors
    and host ints), by the six steps of include/cv_hip.h.  ``wrong``: one of the named wrong results."""
    pts, off = b.points.numpy(), b.offsets.numpy()
    M = pts.shape[0]
    cloud = (np.searchsorted(off, np.arange(M), side="right") - 1).astype(np.int32)
    key = np.concatenate([cloud[:, None], np.floor(pts / res).astype(np.int32)], 1)
    _, idx, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(idx)
    index = idx[order]                                   # first point of every voxel, ascending
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    inverse = rank[np.asarray(inv).reshape(-1)]
    first_row = np.searchsorted(index, off, side="left")
    # 1 survivors, 2 segments
    v = b.seg_vertex.numpy().astype(np.int64)
    vptr, jptr, minv = b.seg_vptr.numpy().astype(np.int64), b.pose_ptr.numpy().astype(np.int64), b.minv.numpy()
    S0 = vptr.size - 1
    seg = np.repeat(np.arange(S0), np.diff(vptr))
    r = inverse[v]
    surv = (r >= 0) if wrong == "occupied" else (index[r] == v)
    lens0 = np.bincount(seg[surv], minlength=S0)
    keep = np.ones(S0, bool) if wrong == "keep_empty" else lens0 > 0
    ks = np.nonzero(keep)[0]
    new_id = np.full(S0, -1)
    new_id[ks] = np.arange(ks.size)
    kv, kr = v[surv], r[surv]
    rows = kr - first_row[cloud[kv]] if reference_indexing else kr
    lens, poses = lens0[ks], np.diff(jptr)[ks]
    prefix = lambda a: np.concatenate([[0], np.cumsum(a)])
    seg_ptr = prefix(lens)
    # 3 targets
    targets, sums = [], []
    for k, s in enumerate(ks):
        p = pts[kv[seg_ptr[k]:seg_ptr[k + 1]]]
        for j in range(jptr[s], jptr[s + 1]):
            targets.append(target_sum(minv[j], p, fused=wrong == "fma"))
            if with_sums:
                pd = p.astype(np.float64)
                sums.append(np.abs(minv[j][None, :, :3] * pd[:, None, :]).sum(-1) + np.abs(minv[j][None, :, 3]))
    t64 = np.concatenate(targets) if targets else np.zeros((0, 3))
    # 4 inverse list
    urow, counts = np.unique(rows, return_counts=True)
    upoint = np.argsort(rows, kind="stable")
    if wrong == "unstable":
        upoint = np.lexsort((-np.arange(rows.size), rows))
    # 5 rows
    o = b.owner.numpy()[index]
    t = b.rgb.numpy()[index].astype(np.float64)
    if b.colour is not None:
        g = b.colour.numpy()[cloud[index]]
        t = t * g[:, :3]
        t = t + g[:, 3:]
        t = t + b.jitter.numpy()[index][:, None]
        t = np.minimum(np.maximum(t, 0.0), 1.0)
    c = (t / 255.0).astype(np.float32)
    if recentre:
        c = c * np.float32(2) - np.float32(1)
    fg = o >= 0
    scale = np.zeros((index.size, 3), np.float32)
    scale[fg] = b.scale.numpy()[o[fg]]
    cls = np.zeros(index.size, np.int64)
    cls[fg] = b.cls.numpy()[o[fg]]
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    out = dict(coords4=key[index], feats=np.concatenate([pts[index], c], 1) if use_xyz else c, scale=scale,
               obj=fg.astype(np.int64), cls=cls, rows=i32(rows), pseg=i32(new_id[seg[surv]]), seg_ptr=i32(seg_ptr),
               pose_ptr=i32(prefix(poses)), tgt_ptr=i32(prefix(lens * poses)), targets=t64.astype(np.float32), urow=i32(urow),
               uptr=i32(prefix(counts)), upoint=i32(upoint), n_segments=int(ks.size), n_jobs=int(poses.sum()),
               max_row=int(rows.max()) if ks.size and rows.size else -1)
    if with_sums:
        out["t64"], out["sums"] = t64, (np.concatenate(sums) if sums else np.zeros((0, 3)))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_equals_host(host, got, what=""):
    """host: collate_sym's tuple (CPU); got: a dict as ``restate`` returns it (numpy arrays and three ints)"""
    _, coords4, feats, sym, scale, obj, cls = host
    for name, h in (("coords4", coords4), ("feats", feats), ("scale", scale), ("obj", obj), ("cls", cls)):
        assert same_bits(h.numpy(), got[name]), (what, name, tuple(h.shape), h.dtype, got[name].shape, got[name].dtype)
    for name in SYM_FIELDS:
        assert same_bits(getattr(sym, name).numpy(), got[name]), (what, name, tuple(getattr(sym, name).shape), got[name].shape)
    assert (sym.n_segments, sym.n_jobs, sym.max_row) == (got["n_segments"], got["n_jobs"], got["max_row"]), what


def recentred(host):
    feats = host[2].clone()
    feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0
    return host[:2] + (feats,) + host[3:]


# ---- generated datasets: tests/test_train_batch.py's on-disk formats with a `sym` per model --------------------------

def world_with_copies(seed, n_voxels, copies):
    """``n_voxels`` points half a metre apart, then ``copies`` exact copies of some of them at the END: vertex i >= n_voxels is
    a LATER duplicate inside its original's voxel, whatever the rigid motion (equal inputs give equal fp32 outputs)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(g.shape[0])[:n_voxels]]
    base = g * 0.5 + rng.uniform(0.1, 0.4, (n_voxels, 3))
    return np.concatenate([base, base[rng.integers(0, n_voxels, copies)]])


def sym_spec(seed, world, models, rgb=None):
    """one scan; models: (catid, sym, segment vertex list, singular) per aligned model"""
    rng = np.random.default_rng(seed)
    m = world.shape[0]
    q, t = _quat_y(0.7 + 0.1 * seed, 0.3), [0.4, 1.1, -0.6]
    scan = (world - np.asarray(t)) @ data.quat_matrix(q)
    out_models, segs = [], []
    for cat, sym, seg, singular in models:
        mod = _model(rng, cat, world[rng.integers(0, m)], singular=singular)
        mod["sym"] = sym
        out_models.append(mod)
        segs.append(np.asarray(seg, np.int64))
    if rgb is None:
        rgb = rng.integers(0, 256, (m, 3))
    return dict(scan=scan.astype(np.float32), rgb=rgb, trs={"translation": t, "rotation": q, "scale": [1.0, 1.0, 1.0]},
                models=out_models, segs=segs)


CHAIR, TABLE, UNKNOWN, SHELF = "03001627", "04379243", "99999999", "02871439"


def _scan_with_q(seed, q_total, n_vox=300, copies=60):
    """one scan whose three models' lists hold ``q_total`` candidates in all (firsts and later duplicates mixed)"""
    rng = np.random.default_rng(seed)
    w = world_with_copies(seed, n_vox, copies)
    a, b = q_total // 3, q_total // 3
    pick = lambda n: rng.integers(0, w.shape[0], n)       # with repeats
    return sym_spec(seed, w, [(CHAIR, NONE, pick(a), False), (TABLE, UP2, pick(b), False),
                              (UNKNOWN, UP4, pick(q_total - a - b), False)])


def cases():
    """name -> (specs, mini_cfg keywords, augment, seed); every generated case of the GPU test, and its CPU half here"""
    out = {}
    for q in (BLOCK - 1, BLOCK, BLOCK + 1):
        out["q%d" % q] = ([_scan_with_q(40 + q, q)], dict(augment_color=True), True, 40 + q)
    out["second_scan_level"] = ([_scan_with_q(50, SPAN + 5, n_vox=1500, copies=300)], dict(), True, 50)
    # dropped candidates: vertices >= n_vox are later duplicates
    w = world_with_copies(60, 200, 80)
    first, later = np.arange(0, 200), np.arange(200, 280)
    out["dropped_first_between_last"] = ([sym_spec(60, w, [(CHAIR, UP2, later[:20], False), (TABLE, NONE, first[:50], False),
                                                           (CHAIR, UP4, later[20:50], False), (UNKNOWN, UP2, first[40:90], False),
                                                           (TABLE, INF, later[50:], False)])], dict(augment_color=True), True, 60)
    out["all_dropped"] = ([sym_spec(61, w, [(CHAIR, UP2, later[:20], False), (TABLE, INF, later[30:], False)])], dict(), True, 61)
    # segment shapes
    rng = np.random.default_rng(62)
    w = world_with_copies(62, 400, 100)
    unsorted = rng.permutation(500)[:120]
    repeated = np.concatenate([np.arange(100, 160), np.arange(100, 130), [100, 100]])
    third = np.arange(200, 290)
    out["shapes"] = ([sym_spec(62, w, [(CHAIR, NONE, [7], False), (TABLE, INF, np.arange(10, 90), False),
                                       (CHAIR, NONE, np.arange(60, 100), False), (SHELF, UP4, np.arange(0, 50), True),
                                       (UNKNOWN, UP2, unsorted, False), (TABLE, UP4, repeated, False),
                                       (CHAIR, UP2, third, False), (TABLE, NONE, np.concatenate([third[60:], np.arange(290, 350)]), False)])],
                     dict(augment_color=True, use_xyz=True), True, 62)
    three = []
    for i, (nv, cp) in enumerate(((350, 70), (200, 30), (410, 90))):
        ww = world_with_copies(70 + i, nv, cp)
        r = np.random.default_rng(70 + i)
        if i == 1:                                          # no model in the table: its only model is singular
            three.append(sym_spec(70 + i, ww, [(SHELF, UP2, r.integers(0, nv, 40), True)]))
        else:
            three.append(sym_spec(70 + i, ww, [(CHAIR, UP4, r.integers(0, nv + cp, 150), False),
                                               (TABLE, NONE, r.integers(0, nv + cp, 90), False),
                                               (CHAIR, INF, r.integers(0, nv + cp, 60), False)]))
    out["three_scans"] = (three, dict(augment_color=True), True, 70)
    out["q0"] = ([sym_spec(80, world_with_copies(80, 150, 30), [(SHELF, UP2, np.arange(30), True)])], dict(augment_color=True), True, 80)
    w = world_with_copies(81, 300, 60)
    r = np.random.default_rng(81)
    clamp_rgb = r.choice([0, 1, 254, 255], (360, 3))
    out["clamps"] = ([sym_spec(81, w, [(CHAIR, UP2, r.integers(0, 360, 100), False)], rgb=clamp_rgb)], dict(augment_color=True), True, 81)
    out["no_colour"] = ([sym_spec(82, w, [(CHAIR, UP2, r.integers(0, 360, 100), False), (TABLE, NONE, r.integers(0, 360, 70), False)],
                                  rgb=clamp_rgb)], dict(use_xyz=True), False, None)
    return out


def host_and_raw(root, case, reference_indexing=True):
    """(collate_sym of ds[i], RawSymBatch of the same draws, dataset)"""
    specs, kw, augment, seed = case
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(root=write_dataset(root, specs), **kw), training=False, augment=augment)
    if seed is not None:
        np.random.seed(seed)
    items = [ds[i] for i in range(len(ds))]
    if seed is not None:
        np.random.seed(seed)
    raws = [ds.raw_item(i) for i in range(len(ds))]
    return data.collate_sym(items, reference_indexing=reference_indexing), data.collate_raw_sym(raws), ds


def gold_item(tag):
    n = int(GOLD[tag + "_nmodels"])
    labels = [[GOLD["%s_m%d_rows" % (tag, i)], list(GOLD["%s_m%d_xyz" % (tag, i)])] for i in range(n)]
    return (str(GOLD[tag + "_id"]), GOLD[tag + "_coords"], GOLD[tag + "_feats"], labels, GOLD[tag + "_scale"], GOLD[tag + "_obj"],
            GOLD[tag + "_cls"])


def golden_raw(tag):
    if tag == "sym0":
        return data.ScanNetXYZProbSymDataset(mini_cfg(), training=False, augment=False).raw_item(0)
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(category="03001627"), training=False, augment=True)
    np.random.seed(11)
    return ds.raw_item(1)


def no_rounding_ties(b):
    """no target lies within 4 * 2^-53 * sum|terms| of the midpoint of two neighbouring fp32 values"""
    out = restate(b, RES, with_sums=True)
    t, bound = out["t64"], 4 * 2.0 ** -53 * out["sums"]
    f = t.astype(np.float32)
    lo, hi = np.nextafter(f, np.float32(-np.inf)).astype(np.float64), np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    dist = np.minimum(np.abs(t - (f + lo) / 2), np.abs(t - (f + hi) / 2))
    return bool((dist > bound).all()), t.size


# ---- exports and host-side argument checks ---------------------------------------------------------------------------

def test_sym_rows_symbols_are_exported_and_the_abi_stays_6(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ("cv_sp_sym_rows_f32", "cv_sp_sym_rows_workspace_bytes", "cv_sp_sym_rows_block", "cv_sp_sym_rows_scan_span",
                 "cv_sizeof_sym_rows_desc"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.cv_abi_version() == _lib.ABI_VERSION == 6
    assert ctypes.sizeof(_lib.SymRowsDesc) == L.cv_sizeof_sym_rows_desc()
    assert L.cv_sp_sym_rows_block() == BLOCK and L.cv_sp_sym_rows_scan_span() == SPAN      # what the generated cases straddle
    assert L.cv_sp_sym_rows_workspace_bytes(1000, 500, 4, 2) > 4 * (1000 + 2 * 500)
    from canonicalvoting_amd import me as ME
    assert callable(ME.utils.sym_rows) and callable(ME.utils.quantize_nowait) and callable(data.device_batch_sym)


def fake_desc(**kw):
    p = 4096                                                               # fake pointers: never dereferenced
    a = dict(d_coords4=p, d_index=p, d_inverse=p, d_quant_counts=p, m_points=200, d_points=p, points_ld=3, d_rgb=p, d_owner=p,
             d_model_scale=p, d_model_cls=p, n_models=4, d_colour=p, d_jitter=p, d_offsets=p, n_clouds=2, d_seg_vertex=p, n_cand=50,
             d_seg_vptr=p, d_seg_pose_ptr=p, n_seg_in=3, d_minv=p, n_jobs_in=5, n_targets_in=90, reference_indexing=1, use_xyz=0,
             recentre=1, d_rows=p, d_pseg=p, d_seg_ptr=p, d_pose_ptr=p, d_tgt_ptr=p, d_targets=p, d_urow=p, d_uptr=p, d_upoint=p,
             d_feats=p, feats_ld=3, d_scale=p, scale_ld=3, d_obj=p, d_cls=p, d_counts=p, h_counts=None, d_ws=p, ws_bytes=1 << 30)
    a.update(kw)
    return _lib.SymRowsDesc(**a)


def test_sym_rows_refuses_bad_descriptors_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    run = lambda **kw: L.cv_sp_sym_rows_f32(ctypes.byref(fake_desc(**kw)), None)
    assert L.cv_sp_sym_rows_f32(None, None) == -22 and b"descriptor" in L.cv_last_error()
    for null in ("d_coords4", "d_index", "d_inverse", "d_quant_counts", "d_points", "d_rgb", "d_owner", "d_model_scale", "d_model_cls",
                 "d_offsets", "d_seg_vertex", "d_seg_vptr", "d_seg_pose_ptr", "d_minv", "d_rows", "d_pseg", "d_seg_ptr", "d_pose_ptr",
                 "d_tgt_ptr", "d_targets", "d_urow", "d_uptr", "d_upoint", "d_feats", "d_scale", "d_obj", "d_cls", "d_counts", "d_ws"):
        assert run(**{null: None}) == -22 and b"null pointer" in L.cv_last_error(), null
    for field, word in (("m_points", b"point count"), ("n_cand", b"candidate count"), ("n_seg_in", b"segment count"),
                        ("n_jobs_in", b"job count"), ("n_targets_in", b"target count"), ("n_models", b"model count")):
        assert run(**{field: -1}) == -22 and word in L.cv_last_error(), field
    assert run(m_points=0) == -22 and run(n_clouds=0) == -22 and b"cloud count" in L.cv_last_error()
    for field, v in (("points_ld", 2), ("feats_ld", 2), ("scale_ld", 2)):
        assert run(**{field: v}) == -22 and b"row stride" in L.cv_last_error(), field
    assert run(use_xyz=1, feats_ld=5) == -22 and b"row stride" in L.cv_last_error()
    assert run(d_jitter=None) == -22 and b"colour table without jitter" in L.cv_last_error()
    assert run(d_colour=None) == -22 and b"jitter without a colour table" in L.cv_last_error()
    assert run(n_targets_in=49) == -22 and b"target bound" in L.cv_last_error()
    assert run(ws_bytes=64) == -12 and b"workspace" in L.cv_last_error()


# ---- the random-stream contract --------------------------------------------------------------------------------------

def test_raw_item_draws_from_the_global_generator_like_getitem():
    for kw, seed in ((dict(augment_color=True), 5), (dict(), 6)):
        ds = data.ScanNetXYZProbSymDataset(mini_cfg(**kw), training=False, augment=True)
        np.random.seed(seed)
        ds[0]
        ds[1]
        want = np.random.get_state()
        np.random.seed(seed)
        a, b = ds.raw_item(0), ds.raw_item(1)
        got = np.random.get_state()
        assert np.array_equal(want[1], got[1]) and want[2:] == got[2:] and want[2] > 0
        assert (a.colour is None) == (not kw) and isinstance(b, data.RawSymScan)


def test_raw_item_redraws_a_scan_without_a_selected_model_like_getitem():
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(), training=False, augment=False)
    ds.cfg.category = "02871439"                                            # only scan 0 has a bookshelf: item 1 redraws until it gets 0
    np.random.seed(2)
    want = ds[1]
    state = np.random.get_state()
    np.random.seed(2)
    raw = ds.raw_item(1)
    assert raw.id_scan == want[0] == "scene0000_00" and np.array_equal(state[1], np.random.get_state()[1])
    assert state[2] == np.random.get_state()[2] and state[2] > 0
    assert raw.cls.shape == (0,) and raw.seg_vertex.shape == (0,) and raw.minv.shape == (0, 3, 4)     # the bookshelf is singular


def test_raw_item_types_and_shapes():
    raw = golden_raw("sym0")
    m, k, q, j = raw.points.shape[0], raw.cls.shape[0], raw.seg_vertex.shape[0], raw.minv.shape[0]
    for a, dt, shape in ((raw.points, np.float32, (m, 3)), (raw.rgb, np.uint8, (m, 3)), (raw.owner, np.int32, (m,)),
                         (raw.scale, np.float32, (k, 3)), (raw.cls, np.int32, (k,)), (raw.seg_vertex, np.int32, (q,)),
                         (raw.seg_vptr, np.int32, (k + 1,)), (raw.pose_ptr, np.int32, (k + 1,)), (raw.minv, np.float64, (j, 3, 4))):
        assert a.dtype == dt and a.shape == shape
    assert np.diff(raw.pose_ptr).tolist() == [1, 2, 1, 36] and raw.pose_ptr[-1] == j and raw.seg_vptr[-1] == q
    assert raw.colour is None and raw.owner.max() == k - 1


# ---- restatement against the reference -------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["sym0", "symaug1"])
def test_restated_contract_on_raw_items_reproduces_the_reference_goldens(tag):
    b = data.collate_raw_sym([golden_raw(tag)])
    for ref in (True, False):
        assert_equals_host(data.collate_sym([gold_item(tag)], reference_indexing=ref), restate(b, RES, reference_indexing=ref), tag)
    ok, n = no_rounding_ties(b)
    assert ok and n > 600


def test_two_golden_scans_in_one_batch_share_rows_under_reference_indexing():
    np.random.seed(3)
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(augment_color=True), training=False, augment=True)
    items = [ds[0], ds[1]]
    np.random.seed(3)
    b = data.collate_raw_sym([ds.raw_item(0), ds.raw_item(1)])
    for ref in (True, False):
        host = data.collate_sym(items, reference_indexing=ref)
        assert_equals_host(host, restate(b, RES, reference_indexing=ref), ref)
        assert_equals_host(recentred(host), restate(b, RES, recentre=True, reference_indexing=ref), ref)
    host = data.collate_sym(items)
    assert int(np.diff(host[3].uptr.numpy()).max()) >= 2                   # rows of the two scans collide


@pytest.mark.parametrize("name", sorted(cases()))
def test_generated_gpu_cases_restate_to_the_dataset_path(tmp_path, name):
    case = cases()[name]
    use_xyz = case[1].get("use_xyz", False)
    for ref in (True, False):
        host, b, _ = host_and_raw(tmp_path / str(ref), case, ref)
        got = restate(b, RES, use_xyz=use_xyz, reference_indexing=ref)
        assert_equals_host(host, got, (name, ref))
    assert_equals_host(recentred(host), restate(b, RES, use_xyz=use_xyz, recentre=True, reference_indexing=False), name)
    assert no_rounding_ties(b)[0]
    sym, n_pose = host[3], np.diff(host[3].pose_ptr.numpy())
    if name.startswith("q2"):
        assert b.n_cand == int(name[1:])
    if name == "second_scan_level":
        assert b.n_cand > SPAN
    if name == "dropped_first_between_last":
        assert b.seg_vptr.shape[0] - 1 == 5 and sym.n_segments == 2 and n_pose.tolist() == [1, 2]
    if name == "all_dropped":
        assert sym.n_segments == 0 and sym.max_row == -1 and sym.rows.shape[0] == 0 and b.n_cand == 70 and host[1].shape[0] > 0
    if name == "shapes":
        lens = np.diff(sym.seg_ptr.numpy())
        assert lens[0] == 1 and 36 in n_pose and 1 in n_pose and b.seg_vptr.shape[0] - 1 == 7          # the singular one is absent
        assert int(np.diff(sym.uptr.numpy()).max()) >= 3                   # repeated vertices and shared models
    if name == "three_scans":
        assert b.offsets.shape[0] == 3 and set(np.unique(b.seg_cloud.numpy())) == {0, 2}
    if name == "q0":
        assert b.n_cand == 0 and b.n_targets == 0 and sym.n_segments == 0 and not host[5].any()
    if name == "clamps":
        f = host[2].numpy()
        assert (f == 0).sum() > 10 and (f == np.float32(1 / 255.0)).sum() > 10
    if name == "no_colour":
        assert b.colour is None and b.jitter is None


# ---- collate checks --------------------------------------------------------------------------------------------------

def test_a_segment_vertex_out_of_range_raises_in_raw_item(tmp_path):
    w = world_with_copies(90, 50, 10)
    for bad in (60, -1):
        root = write_dataset(tmp_path / str(bad), [sym_spec(90, w, [(CHAIR, NONE, [3, bad, 5], False)])])
        ds = data.ScanNetXYZProbSymDataset(mini_cfg(root=root), training=False, augment=False)
        with pytest.raises(IndexError):
            ds.raw_item(0)
    with pytest.raises(IndexError):
        ds.__class__(mini_cfg(root=write_dataset(tmp_path / "g", [sym_spec(90, w, [(CHAIR, NONE, [3, 60], False)])])),
                     training=False, augment=False)[0]                     # numpy's indexing in __getitem__


def test_collate_raw_sym_layout_and_its_int32_bound():
    raw = golden_raw("sym0")
    b = data.collate_raw_sym([raw, raw])
    m, k, q = raw.points.shape[0], raw.cls.shape[0], raw.seg_vertex.shape[0]
    assert isinstance(b, data.RawSymBatch) and b.offsets.tolist() == [0, m] and b.offsets.dtype == torch.int64
    assert b.seg_cloud.tolist() == [0] * k + [1] * k and b.seg_cloud.dtype == torch.int32
    assert (b.n_cand, b.n_jobs) == (2 * q, 2 * raw.minv.shape[0]) and b.n_targets == 2 * int((np.diff(raw.seg_vptr) * np.diff(raw.pose_ptr)).sum())
    assert torch.equal(b.seg_vertex[q:], b.seg_vertex[:q] + m) and torch.equal(b.owner[m:][raw.owner >= 0], b.owner[:m][raw.owner >= 0] + k)
    assert b.seg_vptr.tolist() == raw.seg_vptr.tolist() + (raw.seg_vptr[1:] + q).tolist()
    for t in b:
        assert not torch.is_tensor(t) or (t.device.type == "cpu" and t.is_contiguous())
    # T0 beyond int32: 40 copies of a list of 2^20 entries under 36 poses each (zero-stride views: nothing that large is stored)
    big = raw._replace(seg_vertex=np.zeros(1 << 20, np.int32), seg_vptr=np.array([0, 1 << 20], np.int32),
                       pose_ptr=np.array([0, 36], np.int32), minv=raw.minv[:36], scale=raw.scale[:1], cls=raw.cls[:1])
    with pytest.raises(ValueError, match="int32"):
        data.collate_raw_sym([big] * 60)
    aug = raw._replace(colour=(np.ones(3), np.zeros(3), np.zeros(m)))
    with pytest.raises(ValueError, match="every scan"):
        data.collate_raw_sym([raw, aug])


WORKER_SEED = 93


def _seed_worker(_worker_id):
    np.random.seed(WORKER_SEED)


def test_collate_raw_sym_through_dataloader_workers(tmp_path):
    """data.RawItems under DataLoader workers with collate_raw_sym: the one batch of a two-scan dataset (260 and 195 vertices,
    colour and rotation drawn), made by the worker that starts from WORKER_SEED, is the batch collated in-process from that seed"""
    specs = [_scan_with_q(91, 120, n_vox=220, copies=40), _scan_with_q(92, 90, n_vox=160, copies=35)]
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(root=write_dataset(tmp_path, specs), augment_color=True), training=False, augment=True)
    np.random.seed(WORKER_SEED)
    want = data.collate_raw_sym([ds.raw_item(0), ds.raw_item(1)])
    loader = torch.utils.data.DataLoader(data.RawItems(ds), batch_size=2, shuffle=False, collate_fn=data.collate_raw_sym,
                                         num_workers=2, worker_init_fn=_seed_worker, pin_memory=torch.cuda.is_available())
    (got,) = list(loader)
    assert isinstance(got, data.RawSymBatch) and want.colour is not None and want.points.shape[0] == 260 + 195
    for name, w in want._asdict().items():
        g = getattr(got, name)
        assert same_bits(g.numpy(), w.numpy()) if torch.is_tensor(w) else (type(g) is type(w) and g == w), name


# ---- named wrong results the comparison must reject -------------------------------------------------------------------

@pytest.mark.parametrize("wrong,name", [("occupied", "shapes"), ("unstable", "shapes"), ("keep_empty", "dropped_first_between_last")])
def test_the_comparison_rejects_named_wrong_results(tmp_path, wrong, name):
    host, b, _ = host_and_raw(tmp_path, cases()[name])
    use_xyz = cases()[name][1].get("use_xyz", False)
    assert_equals_host(host, restate(b, RES, use_xyz=use_xyz), name)
    with pytest.raises(AssertionError):
        assert_equals_host(host, restate(b, RES, use_xyz=use_xyz, wrong=wrong), name)


def as_host(d):
    """a restated dict in the shape of collate_sym's tuple"""
    t = torch.from_numpy
    sym = data.SymBatch(*[t(d[k]) for k in SYM_FIELDS], d["n_segments"], d["n_jobs"], d["max_row"])
    return (None, t(d["coords4"]), t(d["feats"]), sym, t(d["scale"]), t(d["obj"]), t(d["cls"]))


def test_the_comparison_rejects_the_fused_form_of_the_target_sum():
    """a case built to differ: m0 x = -1 cancels the leading 1 of m1 y = 1 + 2^-23 + 2^-47 + 2^-70.  Written, the product
    rounds to 1 + 2^-23 + 2^-47 first and the sum 2^-23 (1 + 2^-24) is an fp32 tie that goes to 2^-23; fused, the 2^-70
    survives and the sum rounds up."""
    y = np.float32(1 + 2.0 ** -23)
    m = np.zeros((1, 3, 4))
    m[0, :, 0], m[0, :, 1] = -1.0, 1 + 2.0 ** -47
    b = data.RawSymBatch(("built",), torch.tensor([[1.0, float(y), 0.0]]), torch.zeros((1, 3), dtype=torch.uint8),
                         torch.zeros(1, dtype=torch.int32), torch.ones((1, 3)), torch.ones(1, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
                         torch.tensor([0, 1], dtype=torch.int32), torch.from_numpy(m), torch.zeros(1, dtype=torch.int32), None, None,
                         torch.zeros(1, dtype=torch.int64), 1, 1, 1)
    written, fused = restate(b, RES), restate(b, RES, wrong="fma")
    assert written["targets"].tolist() == [[2.0 ** -23] * 3] and fused["targets"].tolist() == [[2.0 ** -23 * (1 + 2.0 ** -23)] * 3]
    assert not no_rounding_ties(b)[0]                                       # and the tie rule names it
    assert_equals_host(as_host(written), written, "built")
    with pytest.raises(AssertionError):
        assert_equals_host(as_host(written), fused, "built")


def test_the_script_refuses_the_device_loader_without_a_config():
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_separate.py")
    r = subprocess.run([sys.executable, script, "--device-loader"], capture_output=True, text=True)
    assert r.returncode == 2 and "--device-loader needs --config" in r.stderr and "no raw-scan form" in r.stderr
