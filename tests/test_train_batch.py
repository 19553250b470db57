"""Training batches built on the device from raw scans, the parts that need no GPU: the exports and host-side argument
checks of cv_sp_scan_rows_f32, ``raw_item`` / ``collate_raw`` against the reference class's goldens and against
``__getitem__`` on generated datasets, the random-stream contract, and the CPU half of every generated GPU case of
tests/test_train_batch_gpu.py.

Expected values come from ``restate``, a numpy restatement of the kernel's formulas as include/cv_hip.h writes them
(applied to what ``raw_item`` returns), from tests/golden/data_ref.npz (the reference's own class) and from
``__getitem__`` - never from the code under test."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data
from tests.golden.make_data_golden import mini_cfg, write_ply

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "data_ref.npz"))
RES = 0.03
NAMES = ("coords", "feats", "xyz", "scale", "cls")

# tag -> (mini_cfg keywords, augment, seed or None, index); aug0 / aug1 are consecutive items of ONE seeded stream
GOLDEN_CONFIGS = {
    "plain0": (dict(), False, None, 0),
    "plain1": (dict(), False, None, 1),
    "aug0": (dict(augment_color=True), True, 5, 0),
    "aug1": (dict(augment_color=True), True, None, 1),
    "xyz1": (dict(use_xyz=True), True, 9, 1),
    "cat_others": (dict(category="others"), False, None, 0),
    "cat_02871439": (dict(category="02871439"), False, None, 0),      # its only model is singular: empty table, all background
}


def f32(a):
    return np.asarray(a).astype(np.float32)


def restate(raw, res, use_xyz=False, recentre=False):
    """(coords [N, 3] f32, feats, xyz, scale, cls int32) of one RawScan: first point of every voxel in first-point order,
    then the formulas of cv_sp_scan_rows_f32 per kept row, every step rounded where the header says it rounds"""
    p32 = raw.points
    vox = np.floor(p32 / res).astype(np.int32)
    keep = np.sort(np.unique(vox, axis=0, return_index=True)[1])
    coords = np.floor(p32[keep] / res).astype(np.float32)
    c = f32(raw.rgb[keep].astype(np.float64) / 255.0)
    if raw.colour is not None:
        gain, shift, jitter = raw.colour
        c = f32(c.astype(np.float64) * gain[None, :])
        c = f32(c.astype(np.float64) + shift[None, :])
        c = f32(c.astype(np.float64) + jitter[keep][:, None])
        c = np.minimum(np.maximum(c, np.float32(0)), np.float32(1))
    if recentre:
        c = c * np.float32(2) - np.float32(1)
    feats = np.concatenate([p32[keep], c], -1) if use_xyz else c
    o = raw.owner[keep]
    n = keep.size
    xyz, scale, cls = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.full(n, 9, np.int32)
    fg = o >= 0
    if fg.any():
        m, p = raw.minv[o[fg]], p32[keep][fg].astype(np.float64)                     # [F, 3, 4], [F, 3]
        xyz[fg] = f32(((m[:, :, 0] * p[:, None, 0] + m[:, :, 1] * p[:, None, 1]) + m[:, :, 2] * p[:, None, 2]) + m[:, :, 3])
        scale[fg] = raw.scale[o[fg]]
        cls[fg] = raw.cls[o[fg]]
    return coords, feats, xyz, scale, cls


def restate_batch(raws, res, use_xyz=False, recentre=False):
    """the restatement of several scans as ``collate_fn`` lays a batch out: (coords4 int32, feats, xyz, scale, cls int64)"""
    parts = [restate(r, res, use_xyz, recentre) for r in raws]
    coords4 = np.concatenate([np.concatenate([np.full((p[0].shape[0], 1), b, np.int32), p[0].astype(np.int32)], 1)
                              for b, p in enumerate(parts)])
    return (coords4,) + tuple(np.concatenate([p[i] for p in parts]) for i in (1, 2, 3)) + \
        (np.concatenate([p[4] for p in parts]).astype(np.int64),)


def golden_raws(tags):
    """RawScans of the golden configurations ``tags`` (in GOLDEN_CONFIGS order where a seeded stream continues)"""
    out = {}
    for tag, (kw, augment, seed, index) in GOLDEN_CONFIGS.items():
        if tag == "aug1" and "aug1" in tags:                             # continues aug0's stream
            ds = data.ScanNetXYZProbMultiDataset(mini_cfg(**kw), training=False, augment=True)
            np.random.seed(5)
            ds.raw_item(0)
            out[tag] = ds.raw_item(1)
            continue
        if tag not in tags:
            continue
        ds = data.ScanNetXYZProbMultiDataset(mini_cfg(**kw), training=False, augment=augment)
        if seed is not None:
            np.random.seed(seed)
        out[tag] = ds.raw_item(index)
    return out


# ---- generated datasets in the on-disk formats of tests/golden/make_data_golden.py ---------------------------------

def _quat_y(angle, tilt=0.0):
    axis = np.array([tilt, 1.0, -tilt]) / np.linalg.norm([tilt, 1.0, -tilt])
    return [float(np.cos(angle / 2))] + [float(v) for v in np.sin(angle / 2) * axis]


def _model(rng, catid, where, singular=False):
    sc = rng.uniform(0.7, 1.4, 3)
    if singular:
        sc[1] = 5e-4
    return {"catid_cad": catid, "id_cad": "generated", "sym": "__SYM_NONE",
            "trs": {"translation": [float(v) for v in where], "rotation": _quat_y(rng.uniform(0, 2 * np.pi), 0.05),
                    "scale": [float(v) for v in sc]},
            "bbox": [float(v) for v in rng.uniform(0.2, 0.6, 3)], "center": [float(v) for v in rng.uniform(-0.05, 0.05, 3)]}


def scan_spec(seed, world, cats, seg_size, singular=(), rgb=None, general_pose=True):
    """one scan: ``world`` [M, 3] points, one model per entry of ``cats`` whose segment is ``seg_size`` vertices drawn
    independently per model (so segments overlap), models in ``singular`` with a degenerate scale"""
    rng = np.random.default_rng(seed)
    m = world.shape[0]
    if general_pose:
        q, t = _quat_y(0.7 + 0.1 * seed, 0.3), [0.4, 1.1, -0.6]
        R = data.quat_matrix(q)
        scan = (world - np.asarray(t)) @ R                               # inverse of T R
    else:
        q, t, scan = [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], world
    models = [_model(rng, c, world[rng.integers(0, m)], singular=i in singular) for i, c in enumerate(cats)]
    segs = [np.sort(rng.choice(m, size=min(seg_size, m), replace=False)) for _ in cats]
    if rgb is None:
        rgb = rng.integers(0, 256, (m, 3))
        rgb[rng.random((m, 3)) < 0.1] = 0                                # enough black and white for both clamps
        rgb[rng.random((m, 3)) < 0.1] = 255
    return dict(scan=scan.astype(np.float32), rgb=rgb, trs={"translation": t, "rotation": q, "scale": [1.0, 1.0, 1.0]},
                models=models, segs=segs)


def write_dataset(root, specs):
    root = str(root)
    annotations, segments, ids = [], {}, []
    for i, s in enumerate(specs):
        sid = "scene%04d_00" % i
        ids.append(sid)
        write_ply(os.path.join(root, "scans", sid, sid + "_vh_clean_2.ply"), s["scan"], s["rgb"], np.zeros((1, 3), np.int64))
        annotations.append({"id_scan": sid, "trs": s["trs"], "aligned_models": s["models"], "n_aligned_models": len(s["models"])})
        segments[sid] = s["segs"]
    with open(os.path.join(root, "full_annotations.json"), "w") as f:
        json.dump(annotations, f)
    for name in ("train", "val"):
        with open(os.path.join(root, "segments_%s.pkl" % name), "wb") as f:
            pickle.dump(segments, f, protocol=2)
        with open(os.path.join(root, "%s_split.txt" % name), "w") as f:
            f.write("".join(sid + "\n" for sid in ids))
    return root


def lattice_world(seed, n_voxels, copies):
    """``n_voxels`` points half a metre apart plus ``copies`` exact copies of some of them: n_voxels occupied voxels under
    any rigid motion (a copy shares its original's voxel whatever the rounding)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(5), np.arange(8), indexing="ij"), -1).reshape(-1, 3)[:n_voxels]
    base = g * 0.5 + rng.uniform(0.1, 0.4, (n_voxels, 3))
    world = np.concatenate([base, base[rng.integers(0, n_voxels, copies)]])
    return world[rng.permutation(world.shape[0])]


SPARSE_ROOM = np.array([24.0, 8.0, 24.0])      # 70 000 points in 4608 m^3 at 0.03 m: nearly every point its own voxel


def big_specs():
    """the three ~70 000-vertex scans of the GPU test 'against the parent path at size'"""
    out = []
    for i, m in enumerate((70001, 69000, 71003)):
        rng = np.random.default_rng(100 + i)
        world = rng.random((m, 3)) * SPARSE_ROOM - SPARSE_ROOM / 2
        out.append(scan_spec(200 + i, world, ["03001627", "99999999", "04379243", "02871439", "03001627", "02933112"], m // 5,
                             singular=(3,)))
    return out


# name -> (specs, dataset keywords, augment, seed); every GPU case of 'smallest shapes' - and their CPU half below
def small_cases():
    one = np.array([[0.31, 0.52, -0.77]])
    cats3 = ["03001627", "99999999", "04379243"]
    return {
        "one_vertex": ([scan_spec(1, one, ["03001627"], 1)], dict(augment_color=True), True, 3),
        "one_voxel": ([scan_spec(2, np.repeat(one, 40, 0), cats3, 15)], dict(augment_color=True, use_xyz=True), True, 4),
        "n255": ([scan_spec(3, lattice_world(3, 255, 60), cats3, 90)], dict(augment_color=True), True, 5),
        "n256": ([scan_spec(4, lattice_world(4, 256, 60), cats3, 90)], dict(augment_color=True, use_xyz=True), True, 6),
        "n257": ([scan_spec(5, lattice_world(5, 257, 60), cats3, 90)], dict(), True, 7),
        "no_colour": ([scan_spec(6, lattice_world(6, 100, 30), cats3, 40), scan_spec(7, lattice_world(7, 70, 10), cats3, 30)],
                      dict(), False, None),
        "clamps": ([scan_spec(8, lattice_world(8, 120, 30), cats3, 40,
                              rgb=np.random.default_rng(8).choice([0, 1, 254, 255], (150, 3)))], dict(augment_color=True), True, 8),
        "all_background": ([scan_spec(9, lattice_world(9, 90, 20), ["02871439"], 50, singular=(0,))], dict(augment_color=True), True, 9),
        "unknown_catid": ([scan_spec(10, lattice_world(10, 90, 20), ["99999999", "12345678"], 30)], dict(), False, None),
    }


def dataset_and_raws(root, specs, kw, augment, seed):
    """(host batch = collate_fn of ds[i], RawScans of the same draws, dataset)"""
    cfg = mini_cfg(root=write_dataset(root, specs), **kw)
    ds = data.ScanNetXYZProbMultiDataset(cfg, training=False, augment=augment)
    if seed is not None:
        np.random.seed(seed)
    items = [ds[i] for i in range(len(ds))]
    if seed is not None:
        np.random.seed(seed)
    raws = [ds.raw_item(i) for i in range(len(ds))]
    return data.collate_fn(items), raws, ds


def assert_batch_equal(host, got, what):
    """host: collate_fn's tensors; got: numpy arrays in the same order (coords4, feats, xyz, scale, cls)"""
    for name, h, g in zip(NAMES, host[1:], got):
        h = h.numpy()
        assert h.dtype == g.dtype and h.shape == g.shape, (what, name, h.dtype, g.dtype, h.shape, g.shape)
        assert np.array_equal(h.view(np.uint8), np.ascontiguousarray(g).view(np.uint8)), \
            (what, name, int((h != g).sum()), "elements differ")


# ---- exports and argument checks -------------------------------------------------------------------------------------

def test_scan_rows_symbols_are_exported_and_the_abi_stays_6(built_lib):
    L = ctypes.CDLL(built_lib)
    for name in ("cv_sp_scan_rows_f32", "cv_sizeof_scan_rows_desc"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert _lib.lib().cv_abi_version() == _lib.ABI_VERSION == 6
    assert ctypes.sizeof(_lib.ScanRowsDesc) == _lib.lib().cv_sizeof_scan_rows_desc()
    from canonicalvoting_amd import me as ME
    assert callable(ME.utils.scan_rows) and callable(data.device_batch) and callable(data.collate_raw)


def fake_desc(**kw):
    p = 4096                                                               # fake pointers: never dereferenced
    a = dict(d_coords4=p, d_index=p, n=100, m_points=200, d_points=p, points_ld=3, d_rgb=p, d_owner=p, d_minv=p, d_model_scale=p,
             d_model_cls=p, n_models=4, d_colour=p, d_jitter=p, n_clouds=2, use_xyz=0, recentre=1, d_feats=p, feats_ld=3,
             d_xyz=p, xyz_ld=3, d_scale=p, scale_ld=3, d_cls=p, cls_ld=1)
    a.update(kw)
    return _lib.ScanRowsDesc(**a)


def test_scan_rows_refuses_bad_descriptors_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    run = lambda **kw: L.cv_sp_scan_rows_f32(ctypes.byref(fake_desc(**kw)), None)
    assert L.cv_sp_scan_rows_f32(None, None) == -22 and b"descriptor" in L.cv_last_error()
    for null in ("d_coords4", "d_index", "d_points", "d_rgb", "d_owner", "d_feats", "d_xyz", "d_scale", "d_cls",
                 "d_minv", "d_model_scale", "d_model_cls"):
        assert run(**{null: None}) == -22 and b"null pointer" in L.cv_last_error(), null
    for field, v in (("points_ld", 2), ("feats_ld", 2), ("xyz_ld", 2), ("scale_ld", 2), ("cls_ld", 0)):
        assert run(**{field: v}) == -22 and b"row stride" in L.cv_last_error(), field
    assert run(use_xyz=1, feats_ld=5) == -22 and b"row stride" in L.cv_last_error()      # the width is 6 with the points in front
    assert run(n=201) == -22 and b"more kept rows" in L.cv_last_error()
    for n in (0, -3):
        assert run(n=n) == -22 and b"row count" in L.cv_last_error()
    assert run(m_points=0, n=1) == -22 and b"point count" in L.cv_last_error()
    assert run(n_models=-1) == -22 and b"model count" in L.cv_last_error()
    assert run(n_clouds=0) == -22 and b"cloud count" in L.cv_last_error()
    assert run(d_colour=None) == -22 and b"jitter without a colour table" in L.cv_last_error()
    assert run(d_jitter=None) == -22 and b"colour table without jitter" in L.cv_last_error()


# ---- goldens of the reference's own class ----------------------------------------------------------------------------

def test_restated_kernel_formulas_on_raw_items_reproduce_the_reference_goldens():
    raws = golden_raws(set(GOLDEN_CONFIGS))
    elements = 0
    for tag, raw in raws.items():
        use_xyz = GOLDEN_CONFIGS[tag][0].get("use_xyz", False)
        assert raw.id_scan == str(GOLD[tag + "_id"])
        for name, a in zip(NAMES, restate(raw, RES, use_xyz)):
            g = GOLD[tag + "_" + name]
            assert a.dtype == g.dtype and a.shape == g.shape, (tag, name, a.dtype, g.dtype, a.shape, g.shape)
            assert np.array_equal(a, g), (tag, name, int((a != g).sum()))
            elements += a.size
    assert elements > 30000
    empty = raws["cat_02871439"]
    assert empty.cls.shape == (0,) and empty.minv.shape == (0, 3, 4) and empty.scale.shape == (0, 3) and (empty.owner == -1).all()
    assert raws["plain0"].colour is None and len(raws["aug0"].colour) == 3
    assert set(raws["plain0"].cls.tolist()) == {0, 2, 6}                   # the singular bookshelf is not in the table


def test_raw_item_types_and_shapes():
    raw = golden_raws({"aug0"})["aug0"]
    m, k = raw.points.shape[0], raw.cls.shape[0]
    assert isinstance(raw, data.RawScan) and isinstance(raw.id_scan, str)
    for a, dt, shape in ((raw.points, np.float32, (m, 3)), (raw.rgb, np.uint8, (m, 3)), (raw.owner, np.int32, (m,)),
                         (raw.minv, np.float64, (k, 3, 4)), (raw.scale, np.float32, (k, 3)), (raw.cls, np.int32, (k,)),
                         (raw.colour[0], np.float64, (3,)), (raw.colour[1], np.float64, (3,)), (raw.colour[2], np.float64, (m,))):
        assert a.dtype == dt and a.shape == shape
    assert raw.owner.max() == k - 1 and raw.owner.min() == -1


def test_raw_item_draws_from_the_global_generator_like_getitem():
    ds = data.ScanNetXYZProbMultiDataset(mini_cfg(augment_color=True), training=False, augment=True)
    np.random.seed(5)
    ds[0]
    ds[1]
    want = np.random.get_state()
    np.random.seed(5)
    ds.raw_item(0)
    ds.raw_item(1)
    got = np.random.get_state()
    assert want[0] == got[0] and np.array_equal(want[1], got[1]) and want[2:] == got[2:]
    ds = data.ScanNetXYZProbMultiDataset(mini_cfg(), training=False, augment=True)         # rotation alone: two draws
    np.random.seed(6)
    ds[0]
    want = np.random.get_state()
    np.random.seed(6)
    assert ds.raw_item(0).colour is None
    assert np.array_equal(want[1], np.random.get_state()[1]) and want[2] == np.random.get_state()[2]


def test_raw_item_redraws_and_checks_files_like_getitem(tmp_path):
    ds = data.ScanNetXYZProbMultiDataset(mini_cfg(), training=False, augment=False)
    ds.cfg.category = "02871439"                                            # only scan 0 has a bookshelf: item 1 redraws until it gets 0
    np.random.seed(2)
    want = ds[1]
    state = np.random.get_state()
    np.random.seed(2)
    raw = ds.raw_item(1)
    assert raw.id_scan == want[0] == "scene0000_00" and np.array_equal(state[1], np.random.get_state()[1])
    assert state[2] == np.random.get_state()[2] and np.random.get_state()[2] > 0
    cfg = mini_cfg()
    ds = data.ScanNetXYZProbMultiDataset(cfg, training=False, augment=False)
    cfg.data.scannet = str(tmp_path)
    with pytest.raises(FileNotFoundError, match="does not exist"):
        ds.raw_item(0)
    ds.annotations[0]["trs"]["scale"] = [1.0, 1.1, 1.0]
    with pytest.raises(ValueError, match="non-unit scale"):
        ds.raw_item(0)


# ---- collation ----------------------------------------------------------------------------------------------------------

def test_collate_raw_concatenates_and_shifts_the_owners(tmp_path):
    """overlapping segments (the later model wins), owner offsets across clouds and an empty model table in the middle,
    against __getitem__ + collate_fn on a dataset written to disk"""
    specs = [scan_spec(20, lattice_world(20, 150, 40), ["03001627", "99999999", "04379243"], 110),
             scan_spec(21, lattice_world(21, 80, 20), ["02871439"], 50, singular=(0,)),          # m = 0
             scan_spec(22, lattice_world(22, 130, 30), ["02933112", "04256520"], 100)]
    host, raws, _ = dataset_and_raws(tmp_path, specs, dict(augment_color=True, use_xyz=True), True, 12)
    seg = specs[0]["segs"]
    shared = np.intersect1d(seg[1], seg[2])
    assert shared.size > 10 and (raws[0].owner[shared] == 2).all()          # drawn 110 of 190 each: they overlap; the last wins
    assert [r.cls.shape[0] for r in raws] == [3, 0, 2]
    b = data.collate_raw(raws)
    assert isinstance(b, data.RawBatch) and b.id_scans == tuple(r.id_scan for r in raws) == host[0]
    sizes = [r.points.shape[0] for r in raws]
    assert b.offsets.dtype == torch.int64 and b.offsets.tolist() == [0, sizes[0], sizes[0] + sizes[1]]
    for t, dt, shape in ((b.points, torch.float32, (sum(sizes), 3)), (b.rgb, torch.uint8, (sum(sizes), 3)),
                         (b.owner, torch.int32, (sum(sizes),)), (b.minv, torch.float64, (5, 3, 4)), (b.scale, torch.float32, (5, 3)),
                         (b.cls, torch.int32, (5,)), (b.colour, torch.float64, (3, 6)), (b.jitter, torch.float64, (sum(sizes),))):
        assert t.dtype == dt and tuple(t.shape) == shape and t.device.type == "cpu" and t.is_contiguous()
    own = b.owner.numpy()
    assert (own[sizes[0]:sizes[0] + sizes[1]] == -1).all()
    third = own[sizes[0] + sizes[1]:]
    assert set(np.unique(third)) == {-1, 3, 4} and np.array_equal(third >= 0, raws[2].owner >= 0)
    assert np.array_equal(b.colour.numpy()[2], np.concatenate(raws[2].colour[:2]))
    # the concatenated batch, read back per cloud, restates to the host batch
    back = [data.RawScan(r.id_scan, b.points.numpy()[o:o + n], b.rgb.numpy()[o:o + n],
                         np.where(own[o:o + n] >= 0, own[o:o + n] - k, -1).astype(np.int32), b.minv.numpy()[k:k + r.cls.shape[0]],
                         b.scale.numpy()[k:k + r.cls.shape[0]], b.cls.numpy()[k:k + r.cls.shape[0]],
                         (b.colour.numpy()[i, :3], b.colour.numpy()[i, 3:], b.jitter.numpy()[o:o + n]))
            for i, (r, o, n, k) in enumerate(zip(raws, b.offsets.tolist(), sizes, (0, 3, 3)))]
    assert_batch_equal(host, restate_batch(back, RES, use_xyz=True), "collated")


def test_collate_raw_without_colour_and_with_colour_in_part_of_the_batch():
    raws = golden_raws({"plain0", "aug1"})
    b = data.collate_raw([raws["plain0"], raws["plain0"]])
    assert b.colour is None and b.jitter is None
    b = data.collate_raw([raws["plain0"], raws["aug1"]])
    m0 = raws["plain0"].points.shape[0]
    assert b.colour[0].tolist() == [1, 1, 1, 0, 0, 0] and not b.jitter[:m0].any() and b.jitter[m0:].any()
    # the identity operands leave a scan's colours as they are
    same = raws["plain0"]._replace(colour=(np.ones(3), np.zeros(3), np.zeros(m0)))
    assert np.array_equal(restate(same, RES)[1], restate(raws["plain0"], RES)[1])


def test_collate_raw_through_dataloader_workers():
    ds = data.ScanNetXYZProbMultiDataset(mini_cfg(), training=False, augment=False)
    want = data.collate_raw([ds.raw_item(0), ds.raw_item(1)])
    loader = torch.utils.data.DataLoader(data.RawItems(ds), batch_size=2, shuffle=False, collate_fn=data.collate_raw, num_workers=2,
                                         pin_memory=torch.cuda.is_available())
    (got,) = list(loader)
    assert isinstance(got, data.RawBatch) and got.id_scans == want.id_scans and got.colour is None and got.jitter is None
    for name in ("points", "rgb", "owner", "minv", "scale", "cls", "offsets"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name


# ---- the CPU half of the generated GPU cases ----------------------------------------------------------------------------
# For every generated case the restatement equals the dataset path bit for bit.  (A label may legitimately differ where
# its fp64 value lies within the fp64 error bound 4 * 2^-53 * sum|terms| of an fp32 rounding tie, a few 1e-9 of random elements;
# no seed below produced one.  Should a changed seed do so, take the next seed - never loosen the comparison.)

@pytest.mark.parametrize("name", sorted(small_cases()))
def test_small_gpu_cases_restate_to_the_dataset_path(tmp_path, name):
    specs, kw, augment, seed = small_cases()[name]
    host, raws, _ = dataset_and_raws(tmp_path, specs, kw, augment, seed)
    assert_batch_equal(host, restate_batch(raws, RES, use_xyz=kw.get("use_xyz", False)), name)
    n, cls = host[1].shape[0], host[5].numpy()
    if name == "one_vertex":
        assert raws[0].points.shape[0] == 1 and n == 1
    if name == "one_voxel":
        assert raws[0].points.shape[0] == 40 and n == 1
    if name in ("n255", "n256", "n257"):
        assert n == int(name[1:])
    if name == "no_colour":
        assert all(r.colour is None for r in raws)
    if name == "clamps":
        f = host[2].numpy()
        assert (f == 0).sum() > 10 and (f == 1).sum() > 10                 # values pushed past both ends
        gain, shift, jitter = raws[0].colour
        raw_hi = (raws[0].rgb / 255.0) * gain + shift + jitter[:, None]
        assert raw_hi.max() > 1 and raw_hi.min() < 0
    if name == "all_background":
        assert (cls == 9).all() and raws[0].cls.shape[0] == 0
    if name == "unknown_catid":
        assert set(np.unique(cls)) == {0, 9}


def test_big_gpu_case_restates_to_the_dataset_path(tmp_path):
    host, raws, _ = dataset_and_raws(tmp_path, big_specs(), dict(augment_color=True, use_xyz=True), True, 31)
    assert_batch_equal(host, restate_batch(raws, RES, use_xyz=True), "big")
    assert host[1].shape[0] > 131072                                        # beyond one trip of every loop of the kernel
