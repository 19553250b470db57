"""Data contract of the step BEFORE the hot path: synthetic scenes and the real-file reader.

``SyntheticScanDataset[i]`` yields exactly what ``ScanNetXYZProbMultiDataset.__getitem__`` returns
(utils/dataloader.py:118-210): ``(id_scan, coords[N,3] float32 = floor(p/res), feats[N,3] rgb in [0,1],
xyz_labels[N,3], scale_labels[N,3], class_labels[N] int32 in 0..9)`` and ``collate_fn`` batches it like
train_joint.py:78-90 (batch index in column 0 of the int coordinates).  ``gt_lines`` gives the ground truth
in the text format eval_joint.py:285-301 reads (``tx ty tz ry sx sy sz ... category``).
There is no ScanNet/Scan2CAD data in this environment; ``ScanNetXYZProbMultiDataset`` below reads the real file
formats and is checked against the reference's own class on a miniature dataset (tests/golden/scannet_mini).
``raw_item`` / ``collate_raw`` / ``device_batch`` are the same training batch with everything behind the two host
transforms computed on the device.  ``collate_sym`` / ``SymBatch`` / ``sym_to_device`` are the
per-category trainer's symmetry labels packed for the device loss, ``SyntheticSymDataset`` its synthetic items.
``ScanNetXYZProbSymDataset.raw_item`` / ``collate_raw_sym`` / ``device_batch_sym`` build that trainer's batch on the device
from raw scans.  ``RawItems`` is the dataset view both device paths hand to their DataLoader workers.
"""
import typing

import numpy as np
import torch

from .me import utils as me_utils
from .synth import make_scene


class SyntheticScanDataset(torch.utils.data.Dataset):
    def __init__(self, n_scenes=8, n_points=80000, res=0.03, seed0=0, **scene_kw):
        self.n_scenes, self.n_points, self.res, self.seed0, self.kw = n_scenes, n_points, res, seed0, scene_kw
        self._scenes = {}

    def __len__(self):
        return self.n_scenes

    def scene(self, index):
        if index not in self._scenes:
            self._scenes[index] = make_scene(self.seed0 + index, n_points=self.n_points, res=self.res, **self.kw)
        return self._scenes[index]

    def __getitem__(self, index):
        s = self.scene(index)
        return ("synth%04d" % (self.seed0 + index), s.coords.astype(np.float32), s.feats, s.xyz_labels,
                s.scale_labels, s.class_labels)

    def gt_lines(self, index):
        """eval_joint.py:287-288 line format: tx ty tz ry sx sy sz category"""
        return ["%f %f %f %f %f %f %f %d" % tuple(list(b[:7]) + [int(b[7])]) for b in self.scene(index).boxes]

    def gt(self, index):
        return parse_gt_lines(self.gt_lines(index))


def parse_gt_lines(lines):
    """eval_joint.py:285-301: ``tx ty tz ry sx sy sz ... category`` -> [(class index, (tx, ty, tz, ry, sx, sy, sz))].
    The category token is a ShapeNet catid or 'others' in the reference's results_gt files (mapped through
    idx2name, eval_joint.py:111-121) and a plain class index in the synthetic ones."""
    out = []
    for line in lines:
        tok = line.split(" ")
        if len(tok) < 8:
            continue
        cat = tok[-1].strip()
        idx = int(cat) if (cat.isdigit() and len(cat) < 8) else TOP8_CLASSES.get(cat, 0)
        out.append((idx, tuple(float(v) for v in tok[:7])))
    return out


def load_config(path, **overrides):
    """The reference's config/config.yaml layout (data.*, scannet_res, category, use_xyz, augment_color, ...) as
    attribute namespaces, without hydra; ``overrides`` replace top-level keys (``category='all'`` as
    eval_joint.py:137 / train_joint.py do)."""
    import types
    import yaml
    with open(path) as f:
        raw = yaml.safe_load(f)
    raw.pop("hydra", None)
    raw.update(overrides)

    def ns(d):
        return types.SimpleNamespace(**{k: ns(v) if isinstance(v, dict) else v for k, v in d.items()})
    return ns(raw)


def collate_fn(batch):
    """train_joint.py:78-90"""
    id_scans, coords, feats, xyz_labels, scale_labels, class_labels = list(zip(*batch))
    coords_batch = me_utils.batched_coordinates(coords)
    return (id_scans, coords_batch, torch.from_numpy(np.concatenate(feats, 0)).float(),
            torch.from_numpy(np.concatenate(xyz_labels, 0)).float(),
            torch.from_numpy(np.concatenate(scale_labels, 0)).float(),
            torch.from_numpy(np.concatenate(class_labels, 0)).long())


# ----------------------------------------------------------------------------------------------------------------
# Real ScanNet + Scan2CAD files.  Same class name, constructor and item tuple as the reference's
# utils/dataloader.py:89-210 so train_joint.py / eval_joint.py-shaped callers take it unchanged; no plyfile /
# numpy-quaternion / MinkowskiEngine needed.  Checked against tests/golden/scannet_mini (the reference's own
# class run over a miniature dataset in the same on-disk formats, tests/golden/make_data_golden.py).

TOP8_CLASSES = {"03211117": 1, "04379243": 2, "02808440": 3, "02747177": 4, "04256520": 5, "03001627": 6,
                "02933112": 7, "02871439": 8}            # utils/dataloader.py:13-23; every other catid -> 0

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_vertices(path):
    """The ``vertex`` element of a PLY file as a numpy structured array (fields x, y, z, red, green, blue ... as the
    header names them).  ascii and binary (either endianness); the vertex element must come first, as it does in
    ScanNet's ``*_vh_clean_2.ply`` (what utils/dataloader.py:130-134 reads through plyfile)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, count, props, element = None, 0, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header has no end_header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if element is None and tok[1] != "vertex":
                    raise ValueError("%s: first PLY element is %r, expected vertex" % (path, tok[1]))
                element = tok[1]
                if element == "vertex":
                    count = int(tok[2])
            elif tok[0] == "property" and element == "vertex":
                if tok[1] == "list":
                    raise ValueError("%s: list property on the vertex element" % path)
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=count, ndmin=2) if count else np.zeros((0, len(props)))
            out = np.zeros(count, dtype=[(n, t) for n, t in props])
            for i, (n, _) in enumerate(props):
                out[n] = rows[:, i]
            return out
        order = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
        if order is None:
            raise ValueError("%s: unknown PLY format %r" % (path, fmt))
        dt = np.dtype([(n, order + t) for n, t in props])
        buf = f.read(dt.itemsize * count)
        if len(buf) != dt.itemsize * count:
            raise ValueError("%s: truncated vertex data" % path)
        return np.frombuffer(buf, dtype=dt, count=count)


def quat_matrix(q):
    """Rotation matrix of the quaternion (w, x, y, z); a non-unit quaternion rotates like its normalisation
    (numpy-quaternion's as_rotation_matrix, utils/dataloader.py:38,63,77)."""
    w, x, y, z = (float(v) for v in q)
    s = 2.0 / (w * w + x * x + y * y + z * z)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]], np.float64)


def _affine(linear=None, shift=None):
    M = np.eye(4)
    if linear is not None:
        M[:3, :3] = linear
    if shift is not None:
        M[:3, 3] = shift
    return M


def trs_matrix(t, q, s):
    """T R S (utils/dataloader.py:72-82)"""
    return _affine(shift=np.asarray(t, np.float64)) @ _affine(quat_matrix(q)) @ _affine(np.diag(np.asarray(s, np.float64)))


def bbox_matrix(model):
    """unit cube -> world: T R S T_center diag(bbox) of one Scan2CAD aligned model (utils/dataloader.py:49-69)"""
    trs = model["trs"]
    return (trs_matrix(trs["translation"], trs["rotation"], trs["scale"])
            @ _affine(shift=np.asarray(model["center"], np.float64)) @ _affine(np.diag(np.asarray(model["bbox"], np.float64))))


def transform_points(pc, M):
    """utils/dataloader.py:85-86 (homogeneous product in float64)"""
    return (M @ np.concatenate([pc, np.ones((pc.shape[0], 1))], -1).T).T[:, :3]


def _draw_augmentation(n_vertex, augment, augment_color):
    """The augmentation draws from numpy's global generator, in the reference's order: gain 3, shift 3, jitter ``n_vertex``
    (these three only with ``augment_color``), randint(4), random(); without ``augment`` nothing is drawn.  Returns ``(colour
    operands (gain f64 [3], shift f64 [3], jitter f64 [n_vertex]) or None, Ry f64 [3, 3] about the up axis or None, aug f64
    [4, 4])``."""
    colour, Ry, aug = None, None, np.eye(4)
    if augment:
        if augment_color:
            colour = (1 + 0.4 * np.random.random(3) - 0.2, 0.1 * np.random.random(3) - 0.05,
                      0.05 * np.random.random(n_vertex) - 0.025)
        angle = np.random.randint(4) * np.pi / 2.0 + (np.random.random() - 0.5) * 2.0 * np.pi / 9.0
        c, s = np.cos(angle), np.sin(angle)
        Ry = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
        aug[:3, :3] = Ry
    return colour, Ry, aug


class ScanNetXYZProbMultiDataset(torch.utils.data.Dataset):
    """utils/dataloader.py:89-210.  ``cfg`` needs ``data.scan2cad`` (full_annotations.json), ``data.scannet`` (root with
    scans/<id>/<id>_vh_clean_2.ply), ``data.{train,val}_split`` (text, one scan id per line),
    ``data.{train,val}_segments`` (pickle: scan id -> per aligned model, vertex indices), ``category``
    ('all' | 'others' | a catid), ``augment_color``, ``use_xyz``, ``scannet_res``.  Augmentation draws from numpy's
    global generator in the reference's order, so a seeded run reproduces the reference's samples."""

    def __init__(self, cfg, training, augment):
        import json
        import pickle
        self.cfg, self.training, self.augment = cfg, training, augment
        with open(cfg.data.scan2cad) as f:
            annotations = json.load(f)
        with open(cfg.data.train_split if training else cfg.data.val_split) as f:
            wanted = set(f.read().splitlines())
        with open(cfg.data.train_segments if training else cfg.data.val_segments, "rb") as f:
            self.segments = pickle.load(f)
        # :102-110: with a category filter, scans without a matching model are dropped; 'all' keeps every scan
        self.annotations = [a for a in annotations if a["id_scan"] in wanted
                            and (cfg.category == "all" or self._select(a["aligned_models"]))]

    def class_index(self, catid):
        return TOP8_CLASSES.get(catid, 0)

    def _select(self, models):
        cat = self.cfg.category
        if cat == "all":
            return list(models)
        if cat == "others":
            return [m for m in models if self.class_index(m["catid_cad"]) == 0]
        return [m for m in models if m["catid_cad"] == cat]

    def __len__(self):
        return len(self.annotations)

    def gt(self, index):
        """ground-truth boxes of scan ``index`` from ``cfg.data.gt_path/<id_scan>.txt`` (eval_joint.py:285)"""
        import os
        with open(os.path.join(self.cfg.data.gt_path, self.annotations[index]["id_scan"] + ".txt")) as f:
            return parse_gt_lines(f.read().splitlines())

    def _read_scan(self, index):
        """What every item method starts with (utils/dataloader.py:118-150): ``(id_scan, rgb uint8 [M, 3], points f64 [M, 3]
        in the world frame, the selected models with their ``segments`` attached)``.  A scan without a selected model draws
        ``np.random.randint(len(self))`` - nothing else has been drawn by then - and the checks run again on that scan."""
        import os
        while True:
            ann = self.annotations[index]
            id_scan = ann["id_scan"]
            if not np.all(np.abs(np.asarray(ann["trs"]["scale"]) - 1.0) < 1e-7):
                raise ValueError("%s: scan transform has a non-unit scale" % id_scan)
            path = os.path.join(self.cfg.data.scannet, "scans", id_scan, id_scan + "_vh_clean_2.ply")
            if not os.path.exists(path):
                raise FileNotFoundError(path + " does not exist.")
            v = read_ply_vertices(path)
            rgb = np.stack([v["red"], v["green"], v["blue"]], -1).astype(np.uint8, copy=False)
            to_world = trs_matrix(ann["trs"]["translation"], ann["trs"]["rotation"], ann["trs"]["scale"])
            points = transform_points(np.stack([v["x"], v["y"], v["z"]], -1), to_world)
            for model, seg in zip(ann["aligned_models"], self.segments[id_scan]):
                model["segments"] = seg
            models = self._select(ann["aligned_models"])
            if models:
                return id_scan, rgb, points, models
            index = np.random.randint(len(self))

    def _augmented_scan(self, index):
        """``_read_scan``, then ``_draw_augmentation`` and what every item method does with it: ``(id_scan, rgb uint8 [M, 3],
        points f32 [M, 3] rotated, models, colour operands or None, aug f64 [4, 4])`` - the scan up to and including the
        reference's ``points.astype(np.float32)``.  Each trainer applies the colour operands in its own arithmetic."""
        id_scan, rgb, points, models = self._read_scan(index)
        colour, Ry, aug = _draw_augmentation(points.shape[0], self.augment, self.cfg.augment_color)
        if Ry is not None:
            points = points @ Ry.T               # (rebinding releases the fp64 world points before the cast allocates)
        return id_scan, rgb, points.astype(np.float32), models, colour, aug

    def _model_table(self, id_scan, models, aug, n_vertex, sym_poses=False):
        """The table of the non-singular models, in model order: ``(owner int32 [M], minv f64 [J, 3, 4], scale f32 [m, 3],
        cls int32 [m], segs, seg_vptr, pose_ptr)``.  ``owner`` is assigned in model order, so the last model wins a shared
        vertex.  ``minv`` holds the top three rows of inv(aug @ P): one pose per model, or with ``sym_poses`` every
        symmetry-equivalent pose (rows pose_ptr[k]:pose_ptr[k + 1]) - then ``segs`` are the models' vertex lists as int32,
        as they lie, and a vertex outside the scan raises IndexError; without, numpy's own indexing holds."""
        owner = np.full(n_vertex, -1, np.int32)
        minv, scale, cls, segs, vptr, pose_ptr = [], [], [], [], [0], [0]
        for m in models:
            s32 = np.asarray(m["trs"]["scale"], np.float32)
            if s32.min() < 1e-3:                                         # singular annotation (:171-172): not in the table
                continue
            seg, poses = m["segments"], [bbox_matrix(m)]
            if sym_poses:
                seg = np.asarray(seg, np.int64).reshape(-1)
                if seg.size and (seg.min() < 0 or seg.max() >= n_vertex):
                    raise IndexError("%s: segment vertex %d outside the scan's %d vertices"
                                     % (id_scan, int(seg.min() if seg.min() < 0 else seg.max()), n_vertex))
                poses += [poses[0] @ _roty4(a) for a in SYMMETRY_ANGLES.get(m["sym"], [])]
                segs.append(seg.astype(np.int32))                        # unsorted lists and duplicates are kept
                vptr.append(vptr[-1] + seg.size)
            owner[seg] = len(cls)
            minv.extend(np.linalg.inv(aug @ P)[:3] for P in poses)
            scale.append(s32 * np.asarray(m["bbox"], np.float32))        # half extents in metres
            cls.append(self.class_index(m["catid_cad"]))
            pose_ptr.append(pose_ptr[-1] + len(poses))
        return (owner, np.asarray(minv, np.float64).reshape(-1, 3, 4), np.asarray(scale, np.float32).reshape(-1, 3),
                np.asarray(cls, np.int32), segs, np.asarray(vptr, np.int32), np.asarray(pose_ptr, np.int32))

    def __getitem__(self, index):
        id_scan, rgb, points, models, colour, aug = self._augmented_scan(index)
        rgb = (rgb / 255.0).astype(np.float32)
        if colour is not None:                                           # :156-160, float32 in place
            rgb *= colour[0]
            rgb += colour[1]
            rgb += colour[2][:, None]
            rgb = np.clip(rgb, 0, 1)
        n = points.shape[0]
        xyz = np.zeros((n, 3), np.float32)
        scale = np.zeros((n, 3), np.float32)
        cls = np.full(n, 9, np.int32)
        for m in models:
            s32 = np.asarray(m["trs"]["scale"], np.float32)
            if s32.min() < 1e-3:                                         # singular annotation (:171-172)
                continue
            seg = m["segments"]
            xyz[seg] = transform_points(points[seg], np.linalg.inv(aug @ bbox_matrix(m)))
            scale[seg] = s32 * np.asarray(m["bbox"], np.float32)         # half extents in metres
            cls[seg] = self.class_index(m["catid_cad"])
        feats = np.concatenate([points, rgb], -1) if self.cfg.use_xyz else rgb
        keep = me_utils.sparse_quantize(np.ascontiguousarray(points), quantization_size=self.cfg.scannet_res,
                                        return_index=True)[1]
        coords = np.floor(points[keep] / self.cfg.scannet_res).astype(np.float32)
        return id_scan, coords, feats[keep], xyz[keep], scale[keep], cls[keep]

    def raw_item(self, index):
        """``__getitem__`` up to and including ``points.astype(np.float32)``, as a RawScan: the same file checks, the same
        redraw and the same draws from numpy's global generator in the same order; everything behind that line - colours,
        labels, voxelisation, gathers - is left to ``device_batch``, as operands rather than results."""
        id_scan, rgb, points, models, colour, aug = self._augmented_scan(index)
        owner, minv, scale, cls = self._model_table(id_scan, models, aug, points.shape[0])[:4]
        return RawScan(id_scan, points, rgb, owner, minv, scale, cls, colour)


class RawScan(typing.NamedTuple):
    """One scan as ``ScanNetXYZProbMultiDataset.raw_item`` leaves it: per vertex ``points`` f32 [M, 3] (world frame,
    augmentation rotation applied), ``rgb`` uint8 [M, 3] and ``owner`` int32 [M] (row of the model table whose labels the
    vertex gets, -1 = background); the model table ``minv`` f64 [m, 3, 4] (world -> unit cube, top three rows), ``scale``
    f32 [m, 3], ``cls`` int32 [m] (m may be 0); ``colour`` None or (gain f64 [3], shift f64 [3], jitter f64 [M])."""
    id_scan: str
    points: np.ndarray
    rgb: np.ndarray
    owner: np.ndarray
    minv: np.ndarray
    scale: np.ndarray
    cls: np.ndarray
    colour: typing.Optional[tuple]


class RawBatch(typing.NamedTuple):
    """``collate_raw``'s result: the fields of the batch's RawScans one after the other as CPU tensors, ``owner`` counting
    rows of the concatenated model table, ``offsets`` int64 [B] the first vertex of every cloud, ``colour`` f64 [B, 6]
    (gain, shift) with ``jitter`` f64 [M], or both None."""
    id_scans: tuple
    points: torch.Tensor
    rgb: torch.Tensor
    owner: torch.Tensor
    minv: torch.Tensor
    scale: torch.Tensor
    cls: torch.Tensor
    colour: typing.Optional[torch.Tensor]
    jitter: typing.Optional[torch.Tensor]
    offsets: torch.Tensor


def collate_raw(batch):
    """RawScans -> RawBatch (the ``collate_fn`` of the device path; a tuple of tensors, so DataLoader workers and
    ``pin_memory`` handle it).  A scan without colour operands in a batch that has some gets the identity (gain 1, shift 0,
    jitter 0), which leaves its colours as they are."""
    return RawBatch(minv=_cat([s.minv for s in batch]), **_collate_common(batch))


def _cat(arrays):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays, 0)))


def _collate_common(batch):
    """the fields RawBatch and RawSymBatch share, by name: the scans' points, rgb, scale and cls one after the other, ``owner``
    shifted to rows of the concatenated model table, ``offsets``, and the colour operands - ``colour`` f64 [B, 6] with
    ``jitter`` f64 [M], a scan without operands getting the identity, or both None when no scan has any"""
    sizes = [s.points.shape[0] for s in batch]
    first_model = np.cumsum([0] + [s.cls.shape[0] for s in batch[:-1]])
    owner = [np.where(s.owner >= 0, s.owner + np.int32(f), np.int32(-1)).astype(np.int32) for s, f in zip(batch, first_model)]
    colour = jitter = None
    if any(s.colour is not None for s in batch):
        colour = torch.from_numpy(np.stack([np.concatenate(s.colour[:2]) if s.colour is not None
                                            else np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]) for s in batch]).astype(np.float64))
        jitter = _cat([np.asarray(s.colour[2], np.float64) if s.colour is not None else np.zeros(n, np.float64)
                       for s, n in zip(batch, sizes)])
    return dict(id_scans=tuple(s.id_scan for s in batch), points=_cat([s.points for s in batch]), rgb=_cat([s.rgb for s in batch]),
                owner=_cat(owner), scale=_cat([s.scale for s in batch]), cls=_cat([s.cls for s in batch]), colour=colour,
                jitter=jitter, offsets=torch.from_numpy(np.cumsum([0] + sizes[:-1]).astype(np.int64)))


def _upload(batch, dev, host=()):
    """a NamedTuple batch with its tensors on ``dev`` (non-blocking copies in field order: no host wait from pinned memory);
    the fields named in ``host``, host ints and None stay as they are"""
    return batch._replace(**{k: v.to(dev, non_blocking=True) for k, v in batch._asdict().items()
                             if torch.is_tensor(v) and k not in host})


class RawItems(torch.utils.data.Dataset):
    """a ScanNetXYZProbMultiDataset or ScanNetXYZProbSymDataset whose items are its raw scans (``raw_item``): what the
    DataLoader workers of the device path produce, for ``collate_raw`` / ``collate_raw_sym``"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, index):
        return self.ds.raw_item(index)


def device_batch(raw_batch, device, res, use_xyz=False, recentre=True):
    """A RawBatch -> ``(id_scans, coords4, feats, xyz, scale, cls)`` on ``device``: exactly what ``collate_fn([ds[i] ...])``
    moved to the device gives (coords4 int32 [N, 4], feats f32 [N, 3|6], xyz / scale f32 [N, 3], cls int64 [N]), with the
    training script's ``feats[:, -3:] * 2 - 1`` applied when ``recentre``.  On torch's current stream: non-blocking copies,
    the voxelisation (ME.utils.quantize_batch, its one host wait for N) and one cv_sp_scan_rows_f32 launch."""
    dev = torch.device(device)
    b = _upload(raw_batch, dev, host=("offsets",))
    with torch.cuda.device(dev):
        coords4, index = me_utils.quantize_batch(b.points, res, offsets=b.offsets)
        feats, xyz, scale_rows, cls_rows = me_utils.scan_rows(coords4, index, b.points, b.rgb, b.owner, b.minv, b.scale, b.cls,
                                                              b.colour, b.jitter, use_xyz=use_xyz, recentre=recentre)
    return b.id_scans, coords4, feats, xyz, scale_rows, cls_rows


def _roty4(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]])


# rotations about the up axis under which a CAD model looks the same (utils/dataloader.py:444-453)
SYMMETRY_ANGLES = {"__SYM_ROTATE_UP_2": [np.pi], "__SYM_ROTATE_UP_4": [np.pi / 2, np.pi, -np.pi / 2],
                   "__SYM_ROTATE_UP_INF": [2 * np.pi / 36 * i for i in range(1, 36)]}


class ScanNetXYZProbSymDataset(ScanNetXYZProbMultiDataset):
    """utils/dataloader.py:339-476, the dataset of train_separate.py: same files, but the scan is quantised FIRST and
    the object labels are kept per aligned model as ``[rows of the model's points, [their LCC coordinates under each
    symmetry-equivalent pose]]`` so the loss can take the best pose; item = (id_scan, coords, feats, xyz_labels,
    scale_labels, obj_labels (0/1), class_labels (0 = background or 'others'))."""

    def __getitem__(self, index):
        id_scan, rgb, points, models, colour, aug = self._augmented_scan(index)   # rgb stays uint8 until after quantisation (:383)
        if colour is not None:                                           # :400-404 (on the raw 0..255 colours)
            rgb = rgb.astype(np.float64)
            rgb *= colour[0]
            rgb += colour[1]
            rgb += colour[2][:, None]
            rgb = np.clip(rgb, 0, 1)
        n_vertex = points.shape[0]
        keep = me_utils.sparse_quantize(np.ascontiguousarray(points), quantization_size=self.cfg.scannet_res,
                                        return_index=True)[1]
        points = points[keep]
        rgb = (rgb[keep] / 255.0).astype(np.float32)
        new_row = np.full(n_vertex, -1, np.int64)
        new_row[keep] = np.arange(len(keep))
        coords = np.floor(points / self.cfg.scannet_res).astype(np.float32)
        n = points.shape[0]
        scale = np.zeros((n, 3), np.float32)
        obj = np.zeros(n, np.int32)
        cls = np.zeros(n, np.int32)
        xyz_labels = []
        for m in models:
            s32 = np.asarray(m["trs"]["scale"], np.float32)
            if s32.min() < 1e-3:
                continue
            M = bbox_matrix(m)
            poses = [M] + [M @ _roty4(a) for a in SYMMETRY_ANGLES.get(m["sym"], [])]
            rows = new_row[np.asarray(m["segments"], np.int64)]
            rows = rows[rows >= 0]                                       # the model's points that survived quantisation
            pts = points[rows]
            xyzs = [transform_points(pts, np.linalg.inv(aug @ P)) for P in poses]
            scale[rows] = s32 * np.asarray(m["bbox"], np.float32)
            obj[rows] = 1
            cls[rows] = self.class_index(m["catid_cad"])
            xyz_labels.append([rows, xyzs])
        feats = np.concatenate([points, rgb], -1) if self.cfg.use_xyz else rgb
        return id_scan, coords, feats, xyz_labels, scale, obj, cls

    def raw_item(self, index):
        """``__getitem__`` up to and including ``points.astype(np.float32)``, as a RawSymScan: the same file checks, the same
        redraw and the same draws from numpy's global generator in the same order; voxelisation, the survivor filter, the
        targets under every pose and the packing are left to ``device_batch_sym``, as operands rather than results."""
        id_scan, rgb, points, models, colour, aug = self._augmented_scan(index)
        owner, minv, scale, cls, segs, vptr, pose_ptr = self._model_table(id_scan, models, aug, points.shape[0], sym_poses=True)
        return RawSymScan(id_scan, points, rgb, owner, scale, cls, np.concatenate(segs) if segs else np.zeros(0, np.int32), vptr,
                          pose_ptr, minv, colour)


class RawSymScan(typing.NamedTuple):
    """One scan as ``ScanNetXYZProbSymDataset.raw_item`` leaves it: per vertex ``points`` f32 [M, 3], ``rgb`` uint8 [M, 3] and
    ``owner`` int32 [M] (row of the model table, -1 = background; the last model wins a shared vertex); the table of the
    non-singular models ``scale`` f32 [m, 3], ``cls`` int32 [m]; their segment vertex lists one after the other
    ``seg_vertex`` int32 [Q] (list k = seg_vertex[seg_vptr[k]:seg_vptr[k + 1]], as they lie) with ``seg_vptr`` / ``pose_ptr``
    int32 [m + 1]; ``minv`` f64 [J, 3, 4] = the top three rows of inv(aug @ P) of every (model, pose), model k's poses the
    rows pose_ptr[k]:pose_ptr[k + 1] in ``__getitem__``'s pose order; ``colour`` None or (gain f64 [3], shift f64 [3],
    jitter f64 [M]) for the 0..255 colours."""
    id_scan: str
    points: np.ndarray
    rgb: np.ndarray
    owner: np.ndarray
    scale: np.ndarray
    cls: np.ndarray
    seg_vertex: np.ndarray
    seg_vptr: np.ndarray
    pose_ptr: np.ndarray
    minv: np.ndarray
    colour: typing.Optional[tuple]


class RawSymBatch(typing.NamedTuple):
    """``collate_raw_sym``'s result: the fields of the batch's RawSymScans one after the other as CPU tensors - ``owner``
    counts rows of the concatenated model table, ``seg_vertex`` vertices of the concatenated clouds, ``seg_vptr`` /
    ``pose_ptr`` int32 [S0 + 1] are prefix sums over the batch's S0 segments, ``seg_cloud`` int32 [S0] the cloud of every
    segment, ``offsets`` int64 [B] the first vertex of every cloud, ``colour`` f64 [B, 6] (gain, shift) with ``jitter`` f64 [M] or
    both None - and the upper bounds known on the host: ``n_cand`` = Q, ``n_jobs`` = J0, ``n_targets`` = T0 = the sum over the
    segments of list length * poses."""
    id_scans: tuple
    points: torch.Tensor
    rgb: torch.Tensor
    owner: torch.Tensor
    scale: torch.Tensor
    cls: torch.Tensor
    seg_vertex: torch.Tensor
    seg_vptr: torch.Tensor
    pose_ptr: torch.Tensor
    minv: torch.Tensor
    seg_cloud: torch.Tensor
    colour: typing.Optional[torch.Tensor]
    jitter: typing.Optional[torch.Tensor]
    offsets: torch.Tensor
    n_cand: int
    n_jobs: int
    n_targets: int


def collate_raw_sym(batch):
    """RawSymScans -> RawSymBatch (the ``collate_fn`` of the per-category trainer's device path; a tuple of tensors and host
    ints, so DataLoader workers and ``pin_memory`` handle it).  Raises when M or T0 does not fit int32, and when only some
    scans of the batch carry colour operands (the 0..255 clip has no identity operands)."""
    n_vertex = sum(s.points.shape[0] for s in batch)
    lens = np.concatenate([np.diff(s.seg_vptr.astype(np.int64)) for s in batch])
    poses = np.concatenate([np.diff(s.pose_ptr.astype(np.int64)) for s in batch])
    n_targets = int((lens * poses).sum())
    if n_vertex >= 2 ** 31 or n_targets >= 2 ** 31:
        raise ValueError("collate_raw_sym: the batch does not fit int32 pointers (%d vertices, %d target rows)"
                         % (n_vertex, n_targets))
    with_colour = [s.colour is not None for s in batch]
    if any(with_colour) != all(with_colour):
        raise ValueError("collate_raw_sym: colour operands come for every scan of a batch or for none")
    common = _collate_common(batch)
    prefix = lambda a: torch.from_numpy(np.concatenate([[0], np.cumsum(a)]).astype(np.int32))
    return RawSymBatch(seg_vertex=_cat([(s.seg_vertex.astype(np.int64) + f).astype(np.int32)
                                        for s, f in zip(batch, common["offsets"].numpy())]),
                       seg_vptr=prefix(lens), pose_ptr=prefix(poses), minv=_cat([s.minv for s in batch]),
                       seg_cloud=torch.from_numpy(np.repeat(np.arange(len(batch)), [s.cls.shape[0] for s in batch]).astype(np.int32)),
                       n_cand=int(lens.sum()), n_jobs=int(poses.sum()), n_targets=n_targets, **common)


def device_batch_sym(raw_batch, device, res, use_xyz=False, recentre=True, reference_indexing=True):
    """A RawSymBatch -> ``(id_scans, coords4, feats, sym, scale, obj, cls)`` on ``device``: exactly what
    ``collate_sym([ds[i] ...], reference_indexing)`` moved to the device (``sym_to_device``) gives, with the training script's
    ``feats[:, -3:] * 2 - 1`` applied when ``recentre``.  On torch's current stream: non-blocking copies, the voxelisation
    without its host wait (ME.utils.quantize_nowait), cv_sp_sym_rows_f32 on buffers of the host's upper bounds, then ONE host
    wait that reads N, the rejected count, P, S, J, T, U and max_row from pinned memory; the outputs are slices of those
    buffers.  Rejected points raise as ME.utils.quantize_device does."""
    from . import _lib
    dev = torch.device(device)
    b = _upload(raw_batch, dev, host=("seg_cloud",))
    h_counts = torch.empty(8, dtype=torch.int32, pin_memory=True)
    with torch.cuda.device(dev):
        coords4, index, inverse, quant_counts = me_utils.quantize_nowait(b.points, res, raw_batch.offsets)
        o = me_utils.sym_rows(coords4, index, inverse, quant_counts, b.points, b.rgb, b.owner, b.scale, b.cls, b.colour, b.jitter,
                              b.offsets, b.seg_vertex, b.seg_vptr, b.pose_ptr, b.minv, b.n_targets,
                              reference_indexing=reference_indexing, use_xyz=use_xyz, recentre=recentre, h_counts=h_counts)
        torch.cuda.current_stream(dev).synchronize()                     # the batch's one host wait
    c = dict(zip(_lib.SYM_ROWS_COUNTS, h_counts.tolist()))
    if c["rejected"] != 0:
        me_utils.raise_rejected(c["rejected"])
    n, P, S, U = c["N"], c["P"], c["S"], c["U"]
    sym = SymBatch(o["rows"][:P], o["pseg"][:P], o["seg_ptr"][:S + 1], o["pose_ptr"][:S + 1], o["tgt_ptr"][:S + 1],
                   o["targets"][:c["T"]], o["urow"][:U], o["uptr"][:U + 1], o["upoint"][:P], S, c["J"], c["max_row"])
    return b.id_scans, coords4[:n], o["feats"][:n], sym, o["scale"][:n], o["obj"][:n], o["cls"][:n]


def collate_fn_separate(batch):
    """train_separate.py:78-97: like collate_fn, the per-model label lists stay per scan"""
    id_scans, coords, feats, xyz_labels, scale_labels, obj_labels, class_labels = list(zip(*batch))
    xyz_batch = [[[torch.from_numpy(np.asarray(rows)).long(), [torch.from_numpy(x).float() for x in xyzs]]
                  for rows, xyzs in per_scan] for per_scan in xyz_labels]
    return (id_scans, me_utils.batched_coordinates(coords), torch.from_numpy(np.concatenate(feats, 0)).float(), xyz_batch,
            torch.from_numpy(np.concatenate(scale_labels, 0)).float(),
            torch.from_numpy(np.concatenate(obj_labels, 0)).long(),
            torch.from_numpy(np.concatenate(class_labels, 0)).long())


# ----------------------------------------------------------------------------------------------------------------
# The same labels in a form the device consumes: cv_sym_loss_fwd_f32 / cv_sym_loss_bwd_f32 through
# me.utils.sym_loss, train.separate_loss_packed and train.train_step_separate.

class SymBatch(typing.NamedTuple):
    """``collate_sym``'s packed symmetry labels: CPU tensors and three host ints, so DataLoader workers and ``pin_memory``
    carry it.  A segment is one aligned model of one scan, segments in batch order (scan, then model order):
    ``rows`` int32 [P] output row of each labelled point, ``pseg`` int32 [P] its segment, ``seg_ptr`` int32 [S+1] (points of
    segment s: rows[seg_ptr[s]:seg_ptr[s+1]]), ``pose_ptr`` int32 [S+1] prefix of the pose counts (J = pose_ptr[S] jobs),
    ``tgt_ptr`` int32 [S+1] first row of segment s's block [n_pose][len][3] in ``targets`` float32 [T, 3] (the dataset's
    fp32 bits, untouched); the inverse list of the backward: ``urow`` int32 [U] distinct rows ascending, ``uptr`` int32
    [U+1], ``upoint`` int32 [P] the points of each row in ascending point index."""
    rows: torch.Tensor
    pseg: torch.Tensor
    seg_ptr: torch.Tensor
    pose_ptr: torch.Tensor
    tgt_ptr: torch.Tensor
    targets: torch.Tensor
    urow: torch.Tensor
    uptr: torch.Tensor
    upoint: torch.Tensor
    n_segments: int
    n_jobs: int
    max_row: int          # the largest entry of rows (-1 without segments): what the caller compares with the output's rows


def pack_sym(xyz_labels, scan_sizes, reference_indexing=True):
    """Per scan a list of ``[rows, [xyz under each pose]]`` (ScanNetXYZProbSymDataset's labels; numpy or torch) -> SymBatch.
    ``scan_sizes``: rows of every scan.  reference_indexing: ``rows`` are the scan's own row numbers (what
    train_separate.py:270 indexes the BATCH output with); False: offset by the rows of the scans in front.
    A segment without a surviving row is DROPPED (the reference's mean over an empty tensor is NaN and poisons the batch);
    a negative row raises."""
    as_np = lambda a: a.numpy() if torch.is_tensor(a) else np.asarray(a)
    first = np.cumsum([0] + [int(n) for n in scan_sizes[:-1]])
    rows, targets, lens, poses = [], [], [], []
    for j, per_scan in enumerate(xyz_labels):
        for r, xyzs in per_scan:
            r = as_np(r).astype(np.int64).reshape(-1)
            if r.size == 0:
                continue
            if r.min() < 0:
                raise ValueError("collate_sym: negative row %d in a segment of scan %d" % (int(r.min()), j))
            if len(xyzs) == 0:
                raise ValueError("collate_sym: a segment of scan %d has no pose" % j)
            xs = [as_np(x) for x in xyzs]
            if any(x.shape != (r.size, 3) for x in xs):
                raise ValueError("collate_sym: targets of a segment of scan %d are not [%d, 3]" % (j, r.size))
            rows.append(r if reference_indexing else r + first[j])
            targets.extend(np.ascontiguousarray(x, np.float32) for x in xs)
            lens.append(r.size)
            poses.append(len(xs))
    S = len(lens)
    lens, poses = np.asarray(lens, np.int64), np.asarray(poses, np.int64)
    rows = np.concatenate(rows) if S else np.zeros(0, np.int64)
    prefix = lambda a: np.concatenate([[0], np.cumsum(a)])
    seg_ptr, pose_ptr, tgt_ptr = prefix(lens), prefix(poses), prefix(lens * poses)
    if max(int(tgt_ptr[-1]), int(rows.max()) if S else 0) >= 2 ** 31:
        raise ValueError("collate_sym: the batch does not fit int32 pointers")
    order = np.argsort(rows, kind="stable")                     # points by row; equal rows keep their ascending point index
    urow, counts = np.unique(rows, return_counts=True)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32))
    return SymBatch(i32(rows), i32(np.repeat(np.arange(S), lens)), i32(seg_ptr), i32(pose_ptr), i32(tgt_ptr),
                    torch.from_numpy(np.concatenate(targets, 0) if S else np.zeros((0, 3), np.float32)),
                    i32(urow), i32(prefix(counts)), i32(order), S, int(pose_ptr[-1]), int(rows.max()) if S else -1)


def unpack_sym(sym):
    """the flat list of ``[rows int64, [targets per pose]]`` a SymBatch holds, in segment order (rows as packed)"""
    out = []
    for s in range(sym.n_segments):
        a, b, t = int(sym.seg_ptr[s]), int(sym.seg_ptr[s + 1]), int(sym.tgt_ptr[s])
        n_pose = int(sym.pose_ptr[s + 1] - sym.pose_ptr[s])
        out.append([sym.rows[a:b].long(), [sym.targets[t + p * (b - a):t + (p + 1) * (b - a)] for p in range(n_pose)]])
    return out


def collate_sym(batch, reference_indexing=True):
    """``collate_fn_separate`` with the per-model label lists packed for the device: ``(id_scans, coords4, feats, sym,
    scale_labels, obj_labels, class_labels)`` with ``sym`` a SymBatch (``pack_sym``: a segment without a surviving row is
    dropped, a negative row raises).  The scan sizes are known here, so reference_indexing=False needs no bincount later."""
    id_scans, coords, feats, xyz_labels, scale_labels, obj_labels, class_labels = list(zip(*batch))
    sym = pack_sym(xyz_labels, [len(c) for c in coords], reference_indexing)
    return (id_scans, me_utils.batched_coordinates(coords), torch.from_numpy(np.concatenate(feats, 0)).float(), sym,
            torch.from_numpy(np.concatenate(scale_labels, 0)).float(),
            torch.from_numpy(np.concatenate(obj_labels, 0)).long(),
            torch.from_numpy(np.concatenate(class_labels, 0)).long())


def sym_to_device(sym, dev):
    """the SymBatch with its tensors on ``dev`` (non-blocking copies: no host wait from pinned memory)"""
    return _upload(sym, dev)


class SyntheticSymDataset(torch.utils.data.Dataset):
    """``ScanNetXYZProbSymDataset``-shaped items from ``make_scene`` scenes, for the profile and scripts/train_separate.py
    without ScanNet files: one segment per distinct object (object rows grouped by their (scale_labels, class) rows), the
    symmetry classes none / UP_2 / UP_4 / UP_INF cycling over the segments; the targets of a pose are
    ``xyz0 @ Ry(a).T`` evaluated in fp64 and cast once."""

    def __init__(self, n_scenes=6, n_points=20000, res=0.03, seed0=0, **scene_kw):
        self.scenes = SyntheticScanDataset(n_scenes, n_points, res, seed0, **scene_kw)

    def __len__(self):
        return len(self.scenes)

    def __getitem__(self, index):
        id_scan, coords, feats, xyz, scale, cls = self.scenes[index]
        obj_rows = np.nonzero(cls != 9)[0]
        key = np.concatenate([scale[obj_rows], cls[obj_rows, None].astype(np.float32)], 1)
        _, inverse = np.unique(key, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        syms = [None, "__SYM_ROTATE_UP_2", "__SYM_ROTATE_UP_4", "__SYM_ROTATE_UP_INF"]
        xyz_labels = []
        for k in range(int(inverse.max()) + 1 if obj_rows.size else 0):
            rows = obj_rows[inverse == k]
            x0 = xyz[rows].astype(np.float64)
            angles = [0.0] + list(SYMMETRY_ANGLES.get(syms[k % 4], []))
            xyz_labels.append([rows, [(x0 @ _roty4(a)[:3, :3].T).astype(np.float32) for a in angles]])
        obj = (cls != 9).astype(np.int32)
        return id_scan, coords, feats, xyz_labels, scale, obj, np.where(cls == 9, 0, cls).astype(np.int32)
