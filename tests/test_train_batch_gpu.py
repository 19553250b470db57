"""Training batches built on the device from raw scans (data.device_batch = ME.utils.quantize_batch + ONE
cv_sp_scan_rows_f32 launch), every array compared as bits: against the goldens of the reference's own class
(tests/golden/data_ref.npz) and against the host path ``collate_fn([ds[i] ...])`` moved to the device.  The cases and
their datasets are those of tests/test_train_batch.py, which checks on the CPU that the kernel's formulas, restated in
numpy, give the host path's bits for each of them."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data
from canonicalvoting_amd.me import utils as me_utils
from tests import test_train_batch as cases
from tests.golden.make_data_golden import mini_cfg

pytestmark = pytest.mark.gpu

RES = cases.RES
GOLD = cases.GOLD
# cv_sp_scan_rows_f32 gives every output at most 512 workgroups of 256 threads (MAX_BLOCKS, csrc/train_rows.hip):
# from 131 073 elements on a loop takes a second trip.  The shortest loop (cls) has N elements.
ONE_TRIP = 512 * 256


def same_bits(a, b):
    """two tensors (either device): same shape, dtype and bytes"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8))


def assert_same_batch(got, want, what):
    """got: device_batch's tuple; want: collate_fn's tuple (CPU)"""
    assert tuple(got[0]) == tuple(want[0]), what
    for name, g, w in zip(cases.NAMES, got[1:], want[1:]):
        assert g.is_cuda and same_bits(g, w), (what, name, tuple(g.shape), g.dtype, tuple(w.shape), w.dtype)


def recentred(host):
    """the host batch as the training script feeds it: ``feats[:, -3:] * 2 - 1``"""
    feats = host[2].clone()
    feats[:, -3:] = feats[:, -3:] * 2.0 - 1.0
    return host[:2] + (feats,) + host[3:]


def gold_batch(tags):
    out = [[str(GOLD[t + "_id"]) for t in tags]]
    out.append(torch.from_numpy(np.concatenate([np.concatenate([np.full((GOLD[t + "_coords"].shape[0], 1), b, np.int32),
                                                                GOLD[t + "_coords"].astype(np.int32)], 1)
                                                for b, t in enumerate(tags)])))
    for name in ("feats", "xyz", "scale"):
        out.append(torch.from_numpy(np.concatenate([GOLD[t + "_" + name] for t in tags])))
    out.append(torch.from_numpy(np.concatenate([GOLD[t + "_cls"] for t in tags]).astype(np.int64)))
    return tuple(out)


@pytest.fixture(scope="module")
def golden_raws():
    return cases.golden_raws(set(cases.GOLDEN_CONFIGS))


@pytest.mark.parametrize("tags", [("plain0",), ("plain1",), ("aug0",), ("aug1",), ("xyz1",), ("cat_others",), ("cat_02871439",),
                                  ("plain0", "plain1"), ("aug0", "aug1"), ("cat_02871439", "cat_others"), ("plain1", "aug0")])
def test_device_batch_equals_the_reference_goldens(cuda, built_lib, golden_raws, tags):
    """B = 1 and B = 2; cat_02871439 is all background with an empty model table (alone: every table pointer is NULL);
    (plain1, aug0) has colour operands for one of its two clouds"""
    use_xyz = tags[0] == "xyz1"
    got = data.device_batch(data.collate_raw([golden_raws[t] for t in tags]), cuda, RES, use_xyz=use_xyz, recentre=False)
    assert_same_batch(got, gold_batch(tags), tags)
    assert got[1].dtype == torch.int32 and got[5].dtype == torch.int64 and got[2].shape[1] == (6 if use_xyz else 3)


def test_device_batch_equals_the_host_path_at_size(cuda, built_lib, tmp_path):
    """3 generated scans of about 70 000 vertices in a room so large that nearly every vertex is its own voxel: N is beyond
    ONE_TRIP, so every grid-stride loop of the kernel takes a second trip.  Overlapping segments, colour + rotation + use_xyz,
    and recentre=True against the script's recentre line."""
    host, raws, _ = cases.dataset_and_raws(tmp_path, cases.big_specs(), dict(augment_color=True, use_xyz=True), True, 31)
    assert host[1].shape[0] > ONE_TRIP
    batch = data.collate_raw(raws)
    assert_same_batch(data.device_batch(batch, cuda, RES, use_xyz=True, recentre=True), recentred(host), "recentred")
    assert_same_batch(data.device_batch(batch, cuda, RES, use_xyz=True, recentre=False), host, "plain")


@pytest.mark.parametrize("name", sorted(cases.small_cases()))
def test_smallest_shapes_equal_the_host_path(cuda, built_lib, tmp_path, name):
    """M = 1; all points in one voxel (N = 1); N = 255 / 256 / 257; no colour (NULL table and jitter); colours pushed past
    both clamps; owner all -1; class 0 (unknown catid) next to 9"""
    specs, kw, augment, seed = cases.small_cases()[name]
    host, raws, _ = cases.dataset_and_raws(tmp_path, specs, kw, augment, seed)
    batch = data.collate_raw(raws)
    use_xyz = kw.get("use_xyz", False)
    assert_same_batch(data.device_batch(batch, cuda, RES, use_xyz=use_xyz, recentre=False), host, name)
    assert_same_batch(data.device_batch(batch, cuda, RES, use_xyz=use_xyz), recentred(host), name + " recentred")
    assert (batch.colour is None) == (not kw.get("augment_color", False)) and (name != "no_colour" or batch.jitter is None)


@pytest.mark.parametrize("tag", ["xyz1", "aug0"])
def test_c_abi_writes_only_its_windows(cuda, built_lib, golden_raws, tag):
    """cv_sp_scan_rows_f32 called directly: destinations are windows of sentinel-filled buffers with row strides above the
    widths and rows beyond N, ``points`` is a column block of a wider tensor; nothing outside the windows changes.
    xyz1: the points in front, no colour operands (NULL table and jitter); aug0: colour operands, width 3"""
    L = _lib.lib()
    raw = golden_raws[tag]
    use_xyz, fw = tag == "xyz1", 6 if tag == "xyz1" else 3
    b = data.collate_raw([raw])
    assert (b.colour is None) == use_xyz
    want = gold_batch((tag,))
    n = want[1].shape[0]
    wide = torch.full((raw.points.shape[0], 5), float("nan"), device=cuda)
    wide[:, 1:4] = b.points.to(cuda)
    points = wide[:, 1:4]                                                   # row stride 5
    coords4, index = me_utils.quantize_batch(points, RES, offsets=[0])
    assert same_bits(coords4, want[1])
    up = lambda t: None if t is None else t.to(cuda)
    rgb, owner, minv, scale, cls, colour, jitter = (up(t) for t in (b.rgb, b.owner, b.minv, b.scale, b.cls, b.colour, b.jitter))
    SENT_F, SENT_I = -12345.5, -0x0123456789ABCDEF
    feats_buf = torch.full((n + 3, 9), SENT_F, device=cuda)
    xyz_buf = torch.full((n + 3, 4), SENT_F, device=cuda)
    scale_buf = torch.full((n + 3, 7), SENT_F, device=cuda)
    cls_buf = torch.full((n + 3, 2), SENT_I, dtype=torch.int64, device=cuda)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    d = _lib.ScanRowsDesc(vp(coords4), vp(index), n, points.shape[0], vp(points), 5, vp(rgb), vp(owner), vp(minv), vp(scale),
                          vp(cls), cls.shape[0], vp(colour), vp(jitter), 1, int(use_xyz), 0, vp(feats_buf), 9, vp(xyz_buf), 4,
                          vp(scale_buf), 7, vp(cls_buf), 2)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert L.cv_sp_scan_rows_f32(ctypes.byref(d), stream) == 0, L.cv_last_error()
    torch.cuda.synchronize()
    for buf, w, ref in ((feats_buf, fw, want[2]), (xyz_buf, 3, want[3]), (scale_buf, 3, want[4]), (cls_buf, 1, want[5])):
        assert same_bits(buf[:n, :w], ref.reshape(n, w))
        sent = SENT_I if buf.dtype == torch.int64 else SENT_F
        assert bool((buf[:n, w:] == sent).all()) and bool((buf[n:] == sent).all())
    # the same through ME.utils.scan_rows with `out` windows
    outs = (feats_buf[:n, 2:2 + fw], xyz_buf[:n, 1:4], scale_buf[:n, 4:7], cls_buf[:n, 1])
    for t in (feats_buf, xyz_buf, scale_buf):
        t.fill_(SENT_F)
    cls_buf.fill_(SENT_I)
    got = me_utils.scan_rows(coords4, index, points, rgb, owner, minv, scale, cls, colour, jitter, use_xyz=use_xyz, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    assert same_bits(outs[0], want[2]) and same_bits(outs[1], want[3]) and same_bits(outs[2], want[4]) and same_bits(outs[3], want[5])
    assert bool((feats_buf[:, :2] == SENT_F).all()) and bool((feats_buf[:, 2 + fw:] == SENT_F).all()) and bool((feats_buf[n:] == SENT_F).all())
    assert bool((xyz_buf[:, 0] == SENT_F).all()) and bool((scale_buf[:, :4] == SENT_F).all()) and bool((scale_buf[n:] == SENT_F).all())
    assert bool((cls_buf[:, 0] == SENT_I).all()) and bool((cls_buf[n:] == SENT_I).all())
    with pytest.raises(ValueError, match="come together"):
        me_utils.scan_rows(coords4, index, points, rgb, owner, minv, scale, cls, None, torch.zeros(points.shape[0], dtype=torch.float64, device=cuda))


def test_same_bytes_on_every_run_and_on_a_side_stream(cuda, built_lib, golden_raws):
    batch = data.collate_raw([golden_raws["aug0"], golden_raws["aug1"]])
    first = data.device_batch(batch, cuda, RES)
    second = data.device_batch(batch, cuda, RES)
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        third = data.device_batch(batch, cuda, RES)
    side.synchronize()
    torch.cuda.synchronize()
    for other in (second, third):
        assert all(same_bits(a, b) for a, b in zip(first[1:], other[1:]))


def test_one_training_step_from_the_device_batch_gives_the_host_batch_loss_bits(cuda, built_lib):
    from canonicalvoting_amd import train
    from canonicalvoting_amd.minkunet import MinkUNet34C
    ds = data.ScanNetXYZProbMultiDataset(mini_cfg(), training=False, augment=False)
    host = recentred(data.collate_fn([ds[0], ds[1]]))
    dev = data.device_batch(data.collate_raw([ds.raw_item(0), ds.raw_item(1)]), cuda, RES)
    losses = []
    for _, coords, feats, xyz, scale, cls in (host, dev):
        torch.manual_seed(0)
        model = MinkUNet34C(3, 6 * 9 + 9 + 1).to(cuda).train()
        opt = train.make_optimizer(model, lr=1e-3)
        loss, _ = train.train_step(model, opt, coords.to(cuda), feats.to(cuda), xyz.to(cuda), scale.to(cuda), cls.to(cuda))
        losses.append(np.float32(float(loss)).tobytes() if not torch.is_tensor(loss) else loss.detach().cpu().numpy().tobytes())
    assert np.isfinite(np.frombuffer(losses[0], np.float32)).all() and losses[0] == losses[1]
