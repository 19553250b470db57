"""Voxelisation on the device (cv_sp_quantize_f32 / _f64 through ME.utils.sparse_quantize(device=...), quantize_batch and
pipeline.detect_points) against the host numpy path of ME.utils.sparse_quantize.  Every comparison is between integers
or gathered rows: all of them are exact.  Expected values come from the numpy path only."""
import numpy as np
import pytest
import torch

from canonicalvoting_amd import me as ME
from canonicalvoting_amd import pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.me import utils as me_utils
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_raw_scene, synth_predictions

pytestmark = pytest.mark.gpu

ROOM = np.array([5.2, 2.6, 5.2])


def surface_cloud(seed, m, dtype=np.float32, shift=0.0):
    """points on the faces of a 5.2 x 2.6 x 5.2 m room with 5 mm jitter, in scan order along the faces"""
    rng = np.random.default_rng(seed)
    p = rng.random((m, 3)) * ROOM
    face = rng.integers(0, 3, m)
    p[np.arange(m), face] = np.where(rng.random(m) < 0.5, 0.0, ROOM[face])
    p += rng.normal(0, 0.005, p.shape) + shift
    return p.astype(dtype)


def host(points, q):
    """(coords [N,3], index [N]) of the numpy path"""
    assert isinstance(points, np.ndarray)
    return me_utils.sparse_quantize(points, quantization_size=q, return_index=True)


def check_against_host(p, q, cuda, dev_points=None, tag=""):
    want_c, want_i = host(p, q)
    d = torch.from_numpy(p).to(cuda) if dev_points is None else dev_points
    coords, index = me_utils.sparse_quantize(d, quantization_size=q, return_index=True)
    assert coords.is_cuda and index.is_cuda and coords.dtype == torch.int32 and coords.shape == (want_i.size, 3), tag
    assert np.array_equal(index.cpu().numpy(), want_i), tag + ": index"
    assert np.array_equal(coords.cpu().numpy(), want_c), tag + ": coords"
    return coords, index


@pytest.mark.parametrize("q", [0.03, 0.05, None])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000, 300000, 1000000])
def test_device_equals_host(cuda, built_lib, m, dtype, q):
    p = surface_cloud(m, m, dtype)
    if q is None:
        p = np.abs(p)         # (the host path truncates towards zero without a quantization_size, the device floors)
    check_against_host(p, q, cuda, tag="%d points %s q=%s" % (m, np.dtype(dtype).name, q))


@pytest.mark.parametrize("q", [0.03, 0.05])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_negative_coordinates(cuda, built_lib, dtype, q):
    check_against_host(surface_cloud(11, 50000, dtype, shift=-3.7), q, cuda)
    check_against_host(surface_cloud(12, 50000, dtype, shift=-40.0), q, cuda)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_unit_coordinates_without_a_quantization_size(cuda, built_lib, dtype):
    """quantization_size=None on coordinates that are voxel indices already (negative ones included)"""
    p = np.random.default_rng(13).integers(-60, 60, (40000, 3)).astype(dtype)
    check_against_host(p, None, cuda)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_voxel_boundaries(cuda, built_lib, dtype):
    """every coordinate is k * float32(0.03), k in [-300, 300]: the quotient lies at (or one ulp beside) an integer and only
    the correctly rounded division puts it on the side numpy puts it"""
    k = np.arange(-300, 301)
    vals = (k * np.float32(0.03)).astype(np.float32)
    assert vals.dtype == np.float32
    rng = np.random.default_rng(14)
    p = vals[rng.integers(0, vals.size, (60000, 3))]
    p[:601] = vals[:, None]                        # every boundary value at least once on every axis
    p = p.astype(dtype)
    coords, _ = check_against_host(p, 0.03, cuda)
    # the case is not vacuous: some quotients fall below their integer
    qf = np.floor(vals / np.float32(0.03)) if dtype == np.float32 else np.floor(vals.astype(np.float64) / 0.03)
    assert (qf != k).any() and (qf == k).any()
    check_against_host(p, 0.05, cuda)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_voxel_and_all_distinct_voxels(cuda, built_lib, dtype):
    rng = np.random.default_rng(15)
    one = (0.301 + 0.02 * rng.random((5000, 3))).astype(dtype)          # all inside voxel (10, 10, 10)
    coords, index = check_against_host(one, 0.03, cuda)
    assert coords.shape[0] == 1 and int(index[0]) == 0
    g = np.stack(np.meshgrid(np.arange(20), np.arange(15), np.arange(20), indexing="ij"), -1).reshape(-1, 3)
    distinct = ((g[rng.permutation(g.shape[0])] - 7) * 0.03 + 0.015).astype(dtype)
    coords, index = check_against_host(distinct, 0.03, cuda)
    assert coords.shape[0] == distinct.shape[0] and np.array_equal(index.cpu().numpy(), np.arange(distinct.shape[0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strided_input_and_gathered_features(cuda, built_lib, dtype):
    p = surface_cloud(16, 30000, dtype, shift=-1.0)
    wide = torch.zeros((p.shape[0], 7), dtype=torch.from_numpy(p).dtype, device=cuda)
    wide[:, 2:5] = torch.from_numpy(p).to(cuda)
    view = wide[:, 2:5]
    assert not view.is_contiguous()
    check_against_host(p, 0.03, cuda, dev_points=view, tag="row-strided view")
    every_other = torch.zeros((p.shape[0], 6), dtype=wide.dtype, device=cuda)
    every_other[:, ::2] = torch.from_numpy(p).to(cuda)
    check_against_host(p, 0.03, cuda, dev_points=every_other[:, ::2], tag="column-strided view")
    feats = np.random.default_rng(17).random((p.shape[0], 3)).astype(np.float32)
    labels = np.random.default_rng(18).integers(0, 10, p.shape[0])
    wc, wf, wl = me_utils.sparse_quantize(p, feats, labels, quantization_size=0.03)
    c, f, l = me_utils.sparse_quantize(view, torch.from_numpy(feats).to(cuda), torch.from_numpy(labels), quantization_size=0.03)
    assert c.is_cuda and f.is_cuda and l.is_cuda
    assert np.array_equal(c.cpu().numpy(), wc) and np.array_equal(f.cpu().numpy(), wf) and np.array_equal(l.cpu().numpy(), wl)


def test_reference_call_shape_of_the_sunrgbd_caller(cuda, built_lib):
    """sunrgbd/brnetcanon.py:218-225: CPU cloud in, device='cuda', then coord.float() and batched_coordinates"""
    pc = torch.from_numpy(surface_cloud(19, 20000))
    wc, wf = me_utils.sparse_quantize(pc.numpy(), features=pc.numpy(), quantization_size=0.03)
    coord, feat = me_utils.sparse_quantize(pc.cpu(), features=pc.cpu(), quantization_size=0.03, device="cuda")
    assert coord.is_cuda and feat.is_cuda and feat.dtype == torch.float32
    assert np.array_equal(coord.cpu().numpy(), wc) and np.array_equal(feat.cpu().numpy(), wf)
    b = me_utils.batched_coordinates([coord.float(), coord.float()])
    assert b.is_cuda and b.dtype == torch.int32 and b.shape == (2 * wc.shape[0], 4)
    assert torch.equal(b[wc.shape[0]:, 1:], coord) and int(b[-1, 0]) == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [65, 300000])
def test_inverse(cuda, built_lib, m, dtype):
    p = surface_cloud(20, m, dtype, shift=-2.2)
    q = 0.03
    coords, index, inverse = me_utils.sparse_quantize(torch.from_numpy(p).to(cuda), quantization_size=q, return_index=True,
                                                      return_inverse=True)
    coords, index, inverse = coords.cpu().numpy(), index.cpu().numpy(), inverse.cpu().numpy()
    wc, wi = host(p, q)
    assert np.array_equal(coords, wc) and np.array_equal(index, wi)
    assert inverse.shape == (m,) and inverse.min() >= 0 and inverse.max() < index.size
    assert np.array_equal(coords[inverse], np.floor(p / q).astype(np.int32))
    assert np.array_equal(inverse[index], np.arange(index.size))            # index[inverse[i]] == i for the rows of index
    assert np.all(index[inverse] <= np.arange(m))


def test_cloud_above_2_20_points(cuda, built_lib):
    """m = 2^20 + 4097: the scan kernels take two points per thread (per = 2) in 515 blocks; below 2^20 + 1 points they
    take one"""
    m, q = (1 << 20) + 4097, 0.03
    p = surface_cloud(25, m)
    wc, wi = host(p, q)
    check_against_host(p, q, cuda, tag="%d points" % m)
    coords, index, inverse = me_utils.sparse_quantize(torch.from_numpy(p).to(cuda), quantization_size=q, return_index=True,
                                                      return_inverse=True)
    coords, index, inverse = coords.cpu().numpy(), index.cpu().numpy(), inverse.cpu().numpy()
    assert np.array_equal(coords, wc) and np.array_equal(index, wi)
    assert inverse.shape == (m,) and inverse.min() >= 0 and inverse.max() < index.size
    assert np.array_equal(coords[inverse], np.floor(p / q).astype(np.int32))
    assert np.array_equal(inverse[index], np.arange(index.size))
    assert np.all(index[inverse] <= np.arange(m))


def test_batch_of_three_clouds(cuda, built_lib):
    a = surface_cloud(21, 1000)
    b = a[:257].copy()                               # the same points in another cloud: separate voxels
    c = surface_cloud(22, 5000, shift=-1.5)
    clouds = [a, b, c]
    per = [host(x, 0.03) for x in clouds]
    want_c4 = me_utils.batched_coordinates([x[0] for x in per]).numpy()
    off = np.cumsum([0] + [x.shape[0] for x in clouds[:-1]])
    want_i = np.concatenate([x[1] + o for x, o in zip(per, off)])
    dev = [torch.from_numpy(x).to(cuda) for x in clouds]
    c4, index, inverse = me_utils.quantize_batch(dev, 0.03, return_inverse=True)
    assert c4.dtype == torch.int32 and c4.shape == (want_i.size, 4)
    assert np.array_equal(c4.cpu().numpy(), want_c4) and np.array_equal(index.cpu().numpy(), want_i)
    allp = np.concatenate(clouds)
    batch = np.repeat(np.arange(3), [x.shape[0] for x in clouds])
    got = c4.cpu().numpy()[inverse.cpu().numpy()]
    assert np.array_equal(got[:, 1:], np.floor(allp / 0.03).astype(np.int32)) and np.array_equal(got[:, 0], batch)
    n_b = per[1][1].size
    assert (c4[:, 0] == 1).sum().item() == n_b and n_b > 0
    # one tensor plus row offsets
    c4b, indexb = me_utils.quantize_batch(torch.cat(dev), 0.03, offsets=off.tolist())
    assert torch.equal(c4b, c4) and torch.equal(indexb, index)
    # the set goes into a SparseTensor as it is
    ME.CoordinateManager(c4, num_levels=1, check=True)


def test_rejected_points_raise_and_leave_the_stream_usable(cuda, built_lib):
    p = surface_cloud(23, 2000)
    bad = p.copy()
    bad[10, 1] = np.nan
    bad[700, 0] = np.inf
    bad[1999, 2] = 40000 * 0.03
    for dtype in (np.float32, np.float64):
        with pytest.raises(RuntimeError, match=r"\b3 points rejected"):
            me_utils.sparse_quantize(torch.from_numpy(bad.astype(dtype)).to(cuda), quantization_size=0.03)
        check_against_host(p.astype(dtype), 0.03, cuda, tag="after a rejected cloud")
    # the edge of the window itself is accepted, one voxel beyond is not
    edge = np.array([[32703.5, -32704.0, 0.0], [1.0, 2.0, 3.0]], np.float64)
    coords = me_utils.sparse_quantize(torch.from_numpy(edge).to(cuda))
    assert coords.cpu().tolist() == [[32703, -32704, 0], [1, 2, 3]]
    for beyond in ([32704.0, 0.0, 0.0], [0.0, -32704.5, 0.0], [0.0, 0.0, 1e30], [-1e300, 0.0, 0.0]):
        with pytest.raises(RuntimeError, match=r"\b1 points rejected"):
            me_utils.sparse_quantize(torch.tensor([beyond, [0.0, 0.0, 0.0]], dtype=torch.float64, device=cuda))


def test_bit_reproducible_and_stream_independent(cuda, built_lib):
    p = torch.from_numpy(surface_cloud(1000000, 1000000)).to(cuda)
    run = lambda: me_utils.sparse_quantize(p, quantization_size=0.03, return_index=True, return_inverse=True)
    a = [t.cpu().numpy().tobytes() for t in run()]
    b = [t.cpu().numpy().tobytes() for t in run()]
    assert a == b
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        c = [t.cpu().numpy().tobytes() for t in run()]
    torch.cuda.current_stream(cuda).wait_stream(side)
    assert a == c


def test_device_coordinates_go_straight_into_a_sparse_tensor(cuda, built_lib):
    p = torch.from_numpy(surface_cloud(24, 100000, shift=-1.0)).to(cuda)
    c4, index = me_utils.quantize_batch(p, 0.03)
    assert c4.shape[1] == 4 and int(c4[:, 0].max()) == 0
    cm = ME.CoordinateManager(c4, check=True)                 # raises on duplicates or rows outside the key window
    assert cm.counts[0] == c4.shape[0] and all(cm.counts[i] >= cm.counts[i + 1] > 0 for i in range(4))
    x = ME.SparseTensor(p[index.long()].float(), c4, device=cuda)
    assert x.coordinate_manager.kernel_map(3, 1).shape == (c4.shape[0], 27)


def test_detect_points_equals_host_quantise_plus_detect_scene_c(cuda, built_lib):
    res = 0.03
    raw_scene = make_raw_scene(0, 300000)
    torch.manual_seed(0)
    model = MinkUNet34C(3, 64).to(cuda).eval()
    hv = HoughVoting(res, 120)
    feats_raw = (raw_scene.feats * 2 - 1).astype(np.float32)
    pred_raw = synth_predictions(raw_scene)
    # host: quantise with numpy, gather, upload
    wc, wi = host(raw_scene.points, res)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    c4 = torch.cat([torch.zeros((wi.size, 1), dtype=torch.int32), torch.from_numpy(wc)], 1).to(cuda)
    want = pipeline.detect_scene_c(model, hv, c4, t(feats_raw[wi]), res, predictions=tuple(t(a[wi]) for a in pred_raw),
                                   thresh_high=60)
    got = pipeline.detect_points(model, hv, t(raw_scene.points), t(feats_raw), res, predictions=tuple(t(a) for a in pred_raw),
                                 return_inverse=True, thresh_high=60)
    (wd, wr, wy), (gd, gr, gy, index, inverse) = want, got
    assert np.array_equal(index.cpu().numpy(), wi)
    assert np.array_equal(wc[inverse.cpu().numpy()], np.floor(raw_scene.points / res).astype(np.int32))
    assert len(wr["boxes"]) >= 1 and len(wd) >= 1               # the equality below says something
    for k in ("cand_idx", "verdict", "boxes", "scores", "classes"):
        assert wr[k].tobytes() == gr[k].tobytes(), k
    assert len(wd) == len(gd)
    for (c0, b0, s0), (c1, b1, s1) in zip(wd, gd):
        assert c0 == c1 and s0 == s1 and b0.tobytes() == b1.tobytes()
    assert torch.equal(wy, gy)
    assert len(pipeline.detect_points(model, hv, t(raw_scene.points), t(feats_raw), res, thresh_high=60)) == 4
