"""The per-category trainer's batch built on the device from raw scans (cv_sp_sym_rows_f32 behind the voxeliser, DESIGN.md
4.5c), every array compared as bits: with the numpy restatement of the contract, with the host batch
``collate_sym([ds[i] ...])`` and with the goldens of the reference's own class.  The kernel goes through the C ABI into
sentinel-filled buffers of upper-bound size: everything behind the written counts must still be the sentinel.  The cases
and their datasets are those of tests/test_sym_batch.py, which checks on the CPU that the restatement gives the host
path's bits for each of them and that none of their targets is an fp32 rounding tie."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data
from canonicalvoting_amd.me import utils as me_utils
from tests import test_sym_batch as cases

pytestmark = pytest.mark.gpu

RES = cases.RES
SENT_I, SENT_F, SENT_L = -0x01234567, -12345.5, -0x0123456789ABCDEF
COUNTS = _lib.SYM_ROWS_COUNTS


def run_c_abi(dev, b, reference_indexing=True, use_xyz=False, recentre=False):
    """cv_sp_sym_rows_f32 behind quantize_nowait on torch's current stream, into sentinel-filled upper-bound buffers;
    returns (buffers, counts dict) after a wait.  The row arrays get strides above their widths."""
    L = _lib.lib()
    up = lambda t: None if t is None else t.to(dev)
    points, rgb, owner, scale, cls, seg_vertex, seg_vptr, pose_ptr, minv, colour, jitter, offsets = (
        up(t) for t in (b.points, b.rgb, b.owner, b.scale, b.cls, b.seg_vertex, b.seg_vptr, b.pose_ptr, b.minv, b.colour, b.jitter,
                        b.offsets))
    m, q, s0, fw = points.shape[0], b.n_cand, seg_vptr.shape[0] - 1, 6 if use_xyz else 3
    coords4, index, inverse, qcounts = me_utils.quantize_nowait(points, RES, b.offsets)
    full = lambda shape, v, dt=torch.int32: torch.full(shape, v, dtype=dt, device=dev)
    o = dict(rows=full((q + 3,), SENT_I), pseg=full((q + 3,), SENT_I), seg_ptr=full((s0 + 4,), SENT_I), pose_ptr=full((s0 + 4,), SENT_I),
             tgt_ptr=full((s0 + 4,), SENT_I), targets=full((b.n_targets + 3, 3), SENT_F, torch.float32), urow=full((q + 3,), SENT_I),
             uptr=full((q + 4,), SENT_I), upoint=full((q + 3,), SENT_I), feats=full((m + 3, fw + 2), SENT_F, torch.float32),
             scale=full((m + 3, 5), SENT_F, torch.float32), obj=full((m + 3,), SENT_L, torch.int64), cls=full((m + 3,), SENT_L, torch.int64),
             counts=full((8,), SENT_I))
    h_counts = torch.full((8,), SENT_I, dtype=torch.int32).pin_memory()
    ws = torch.empty(int(L.cv_sp_sym_rows_workspace_bytes(m, q, s0, offsets.shape[0])), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    ptr = lambda t: vp(t.data_ptr()) if t is not None and t.numel() else None
    d = _lib.SymRowsDesc(ptr(coords4), ptr(index), ptr(inverse), ptr(qcounts), m, ptr(points), 3, ptr(rgb), ptr(owner), ptr(scale),
                         ptr(cls), cls.shape[0], ptr(colour), ptr(jitter), ptr(offsets), offsets.shape[0], ptr(seg_vertex), q,
                         ptr(seg_vptr), ptr(pose_ptr), s0, ptr(minv), minv.shape[0], b.n_targets, int(reference_indexing),
                         int(use_xyz), int(recentre), ptr(o["rows"]), ptr(o["pseg"]), ptr(o["seg_ptr"]), ptr(o["pose_ptr"]),
                         ptr(o["tgt_ptr"]), ptr(o["targets"]), ptr(o["urow"]), ptr(o["uptr"]), ptr(o["upoint"]), ptr(o["feats"]), fw + 2,
                         ptr(o["scale"]), 5, ptr(o["obj"]), ptr(o["cls"]), ptr(o["counts"]), vp(h_counts.data_ptr()), vp(ws.data_ptr()),
                         ws.numel())
    stream = torch.cuda.current_stream(dev)
    assert L.cv_sp_sym_rows_f32(ctypes.byref(d), vp(stream.cuda_stream)) == 0, L.cv_last_error()
    stream.synchronize()
    c = dict(zip(COUNTS, h_counts.tolist()))
    assert o["counts"].cpu().tolist() == h_counts.tolist()
    o["coords4"] = coords4[:max(c["N"], 0)]                                # (the voxeliser's own buffer: not sentinel-filled behind N)
    return o, c


def check_against(o, c, want, fw):
    """the written prefixes equal ``want`` (a dict as cases.restate returns) bit for bit; behind them, the sentinel"""
    n, P, S, T, U = c["N"], c["P"], c["S"], c["T"], c["U"]
    assert c["rejected"] == 0 and n == want["coords4"].shape[0]
    assert (S, c["J"], c["max_row"], P, T, U) == (want["n_segments"], want["n_jobs"], want["max_row"], want["rows"].shape[0],
                                                   want["targets"].shape[0], want["urow"].shape[0])
    cpu = {k: v.cpu() for k, v in o.items()}
    for name, cnt in (("rows", P), ("pseg", P), ("upoint", P), ("urow", U), ("uptr", U + 1), ("seg_ptr", S + 1), ("pose_ptr", S + 1),
                      ("tgt_ptr", S + 1), ("targets", T)):
        assert cases.same_bits(cpu[name][:cnt].numpy(), want[name]), name
        sent = SENT_F if name == "targets" else SENT_I
        assert bool((cpu[name][cnt:] == sent).all()), name + ": written behind its count"
    assert cases.same_bits(cpu["coords4"][:n].numpy(), want["coords4"])
    for name, w in (("feats", fw), ("scale", 3)):
        assert cases.same_bits(cpu[name][:n, :w].numpy(), want[name]), name
        assert bool((cpu[name][n:] == SENT_F).all()) and bool((cpu[name][:, w:] == SENT_F).all()), name
    for name in ("obj", "cls"):
        assert cases.same_bits(cpu[name][:n].numpy(), want[name]), name
        assert bool((cpu[name][n:] == SENT_L).all()), name


@pytest.mark.parametrize("name", sorted(cases.cases()))
def test_generated_cases_equal_the_restatement_and_the_host_batch(cuda, built_lib, tmp_path, name):
    case = cases.cases()[name]
    use_xyz = case[1].get("use_xyz", False)
    fw = 6 if use_xyz else 3
    for ref in (True, False):
        host, b, _ = cases.host_and_raw(tmp_path / str(ref), case, ref)
        want = cases.restate(b, RES, use_xyz=use_xyz, reference_indexing=ref)
        cases.assert_equals_host(host, want, name)                          # the expected values are the host batch's
        o, c = run_c_abi(cuda, b, reference_indexing=ref, use_xyz=use_xyz)
        check_against(o, c, want, fw)
    o, c = run_c_abi(cuda, b, reference_indexing=False, use_xyz=use_xyz, recentre=True)
    check_against(o, c, cases.restate(b, RES, use_xyz=use_xyz, recentre=True, reference_indexing=False), fw)


def assert_same_batch(got, want, what):
    """got: device_batch_sym's tuple; want: collate_sym's tuple (CPU)"""
    assert tuple(got[0]) == tuple(want[0]), what
    d = {k: getattr(got[3], k).cpu().numpy() for k in cases.SYM_FIELDS}
    assert all(getattr(got[3], k).is_cuda for k in cases.SYM_FIELDS) and got[1].is_cuda
    d.update(coords4=got[1].cpu().numpy(), feats=got[2].cpu().numpy(), scale=got[4].cpu().numpy(), obj=got[5].cpu().numpy(),
             cls=got[6].cpu().numpy(), n_segments=got[3].n_segments, n_jobs=got[3].n_jobs, max_row=got[3].max_row)
    cases.assert_equals_host(want, d, what)


@pytest.mark.parametrize("tag", ["sym0", "symaug1"])
def test_device_batch_sym_equals_the_reference_goldens(cuda, built_lib, tag):
    b = data.collate_raw_sym([cases.golden_raw(tag)])
    for ref in (True, False):
        got = data.device_batch_sym(b, cuda, RES, recentre=False, reference_indexing=ref)
        assert_same_batch(got, data.collate_sym([cases.gold_item(tag)], reference_indexing=ref), tag)
    o, c = run_c_abi(cuda, b)
    check_against(o, c, cases.restate(b, RES), 3)


def test_same_bytes_on_every_run_and_on_a_side_stream(cuda, built_lib, tmp_path):
    _, b, _ = cases.host_and_raw(tmp_path, cases.cases()["three_scans"])
    first, c1 = run_c_abi(cuda, b)
    second, c2 = run_c_abi(cuda, b)
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        third, c3 = run_c_abi(cuda, b)
    side.synchronize()
    torch.cuda.synchronize()
    assert c1 == c2 == c3 and c1["U"] < c1["P"]                            # rows with several points: the atomic slots get sorted
    for other in (second, third):
        for k in first:
            assert cases.same_bits(first[k].cpu().numpy(), other[k].cpu().numpy()), k


def test_device_batch_sym_end_to_end_with_one_host_synchronisation(cuda, built_lib, tmp_path, monkeypatch):
    case = cases.cases()["three_scans"]
    waits = []
    for owner, name in ((torch.cuda, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"),
                        (torch.cuda.Stream, "wait_event"), (torch.cuda.Event, "wait")):
        orig = getattr(owner, name)
        monkeypatch.setattr(owner, name, (lambda orig, name: lambda *a, **k: (waits.append(name), orig(*a, **k))[1])(orig, name))
    for ref in (True, False):
        host, b, _ = cases.host_and_raw(tmp_path / str(ref), case, ref)
        b = b._replace(**{k: v.pin_memory() for k, v in b._asdict().items() if torch.is_tensor(v)})     # as the DataLoader hands it over
        del waits[:]
        got = data.device_batch_sym(b, cuda, RES, reference_indexing=ref)
        assert waits == ["synchronize"], waits
        assert_same_batch(got, cases.recentred(host), ref)
        got = data.device_batch_sym(b, cuda, RES, recentre=False, reference_indexing=ref)
        assert_same_batch(got, host, ref)
    # the tensors feed the loss as they are: contiguous slices of the upper-bound buffers
    assert all(getattr(got[3], k).is_contiguous() for k in cases.SYM_FIELDS) and got[2].is_contiguous()


def test_rejected_points_raise_like_the_voxeliser(cuda, built_lib):
    raw = cases.golden_raw("sym0")
    pts = raw.points.copy()
    pts[5, 1] = np.nan
    with pytest.raises(RuntimeError, match="1 points rejected"):
        data.device_batch_sym(data.collate_raw_sym([raw._replace(points=pts)]), cuda, RES)


ROOM = np.array([1.5, 0.9, 1.5])


def training_specs():
    """three room-shaped scans of about 2 000 rows (2 600 vertices on the six faces of a 1.5 x 0.9 x 1.5 m room, 5 mm
    jitter), four models of every symmetry class each; a model's segment is the vertices within 0.3 m of it, so the models
    overlap and the canonical coordinates stay of order one"""
    out = []
    for i in range(3):
        r = np.random.default_rng(300 + i)
        n = 2600
        w = r.random((n, 3)) * ROOM
        face = r.integers(0, 3, n)
        w[np.arange(n), face] = np.where(r.random(n) < 0.5, 0.0, ROOM[face])
        w += r.normal(0, 0.005, w.shape)
        spec = cases.sym_spec(300 + i, w, [(cases.CHAIR, sym, [0], False) for sym in (cases.NONE, cases.UP2, cases.UP4, cases.INF)])
        for k, mod in enumerate(spec["models"]):
            centre = w[r.integers(0, n)]
            mod["trs"]["translation"] = [float(v) for v in centre]
            spec["segs"][k] = np.flatnonzero(np.abs(w - centre).max(1) < 0.3)
        out.append(spec)
    return out


def test_one_training_step_from_the_device_batch_gives_the_host_batch_bits(cuda, built_lib, tmp_path):
    from canonicalvoting_amd import me as ME
    from canonicalvoting_amd import train
    from canonicalvoting_amd.minkunet import MinkUNet34C
    host, b, _ = cases.host_and_raw(tmp_path, (training_specs(), dict(augment_color=True), True, 300))
    host = cases.recentred(host)
    assert 5000 < host[1].shape[0] < 7800 and host[3].n_segments == 12 and host[3].rows.shape[0] > 1000
    dev = data.device_batch_sym(b, cuda, RES)
    results = []
    for _, coords, feats, sym, scale, obj, _ in (host, dev):
        torch.manual_seed(0)
        model = MinkUNet34C(3, 8).to(cuda).train()
        before = [p.detach().clone() for p in model.parameters()]
        opt = train.make_optimizer(model, lr=1e-3)
        res = train.train_step_separate(model, opt, coords.to(cuda), feats.to(cuda), sym, scale, obj)
        assert res is not None
        torch.cuda.synchronize()
        # a healthy step: inside the fp16 range (the update is not skipped, and no raised flag is left to later steps)
        assert int(ME.range_flag(cuda)) == 0 and sum(not torch.equal(a, b) for a, b in zip(before, model.parameters())) > 50
        loss = res[0].detach().cpu().numpy().tobytes()
        grads = [p.grad.detach().cpu().numpy().tobytes() for p in model.parameters() if p.grad is not None]
        params = [p.detach().cpu().numpy().tobytes() for p in model.parameters()]
        results.append((loss, grads, params))
    assert np.isfinite(np.frombuffer(results[0][0], np.float32)).all() and len(results[0][1]) > 50
    assert results[0][0] == results[1][0], "loss bits differ"
    assert results[0][1] == results[1][1], "a parameter gradient differs"
    assert results[0][2] == results[1][2], "a stepped parameter differs"
