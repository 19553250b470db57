"""Packed symmetry labels (data.collate_sym / SymBatch) and the fp64 oracle of the device pose loss, without a GPU: the
round trip of the layout, the oracle against the golden values of the reference's own lines, the fp32 restatement of the
kernels' sequence inside the derived bounds, named wrong results far outside them, and the decidable minimum of every case
tests/test_sym_loss_gpu.py runs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, data
from tests import sym_loss_ref as ref
from tests.golden.make_loss_golden import make_separate_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_ref.npz")


@pytest.fixture(scope="module")
def mini():
    """(collate_fn_separate batch of the mini dataset's two scans, seeded 8-channel output, scan sizes, raw items)"""
    from tests.golden.make_data_golden import mini_cfg
    ds = data.ScanNetXYZProbSymDataset(mini_cfg(), training=False, augment=False)
    items = [ds[0], ds[1]]
    batch, F = make_separate_inputs()
    return batch, F, [len(it[1]) for it in items], items


@pytest.fixture(scope="module")
def cases():
    return ref.named_cases(256)


@pytest.fixture(scope="module")
def all_cases(cases):
    return {**cases, **ref.golden_cases()[0]}


def test_collate_sym_round_trip(mini):
    batch, _, sizes, items = mini
    flat = [seg for per_scan in batch[3] for seg in per_scan]
    scan_of = [j for j, per_scan in enumerate(batch[3]) for _ in per_scan]
    first = np.cumsum([0] + sizes[:-1])
    for ref_idx in (True, False):
        out = data.collate_sym(items, reference_indexing=ref_idx)
        sym = out[3]
        for a, b in zip(out[:3] + out[4:], batch[:3] + batch[4:]):          # everything but the labels: collate_fn_separate's
            assert a == b if isinstance(a, tuple) else torch.equal(a, b)
        assert isinstance(sym, data.SymBatch) and sym.n_segments == len(flat) == 7
        assert all(t.dtype == torch.int32 for t in (sym.rows, sym.pseg, sym.seg_ptr, sym.pose_ptr, sym.tgt_ptr, sym.urow,
                                                    sym.uptr, sym.upoint)) and sym.targets.dtype == torch.float32
        back = data.unpack_sym(sym)
        assert len(back) == len(flat)
        for (rows, xyzs), (rows0, xyzs0), j in zip(back, flat, scan_of):
            assert torch.equal(rows, rows0 + (0 if ref_idx else int(first[j])))
            assert len(xyzs) == len(xyzs0) and all(torch.equal(x.view(torch.int32), x0.view(torch.int32)) for x, x0 in zip(xyzs, xyzs0))
        assert sorted({len(x) for _, x in flat}) == [1, 2, 36]
        P = sym.rows.shape[0]
        assert sym.n_jobs == sum(len(x) for _, x in flat) == int(sym.pose_ptr[-1])
        assert int(sym.seg_ptr[-1]) == P and int(sym.tgt_ptr[-1]) == sym.targets.shape[0]
        assert torch.equal(sym.pseg.long(), torch.repeat_interleave(torch.arange(7), (sym.seg_ptr[1:] - sym.seg_ptr[:-1]).long()))
        assert sym.max_row == int(sym.rows.max())
        urow, uptr, upoint = sym.urow.numpy(), sym.uptr.numpy(), sym.upoint.numpy()
        assert (np.diff(urow) > 0).all() and uptr[0] == 0 and uptr[-1] == P
        assert np.array_equal(np.sort(upoint), np.arange(P))
        for u, r in enumerate(urow):
            pts = upoint[uptr[u]:uptr[u + 1]]
            assert pts.size and (np.diff(pts) > 0).all() and (sym.rows.numpy()[pts] == r).all()
    assert (np.diff(data.collate_sym(items)[3].uptr.numpy()) > 1).any()         # the golden batch has rows in two segments


def test_collate_sym_drops_empty_segments_and_refuses_negative_rows(mini):
    _, _, sizes, items = mini
    plain = data.collate_sym(items)[3]
    it = list(items[0])
    it[3] = [it[3][0], [np.zeros(0, np.int64), [np.zeros((0, 3), np.float32)] * 2]] + list(it[3][1:])
    sym = data.collate_sym([tuple(it), items[1]])[3]
    assert sym.n_segments == plain.n_segments and all(torch.equal(a, b) for a, b in zip(sym[:9], plain[:9]))
    bad = list(items[0])
    rows = np.asarray(bad[3][0][0]).copy()
    rows[0] = -1
    bad[3] = [[rows, bad[3][0][1]]] + list(bad[3][1:])
    with pytest.raises(ValueError, match="negative row"):
        data.collate_sym([tuple(bad), items[1]])
    empty = data.pack_sym([[], []], [5, 5])
    assert empty.n_segments == 0 and empty.n_jobs == 0 and empty.max_row == -1 and empty.rows.numel() == 0


def test_sym_batch_travels_through_a_dataloader():
    ds = data.SyntheticSymDataset(2, 1500, seed0=5, room=(1.5, 0.9, 1.5), n_boxes=3, margin=0.5, box_scale=0.4, res=0.06)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=data.collate_sym)
    _, coords4, feats, sym, scale, obj, cls = next(iter(loader))
    assert isinstance(sym, data.SymBatch) and sym.n_segments >= 4 and sym.max_row < coords4.shape[0]
    poses = (sym.pose_ptr[1:] - sym.pose_ptr[:-1]).tolist()
    assert set(poses) <= {1, 2, 4, 36} and len(set(poses)) >= 3
    assert int(obj.sum()) == sym.rows.shape[0] > sym.urow.shape[0]           # one segment per object row; the two scans' rows collide
    # pose 0 of every segment is the scene's own label; pose k its rotation in fp64, cast once
    item = ds[0]
    rows, xyzs = item[3][1]
    assert np.array_equal(xyzs[0], ds.scenes[0][3][rows])
    a = data.SYMMETRY_ANGLES["__SYM_ROTATE_UP_2"][0]
    assert np.array_equal(xyzs[1], (xyzs[0].astype(np.float64) @ data._roty4(a)[:3, :3].T).astype(np.float32))


def test_oracle_reproduces_the_golden_loss_and_gradient(mini):
    batch, F, sizes, _ = mini
    z = np.load(GOLDEN)
    sym = data.pack_sym(batch[3], sizes)
    r = ref.oracle(F, sym)
    assert abs(r["loss"] - float(z["sep_loss_xyz"])) < 1e-6 * max(1.0, abs(float(z["sep_loss_xyz"])))
    # the golden gradient holds all three terms; columns 0..2 belong to the coordinate loss alone
    np.testing.assert_allclose(r["grad"], z["sep_grad"][:, :3], rtol=1e-5, atol=1e-8)
    assert sorted(set(np.diff(sym.pose_ptr.numpy()).tolist())) == [1, 2, 36]
    assert ref.decidable(r) > 1.0
    print("golden batch: smallest (second - best) / (4 x pose bound) = %.1f" % ref.decidable(r))


def test_restatement_stays_inside_the_bounds(all_cases):
    for name, (out, sym, w, xf) in all_cases.items():
        r = ref.oracle(out, sym, w, xf, grad_loss=0.75)
        ref.assert_within(ref.restate(out, sym, w, xf, grad_loss=0.75), r, name)


def test_every_case_has_a_decidable_minimum(all_cases):
    """No segment is exempt: the best and the second-best pose loss of every segment of every case differ by more than four
    times the pose bound, so the fp32 minimum of the kernel and the fp64 minimum of the oracle are the same pose, and no two
    poses tie (torch's even split of the gradient over ties does not arise)."""
    for name, (out, sym, w, xf) in all_cases.items():
        margin = ref.decidable(ref.oracle(out, sym, w, xf))
        assert margin > 1.0, (name, margin)
    g = ref.oracle(*all_cases["golden_reference"][:2])
    many = np.isfinite(g["second"])
    rel = np.min((g["second"][many] - g["seg_loss"][many]) / g["second"][many])
    assert 1.3e-4 < rel < 1.6e-4                                          # 1.46e-4 = 2441 u against the bound of 8 u


def test_cases_cover_what_they_are_named_for(cases):
    lens = lambda sym: np.diff(sym.seg_ptr.numpy()).tolist()
    poses = lambda sym: np.diff(sym.pose_ptr.numpy()).tolist()
    seen = set()
    for shift in range(4):
        out, sym, w, xf = cases["lengths_%d" % shift]
        assert lens(sym) == ref.edge_lengths(256)
        best = ref.oracle(out, sym, w, xf)["best"]
        seen |= {(ln, n, "first" if b == 0 else "last") for ln, n, b in zip(lens(sym), poses(sym), best) if n > 1 and b in (0, n - 1)}
        seen |= {(ln, 1, "first") for ln, n in zip(lens(sym), poses(sym)) if n == 1}
    assert {ln for ln, _, _ in seen} == set(ref.edge_lengths(256))
    assert {(n, at) for _, n, at in seen} >= {(1, "first"), (2, "first"), (2, "last"), (4, "first"), (4, "last"), (36, "first"), (36, "last")}
    assert cases["segments_300"][1].n_segments == 300 and cases["one_segment_4"][1].n_segments == 1
    mult = np.diff(cases["shared_rows"][1].uptr.numpy())
    assert (mult == 2).any() and (mult == 3).any()
    a, b = cases["two_scans_reference"][1], cases["two_scans_offset"][1]
    assert (np.diff(a.uptr.numpy()) > 1).any() and (np.diff(b.uptr.numpy()) == 1).all()      # collisions only under the reference's indexing
    assert {cases[k][0].shape[1] for k in cases} == {8, 11}


def test_named_wrong_results_land_far_outside_the_bounds(cases):
    """each mistake an implementation could make moves the loss or a gradient element by at least 10 x its bound"""
    def outside(got, r):
        w = ref.worst_ratios({k: got[k] for k in ("pose_loss", "best", "seg_loss", "loss", "grad")}, r)
        return max(w["loss"], w["grad"])

    out, sym, w, xf = cases["shared_rows"]                                   # w = (0.5, 2, 1.25), poses 1 / 2 / 4 / 36
    r = ref.oracle(out, sym, w, xf)
    assert (r["best"] > 0).any()
    for mutant in ("mean_len", "max", "no_weights", "pose0", "no_factor2"):
        assert outside(ref.oracle(out, sym, w, xf, mutate=mutant), r) > 10.0, mutant
    out, sym, w, xf = cases["two_scans_offset"]
    forgot = cases["two_scans_reference"][1]
    assert outside(ref.oracle(out, forgot, w, xf), ref.oracle(out, sym, w, xf)) > 10.0
    assert outside(ref.restate(out, sym, w, xf), ref.oracle(out, sym, w, xf)) <= 1.0          # (and the right one is inside)


def test_the_library_exports_the_sym_loss_abi_and_checks_its_arguments(built_lib):
    L = _lib.lib()
    assert L.cv_sizeof_sym_loss_desc() == ctypes.sizeof(_lib.SymLossDesc)
    chunk = L.cv_sym_loss_chunk_rows()
    assert chunk == 256
    assert L.cv_sym_loss_workspace_bytes(10 * chunk + 5, 7) >= 8 * (10 + 7)
    FAKE = 0x1000                                                            # never dereferenced: every call below is refused first
    assert L.cv_sym_loss_fwd_f32(None, None) == -22 and b"null" in L.cv_last_error()

    def desc(**kw):
        d = _lib.SymLossDesc()
        for f in ("d_out", "d_rows", "d_pseg", "d_seg_ptr", "d_pose_ptr", "d_tgt_ptr", "d_targets", "d_urow", "d_uptr", "d_upoint",
                  "d_loss", "d_pose_loss", "d_best", "d_seg_loss", "d_grad_loss", "d_grad", "d_ws"):
            setattr(d, f, FAKE)
        d.n_rows, d.ld, d.n_points, d.n_segments, d.n_jobs, d.n_targets, d.n_urows, d.grad_ld = 100, 8, 40, 2, 3, 60, 30, 8
        d.ws_bytes = 1 << 20
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn in (L.cv_sym_loss_fwd_f32, L.cv_sym_loss_bwd_f32):
        assert fn(ctypes.byref(desc(d_out=None)), None) == -22 and b"null pointer" in L.cv_last_error()
        assert fn(ctypes.byref(desc(d_targets=None)), None) == -22
        assert fn(ctypes.byref(desc(ld=2)), None) == -22 and b"stride" in L.cv_last_error()
        for f in ("n_segments", "n_jobs", "n_points", "n_targets", "n_urows", "n_rows"):
            assert fn(ctypes.byref(desc(**{f: -1})), None) == -22 and b"negative count" in L.cv_last_error(), f
    assert L.cv_sym_loss_bwd_f32(ctypes.byref(desc(grad_ld=2)), None) == -22
    assert L.cv_sym_loss_bwd_f32(ctypes.byref(desc(d_grad_loss=None)), None) == -22
    assert L.cv_sym_loss_fwd_f32(ctypes.byref(desc(d_loss=None)), None) == -22
    need = L.cv_sym_loss_workspace_bytes(60, 3)
    assert L.cv_sym_loss_fwd_f32(ctypes.byref(desc(ws_bytes=need - 1)), None) == -12
    assert (b"needs %d bytes" % need) in L.cv_last_error()
    assert L.cv_sym_loss_fwd_f32(ctypes.byref(desc(d_ws=None)), None) == -12
    assert L.cv_sym_loss_bwd_f32(ctypes.byref(desc(n_segments=0, n_jobs=0)), None) == 0       # nothing to do, nothing launched


def test_train_separate_script_parses():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "train_separate.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--category" in r.stdout and "--config" in r.stdout
