"""cv_decode_instances_f32 on the device (csrc/hv_decode.hip: inst_boxes, inst_assign) against the numpy fp32 restatement of
tests/test_instances.py, bit for bit: every case goes through the C ABI into sentinel-filled outputs with guard words on
both sides.  Box counts sit around INST_GROUP = 64 (the boxes staged in LDS at a time) and two groups: 0, 1, 63, 64, 65, 130.
End to end, pipeline.scene_instances on 3k-point teacher scenes is pinned to the decode itself: the members of every accepted
box alone have the max prob the decode reported as that box's score (its own ``probmax``, from dec_backproject)."""
import ctypes

import numpy as np
import pytest
import torch

from canonicalvoting_amd import _lib, decode, pipeline
from canonicalvoting_amd.hough import HoughVoting
from canonicalvoting_amd.minkunet import MinkUNet34C
from canonicalvoting_amd.synth import make_raw_scene, make_scene, synth_predictions
from tests import test_instances as ti

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
GUARD = 64


class Guarded:
    """int32 [rows, cols] device output between two runs of guard words, everything filled with the sentinel"""

    def __init__(self, dev, rows, cols):
        self.rows, self.cols = rows, cols
        self.buf = torch.full((2 * GUARD + rows * cols,), SENT, dtype=torch.int32, device=dev)

    def ptr(self):
        return _lib.vp(self.buf.data_ptr() + 4 * GUARD)

    def get(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENT).all() and (h[-GUARD:] == SENT).all(), "guard words overwritten"
        return h[GUARD:-GUARD].reshape(self.rows, self.cols)


def call_abi(dev, cats, confident=True, counts=True, max_boxes=None, labels=None, cells=None, prob_thresh=0.3, null_prob=False):
    """K = len(cats) categories (cases that share points, grid shape, corner and res) through cv_decode_instances_f32.
    -> owner [K, n], count_in [K, max_boxes] or None, count_owned (numpy; untouched words hold SENT)"""
    L = _lib.lib()
    K = len(cats)
    c0 = cats[0]
    n = len(c0["points"])
    cells = [c["cells"] for c in cats] if cells is None else cells
    nb = np.array([len(c) for c in cells], np.int32)
    M = int(nb.max()) + 3 if max_boxes is None else max_boxes
    h_cells, h_label = np.full((K, max(M, 1)), -7, np.int64), np.full((K, max(M, 1)), -9, np.int32)     # (garbage beyond n_boxes)
    for k in range(K):
        h_cells[k, :nb[k]] = cells[k]
        h_label[k, :nb[k]] = np.arange(nb[k]) if labels is None else labels[k]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rot, scale = t(np.stack([c["grid_rot"] for c in cats])), t(np.stack([c["grid_scale"] for c in cats]))
    pts, prob = t(c0["points"]), t(np.stack([c["prob"] for c in cats]))
    owner = Guarded(dev, K, n)
    cin, cown = (Guarded(dev, K, M), Guarded(dev, K, M)) if counts else (None, None)
    ws_bytes = L.cv_decode_instances_workspace_bytes(K, M)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    rc = L.cv_decode_instances_f32(_lib.ptr(rot), _lib.ptr(scale), (ctypes.c_int * 3)(*c0["grid_rot"].shape[:3]),
                                   (ctypes.c_float * 3)(*[float(v) for v in c0["corner"]]), ctypes.c_float(float(c0["res"])),
                                   _lib.ptr(pts), None if null_prob else _lib.ptr(prob), n, K, h_cells.ctypes.data_as(_lib.c_i64_p),
                                   h_label.ctypes.data_as(_lib.c_i32_p), nb.ctypes.data_as(_lib.c_int_p), M,
                                   ctypes.c_float(prob_thresh), 1 if confident else 0, owner.ptr(),
                                   cin.ptr() if counts else None, cown.ptr() if counts else None, _lib.ptr(ws), ws_bytes,
                                   _lib.stream(dev))
    h_cells[:], h_label[:] = -1, -1          # the host lists may be reused as soon as the call returns
    _lib.check(rc, "cv_decode_instances_f32")
    torch.cuda.synchronize()
    return owner.get(), (cin.get() if counts else None), (cown.get() if counts else None)


def check_case(dev, case, confident, max_boxes=None, labels=None):
    """one category against the restatement, with and without the count outputs; returns the owners"""
    want_owner, want_in, want_own = ti.run_contract(case, confident=confident, label_of=labels)
    B = len(case["cells"])
    owner, cin, cown = call_abi(dev, [case], confident, True, max_boxes, None if labels is None else [labels])
    assert owner.dtype == np.int32 and np.array_equal(owner[0], want_owner)
    assert np.array_equal(cin[0, :B], want_in) and np.array_equal(cown[0, :B], want_own)
    assert (cin[0, B:] == SENT).all() and (cown[0, B:] == SENT).all() and cin.shape[1] > B       # the tail is left alone
    assert cown[0, :B].sum() == (owner[0] != -1).sum()
    assert (cin[0, :B] >= cown[0, :B]).all()
    first_hit, _, _ = call_abi(dev, [case], confident, False, max_boxes, None if labels is None else [labels])
    assert np.array_equal(first_hit, owner)             # the walk that stops at the first hit gives the same owners
    return owner[0]


@pytest.mark.parametrize("confident", [True, False], ids=["confident", "inside"])
@pytest.mark.parametrize("n", ti.N_SWEEP)
def test_point_counts(cuda, built_lib, n, confident):
    owner = check_case(cuda, ti.gpu_cases()["n%d" % n], confident, max_boxes=8)
    if n >= 255:
        assert (owner >= 0).any() and (owner == -1).any()


@pytest.mark.parametrize("confident", [True, False], ids=["confident", "inside"])
@pytest.mark.parametrize("b", ti.B_SWEEP)
def test_box_counts_around_the_lds_group(cuda, built_lib, b, confident):
    case = ti.gpu_cases()["b%d" % b]
    owner = check_case(cuda, case, confident)
    if b == 0:
        assert (owner == -1).all()
    if b >= 65:                       # boxes of the second (and third) group own points too
        assert (owner >= ti.GROUP).any()


def test_inside_support_takes_a_null_prob(cuda, built_lib):
    case = ti.gpu_cases()["b65"]
    owner, _, _ = call_abi(cuda, [case], confident=False, counts=False, null_prob=True)
    assert np.array_equal(owner[0], ti.run_contract(case, confident=False)[0])


def test_special_values_and_faces(cuda, built_lib):
    """the hand-worked case: points exactly on faces (rot vectors (1,0) and (-1,0)), a zero scale component, NaN and inf
    points, a NaN prob and a prob equal to prob_thresh"""
    case, want = ti.special_case()
    for confident in (True, False):
        owner = check_case(cuda, case, confident)
        if confident:
            assert owner.tolist() == want.tolist()
    nan_rows = ~np.isfinite(case["points"]).all(1)
    assert nan_rows.sum() == 7 and (check_case(cuda, case, False)[nan_rows] == -1).all()


def test_disjoint_boxes_own_all_their_members(cuda, built_lib):
    case, _ = ti.special_case()
    cell = lambda x, y, z: (x * 4 + y) * 4 + z
    case = dict(case, cells=np.array([cell(0, 1, 1), cell(3, 1, 1)], np.int64))       # x in (.5, 1.5) and (2, 3)
    _, cin, cown = call_abi(cuda, [case], confident=False)
    check_case(cuda, case, False)
    assert np.array_equal(cin[0, :2], cown[0, :2]) and cin[0, :2].min() >= 2


def test_priority_is_the_list_order(cuda, built_lib):
    """the same boxes in reversed list order (labels kept with their boxes) flip exactly the points that two or more boxes share"""
    case = ti.gpu_cases()["b65"]
    B = len(case["cells"])
    member = np.stack([ti.inside(case["points"], *ti.box_geometry(case["grid_rot"], case["grid_scale"], case["corner"], case["res"],
                                                                 int(c))) for c in case["cells"]])
    shared = member.sum(0) >= 2
    assert shared.sum() >= 20 and (member.sum(0) == 1).sum() >= 20
    fwd, _, _ = call_abi(cuda, [case], confident=False)
    rev, _, _ = call_abi(cuda, [dict(case, cells=case["cells"][::-1].copy())], confident=False, labels=[np.arange(B)[::-1].copy()])
    assert np.array_equal(fwd[0] != rev[0], shared)
    assert np.array_equal(rev[0], ti.run_contract(case, confident=False, last=True)[0])


def test_label_of_is_honoured(cuda, built_lib):
    case = ti.gpu_cases()["b130"]
    labels = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, 130).astype(np.int32)
    labels[labels == -1] = 12345
    owner = check_case(cuda, case, True, labels=labels)
    plain = ti.run_contract(case)[0]
    assert np.array_equal(owner[plain >= 0], labels[plain[plain >= 0]]) and (owner[plain < 0] == -1).all()


@pytest.mark.parametrize("confident", [True, False], ids=["confident", "inside"])
def test_three_categories_equal_their_single_calls(cuda, built_lib, confident):
    cats = [ti.gpu_cases()["k%d" % k] for k in range(3)]
    assert [len(c["cells"]) for c in cats] == [70, 0, 9]
    owner, cin, cown = call_abi(cuda, cats, confident, max_boxes=72)
    first_hit, _, _ = call_abi(cuda, cats, confident, counts=False, max_boxes=72)
    assert np.array_equal(first_hit, owner)
    for k, c in enumerate(cats):
        o1, i1, w1 = call_abi(cuda, [c], confident, max_boxes=72)
        assert np.array_equal(owner[k], o1[0]) and np.array_equal(cin[k], i1[0]) and np.array_equal(cown[k], w1[0])
        want = ti.run_contract(c, confident=confident)
        B = len(c["cells"])
        assert np.array_equal(owner[k], want[0]) and np.array_equal(cin[k, :B], want[1]) and np.array_equal(cown[k, :B], want[2])
        assert (cin[k, B:] == SENT).all() and (cown[k, B:] == SENT).all()
    assert (owner[1] == -1).all()


def test_python_call_matches_the_abi(cuda, built_lib):
    """decode.instance_labels, single and [K, ...] form, counts cut to the longest list"""
    cats = [ti.gpu_cases()["k%d" % k] for k in range(3)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    c = cats[0]
    got = decode.instance_labels(t(c["grid_rot"]), t(c["grid_scale"]), c["corner"], c["res"], t(c["points"]), t(c["prob"]), c["cells"],
                                 counts=True)
    for g, w in zip(got, ti.run_contract(c)):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
    owner = decode.instance_labels(t(np.stack([c["grid_rot"] for c in cats])), t(np.stack([c["grid_scale"] for c in cats])),
                                   c["corner"], c["res"], t(c["points"]), None, [c["cells"] for c in cats], support="inside")
    assert tuple(owner.shape) == (3, 300)
    for k in range(3):
        assert np.array_equal(owner[k].cpu().numpy(), ti.run_contract(cats[k], confident=False)[0])
    with pytest.raises(ValueError):
        decode.instance_labels(t(c["grid_rot"]), t(c["grid_scale"]), c["corner"], c["res"], t(c["points"]), None, c["cells"])


# ---- end to end: 3k-point teacher scenes, as the scene tests build them -------------------------------------------------------------

RES, THRESH = 0.06, 20
SMALL = dict(room=(2.0, 1.0, 2.0), n_boxes=3, margin=0.6, box_scale=0.5)
K = 3


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def joint_model(cuda, built_lib):
    torch.manual_seed(0)
    return MinkUNet34C(3, 64).to(cuda).eval()


def restate_scene(keep, dets, pts, confident, k=None, members=None):
    """contract() on a scene's keep (category k of a separate scene) for the detections ``members`` (positions in dets; all
    by default): priority by score, ties by position, boxes matched to accepted cells by exact corner equality"""
    raw = keep["raw"] if k is None else keep["raw"][k]
    pick = lambda a: a.cpu().numpy() if k is None else a[k].cpu().numpy()
    accepted = raw["cand_idx"][raw["verdict"] == 0]
    assert len(accepted) == len(raw["boxes"])
    members = list(range(len(dets))) if members is None else members
    order = sorted(members, key=lambda p: (-dets[p][2], p))
    used, cells = set(), []
    for p in order:
        i = next(i for i in range(len(accepted)) if i not in used and np.array_equal(raw["boxes"][i], dets[p][1]))
        used.add(i)
        cells.append(int(accepted[i]))
    return ti.contract(pick(keep["grids"][1]), pick(keep["grids"][2]), np.array(keep["corner"], np.float32), np.float32(keep["res"]),
                       pts.cpu().numpy(), pick(keep["decode_prob"]), cells, label_of=order, confident=confident)


def check_boxes_alone(keep, pts, raws, make_det, prob_of):
    """every accepted box alone, support 'inside': the members' max prob is the decode's own probmax, bit for bit"""
    seen = 0
    for k, raw in enumerate(raws):
        prob = prob_of(k)
        for i in range(len(raw["boxes"])):
            out = pipeline.scene_instances(keep, [make_det(k, raw["boxes"][i], float(raw["scores"][i]))], pts, support="inside",
                                           counts=True)
            owner = out["owner"] if out["owner"].dim() == 1 else out["owner"][k]
            m = owner == 0
            assert int(m.sum()) == int(out["count_in"][0]) == int(out["count_owned"][0]) > 0
            assert prob[m].max().cpu().numpy().view(np.uint32) == np.float32(raw["scores"][i]).view(np.uint32), (k, i)
            seen += 1
    return seen


def check_joint(keep, dets, pts, inverse=None):
    assert len(dets) >= 2
    for support in ("confident", "inside"):
        out = pipeline.scene_instances(keep, dets, pts, support=support, counts=True, inverse=inverse)
        want_owner, want_in, want_own = restate_scene(keep, dets, pts, support == "confident")
        order = sorted(range(len(dets)), key=lambda p: (-dets[p][2], p))
        assert out["owner"].dtype == torch.int32 and np.array_equal(out["owner"].cpu().numpy(), want_owner)
        assert np.array_equal(out["count_in"].cpu().numpy()[order], want_in)
        assert np.array_equal(out["count_owned"].cpu().numpy()[order], want_own)
        assert (want_owner >= 0).sum() > 0
        if inverse is not None:
            assert np.array_equal(out["raw_owner"].cpu().numpy(), want_owner[inverse.cpu().numpy()])
    raw = keep["raw"]
    n = check_boxes_alone(keep, pts, [raw], lambda k, b, s: (0, b, s), lambda k: keep["decode_prob"])
    assert n == len(raw["boxes"]) >= 2


def test_scene_call_end_to_end(cuda, joint_model):
    sc = make_scene(1, n_points=3000, res=RES, **SMALL)
    t = _t(cuda)
    c4 = torch.cat([torch.zeros((3000, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(cuda)
    feats = (t(sc.feats) * 2 - 1).contiguous()
    pts = (c4[:, 1:] * sc.res).float().contiguous()
    xyz, scale, prob, cls = [t(a) for a in synth_predictions(sc)]
    keep = {}
    dets, raw, _ = pipeline.detect_scene_c(joint_model, HoughVoting(RES, 120), c4, feats, RES, scan_points=pts,
                                           predictions=(xyz, scale, prob, cls.int()), keep=keep, thresh_high=THRESH)
    check_joint(keep, dets, pts)
    # a keep without grids (a scene redone call by call hands none out) is refused
    for bad in ({}, {k: v for k, v in keep.items() if k != "grids"}):
        with pytest.raises(RuntimeError, match="no grids"):
            pipeline.scene_instances(bad, dets, pts)


def test_raw_cloud_call_end_to_end(cuda, joint_model):
    raw_scene = make_raw_scene(1, 6000, **SMALL)
    t = _t(cuda)
    teacher = tuple(t(a) for a in synth_predictions(raw_scene))
    feats = (t(raw_scene.feats) * 2 - 1).contiguous()
    keep = {}
    dets, raw, _, index, inverse = pipeline.detect_points_c(joint_model, HoughVoting(RES, 120), t(raw_scene.points), feats, RES,
                                                            predictions=teacher, return_inverse=True, keep=keep, thresh_high=THRESH)
    assert inverse.shape[0] == 6000 > keep["scan_points"].shape[0]
    check_joint(keep, dets, keep["scan_points"], inverse)
    # scan_points default to the ones the call kept
    a = pipeline.scene_instances(keep, dets)["owner"]
    assert torch.equal(a, pipeline.scene_instances(keep, dets, keep["scan_points"])["owner"])


def test_separate_scene_call_end_to_end(cuda, built_lib):
    models = {}
    for c in range(K):
        torch.manual_seed(100 + c)
        models["cat%d" % c] = MinkUNet34C(3, 8).to(cuda).eval()
    names = list(models)
    sc = make_scene(1, n_points=3000, res=RES, **SMALL)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)
    c4 = torch.cat([torch.zeros((3000, 1), dtype=torch.int32), torch.from_numpy(sc.coords).int()], 1).to(cuda)
    feats = (t(sc.feats) * 2 - 1).contiguous()
    pts = (c4[:, 1:] * sc.res).float().contiguous()
    xyz, scale, prob, cls = synth_predictions(sc)
    rng = np.random.default_rng(1)
    P = np.stack([np.where(cls % K == c, prob, rng.uniform(1e-3, 0.1, 3000)) for c in range(K)])
    keep = {}
    dets = pipeline.detect_scene_separate_c(models, HoughVoting(RES, 120), c4, feats, RES,
                                            predictions=(t(np.stack([xyz] * K)), t(np.stack([scale] * K)), t(P)), keep=keep,
                                            thresh_high=THRESH)
    assert len(dets) >= 2
    cat_of = [names.index(d[0]) for d in dets]
    score = np.array([d[2] for d in dets])
    for support in ("confident", "inside"):
        out = pipeline.scene_instances(keep, dets, pts, support=support, counts=True)
        assert tuple(out["owner"].shape) == (K, 3000) and tuple(out["merged"].shape) == (3000,)
        owner = out["owner"].cpu().numpy()
        want = np.full((K, 3000), -1, np.int32)
        for k in range(K):
            mine = [p for p in range(len(dets)) if cat_of[p] == k]
            want[k], w_in, w_own = restate_scene(keep, dets, pts, support == "confident", k, mine)
            order = sorted(mine, key=lambda p: (-dets[p][2], p))
            assert np.array_equal(out["count_in"].cpu().numpy()[order], w_in) and np.array_equal(out["count_owned"].cpu().numpy()[order], w_own)
        assert np.array_equal(owner, want)
        # merged: over the categories, the owner with the best score (ties: the earlier detection)
        merged = np.full(3000, -1, np.int32)
        for i in range(3000):
            cand = [int(p) for p in want[:, i] if p >= 0]
            if cand:
                merged[i] = min(cand, key=lambda p: (-score[p], p))
        assert np.array_equal(out["merged"].cpu().numpy(), merged) and (merged >= 0).any()
    n = check_boxes_alone(keep, pts, keep["raw"], lambda k, b, s: (names[k], b, s), lambda k: keep["decode_prob"][k])
    assert n == sum(len(r["boxes"]) for r in keep["raw"]) >= 2


def test_separate_raw_cloud_call_keeps_its_world_points(cuda, built_lib):
    """detect_points_separate_c: scene_instances runs on the world points the call kept (the voxel coordinates times res, as the
    scene formed them) and labels the raw points through ``inverse`` from the merged owners"""
    models = {}
    for c in range(K):
        torch.manual_seed(100 + c)
        models["cat%d" % c] = MinkUNet34C(3, 8).to(cuda).eval()
    raw_scene = make_raw_scene(1, 6000, **SMALL)
    xyz, scale, prob, cls = synth_predictions(raw_scene)
    rng = np.random.default_rng(1)
    P = np.stack([np.where(cls % K == c, prob, rng.uniform(1e-3, 0.1, 6000)) for c in range(K)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)
    keep = {}
    dets, index, inverse = pipeline.detect_points_separate_c(models, HoughVoting(RES, 120), t(raw_scene.points),
                                                             (t(raw_scene.feats) * 2 - 1).contiguous(), RES,
                                                             predictions=(t(np.stack([xyz] * K)), t(np.stack([scale] * K)), t(P)),
                                                             return_inverse=True, keep=keep, thresh_high=THRESH)
    assert len(dets) >= 2
    pts = (keep["coords4"][:, 1:] * RES).float().contiguous()
    assert torch.equal(pts, keep["world_points"])
    out = pipeline.scene_instances(keep, dets, inverse=inverse)
    given = pipeline.scene_instances(keep, dets, pts)
    assert torch.equal(out["owner"], given["owner"]) and torch.equal(out["merged"], given["merged"])
    assert tuple(out["raw_owner"].shape) == (6000,) and torch.equal(out["raw_owner"], out["merged"][inverse.long()])
    assert (out["merged"] >= 0).any()
    names = list(models)
    for k in range(K):
        mine = [p for p in range(len(dets)) if dets[p][0] == names[k]]
        assert np.array_equal(out["owner"][k].cpu().numpy(), restate_scene(keep, dets, pts, True, k, mine)[0])
