"""Model-axis entry points of the C ABI (cv_net_run_models_f32 and its helpers, cv_head_separate_models_f32,
cv_scene_separate_desc.models_per_pass) without a GPU: exported, sizes that reduce to the single-model ones at K = 1 and are
K times them at K = 9, and bad input refused with CV_EINVAL by host-side checks before anything reaches the device (the
device pointers below are fake and never dereferenced)."""
import ctypes

import pytest

from canonicalvoting_amd import _lib

EINVAL = -22
NEW = ("cv_net_models_params_bytes", "cv_net_models_params_fill", "cv_net_models_arena_bytes", "cv_net_models_workspace_bytes",
       "cv_net_run_models_f32", "cv_head_separate_models_f32")
vp = ctypes.c_void_p
FAKE = 4096


def test_model_axis_symbols_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in _lib.SIGNATURES, s
    assert _lib.lib().cv_abi_version() == _lib.ABI_VERSION >= 5
    names = [f[0] for f in _lib.SceneSeparateDesc._fields_]
    assert names[-2:] == ["models_per_pass", "d_model_params"]          # appended: the fields in front keep their offsets
    assert ctypes.sizeof(_lib.NetModelParams) == 48


def program(n_ops=2, cout=32):
    """a tiny fp16-pair program on fake device pointers: slot 0 / 1 the caller's input / output, slot 2 an arena buffer;
    op 0 reads the caller's input"""
    bufs = (_lib.NetBuf * 3)(_lib.NetBuf(-1, 3, 0, 0), _lib.NetBuf(-1, 8, 0, 0), _lib.NetBuf(0, 32, 0, 1))
    ops = (_lib.NetOp * n_ops)()
    for k in range(n_ops):
        ops[k] = _lib.NetOp(in_buf=2 if k else 0, in_col=0, cin=32 if k else 3, out_buf=2 if k + 1 < n_ops else 1, out_col=0, cout=cout, res_buf=-1, res_col=0,
                            map=5, K=27, perm=-1, perm_groups=0, relu=1, weight=FAKE, scale=None, shift=FAKE, weight_x6=FAKE,
                            in2_buf=-1, in2_col=0, cin2=0, weight2_x6=None, weight_pieces=2, acc_scale=0.5)
    return ops, bufs


@pytest.mark.parametrize("rows", [(3000, 700, 160, 40, 12), (80000, 19000, 4700, 1200, 300), (300000, 80000, 20000, 5000, 1300)])
def test_sizes_reduce_to_the_single_model_ones(built_lib, rows):
    L = _lib.lib()
    ops, bufs = program()
    r = (ctypes.c_int64 * 5)(*rows)
    one = L.cv_net_arena_bytes(bufs, 3, r, 5)
    assert one > 0 and L.cv_net_models_arena_bytes(bufs, 3, r, 5, 1) == one
    assert L.cv_net_models_arena_bytes(bufs, 3, r, 5, 9) == 9 * one
    masked = (ctypes.c_int * 5)(*[n >= 16384 for n in rows])
    ws = L.cv_sp_scene_conv_workspace_bytes(r, masked, 3, 256)
    assert ws > 0 and ws % 256 == 0
    assert L.cv_net_models_workspace_bytes(ws, 1) == ws and L.cv_net_models_workspace_bytes(ws, 9) == 9 * ws
    assert L.cv_net_models_workspace_bytes(1000, 1) == 1000 and L.cv_net_models_workspace_bytes(1000, 3) == 2 * 1024 + 1000
    for k in (0, -1, 17):
        assert L.cv_net_models_arena_bytes(bufs, 3, r, 5, k) == 0 and L.cv_net_models_workspace_bytes(ws, k) == 0
        assert L.cv_net_models_params_bytes(10, k) == 0
    assert L.cv_net_models_params_bytes(102, 1) == 102 * 48 and L.cv_net_models_params_bytes(102, 9) == 9 * 102 * 48


def test_params_table_is_op_major_and_normalises_acc_scale(built_lib):
    L = _lib.lib()
    K = 3
    progs = [program() for _ in range(K)]
    for m, (ops, _) in enumerate(progs):
        ops[0].weight_x6, ops[0].acc_scale = FAKE + 256 * m, 0.0
        ops[1].shift, ops[1].acc_scale = FAKE + 512 * m, 0.25 * (m + 1)
    tab = (_lib.NetModelParams * (2 * K))()
    c_ops = (vp * K)(*[ctypes.cast(p[0], vp) for p in progs])
    nbytes = L.cv_net_models_params_bytes(2, K)
    assert nbytes == ctypes.sizeof(tab)
    assert L.cv_net_models_params_fill(c_ops, 2, K, ctypes.cast(tab, vp), nbytes) == 0
    for m in range(K):
        assert tab[m].weight_x6 == FAKE + 256 * m and tab[m].acc_scale == 1.0 and tab[m].scale is None      # 0 means 1
        assert tab[K + m].shift == FAKE + 512 * m and tab[K + m].acc_scale == 0.25 * (m + 1)
    assert L.cv_net_models_params_fill(c_ops, 2, K, ctypes.cast(tab, vp), nbytes - 1) == -12
    assert L.cv_net_models_params_fill(c_ops, 2, 17, ctypes.cast(tab, vp), nbytes) == EINVAL and b"out of range" in L.cv_last_error()
    c_ops[1] = None
    assert L.cv_net_models_params_fill(c_ops, 2, K, ctypes.cast(tab, vp), nbytes) == EINVAL and b"model 1" in L.cv_last_error()


def run_models(L, progs, K, table=FAKE, n_ops=2, ext=None, params_ld=None):
    c_ops = (vp * len(progs))(*[ctypes.cast(p[0], vp) if p is not None else None for p in progs])
    c_bufs = (vp * len(progs))(*[ctypes.cast(p[1], vp) if p is not None else None for p in progs])
    rows = (ctypes.c_int64 * 5)(3000, 700, 160, 40, 12)
    tabs = [(vp * 2)(FAKE, FAKE + 65536 * (m + 1)) for m in range(len(progs))] if ext is None else ext
    c_ext = (vp * len(progs))(*[ctypes.cast(t, vp) for t in tabs])
    ld = (ctypes.c_int * 2)(3, 8)
    maps, perms = (vp * 15)(*[FAKE] * 15), (vp * 9)()
    return L.cv_net_run_models_f32(c_ops, c_bufs, n_ops, 3, K, rows, 5, vp(FAKE), 1 << 30, c_ext, ld, maps, 15, perms, 9, vp(FAKE),
                                   1 << 30, None, vp(table) if table else None, K if params_ld is None else params_ld, None)


def test_run_models_refuses_bad_input_before_touching_the_gpu(built_lib):
    L = _lib.lib()
    progs = [program() for _ in range(3)]
    for k in (0, -1, 17):
        assert run_models(L, progs, k) == EINVAL and b"out of range" in L.cv_last_error()
    assert run_models(L, progs, 3, table=None) == EINVAL and b"parameter table" in L.cv_last_error()
    assert run_models(L, progs, 3, params_ld=2) == EINVAL and b"params_ld" in L.cv_last_error()
    assert run_models(L, [progs[0], None, progs[2]], 3) == EINVAL and b"model 1" in L.cv_last_error()
    # one op's cout differs: the message names the op and the model
    odd = [program(), program(), program()]
    odd[2][0][1].cout = 64
    assert run_models(L, odd, 3) == EINVAL
    msg = L.cv_last_error()
    assert b"op 1 of model 2" in msg and b"structurally identical" in msg
    odd = [program(), program()]
    odd[1][1][2].channels = 64
    assert run_models(L, odd, 2) == EINVAL and b"buffer 2 of model 1" in L.cv_last_error()
    # a pointer that is NULL in one model only is a structural difference too
    odd = [program(), program()]
    odd[1][0][0].shift = None
    assert run_models(L, odd, 2) == EINVAL and b"op 0 of model 1" in L.cv_last_error()
    # bf16 triples are not a batched program
    odd = [program(), program()]
    for ops, _ in odd:
        ops[0].weight_pieces = 3
    assert run_models(L, odd, 2) == EINVAL and b"fp16-pair" in L.cv_last_error()
    # a model without its output tensor; models that read different input tensors
    ext = [(vp * 2)(FAKE, FAKE), (vp * 2)(FAKE, None)]
    assert run_models(L, progs[:2], 2, ext=ext) == EINVAL and b"model 1" in L.cv_last_error()
    ext = [(vp * 2)(FAKE, FAKE), (vp * 2)(FAKE + 64, FAKE + 4096)]
    assert run_models(L, progs[:2], 2, ext=ext) == EINVAL and b"same tensor" in L.cv_last_error()


def test_head_models_refuses_bad_input(built_lib):
    L = _lib.lib()
    f = (vp * 3)(FAKE, None, FAKE)
    for k in (0, 17):
        assert L.cv_head_separate_models_f32(f, k, 100, 8, 1, vp(FAKE), vp(FAKE), vp(FAKE), None) == EINVAL
        assert b"out of range" in L.cv_last_error()
    assert L.cv_head_separate_models_f32(f, 3, 100, 8, 1, vp(FAKE), vp(FAKE), vp(FAKE), None) == EINVAL
    assert b"model 1" in L.cv_last_error()


def fake_scene_desc(K=3):
    d = _lib.SceneSeparateDesc()
    keep = [(vp * K)(*[FAKE] * K) for _ in range(3)] + [(ctypes.c_int * K)(*[10] * K), (ctypes.c_int * K)(*[5] * K)]
    for f in ("d_coords4", "d_feats", "d_points", "h_pinned", "d_ws", "h_boxes", "h_scores", "h_cand_idx", "h_verdict",
              "h_det_cat", "h_det_box"):
        setattr(d, f, vp(FAKE))
    d.ops, d.bufs, d.d_out_feats = ctypes.cast(keep[0], vp), ctypes.cast(keep[1], vp), ctypes.cast(keep[2], vp)
    d.n_ops, d.n_bufs = ctypes.cast(keep[3], vp), ctypes.cast(keep[4], vp)
    d.n, d.out_ld, d.out_channels, d.pinned_bytes, d.max_candidates, d.num_models = 100, 8, 8, 4096, 8, K
    return d, keep


def test_scene_descriptor_models_per_pass(built_lib):
    L = _lib.lib()
    r = _lib.SceneSeparateResult()
    # a descriptor that never heard of models_per_pass (zero) still reaches the last check of the parent
    d, keep = fake_scene_desc()
    assert d.models_per_pass == 0 and d.d_model_params is None
    d.conv_split_target = -1
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
    assert b"negative launch sizing" in L.cv_last_error()
    d.conv_split_target = 0
    d.models_per_pass = -1
    r.host_us[0] = 7.0
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
    assert b"negative models_per_pass" in L.cv_last_error() and r.host_us[0] == 0.0
    d.models_per_pass = 2                       # batched, but no parameter table
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
    assert b"d_model_params" in L.cv_last_error()
    d.d_model_params = vp(FAKE)
    keep[3][2] = 11                             # a program of another length cannot share the launches
    assert L.cv_detect_scene_separate_f32(ctypes.byref(d), ctypes.byref(r), None) == EINVAL
    assert b"model 2" in L.cv_last_error()


def test_pipeline_keyword_defaults_to_the_sequential_path(built_lib):
    import inspect

    from canonicalvoting_amd import pipeline
    assert inspect.signature(pipeline.detect_scene_separate_c).parameters["models_per_pass"].default is None
