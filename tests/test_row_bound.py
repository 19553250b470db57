"""CPU pin of the float64 row-kernel oracle and its per-element bounds (oracle/sparse_oracle.py ROW_ERROR_MODEL) that
tests/test_row_kernels_gpu.py holds the HIP kernels to.  For every quantity: (a) a numpy float32 restatement of the
kernel's operation order stays within the bound at a ratio <= 0.6; (b) named wrong results are at least 10 x outside
it; (c) the float64 heads agree with the torch head split of the oracle."""
import numpy as np
import pytest
import torch

from oracle import sparse_oracle as so

SHAPES = [(1, 32), (2, 4), (257, 96), (1000, 37), (4099, 128)]
EPS = 1e-5
MOM = 0.1
f32 = np.float32
RATIOS = {}                     # quantity -> worst ratio of a restatement (printed by the last test)
# Every restatement is held to 0.6 of its bound, except where the stated constant is less than 1 / 0.6 times the worst-case
# count of fp32 roundings; there elements near the analytic ceiling exist at every size and the ceiling is the pin:
#   affine: three roundings of at most u against 4u: 0.75 (0.67 at 4099 x 128 here)
#   folded shift of the statistics call: its direct part u (|beta| + 2 |mean * scale|) IS the worst case of the product
#     and the subtraction; only the propagated parts carry margin: 1 (0.60 at 4099 x 128 here)
#   affine hl twin: 3u (...) + 2u |z| (the format's worst case) against 4u (...) + u |z| with |z| <= (...): 1
# The constants of the bounds stay as stated.
LIMIT = {"affine": 0.75, "shift": 1.0, "affine hl twin": 1.0}


def ratio(got, ref, bound, what=None):
    ok, i, r = so.within(got, ref, bound)
    if what is not None:
        RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    return r


# ---- numpy float32 restatements in the kernels' operation order ---------------------------------------------------------
def bn_chunks(n):
    return min(1024, max(1, n // 256))


def col_chunks(n):
    return min(256, -(-n // 1024))


def fma32(a, b, c):
    """one rounding: float32(a * b + c), the products of float32 values are exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def affine32(x, scale, shift, res, relu, fma):
    v = x
    if scale is not None:
        sh = np.zeros_like(scale) if shift is None else shift
        v = fma32(v, scale, sh) if fma else (v * scale).astype(f32) + sh
    if res is not None:
        v = v + res
    return np.maximum(v, f32(0)) if relu else v


def fold32(gamma, beta, mean, var, bias, fma):
    s = gamma / np.sqrt(var + f32(EPS))
    sh = fma32(-mean, s, beta) if fma else beta - mean * s
    if bias is not None:
        sh = fma32(bias, s, sh) if fma else sh + bias * s
    return s, sh


def chunk_reduce(cols, n, chunks, lanes=8):
    """the two-level column reduction of bn_col_reduce (double accumulators): per row chunk `lanes` row lanes walk their
    rows in order, a thread adds the lanes in order; then bn_col_finish: 16 sub-sums over every 16th chunk, a butterfly"""
    parts = []
    for q in range(chunks):
        lo, hi = n * q // chunks, n * (q + 1) // chunks
        t = np.zeros(cols.shape[1])
        for ry in range(lanes):
            rows = cols[lo + ry:hi:lanes]
            if len(rows):
                t = t + np.cumsum(rows, 0, dtype=np.float64)[-1]
        parts.append(t)
    sub = [sum(parts[s::16], np.zeros(cols.shape[1])) for s in range(16)]
    while len(sub) > 1:
        sub = [sub[i] + sub[i + len(sub) // 2] for i in range(len(sub) // 2)]
    return sub[0]


def stats32(x, gamma, beta, rm, rv, lanes=8):
    n = x.shape[0]
    x64 = x.astype(np.float64)
    t0 = chunk_reduce(x64, n, bn_chunks(n), lanes)
    t1 = chunk_reduce(x64 * x64, n, bn_chunks(n), lanes)
    mu = t0 / n
    v = np.maximum(t1 / n - mu * mu, 0.0)
    unb = v * n / (n - 1) if n > 1 else v
    m = f32(MOM)
    out = {"mean": mu.astype(f32), "var": v.astype(f32)}
    out["running_mean"] = (f32(1) - m) * rm + m * mu.astype(f32)
    out["running_var"] = (f32(1) - m) * rv + m * unb.astype(f32)
    sc = gamma / np.sqrt(v.astype(f32) + f32(EPS))
    out["scale"] = sc
    out["shift"] = beta - mu.astype(f32) * sc
    return out


def backward32(x, dy, mask, mean, var, gamma, lanes=8, inv_n=None, eps=EPS, drop_row=None):
    n = x.shape[0]
    istd = f32(1) / np.sqrt(var + f32(eps))
    xh = (x - mean) * istd
    g = dy if mask is None else np.where(mask, dy, f32(0))
    gs, ps = g.astype(np.float64), (g * xh).astype(np.float64)
    if drop_row is not None:
        gs, ps = np.delete(gs, drop_row, 0), np.delete(ps, drop_row, 0)
    dbeta = chunk_reduce(gs, len(gs), bn_chunks(n), lanes).astype(f32)
    dgamma = chunk_reduce(ps, len(ps), bn_chunks(n), lanes).astype(f32)
    inv_n = f32(1) / f32(n) if inv_n is None else f32(inv_n)
    dx = gamma * istd * (g - dbeta * inv_n - xh * dgamma * inv_n)
    assert dx.dtype == f32
    return {"dbeta": dbeta, "dgamma": dgamma, "dx": dx, "dres": g}


def col_sum32(x, drop_chunk=None):
    n, chunks = x.shape[0], col_chunks(x.shape[0])
    parts = []
    for q in range(chunks):
        lo, hi = n * q // chunks, n * (q + 1) // chunks
        t = np.zeros(x.shape[1], f32)
        for ry in range(8):
            rows = x[lo + ry:hi:8]
            t = t + (np.cumsum(rows, 0, dtype=f32)[-1] if len(rows) else f32(0))
        parts.append(t)
    if drop_chunk is not None:
        del parts[drop_chunk]
    s = [np.zeros(x.shape[1], f32) for _ in range(4)]
    k = 0
    while k + 3 < len(parts):
        for i in range(4):
            s[i] = s[i] + parts[k + i]
        k += 4
    for p in parts[k:]:
        s[0] = s[0] + p
    return (s[0] + s[1]) + (s[2] + s[3])


def head_joint32(f, ncls, log_scale, background_rule=True, prob_over_all=False):
    """head_joint of row_ops.hip in float32"""
    n = f.shape[0]
    logit = f[:, 6 * ncls:7 * ncls + 1]
    am = logit.argmax(1)
    mx = logit.max(1)
    ao = logit[:, :ncls].argmax(1)
    mo = logit[:, :ncls].max(1)
    e = np.exp(logit - mx[:, None])
    den = np.cumsum(e, 1, dtype=f32)[:, -1]
    h = np.where(am == ncls, 0, am) if background_rule else np.minimum(am, ncls - 1)
    rows = np.arange(n)
    xyz = f[:, :3 * ncls].reshape(n, ncls, 3)[rows, h]
    s = f[:, 3 * ncls:6 * ncls].reshape(n, ncls, 3)[rows, h]
    prob = (f32(1) if prob_over_all else np.exp(mo - mx)) / den
    return xyz, np.exp(s) if log_scale else s, prob, ao


def head_rows(n, ncls, ld, seed=0):
    """network outputs [n, ld]: logits in [-80, 80], log-scales in [-10, 10]; the first rows planted: two equal maxima,
    equal maxima of which one is the background, the background strictly largest, all logits equal"""
    rng = np.random.default_rng(seed + 17 * n + ncls)
    f = rng.normal(0, 1, (n, ld))
    f[:, 3 * ncls:6 * ncls] = rng.uniform(-10, 10, (n, 3 * ncls))
    f[:, 6 * ncls:7 * ncls + 1] = rng.uniform(-80, 80, (n, ncls + 1))
    f[::5, 6 * ncls:7 * ncls + 1] = rng.uniform(-3, 3, (len(f[::5]), ncls + 1))       # ... and rows of comparable logits
    lg = f[:, 6 * ncls:7 * ncls + 1]
    planted = []
    for kind in range(4):
        for r in range(kind, n, 64):           # every 64th row, so that every 256-row block of a larger n has some
            if kind == 0 and ncls >= 2:
                lg[r, ncls - 1] = lg[r, 0] = lg[r].max() + 1.0
            elif kind == 1:
                lg[r, ncls] = lg[r, ncls - 1] = lg[r].max() + 1.0
            elif kind == 2:
                lg[r, ncls] = lg[r].max() + 2.0
            elif kind == 3:
                lg[r] = 0.25
            planted.append(r)
    return f.astype(f32), np.unique(planted)


# ---- (a) the restatements sit inside the bounds, ratio <= 0.6 ------------------------------------------------------------
@pytest.mark.parametrize("n,c", SHAPES)
def test_affine_and_fold_restatements(n, c):
    d = so.row_case(n, c)
    sc, sh = d["gamma"], d["beta"]
    for scale, shift, res, relu in ((sc, sh, d["res"], True), (sc, sh, None, False), (sc, None, d["res"], False),
                                    (None, None, None, True), (None, None, d["res"], True)):
        z, b = so.affine64(d["x"], scale, shift, res, relu)
        for fma in (False, True):
            assert ratio(affine32(d["x"], scale, shift, res, relu, fma), z, b, "affine") <= LIMIT["affine"]
    if c % 32 == 0:
        z, b = so.affine64(d["x"], sc, sh, d["res"], True, hl_out=True)
        y = affine32(d["x"], sc, sh, d["res"], True, True)
        assert ratio(so.hl_decode(so.hl_bits(y)), z, b, "affine hl twin") <= LIMIT["affine hl twin"]
    var = np.abs(d["running_var"])
    for bias in (None, d["bias"]):
        (s64, bs), (h64, bh) = so.bn_fold64(d["gamma"], d["beta"], d["running_mean"], var, bias, EPS)
        for fma in (False, True):
            s, h = fold32(d["gamma"], d["beta"], d["running_mean"], var, bias, fma)
            assert ratio(s, s64, bs, "fold scale") <= 0.6
            assert ratio(h, h64, bh, "fold shift") <= 0.6


@pytest.mark.parametrize("n,c", SHAPES)
def test_stats_restatement(n, c):
    d = so.row_case(n, c)
    ref = so.bn_stats64(d["x"], n, d["gamma"], d["beta"], EPS, MOM, d["running_mean"], d["running_var"])
    for lanes in (8, 2):                     # the scalar kernel's 8 row lanes; few lanes of the float4 kernel at wide c
        got = stats32(d["x"], d["gamma"], d["beta"], d["running_mean"], d["running_var"], lanes)
        for k, (v, b) in ref.items():
            assert ratio(got[k], v, b, k) <= LIMIT.get(k, 0.6), k
    if c >= 3 and n > 1:
        assert ref["var"][0][c - 1] == 0.0 and ref["var"][0][c // 2] < 1e-6


@pytest.mark.parametrize("n,c", SHAPES)
def test_backward_restatement(n, c):
    d = so.row_case(n, c)
    st = stats32(d["x"], d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    y = affine32(d["x"], st["scale"], st["shift"], d["res"], True, True)
    for mask in (None, y > 0):
        ref = so.bn_backward64(d["x"], d["dy"], mask, st["mean"], st["var"], d["gamma"], n, EPS)
        got = backward32(d["x"], d["dy"], mask, st["mean"], st["var"], d["gamma"])
        for k, (v, b) in ref.items():
            if k == "dres":
                assert np.array_equal(got[k], v)
            else:
                assert ratio(got[k], v, b, k) <= 0.6, k


@pytest.mark.parametrize("n,c", SHAPES)
def test_col_sum_restatement(n, c):
    x = so.row_case(n, c)["x"]
    s, b = so.col_sum64(x, col_chunks(n))
    assert ratio(col_sum32(x), s, b, "col_sum") <= 0.6


def test_col_sum_chunk_counts():
    assert [col_chunks(n) for n in (1, 1024, 1025, 262144, 262145, 10 ** 7)] == [1, 1, 2, 256, 256, 256]
    assert [bn_chunks(n) for n in (1, 255, 256, 511, 512, 262143, 262144, 262400)] == [1, 1, 1, 1, 2, 1023, 1024, 1024]


@pytest.mark.parametrize("n,c", [(1, 32), (257, 96), (4099, 128)])
def test_hl_bits_model(n, c):
    """h + l reproduces x to 2^-23 relative plus 2^-25 absolute (a subnormal l); the layout is 32 h then 32 l per chunk"""
    x = so.row_case(n, c)["x"]
    x[0, :4] = [0.0, 2.0 ** -14, 3e-6, 65000.0]
    bits = so.hl_bits(x)
    assert bits.shape == x.shape and bits.dtype == np.uint32
    back = so.hl_decode(bits).astype(np.float64)
    assert (np.abs(back - x) <= 2 * so.U24 * np.abs(x) + 2.0 ** -25).all()
    big = np.abs(x) >= 0.25                  # a subnormal l's 2^-25 is within 2u |x| from here on: purely relative
    assert (np.abs(back - x)[big] <= 2 * so.U24 * np.abs(x)[big]).all()
    h = np.ascontiguousarray(bits).view(np.float16).reshape(n, c // 32, 2, 32)
    assert np.array_equal(h[:, :, 0].reshape(n, c), x.astype(np.float16))


@pytest.mark.parametrize("ncls,ld", [(1, 8), (9, 64), (20, 141)])
@pytest.mark.parametrize("log_scale", [0, 1])
def test_head_restatements(ncls, ld, log_scale):
    f, planted = head_rows(1000, ncls, ld)
    xyz, scale, prob, cls = so.head_joint64(f, ncls, log_scale)
    gx, gs, gp, gc = head_joint32(f, ncls, log_scale)
    assert np.array_equal(gx, xyz) and np.array_equal(gc, cls)
    if log_scale:
        assert ratio(gs, scale, 2e-6 * np.abs(scale), "head scale") <= 0.6
    else:
        assert np.array_equal(gs, scale)
    assert ratio(gp, prob, np.where(prob >= 1e-3, 2e-6 * prob, 2e-6 * prob + 1e-7), "head prob") <= 0.6
    fs = f[:, :8]
    x64, s64, p64 = so.head_separate64(fs, log_scale)
    mx = np.maximum(fs[:, 6], fs[:, 7])
    e0, e1 = np.exp(fs[:, 6] - mx), np.exp(fs[:, 7] - mx)
    assert ratio(e1 / (e0 + e1), p64, np.where(p64 >= 1e-3, 2e-6 * p64, 2e-6 * p64 + 1e-7), "head prob") <= 0.6


# ---- (b) named wrong results are far outside ------------------------------------------------------------------------------
MUT = [(257, 96), (4099, 128)]


def _bwd_case(n, c):
    d = so.row_case(n, c)
    st = stats32(d["x"], d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    y = affine32(d["x"], st["scale"], st["shift"], d["res"], True, True)
    return d, st, y


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_a_dropped_row(n, c):
    d, st, y = _bwd_case(n, c)
    ref = so.bn_backward64(d["x"], d["dy"], None, st["mean"], st["var"], d["gamma"], n, EPS)
    bad = backward32(d["x"], d["dy"], None, st["mean"], st["var"], d["gamma"], drop_row=n // 2)
    assert ratio(bad["dbeta"], *ref["dbeta"]) >= 10
    assert ratio(bad["dgamma"], *ref["dgamma"]) >= 10


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_mask_taken_as_not_negative(n, c):
    d, st, y = _bwd_case(n, c)
    assert (y == 0).any()
    ref = so.bn_backward64(d["x"], d["dy"], y > 0, st["mean"], st["var"], d["gamma"], n, EPS)
    bad = backward32(d["x"], d["dy"], y >= 0, st["mean"], st["var"], d["gamma"])
    for k in ("dbeta", "dgamma", "dx"):
        assert ratio(bad[k], *ref[k]) >= 10, k
    assert not np.array_equal(bad["dres"], ref["dres"][0])


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_n_minus_one_in_dx(n, c):
    d, st, y = _bwd_case(n, c)
    ref = so.bn_backward64(d["x"], d["dy"], y > 0, st["mean"], st["var"], d["gamma"], n, EPS)
    bad = backward32(d["x"], d["dy"], y > 0, st["mean"], st["var"], d["gamma"], inv_n=1.0 / (n - 1))
    assert ratio(bad["dx"], *ref["dx"]) >= 10


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_unbiased_variance(n, c):
    d = so.row_case(n, c)
    ref = so.bn_stats64(d["x"], n, d["gamma"], d["beta"], EPS)
    got = stats32(d["x"], d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    assert ratio((got["var"].astype(np.float64) * n / (n - 1)).astype(f32), *ref["var"]) >= 10


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_missing_eps(n, c):
    """on the channel of variance < 1e-6 (eps = 1e-5 is most of var + eps there)"""
    d, st, y = _bwd_case(n, c)
    k = c // 2
    assert st["var"][k] < 1e-6
    ref = so.bn_backward64(d["x"], d["dy"], y > 0, st["mean"], st["var"], d["gamma"], n, EPS)
    with np.errstate(divide="ignore", invalid="ignore"):          # (the constant channel: 1 / sqrt(0))
        bad = backward32(d["x"], d["dy"], y > 0, st["mean"], st["var"], d["gamma"], eps=0.0)
    for q in ("dgamma", "dx"):
        v, b = ref[q]
        assert ratio(bad[q][..., k], v[..., k], b[..., k]) >= 10, q
    # ... and in the folded scale of the statistics call
    s = so.bn_stats64(d["x"], n, d["gamma"], d["beta"], EPS)["scale"]
    assert ratio((d["gamma"][k:k + 1] / np.sqrt(st["var"][k:k + 1])), s[0][k:k + 1], s[1][k:k + 1]) >= 10


@pytest.mark.parametrize("n,c", MUT)
def test_bound_rejects_residual_after_relu(n, c):
    d = so.row_case(n, c)
    z, b = so.affine64(d["x"], d["gamma"], d["beta"], d["res"], True)
    bad = affine32(d["x"], d["gamma"], d["beta"], None, True, True) + d["res"]
    assert ratio(bad, z, b) >= 10


@pytest.mark.parametrize("n,c", [(4099, 128), (2049, 33)])
def test_bound_rejects_a_dropped_chunk(n, c):
    x = so.row_case(n, c)["x"]
    s, b = so.col_sum64(x, col_chunks(n))
    assert col_chunks(n) >= 2
    r = np.abs(col_sum32(x, drop_chunk=1).astype(np.float64) - s) / b
    assert r[:c // 2].min() >= 10            # every channel that is not (nearly) constant zero-mean noise


def test_hl_bits_rejects_truncation():
    """pieces cut off instead of rounded to nearest even: the words differ (the GPU check is bit-exact)"""
    x = so.row_case(257, 96)["x"]

    def trunc16(a):
        h = a.astype(np.float16)
        up = np.abs(h.astype(np.float32)) > np.abs(a)
        return np.where(up, np.nextafter(h, np.float16(0)), h).astype(np.float16)

    h = trunc16(x)
    l = trunc16(x - h.astype(f32))
    bad = np.ascontiguousarray(np.stack([h.reshape(257, 3, 32), l.reshape(257, 3, 32)], 2)).view(np.uint32).reshape(257, 96)
    assert (bad != so.hl_bits(x)).mean() > 0.4


@pytest.mark.parametrize("ncls,ld", [(9, 64), (20, 141)])
def test_heads_reject_the_named_mistakes(ncls, ld):
    f, planted = head_rows(1000, ncls, ld)
    xyz, scale, prob, cls = so.head_joint64(f, ncls, 1)
    bad_xyz = head_joint32(f, ncls, 1, background_rule=False)[0]
    bg = f[:, 6 * ncls:7 * ncls + 1].argmax(1) == ncls
    assert bg.sum() >= 10 and (bad_xyz[bg] != xyz[bg]).any(1).all() and np.array_equal(bad_xyz[~bg], xyz[~bg])
    bad_prob = head_joint32(f, ncls, 1, prob_over_all=True)[2]
    tol = np.where(prob >= 1e-3, 2e-6 * prob, 2e-6 * prob + 1e-7)
    assert (np.abs(bad_prob - prob)[bg] / tol[bg]).min() >= 10


# ---- (c) the float64 heads against the torch head split ------------------------------------------------------------------
@pytest.mark.parametrize("ncls,ld", [(1, 8), (9, 64), (20, 141)])
@pytest.mark.parametrize("log_scale", [False, True])
def test_heads64_match_the_torch_oracle(ncls, ld, log_scale):
    f, planted = head_rows(1000, ncls, ld)
    keep = np.setdiff1d(np.arange(1000), planted)
    f64 = torch.from_numpy(f[keep, :7 * ncls + 1].astype(np.float64))
    got = so.head_joint64(f[keep], ncls, log_scale)
    for a, b in zip(got, so.head_joint_eval(f64, ncls, log_scale)):
        assert (np.abs(a - b.numpy()) <= 1e-12 * np.maximum(1.0, np.abs(a))).all()
    got = so.head_separate64(f[:, :8], log_scale)
    for a, b in zip(got, so.head_separate_eval(torch.from_numpy(f[:, :8].astype(np.float64)), log_scale)):
        assert (np.abs(a - b.numpy()) <= 1e-12 * np.maximum(1.0, np.abs(a))).all()
    # ties: the first index wins, the background selects head 0
    if ncls >= 2:
        xyz, _, _, cls = so.head_joint64(f[planted], ncls, log_scale)
        lg = f[planted, 6 * ncls:7 * ncls + 1]
        both = (lg[:, 0] == lg[:, ncls - 1]) & (lg[:, 0] == lg.max(1))
        assert both.any() and (cls[both] == 0).all() and np.array_equal(xyz[both], f[planted][both, :3])


def test_zz_report_ratios():
    """not a check of its own: prints the worst restatement ratios of this run (pytest -s)"""
    for k in sorted(RATIOS):
        print("%-14s %.3f" % (k, RATIOS[k]))
        assert RATIOS[k] <= LIMIT.get(k, 0.6)
