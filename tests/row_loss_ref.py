"""fp64 oracle, error bounds, restatement of the kernels' sequence and case generator of the per-row losses
(cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32, canonicalvoting_amd/csrc/row_loss.hip; definitions in include/cv_hip.h), shared by
tests/test_row_loss.py, tests/test_row_loss_gpu.py and tests/test_validate_gpu.py.

Error model (derived, not fitted), u = 2^-24 the unit roundoff of fp32, eps = 2^-53 that of fp64.  The kernels read fp32
inputs, form every term in fp64 (the difference of two fp32 values is exact there), add in fp64 and round to fp32 once per
output.  n <= 2^31 rows, so every fp64 sum of n non-negative terms grows by at most n eps < 2^-22 u relative to its value.

  loss_xyz    terms w_c (p - x)^2 with 2 roundings (<= 2 eps each, relative), the sum (3 cnt eps), one product with the factor,
              one division, ONE rounding to fp32: <= u + (3 cnt + 6) eps of the value.  Bound: 4 u * value.
  loss_scale  the same, plus the target t = log(s) when log_scale: a correctly-rounded-or-nearly log is within 2 eps |t| (the
              kernel's and this oracle's each), which moves a term w (p - t)^2 by up to w (2 |p - t| + dt) dt, dt = 4 eps |t| -
              an ABSOLUTE amount that does not shrink with the term.  Bound: 4 u * value + factor / denom * sum of that with
              eps taken as 2^-50 (8 x).
  loss_class  ce = (mx + log(sum_k exp(l_k - mx))) - l_target per row: the exponentials and their sum of <= 16 are within
              20 eps relative, so log(sum) is within 20 eps + eps |log(sum)| absolute; mx + . rounds by eps |lse|, the
              difference by eps |ce| <= eps (|lse| + |l_target|).  Per row <= eps * A, A = 3 |lse| + |l_target| + 24, absolute (the
              cancellation at a confident row - lse = l_target - leaves no relative bound: logits +-90 give ce = 0 exactly where
              the true value is 1e-77).  Bound: 4 u * value + 2^-50 * mean(A).
  total       (loss_scale + loss_xyz) + loss_class in fp32 from the three rounded values: two roundings of partial sums of
              non-negative values.  Bound: the three bounds + 2 u * (sum of the three values).
  gradient    head columns ((g factor 2 w) (p - t)) / denom: 4 fp64 roundings and one to fp32, <= (1 + 2^-27) u |value|; with
              log_scale the target's 4 eps |t| adds |g factor 2 w / denom| * 4 eps |t|.  Bound: 4 u |value| + that with 2^-50.
              logit columns (g (e_k / sum - [k = target])) / n: e_k / sum within 24 eps relative, the subtraction of 1 cancels:
              absolute 24 eps softmax_k |g| / n.  Bound: 4 u |value| + 2^-48 * softmax_k |g| / n.
              every other column: exactly 0.
  underflow   a rounding to fp32 of a value below 2^-126 is absolute, at most 2^-150 (half the smallest subnormal; a cold logit
              at -90 under a hot one at +90 has a softmax of 1e-78): every bound carries + 2^-149.

The kernel's arithmetic is well inside these bounds (tests/test_row_loss.py measures the restatement against them); they come
from the number formats and are not to be moved towards what a GPU returns.
"""
import numpy as np

U = 2.0 ** -24
REL = 4.0                     # every bound's relative part, in units of u
ABS_EPS = 2.0 ** -50          # the eps of the absolute parts (8 x 2^-53)
TINY32 = 2.0 ** -149          # the smallest fp32 subnormal: twice the absolute error of a rounding below the normal range
LAYOUTS = {"joint": dict(heads=9, n_logits=10, xyz_col=0, scale_col=27, logit_col=54, obj_lo=0, obj_hi=8, with_xyz=1),
           "separate": dict(heads=1, n_logits=2, xyz_col=0, scale_col=3, logit_col=6, obj_lo=1, obj_hi=1, with_xyz=0)}
MUTANTS = ("argmax_head", "denom_cnt", "times_zero", "no_max_fp32", "neg_index")


def config(layout="joint", gather="label", empty="zero", log_scale=True, w=(1.0, 1.0, 1.0), xyz_factor=1.0, scale_factor=1.0,
           grad_loss=1.0):
    c = dict(LAYOUTS[layout])
    c.update(layout=layout, gather=gather, empty=empty, log_scale=bool(log_scale), w=tuple(w), xyz_factor=xyz_factor,
             scale_factor=scale_factor, grad_loss=grad_loss)
    return c


def _first_argmax(logits32):
    """the first maximum under fp32 `>` (cv_head_joint_f32's comparison)"""
    return np.argmax(logits32, axis=1)


def _rows(out, labels, c, head_from_argmax=None, neg_index=False):
    """what every row needs, fp64 from the fp32 inputs: obj, head, target, logits"""
    out = np.asarray(out, np.float32)
    y = np.asarray(labels, np.int64)
    L, H = c["n_logits"], c["heads"]
    logits = out[:, c["logit_col"]:c["logit_col"] + L]
    obj = (y >= c["obj_lo"]) & (y <= c["obj_hi"])
    use_argmax = (c["gather"] == "argmax") if head_from_argmax is None else head_from_argmax
    if H == 1:
        h = np.zeros(len(y), np.int64)
    elif use_argmax:
        am = _first_argmax(logits)
        h = np.where(am == L - 1, 0, am)
    else:
        h = np.where(obj, y, 0)
    bad = y > L - 1
    tgt = np.where(y < 0, y if neg_index else L - 1, np.where(bad, 0, y))
    return out, y, logits.astype(np.float64), obj, h, tgt, bad


def oracle(out, labels, xyz_labels, scale_labels, c, mutate=None):
    """fp64 losses and gradient, with the bound of every output.  Returns dict: losses [4] = (loss_xyz, loss_scale, loss_class,
    total), loss_bounds [4], cnt, n_bad, grad [N, C], grad_bounds [N, C], grad_zero [N, C] (where the gradient is an exact 0).
    mutate: one of MUTANTS, the named wrong results."""
    assert mutate is None or mutate in MUTANTS
    out, y, logits, obj, h, tgt, bad = _rows(out, labels, c, head_from_argmax=True if mutate == "argmax_head" else None,
                                             neg_index=mutate == "neg_index")
    n, C = out.shape
    L = c["n_logits"]
    w = np.asarray(c["w"], np.float32).astype(np.float64)
    xf, sf, gl = (float(np.float32(c[k])) for k in ("xyz_factor", "scale_factor", "grad_loss"))
    cnt = int(obj.sum())
    per = 1.0 if mutate == "denom_cnt" else 3.0
    denom = np.float64(per * cnt if c["empty"] == "nan" else max(per * cnt, 1.0))
    rows = np.nonzero(obj)[0]
    if mutate == "times_zero":
        rows = np.arange(n)                         # every row goes through the arithmetic and is multiplied by its mask
    mask = obj[rows].astype(np.float64)[:, None]
    hh = h[rows]
    cols3 = np.arange(3)[None, :]
    grad = np.zeros((n, C))
    gb = np.zeros((n, C))
    with np.errstate(all="ignore"):
        # scale term
        s_lab = np.asarray(scale_labels, np.float32)[rows].astype(np.float64)
        t = np.log(s_lab) if c["log_scale"] else s_lab
        dt = 4.0 * ABS_EPS * np.abs(t) if c["log_scale"] else np.zeros_like(t)
        sc = c["scale_col"] + 3 * hh[:, None] + cols3
        ds = out[rows[:, None], sc].astype(np.float64) - t
        sum_scale = float((w * ds * ds * mask).sum()) if len(rows) else 0.0
        abs_scale = float((w * (2.0 * np.abs(ds) + dt) * dt).sum()) if len(rows) else 0.0
        loss_scale = sf * sum_scale / denom if (cnt or c["empty"] == "nan") else 0.0
        b_scale = REL * U * abs(loss_scale) + (abs(sf) * abs_scale / denom if cnt else 0.0)
        g = gl * sf * 2.0 * w * ds * mask / denom
        grad[rows[:, None], sc] = g
        gb[rows[:, None], sc] = REL * U * np.abs(g) + np.abs(gl * sf * 2.0 * w / denom) * dt
        # coordinate term
        sum_xyz = 0.0
        if c["with_xyz"]:
            xc = c["xyz_col"] + 3 * hh[:, None] + cols3
            dx = out[rows[:, None], xc].astype(np.float64) - np.asarray(xyz_labels, np.float32)[rows].astype(np.float64)
            sum_xyz = float((w * dx * dx * mask).sum()) if len(rows) else 0.0
            g = gl * xf * 2.0 * w * dx * mask / denom
            grad[rows[:, None], xc] = g
            gb[rows[:, None], xc] = REL * U * np.abs(g)
        loss_xyz = xf * sum_xyz / denom if (cnt or c["empty"] == "nan") else 0.0
        b_xyz = REL * U * abs(loss_xyz)
        # cross entropy
        if mutate == "no_max_fp32":
            e = np.exp(out[:, c["logit_col"]:c["logit_col"] + L]).astype(np.float64)          # fp32, nothing subtracted
            lse = np.log(e.sum(1))
        else:
            mx = logits.max(1)
            e = np.exp(logits - mx[:, None])
            lse = mx + np.log(e.sum(1))
        picked = out[np.arange(n), c["logit_col"] + tgt].astype(np.float64) if n else np.zeros(0)
        ce = np.where(bad, np.nan, lse - picked)
        loss_class = float(ce.sum() / n) if n else float("nan")
        A = 3.0 * np.abs(lse) + np.abs(picked) + 24.0
        b_class = REL * U * abs(loss_class) + ABS_EPS * (float(A.mean()) if n else 0.0)
        soft = e / e.sum(1, keepdims=True)
        onehot = (np.arange(L)[None, :] == tgt[:, None]).astype(np.float64)
        gl_logit = np.where(bad[:, None], np.nan, gl * (soft - onehot) / max(n, 1))
        lc = slice(c["logit_col"], c["logit_col"] + L)
        grad[:, lc] = gl_logit
        gb[:, lc] = REL * U * np.abs(gl_logit) + 4.0 * ABS_EPS * soft * abs(gl) / max(n, 1)
    if n == 0:
        vals = [float("nan")] * 3 if c["empty"] == "nan" else [0.0] * 3
        loss_xyz, loss_scale, loss_class = vals
    total = (loss_scale + loss_xyz) + loss_class
    b_total = b_xyz + b_scale + b_class + 2.0 * U * (abs(loss_scale) + abs(loss_xyz) + abs(loss_class))
    live = gb != 0                                  # (NaN bounds of a bad label's row included)
    return {"losses": np.array([loss_xyz, loss_scale, loss_class, total]),
            "loss_bounds": np.array([b_xyz, b_scale, b_class, b_total]) + TINY32,
            "cnt": cnt, "n_bad": int(bad.sum()), "grad": grad, "grad_bounds": np.where(live, gb + TINY32, 0.0), "grad_zero": ~live}


def worst_ratios(got_losses, got_grad, ref):
    """largest |got - ref| / bound: (per loss [4], over the gradient elements).  A ratio <= 1 is inside.  NaN agrees with NaN
    only; any other non-finite disagreement is inf."""
    tiny = np.finfo(np.float64).tiny

    def ratio(x, r, b):
        x, r, b = (np.asarray(v, np.float64) for v in (x, r, b))
        with np.errstate(all="ignore"):
            q = np.abs(x - r) / np.maximum(b, tiny)
        q = np.where(np.isnan(x) & np.isnan(r), 0.0, q)
        q = np.where((np.isnan(x) != np.isnan(r)) | (np.isinf(x) & ~(x == r)), np.inf, q)
        q = np.where((x == r), 0.0, q)
        return q

    lr = ratio(got_losses, ref["losses"], ref["loss_bounds"])
    gr = ratio(got_grad, ref["grad"], ref["grad_bounds"]) if got_grad is not None else np.zeros(1)
    return lr, (float(gr.max()) if gr.size else 0.0)


def assert_within(got_losses, got_grad, ref, what=""):
    lr, gr = worst_ratios(got_losses, got_grad, ref)
    print("%s: error / bound  xyz %.3f  scale %.3f  class %.3f  total %.3f  grad %.3f" % ((what,) + tuple(lr) + (gr,)))
    assert (lr <= 1.0).all() and gr <= 1.0, (what, lr, gr)
    if got_grad is not None:
        assert not np.asarray(got_grad)[ref["grad_zero"]].any(), what       # exactly zero, not merely small


def _halve(v):
    """halving tree over the last axis (a power of two): lane t += lane t + half - the kernels' LDS trees and, for the sum
    every lane ends with, their xor butterfly"""
    v = np.array(v, np.float64)
    while v.shape[-1] > 1:
        half = v.shape[-1] // 2
        v = v[..., :half] + v[..., half:]
    return v[..., 0]


def lanes_per_row(c):
    last = max(c["logit_col"] + c["n_logits"], c["scale_col"] + 3 * c["heads"], (c["xyz_col"] + 3 * c["heads"]) if c["with_xyz"] else 0)
    return 4 if (c["n_logits"] <= 4 and last <= 16) else 16


def restate(out, labels, xyz_labels, scale_labels, c, chunk=256, n_cols=None):
    """The kernels' own sequence in numpy: per row exp(logit - max) per lane and a halving tree over the LPR lanes, the squared
    errors (c0 + c1) + c2; per chunk of 256 rows lane 0 of group g adds rows g, g + R, ... in pass order (R = 256 / LPR), a
    halving tree over the R groups; the finish pass adds contiguous stretches of ceil(chunks / 256) partials per lane in order
    and halves over 256 lanes; one rounding to fp32 per output, the total in fp32.  The gradient element by element in the
    kernel's order of operations.  Returns (losses [4] float32, info [2], grad [N, n_cols] float32 or None for argmax)."""
    assert chunk == 256, "the lane layout below is written for 256-thread workgroups of 256 rows"
    out, y, logits, obj, h, tgt, bad = _rows(out, labels, c)
    n, C = out.shape
    n_cols = C if n_cols is None else n_cols
    L, LPR = c["n_logits"], lanes_per_row(c)
    R = 256 // LPR
    w = np.asarray(c["w"], np.float32).astype(np.float64)
    xf, sf, gl = (float(np.float32(c[k])) for k in ("xyz_factor", "scale_factor", "grad_loss"))
    if n == 0:
        fill = np.float32(np.nan if c["empty"] == "nan" else 0.0)
        return np.full(4, fill, np.float32), np.zeros(2, np.int64), np.zeros((0, n_cols), np.float32)
    with np.errstate(all="ignore"):
        l32 = out[:, c["logit_col"]:c["logit_col"] + L]
        mx = l32[np.arange(n), _first_argmax(l32)].astype(np.float64)
        e = np.zeros((n, LPR))
        e[:, :L] = np.exp(logits - mx[:, None])
        ssum = _halve(e)
        picked = np.where(bad, np.nan, out[np.arange(n), c["logit_col"] + tgt].astype(np.float64))
        ce = (mx + np.log(ssum)) - picked
        cols3 = np.arange(3)[None, :]
        safe = np.where(obj[:, None], np.asarray(scale_labels, np.float32).astype(np.float64), 1.0)
        t = np.log(safe) if c["log_scale"] else safe
        ds = out[np.arange(n)[:, None], c["scale_col"] + 3 * h[:, None] + cols3].astype(np.float64) - t
        ts = np.where(obj[:, None], w * (ds * ds), 0.0)
        e_scale = (ts[:, 0] + ts[:, 1]) + ts[:, 2]
        e_xyz = np.zeros(n)
        if c["with_xyz"]:
            dx = out[np.arange(n)[:, None], c["xyz_col"] + 3 * h[:, None] + cols3].astype(np.float64) \
                - np.asarray(xyz_labels, np.float32).astype(np.float64)
            tx = np.where(obj[:, None], w * (dx * dx), 0.0)
            e_xyz = (tx[:, 0] + tx[:, 1]) + tx[:, 2]
        chunks = (n + chunk - 1) // chunk
        vals = np.zeros((4, chunks * chunk))
        vals[0, :n], vals[1, :n], vals[2, :n], vals[3, :n] = e_xyz, e_scale, ce, obj
        vals = vals.reshape(4, chunks, chunk // R, R)
        acc = np.zeros((4, chunks, R))
        for p in range(chunk // R):
            acc = acc + vals[:, :, p, :]
        partial = _halve(acc)                                               # [4, chunks]
        per = (chunks + 255) // 256
        lanes = np.zeros((4, 256))
        for t_ in range(256):
            for b in range(min(t_ * per, chunks), min(t_ * per + per, chunks)):
                lanes[:, t_] = lanes[:, t_] + partial[:, b]
        tot = _halve(lanes)
        cnt = tot[3]
        denom = 3.0 * cnt if c["empty"] == "nan" else max(3.0 * cnt, 1.0)
        lx = np.float32((xf * tot[0]) / denom)
        ls = np.float32((sf * tot[1]) / denom)
        lc = np.float32(tot[2] / float(n))
        losses = np.array([lx, ls, lc, np.float32(np.float32(ls + lx) + lc)], np.float32)
        info = np.array([int(cnt), int(bad.sum())], np.int64)
        if c["gather"] == "argmax":
            return losses, info, None
        grad = np.zeros((n, C))
        onehot = (np.arange(L)[None, :] == tgt[:, None]).astype(np.float64)
        grad[:, c["logit_col"]:c["logit_col"] + L] = np.where(bad[:, None], np.nan, (gl * (e[:, :L] / ssum[:, None] - onehot)) / float(n))
        r = np.nonzero(obj)[0]
        c_xyz, c_scale = (gl * xf) * 2.0, (gl * sf) * 2.0
        grad[r[:, None], c["scale_col"] + 3 * h[r][:, None] + cols3] = ((c_scale * w) * ds[r]) / denom
        if c["with_xyz"]:
            grad[r[:, None], c["xyz_col"] + 3 * h[r][:, None] + cols3] = ((c_xyz * w) * dx[r]) / denom
    return losses, info, grad[:, :n_cols].astype(np.float32)


def make_case(seed, n, layout="joint", ld=None, labels="mixed", logits=None, poison=False, bad_label=False):
    """(out [n, ld] float32, labels int64 [n], xyz_labels [n, 3], scale_labels [n, 3]).  labels: 'mixed' (joint: -1 .. 9, so
    both background values; separate: 0 / 1), 'objects', 'background'.  logits 'pm90': every logit +90 or -90, one +90 per row.
    poison: NaN / +-Inf in the coordinate and scale columns (all heads) of background rows.  bad_label: row n // 2 gets the
    label n_logits (one above the last logit)."""
    c = LAYOUTS[layout]
    rng = np.random.default_rng(seed)
    width = c["logit_col"] + c["n_logits"]
    ld = width if ld is None else ld
    out = rng.normal(0, 0.5, (n, ld)).astype(np.float32)
    if layout == "joint":
        y = {"mixed": rng.integers(-1, 10, n), "objects": rng.integers(0, 9, n), "background": rng.choice([-1, 9], n)}[labels]
    else:
        y = {"mixed": rng.integers(0, 2, n), "objects": np.ones(n, np.int64), "background": np.zeros(n, np.int64)}[labels]
    y = y.astype(np.int64)
    if bad_label and n:
        y[n // 2] = c["n_logits"]
    if logits == "pm90":
        hot = rng.integers(0, c["n_logits"], n)
        lg = np.full((n, c["n_logits"]), -90.0, np.float32)
        lg[np.arange(n), hot] = 90.0
        out[:, c["logit_col"]:width] = lg
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    scale = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
    if poison:
        bg = np.nonzero(~((y >= c["obj_lo"]) & (y <= c["obj_hi"])))[0]
        vals = np.array([np.nan, np.inf, -np.inf], np.float32)
        for i, r in enumerate(bg):
            out[r, :c["logit_col"]] = vals[i % 3]
    return out, y, xyz, scale
