"""fp64 oracle, error bounds, fp32 restatement and case generator of the packed symmetry loss (cv_sym_loss_fwd_f32 /
cv_sym_loss_bwd_f32, canonicalvoting_amd/csrc/sym_loss.hip), shared by tests/test_sym_loss.py and tests/test_sym_loss_gpu.py.

Error model (derived, not fitted), u = 2^-24 the unit roundoff of fp32.  The kernels read fp32 predictions, targets and
weights, form every term w_c * (p - x)^2 in fp64 (the difference of two fp32 values is exact in fp64), add in fp64 and round to
fp32 once per output.  With eps = 2^-53:

  pose loss   fp64 sum of n = 3 len non-negative terms, each with at most 2 eps relative error (square, times weight), in a
              tree of depth <= 3 + 6 + 2 + chunks: relative error <= (n + 2) eps of the value since sum|t| = value; one fp64
              division (eps) and ONE rounding to fp32 (u).  Total <= u + (n + 4) eps < 1.001 u for n < 2^18.  The bound the
              tests hold it to is 8 u * value.
  loss        the selected fp32 pose losses (each within the above of the oracle's), an fp64 sum over the segments, one division,
              one product with xyz_factor (fp32 -> fp64 exact), one rounding to fp32: <= 2 u + O(S eps) of the value, all terms
              non-negative.  The bound is 12 u * value.
  gradient    element with m contributions c_i = coef * w * (p - x) / den: each c_i carries 4 fp64 roundings (<= 4 eps |c_i|),
              the fp64 sum m eps sum|c_i|, one rounding to fp32 of the sum (u |sum c_i| <= u sum|c_i|): <= (1 + (m + 4) 2^-29) u
              sum|c_i|.  The bound is (8 + m) u * sum_i |c_i| with the sum from this oracle.

The kernel's arithmetic is well inside the three bounds; they are the ones the feature was specified with and are not to be
moved towards what a GPU returns.
The minimum over poses is taken on the fp32 pose losses: it agrees with the oracle's fp64 minimum whenever best and second-best
differ by more than their two bounds, and `decidable` requires 4 x the bound for every segment of every case.
"""
import numpy as np

from canonicalvoting_amd import data

U = 2.0 ** -24
POSE_BOUND, LOSS_BOUND, GRAD_BOUND = 8.0, 12.0, 8.0            # in units of u; GRAD_BOUND + m per gradient element


def _np(sym):
    """the SymBatch's arrays as numpy"""
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in sym._asdict().items()}


def oracle(out, sym, w=(1.0, 1.0, 1.0), xyz_factor=1.0, grad_loss=1.0, mutate=None):
    """fp64 loss and gradient of predictions ``out`` [N, >= 3] (float32) over a CPU SymBatch.
    Returns dict: pose_loss [J], best [S], second [S] (second-smallest pose loss, inf with one pose), seg_loss [S], loss,
    grad [N, 3], grad_abs [N, 3] (sum of |contribution|), grad_m [N] (contributions per element).
    mutate: one of the named wrong results - 'mean_len', 'max', 'no_weights', 'pose0', 'no_factor2'."""
    a = _np(sym)
    S = sym.n_segments
    p64 = np.asarray(out, np.float32)[:, :3].astype(np.float64)
    w64 = np.asarray(w, np.float32).astype(np.float64)
    if mutate == "no_weights":
        w64 = np.ones(3)
    xf = float(np.float32(xyz_factor))
    gl = float(np.float32(grad_loss))
    pose_loss = np.zeros(sym.n_jobs)
    best = np.zeros(S, np.int64)
    second = np.full(S, np.inf)
    seg_loss = np.zeros(S)
    n = p64.shape[0]
    grad, grad_abs, grad_m = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
    for s in range(S):
        b, e = int(a["seg_ptr"][s]), int(a["seg_ptr"][s + 1])
        ln = e - b
        rows = a["rows"][b:e].astype(np.int64)
        j0, j1 = int(a["pose_ptr"][s]), int(a["pose_ptr"][s + 1])
        t0 = int(a["tgt_ptr"][s])
        tg = a["targets"][t0:t0 + (j1 - j0) * ln].astype(np.float64).reshape(j1 - j0, ln, 3)
        pl = ((p64[rows][None] - tg) ** 2 * w64).sum((1, 2)) / (ln if mutate == "mean_len" else 3.0 * ln)
        pose_loss[j0:j1] = pl
        if np.isnan(pl).any():
            k = int(np.argmax(np.isnan(pl)))
        else:
            k = int(np.argmax(pl)) if mutate == "max" else int(np.argmin(pl))      # argmin: the lowest index on ties
        best[s], seg_loss[s] = k, pl[k]
        if j1 - j0 > 1:
            second[s] = np.sort(pl)[1] if mutate != "max" else np.sort(pl)[-2]
        kg = 0 if mutate == "pose0" else k
        c = gl * xf * (1.0 if mutate == "no_factor2" else 2.0) * w64 * (p64[rows] - tg[kg]) / (3.0 * ln * S)
        np.add.at(grad, rows, c)
        np.add.at(grad_abs, rows, np.abs(c))
        np.add.at(grad_m, rows, 1)
    loss = xf * seg_loss.sum() / S if S else 0.0
    return {"pose_loss": pose_loss, "best": best, "second": second, "seg_loss": seg_loss, "loss": loss, "grad": grad,
            "grad_abs": grad_abs, "grad_m": grad_m}


def decidable(ref):
    """smallest margin over the segments of |second - best| / (4 x the pose bound of the larger one): > 1 everywhere means the
    fp32 minimum is the fp64 minimum.  inf for a case whose segments all have one pose."""
    many = np.isfinite(ref["second"])
    if not many.any():
        return np.inf
    gap = np.abs(ref["second"][many] - ref["seg_loss"][many])
    return float(np.min(gap / (4.0 * POSE_BOUND * U * np.maximum(ref["second"][many], ref["seg_loss"][many]))))


def worst_ratios(got, ref):
    """largest |got - ref| / bound per output group (a ratio <= 1 is inside): dict pose_loss, seg_loss, loss, grad; and whether
    best matches exactly.  got: dict with pose_loss [J], best [S], seg_loss [S], loss (scalar), grad [N, 3]."""
    tiny = np.finfo(np.float64).tiny

    def ratio(x, r, bound):
        x, r, bound = np.asarray(x, np.float64), np.asarray(r, np.float64), np.asarray(bound, np.float64)
        if x.size == 0:
            return 0.0
        assert np.isfinite(x).all() and np.isfinite(r).all(), "non-finite value in a comparison of finite cases"
        return float(np.max(np.abs(x - r) / np.maximum(bound, tiny)))

    return {"pose_loss": ratio(got["pose_loss"], ref["pose_loss"], POSE_BOUND * U * ref["pose_loss"]),
            "seg_loss": ratio(got["seg_loss"], ref["seg_loss"], POSE_BOUND * U * ref["seg_loss"]),
            "loss": ratio(got["loss"], ref["loss"], LOSS_BOUND * U * ref["loss"]),
            "grad": ratio(got["grad"], ref["grad"], (GRAD_BOUND + ref["grad_m"][:, None]) * U * ref["grad_abs"]),
            "best": bool(np.array_equal(np.asarray(got["best"], np.int64), ref["best"]))}


def assert_within(got, ref, what=""):
    r = worst_ratios(got, ref)
    print("%s: error / bound  pose %.3f  seg %.3f  loss %.3f  grad %.3f  best exact %s"
          % (what, r["pose_loss"], r["seg_loss"], r["loss"], r["grad"], r["best"]))
    assert r["best"], what
    for k in ("pose_loss", "seg_loss", "loss", "grad"):
        assert r[k] <= 1.0, (what, k, r[k])
    unlabelled = ref["grad_m"] == 0
    assert not np.asarray(got["grad"])[unlabelled].any(), what          # exactly zero, not merely small


def restate(out, sym, w=(1.0, 1.0, 1.0), xyz_factor=1.0, grad_loss=1.0, chunk=256):
    """The kernels' own sequence in numpy: fp64 terms from fp32 inputs, per lane elements t, t + 256, t + 512 of a chunk's
    3 * chunk row-major elements, the shuffle tree over a wave, waves 0 + 1 + 2 + 3, chunk partials in chunk order, one
    division, one rounding to fp32; the minimum on the fp32 values; the segment losses per lane (t, t + 256, ...) and a halving
    tree over 256 lanes; the gradient per row over its points in ascending point order.  Same keys as the kernel's outputs."""
    assert chunk == 256, "the lane layout below is written for 256-thread workgroups of 256 rows"
    a = _np(sym)
    S = sym.n_segments
    p32 = np.asarray(out, np.float32)[:, :3]
    w64 = np.asarray(w, np.float32).astype(np.float64)
    xf, gl = float(np.float32(xyz_factor)), float(np.float32(grad_loss))
    pose_loss = np.zeros(sym.n_jobs, np.float32)
    best = np.zeros(S, np.int32)
    seg_loss = np.zeros(S, np.float32)
    for s in range(S):
        b, e = int(a["seg_ptr"][s]), int(a["seg_ptr"][s + 1])
        ln = e - b
        rows = a["rows"][b:e].astype(np.int64)
        j0, j1 = int(a["pose_ptr"][s]), int(a["pose_ptr"][s + 1])
        t0 = int(a["tgt_ptr"][s])
        pred = p32[rows].astype(np.float64).reshape(-1)
        wc = np.tile(w64, ln)
        for p in range(j1 - j0):
            tg = a["targets"][t0 + p * ln:t0 + (p + 1) * ln].astype(np.float64).reshape(-1)
            term = wc * ((pred - tg) * (pred - tg))
            total = 0.0
            for c0 in range(0, 3 * ln, 3 * chunk):
                el = np.zeros(3 * chunk)
                part = term[c0:c0 + 3 * chunk]
                el[:part.size] = part
                lane = (el[0:256] + el[256:512]) + el[512:768]          # acc = 0; acc += k0; += k1; += k2 (0 + x is exact)
                v = lane.reshape(4, 64).copy()
                for off in (32, 16, 8, 4, 2, 1):
                    v = v[:, :off] + v[:, off:2 * off]
                v = v[:, 0]
                total = total + (((v[0] + v[1]) + v[2]) + v[3])
            pose_loss[j0 + p] = np.float32(total / (3.0 * ln))
        pl = pose_loss[j0:j1]
        k = 0
        for p in range(1, j1 - j0):
            if pl[p] < pl[k] or (np.isnan(pl[p]) and not np.isnan(pl[k])):
                k = p
        best[s], seg_loss[s] = k, pl[k]
    lanes = np.zeros(256)
    for s in range(S):
        lanes[s % 256] += float(seg_loss[s])
    half = 128
    while half:
        lanes[:half] = lanes[:half] + lanes[half:2 * half]
        half //= 2
    loss = np.float32(xf * (lanes[0] / S)) if S else np.float32(0.0)
    grad = np.zeros((p32.shape[0], 3), np.float32)
    coef = (gl * xf) * 2.0
    for u, r in enumerate(a["urow"]):
        g = np.zeros(3)
        for i in a["upoint"][a["uptr"][u]:a["uptr"][u + 1]]:
            s = int(a["pseg"][i])
            b, ln = int(a["seg_ptr"][s]), int(a["seg_ptr"][s + 1] - a["seg_ptr"][s])
            x = a["targets"][int(a["tgt_ptr"][s]) + int(best[s]) * ln + (int(i) - b)].astype(np.float64)
            g = g + ((coef * w64) * (p32[r].astype(np.float64) - x)) / ((3.0 * ln) * S)
        grad[r] = g.astype(np.float32)
    return {"pose_loss": pose_loss, "best": best, "seg_loss": seg_loss, "loss": loss, "grad": grad}


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])


def make_case(seed, lens, poses, best_at, n_rows=None, ld=8, share=None):
    """A synthetic case: segment i has lens[i] points and poses[i] poses (rotations by 2 pi k / poses[i] about the up axis of
    points at a radius of 0.3 or more); the predictions are the targets of pose 0 (best_at[i] == 'first') or of the last pose
    ('last') plus 0.05 noise.  Rows are disjoint and shuffled over ``n_rows`` (default: 1.25 x the points + 7, so some rows
    stay unlabelled) unless ``share`` names, per segment, an earlier segment whose rows it re-uses (its first
    min(len, len_other) rows - those rows keep the earlier segment's predictions).
    Returns (out [n_rows, ld] float32 with the foreign columns random, nested label list for data.pack_sym of ONE scan)."""
    rng = np.random.default_rng(seed)
    total = int(sum(lens))
    n_rows = n_rows or int(total * 1.25) + 7
    free = rng.permutation(n_rows)
    out = rng.normal(0, 0.5, (n_rows, ld)).astype(np.float32)
    labels, taken = [], 0
    for i, (ln, n_pose, at) in enumerate(zip(lens, poses, best_at)):
        other = share[i] if share is not None else None
        if other is not None:
            reuse = labels[other][0][:min(ln, len(labels[other][0]))]
            rows = np.concatenate([reuse, free[taken:taken + ln - len(reuse)]])
            taken += ln - len(reuse)
        else:
            rows = free[taken:taken + ln]
            taken += ln
        ang = rng.uniform(0, 2 * np.pi, ln)
        rad = rng.uniform(0.3, 1.0, ln)
        x0 = np.stack([rad * np.cos(ang), rng.uniform(-1, 1, ln), rad * np.sin(ang)], 1)
        xyzs = [(x0 @ _ry(2 * np.pi * k / n_pose).T).astype(np.float32) for k in range(n_pose)]
        chosen = xyzs[0 if at == "first" else n_pose - 1]
        fresh = np.ones(ln, bool) if other is None else np.arange(ln) >= len(reuse)
        out[rows[fresh], :3] = (chosen + rng.normal(0, 0.05, (ln, 3)).astype(np.float32))[fresh]
        labels.append([rows.astype(np.int64), xyzs])
    assert taken <= n_rows
    return out, labels


def edge_lengths(chunk):
    return sorted({1, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 1})


def named_cases(chunk=256):
    """{name: (out, SymBatch, w, xyz_factor)}: the shapes tests/test_sym_loss_gpu.py runs through the C ABI and
    tests/test_sym_loss.py checks the restatement, the mutants and the decidable minimum on."""
    cases = {}
    lens = edge_lengths(chunk)
    k = len(lens)
    cyc = lambda seq, shift=0: [seq[(i + shift) % len(seq)] for i in range(k)]
    # every length with every pose count, the best pose first and last: four cases that rotate the pose counts over the lengths
    for shift in range(4):
        at = ["first" if (i + shift // 2) % 2 == 0 else "last" for i in range(k)]
        ld, w = (8, (1.0, 1.0, 1.0)) if shift % 2 == 0 else (11, (0.5, 2.0, 1.25))
        out, lab = make_case(100 + shift, lens, cyc([1, 2, 4, 36], shift), at, ld=ld)
        cases["lengths_%d" % shift] = (out, data.pack_sym([lab], [out.shape[0]]), w, 1.0)
    for n_pose, at in ((1, "first"), (4, "last"), (36, "first")):
        out, lab = make_case(200 + n_pose, [257], [n_pose], [at], ld=8)
        cases["one_segment_%d" % n_pose] = (out, data.pack_sym([lab], [out.shape[0]]), (1.0, 1.0, 1.0), 0.5)
    rng = np.random.default_rng(300)
    out, lab = make_case(300, rng.integers(1, 28, 300).tolist(), [[1, 2, 4, 36][i % 4] for i in range(300)],
                         ["first" if i % 3 else "last" for i in range(300)], ld=11)
    cases["segments_300"] = (out, data.pack_sym([lab], [out.shape[0]]), (0.5, 2.0, 1.25), 1.0)
    # rows shared by two and by three segments (segment 1 and 2 re-use rows of 0; 4 of 3)
    out, lab = make_case(400, [300, 200, 120, 70, 70, 9], [4, 2, 36, 1, 4, 2], ["last", "first", "last", "first", "last", "first"],
                         share=[None, 0, 0, None, 3, None])
    cases["shared_rows"] = (out, data.pack_sym([lab], [out.shape[0]]), (0.5, 2.0, 1.25), 2.0)
    # two scans: under the reference's indexing their row numbers collide, under the repaired one they are offset
    out_a, lab_a = make_case(500, [130, 40], [4, 2], ["last", "first"], n_rows=260)
    out_b, lab_b = make_case(501, [90, 257], [36, 1], ["first", "first"], n_rows=400)
    both = np.concatenate([out_a, out_b])
    for ref_idx in (True, False):
        cases["two_scans_%s" % ("reference" if ref_idx else "offset")] = (
            both, data.pack_sym([lab_a, lab_b], [260, 400], reference_indexing=ref_idx), (1.0, 1.0, 1.0), 1.0)
    return cases


def golden_cases():
    """the mini dataset's two-scan batch (tests/golden/make_loss_golden.make_separate_inputs: 3 076 rows, 7 segments with
    1 / 2 / 36 poses, rows shared by two segments) under both indexings, in named_cases' form; plus the collated batch"""
    from tests.golden.make_loss_golden import make_separate_inputs
    batch, F = make_separate_inputs()
    sizes = np.bincount(batch[1][:, 0].numpy()).tolist()
    return {"golden_reference": (F, data.pack_sym(batch[3], sizes), (1.0, 1.0, 1.0), 1.0),
            "golden_offset": (F, data.pack_sym(batch[3], sizes, reference_indexing=False), (0.5, 2.0, 1.25), 1.0)}, batch
