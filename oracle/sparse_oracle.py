"""CPU oracle of the sparse-voxel network -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates, with torch CPU fp32 gather-matmul-scatter, the subset of MinkowskiEngine 0.5.3
that the reference network uses, and the reference's own topology:

  MinkUNet34C forward      <- utils/minkunet.py:50-120 (modules), :122-180 (forward),
                              :193-195,:244-245 (LAYERS / PLANES of MinkUNet34C)
  _make_layer / BasicBlock <- utils/resnet.py:118-154 (1x1 conv + BN downsample iff channels
                              change); BasicBlock is ME's (conv1,norm1,relu,conv2,norm2,+res,relu)
  head split (eval)        <- eval_joint.py:173-190

PARITY STATUS: the COMPOSITION (layer order, widths, strides, concatenations, residual adds,
BN/ReLU placement, parameter names and shapes) and the head split are PINNED BY REFERENCE
EXECUTION: tests/golden/make_net_golden.py imports the reference's own MinkUNet34C class and
runs its forward with the MinkowskiEngine names bound to the primitives below
(tests/golden/net_ref.npz); make_decode_golden.py exec()s eval_joint.py:173-190 for the head.
The PRIMITIVE ARITHMETIC is "parity unpinned": MinkowskiEngine v0.5.3 (README.md:53) is an external
dependency that is neither vendored in the reference nor installed here, and the reference
has no test at this boundary.  The [ME-ext] semantics below are the published algorithm
(Choy et al., 4D Spatio-Temporal ConvNets, generalized sparse convolution):
  out[u] = sum_{o in K} W_o^T x[u*s + o*ts]        over ACTIVE inputs only
  - odd kernels are centred, even kernels use offsets 0..k-1
  - stride-2 output coordinates = unique(floor(c / (2 ts)) * 2 ts)
  - transposed k2s2 conv writes onto the existing finer coordinate set:
    out[v] = W_{oct(v)}^T x[parent(v)]
  - weight `kernel` is [K^3, Cin, Cout] ([Cin, Cout] when K = 1), kernel-offset index runs
    with the FIRST spatial axis fastest (KERNEL_OFFSET_ORDER is the one place to flip it
    when a real checkpoint is available)
  - MinkowskiBatchNorm = nn.BatchNorm1d over the [N, C] feature rows (eps 1e-5)
It is pinned here by tests/test_sparse_oracle.py against dense torch.nn.functional
conv3d / conv_transpose3d / batch_norm on densified grids masked to the active set.
"""
import numpy as np
import torch
import torch.nn.functional as F

KERNEL_OFFSET_ORDER = "x_fastest"

LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)              # utils/minkunet.py:193-195 (MinkUNet34)
PLANES = (32, 64, 128, 256, 256, 128, 96, 96)  # utils/minkunet.py:244-245 (MinkUNet34C)
INIT_DIM = 32


def kernel_offsets(k):
    """[K^3, 3] integer offsets (units of the input tensor stride), kernel-index order."""
    rng = np.arange(k) - k // 2 if k % 2 == 1 else np.arange(k)
    if KERNEL_OFFSET_ORDER == "x_fastest":
        zz, yy, xx = np.meshgrid(rng, rng, rng, indexing="ij")
    else:
        xx, yy, zz = np.meshgrid(rng, rng, rng, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1).astype(np.int64)


def _keys(coords):
    """[N,4] (b,x,y,z) int -> unique int64 key"""
    c = np.asarray(coords, np.int64)
    return ((c[:, 0] << 48) | ((c[:, 1] + 32768) << 32) | ((c[:, 2] + 32768) << 16) | (c[:, 3] + 32768))


def downsample_coords(coords, ts):
    """unique(floor(c / (2ts)) * 2ts) in order of first appearance."""
    c = np.asarray(coords, np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], 2 * ts) * (2 * ts)
    _, first = np.unique(_keys(c), return_index=True)
    return c[np.sort(first)]


def _lookup(keys_sorted, order, q):
    pos = np.searchsorted(keys_sorted, q)
    pos = np.clip(pos, 0, len(keys_sorted) - 1)
    hit = keys_sorted[pos] == q
    return np.where(hit, order[pos], -1)


def kernel_map(in_coords, out_coords, k, ts_in, stride):
    """nbr[N_out, K^3]: index into in_coords of out_coord + offset*ts_in, or -1."""
    kin = _keys(in_coords)
    order = np.argsort(kin, kind="stable")
    ks = kin[order]
    offs = kernel_offsets(k) * ts_in
    oc = np.asarray(out_coords, np.int64)
    nbr = np.empty((len(oc), len(offs)), np.int64)
    for j, o in enumerate(offs):
        q = oc.copy()
        q[:, 1:] += o[None]
        nbr[:, j] = _lookup(ks, order, _keys(q))
    return nbr


def conv(x, kernel, nbr, bias=None):
    """x [N_in,Cin], kernel [K,Cin,Cout] or [Cin,Cout], nbr [N_out,K] -> [N_out,Cout]"""
    if kernel.dim() == 2:
        kernel = kernel[None]
    out = torch.zeros((nbr.shape[0], kernel.shape[2]), dtype=x.dtype)
    for j in range(kernel.shape[0]):
        src = nbr[:, j]
        sel = np.nonzero(src >= 0)[0]
        if sel.size:
            out[sel] += x[src[sel]] @ kernel[j]
    if bias is not None:
        out = out + bias.reshape(1, -1)
    return out


def conv_transpose_k2s2(x, kernel, nbr_down):
    """x at the coarse set, nbr_down [N_coarse, 8] (map of the matching k2s2 conv: coarse <- fine).
    Output on the fine set: out[fine] = W_o^T x[coarse] for the (coarse, o) that contains it."""
    n_fine = int(nbr_down.max()) + 1
    out = torch.zeros((n_fine, kernel.shape[2]), dtype=x.dtype)
    for j in range(kernel.shape[0]):
        fine = nbr_down[:, j]
        sel = np.nonzero(fine >= 0)[0]
        if sel.size:
            out[fine[sel]] = x[sel] @ kernel[j]
    return out


# Test hook: an iterator of boolean masks, one per ReLU of the forward in call order (or None).  With it the k-th ReLU is
# x * mask_k instead of max(x, 0): a second evaluation (another precision, the HIP path) can be given the FIRST one's
# activation pattern, so that gradients are compared on the same piecewise-linear branch - pre-activations within
# rounding of zero otherwise pick different branches and change a gradient element by its whole value
# (tests/test_production_size_gpu.py).  relu_trace, when a list, receives every ReLU's mask (x > 0); relu_peaks, when a
# list, the largest value every ReLU lets through (the inputs of the next convolution: tests/test_train_gpu.py checks
# them against the fp16 range on trained weights).
relu_masks = None
relu_trace = None
relu_peaks = None


def _relu(x):
    if relu_masks is not None:
        m = next(relu_masks)
        y = x * torch.as_tensor(m).to(x.dtype)
    else:
        y = torch.relu(x)
    if relu_trace is not None:
        relu_trace.append((y.detach() > 0))
    if relu_peaks is not None:
        relu_peaks.append(float(y.detach().abs().max()) if y.numel() else 0.0)
    return y


def batch_norm(x, sd, prefix, training=False, eps=1e-5):
    return F.batch_norm(x, sd[prefix + ".bn.running_mean"], sd[prefix + ".bn.running_var"],
                        sd[prefix + ".bn.weight"], sd[prefix + ".bn.bias"], training=training,
                        momentum=0.1, eps=eps)


class CoordinateManager:
    """Coordinate sets per tensor stride and the 10 kernel maps of one forward."""

    def __init__(self, coords):
        self.coords = {1: np.asarray(coords, np.int64)}
        for ts in (1, 2, 4, 8):
            self.coords[2 * ts] = downsample_coords(self.coords[ts], ts)
        self.maps = {}

    def map(self, k, ts, stride=1):
        key = (k, ts, stride)
        if key not in self.maps:
            out = self.coords[ts * stride]
            self.maps[key] = kernel_map(self.coords[ts], out, k, ts, stride)
        return self.maps[key]


def _block(x, sd, name, cm, ts, training):
    """ME BasicBlock (expansion 1) with the optional downsample of resnet.py:126-134."""
    nbr = cm.map(3, ts)
    out = conv(x, sd[name + ".conv1.kernel"], nbr)
    out = _relu(batch_norm(out, sd, name + ".norm1", training))
    out = conv(out, sd[name + ".conv2.kernel"], nbr)
    out = batch_norm(out, sd, name + ".norm2", training)
    if name + ".downsample.0.kernel" in sd:
        res = conv(x, sd[name + ".downsample.0.kernel"], cm.map(1, ts))
        res = batch_norm(res, sd, name + ".downsample.1", training)
    else:
        res = x
    return _relu(out + res)


def _layer(x, sd, name, n, cm, ts, training):
    for i in range(n):
        x = _block(x, sd, "%s.%d" % (name, i), cm, ts, training)
    return x


def minkunet34c_forward(sd, coords, feats, training=False, return_intermediates=False, dtype=torch.float32):
    """utils/minkunet.py:122-180 on (coords [N,4] int (b,x,y,z), feats [N,Cin]) -> [N, Cout].
    dtype=torch.float64 runs the same graph in double precision: the yardstick that says how far ANY fp32 evaluation
    (this oracle's or the HIP path's) sits from the exact result - ReLU masks of values within rounding of zero flip
    between two fp32 evaluations, and a flipped mask changes a gradient element by its whole value."""
    # tensors that require grad are used as they are so torch autograd can differentiate the oracle
    sd = {k: (v if (torch.is_tensor(v) and v.requires_grad) else
              (v.detach().to(dtype if v.dtype.is_floating_point else v.dtype).cpu().clone() if torch.is_tensor(v) else v))
          for k, v in sd.items()}
    cm = CoordinateManager(coords)
    x = torch.as_tensor(feats, dtype=dtype)
    inter = {}

    def cbr(x, conv_name, bn_name, k, ts, stride=1):
        y = conv(x, sd[conv_name + ".kernel"], cm.map(k, ts, stride))
        return _relu(batch_norm(y, sd, bn_name, training))

    def up(x, conv_name, bn_name, ts_coarse):
        y = conv_transpose_k2s2(x, sd[conv_name + ".kernel"], cm.map(2, ts_coarse // 2, 2))
        return _relu(batch_norm(y, sd, bn_name, training))

    out_p1 = cbr(x, "conv0p1s1", "bn0", 5, 1)                                    # :123-125
    out = cbr(out_p1, "conv1p1s2", "bn1", 2, 1, 2)                               # :127-129
    out_b1p2 = _layer(out, sd, "block1", LAYERS[0], cm, 2, training)             # :130
    out = cbr(out_b1p2, "conv2p2s2", "bn2", 2, 2, 2)
    out_b2p4 = _layer(out, sd, "block2", LAYERS[1], cm, 4, training)
    out = cbr(out_b2p4, "conv3p4s2", "bn3", 2, 4, 2)
    out_b3p8 = _layer(out, sd, "block3", LAYERS[2], cm, 8, training)
    out = cbr(out_b3p8, "conv4p8s2", "bn4", 2, 8, 2)                             # :147-149
    out = _layer(out, sd, "block4", LAYERS[3], cm, 16, training)
    inter["block4"] = out
    out = up(out, "convtr4p16s2", "bntr4", 16)                                   # :153-155
    out = _layer(torch.cat([out, out_b3p8], 1), sd, "block5", LAYERS[4], cm, 8, training)
    out = up(out, "convtr5p8s2", "bntr5", 8)
    out = _layer(torch.cat([out, out_b2p4], 1), sd, "block6", LAYERS[5], cm, 4, training)
    out = up(out, "convtr6p4s2", "bntr6", 4)
    out = _layer(torch.cat([out, out_b1p2], 1), sd, "block7", LAYERS[6], cm, 2, training)
    out = up(out, "convtr7p2s2", "bntr7", 2)
    out = _layer(torch.cat([out, out_p1], 1), sd, "block8", LAYERS[7], cm, 1, training)
    inter["block8"] = out
    y = conv(out, sd["final.kernel"], cm.map(1, 1), sd["final.bias"])            # :180
    if return_intermediates:
        inter["out_p1"] = out_p1
        inter["out_b1p2"] = out_b1p2
        return y, inter, cm
    return y


def head_joint_eval(out, nclasses=9, log_scale=True):
    """eval_joint.py:173-190: per-point head select by argmax class."""
    out = torch.as_tensor(out)
    o_xyz = out[:, :3 * nclasses]
    o_scale = out[:, 3 * nclasses:6 * nclasses]
    o_class = out[:, 6 * nclasses:]
    idx = o_class.argmax(-1)
    idx = torch.where(idx == nclasses, torch.zeros_like(idx), idx)
    g = idx[:, None, None].expand(-1, 1, 3)
    xyz = torch.gather(o_xyz.reshape(-1, nclasses, 3), 1, g)[:, 0]
    scale = torch.gather(o_scale.reshape(-1, nclasses, 3), 1, g)[:, 0]
    if log_scale:
        scale = torch.exp(scale)
    cls = torch.argmax(o_class[..., :-1], dim=-1)
    prob = torch.max(torch.softmax(o_class, dim=-1)[..., :-1], dim=-1)[0]
    return xyz, scale, prob, cls


def head_separate_eval(out, log_scale=True):
    """eval_separate.py:170-181"""
    out = torch.as_tensor(out)
    scale = torch.exp(out[:, 3:6]) if log_scale else out[:, 3:6]
    return out[:, :3], scale, torch.softmax(out[:, 6:8], dim=-1)[:, 1]


def make_state_dict(in_channels=3, out_channels=64, seed=0):
    """Random MinkUNet34C parameters with the reference's names and init
    (utils/resnet.py:109-116: kaiming-normal fan_out/relu on conv kernels, BN gamma 1 beta 0;
    transposed convs keep a uniform default).  BN running stats are randomised so that eval
    mode is a non-trivial affine map."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv_w(name, k, cin, cout, transposed=False):
        K = k ** 3
        shape = (cin, cout) if K == 1 else (K, cin, cout)
        if transposed:
            bound = 1.0 / np.sqrt(cin * K)
            w = (torch.rand(shape, generator=g) * 2 - 1) * bound
        else:
            std = np.sqrt(2.0 / (cout * K))          # fan_out = Cout * K^3
            w = torch.randn(shape, generator=g) * std
        sd[name + ".kernel"] = w

    def bn(name, c):
        sd[name + ".bn.weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        sd[name + ".bn.bias"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".bn.running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[name + ".bn.running_var"] = 1.0 + 0.2 * torch.rand(c, generator=g)
        sd[name + ".bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)

    inpl = INIT_DIM
    conv_w("conv0p1s1", 5, in_channels, inpl); bn("bn0", inpl)

    def layer(name, planes, n, inplanes):
        for i in range(n):
            p = "%s.%d" % (name, i)
            cin = inplanes if i == 0 else planes
            conv_w(p + ".conv1", 3, cin, planes); bn(p + ".norm1", planes)
            conv_w(p + ".conv2", 3, planes, planes); bn(p + ".norm2", planes)
            if i == 0 and cin != planes:
                conv_w(p + ".downsample.0", 1, cin, planes); bn(p + ".downsample.1", planes)
        return planes

    for lvl, (cname, bname) in enumerate((("conv1p1s2", "bn1"), ("conv2p2s2", "bn2"),
                                          ("conv3p4s2", "bn3"), ("conv4p8s2", "bn4"))):
        conv_w(cname, 2, inpl, inpl); bn(bname, inpl)
        inpl = layer("block%d" % (lvl + 1), PLANES[lvl], LAYERS[lvl], inpl)
    skips = (PLANES[2], PLANES[1], PLANES[0], INIT_DIM)
    for j, (cname, bname) in enumerate((("convtr4p16s2", "bntr4"), ("convtr5p8s2", "bntr5"),
                                        ("convtr6p4s2", "bntr6"), ("convtr7p2s2", "bntr7"))):
        conv_w(cname, 2, inpl, PLANES[4 + j], transposed=True); bn(bname, PLANES[4 + j])
        inpl = layer("block%d" % (5 + j), PLANES[4 + j], LAYERS[4 + j], PLANES[4 + j] + skips[j])
    conv_w("final", 1, PLANES[7], out_channels)
    sd["final.bias"] = 0.1 * torch.randn(1, out_channels, generator=g)
    return sd


# ---- float64 convolution with per-element error bounds (tests/test_conv_paths_gpu.py) ---------------------------------
ERROR_MODEL = """Error model of the HIP convolution paths, per output element e.

The exact result is y64 = sum over the (row, offset, input channel) terms t of x_t * w_t, computed here in float64
(its own error, ~2^-53 * mag, is far below everything else).  mag[e] = sum |x_t| * |w_t| over the same terms.  A
path that forms every product to relative accuracy u_prod and adds the products with n_seq fp32 roundings on the way
to the element (standard first-order model: every rounded addition is off by at most 2^-24 of the partial sums it
combines, and a partial sum never exceeds mag) stays within

    |got - y64| <= (u_prod + (n_seq + 2) * 2^-24) * mag + floor

n_seq: every matrix-core instruction that accumulates into the element rounds once (the instruction's own k-products
are summed inside it), so one 32-channel unit (one kernel offset x one 32-channel chunk of the input) costs
STEPS_PER_UNIT[path] roundings; on top come the additions of the split-K partial tiles (at most SPLIT_CAP = 64, the
dispatcher's cap) and the finish launch's tree of 4 quarter sums.  Taking the whole offset range's units instead of
a workgroup's share keeps the count independent of how the dispatcher splits the launch:

    n_seq = STEPS_PER_UNIT[path] * units + SPLIT_CAP + 4,    units = (kernel offsets) * ceil(Cin / 32)

The price of that independence is looseness on split launches at wide Cin: a 27-way split of a 256-channel 3x3x3
convolution walks about 8 units per workgroup, but the bound charges all 216 (n_seq 2660 instead of about 130 on
"h2").  Errors that grow linearly with the reduction length - products of fp16 high pieces alone, say - can then fall
inside the bound at such shapes.  What keeps the tests sensitive is that mag is per element: rows with one or two
neighbours (isolated voxels, sheet edges, the partial last layer of a box) and narrow inputs (Cin 32, 1x1 kernels)
have a small mag and a small n_seq, and there one dropped contribution or one missing low piece is far outside the
bound (tests/test_conv_bound.py shows both at Cin 32).

Per path (u_prod, STEPS_PER_UNIT), from the kernel comments:
  "f32"   v_mfma_f32_32x32x2_f32, exact fp32 products (conv_rows, the wgrad pieces = 0 mode): u_prod = 0, 16 steps
  "x6"    bf16 triples x = h + m + l (24 significant bits), six of the nine piece products (conv_rows_wp.hip, the
          bf16x6 comment): the representation is exact and the three dropped products are <= 2^-24 relative each,
          u_prod = 2^-22; six 32x32x16 instructions per 16 channels: 12 steps
  "h2"    fp16 pairs x = h + l, h = RNE16(x), l = RNE16(x - h) (sparse_conv_common.h): each operand to 2^-24
          relative, the dropped l*l product <= 2^-22 relative, u_prod = 2^-22; three instructions per 16 channels:
          6 steps.  Below 2^-14 an activation's pair carries an absolute error of up to 2^-25, hence the floor
          2^-25 * sum |w_t| (weights are scaled by a power of two into the fp16 range before they are split)
  "bf16"  the opt-in bf16 mode (pieces = 1): compared with y64 of the bf16-RNE-rounded operands, whose products
          the matrix core forms exactly: u_prod = 0, two instructions per 32 channels: 2 steps
An hl-format output stores h + l of the fp32 value: 2^-24 * |y| more, and 2^-25 absolute below 2^-14.

The fused epilogue z = (y + acc_in) * scale + shift + residual is propagated explicitly: |scale| * bound(y) plus three
roundings of at most 2^-24 * (|y * scale| + |shift| + |residual|) each (and an hl residual's own 2^-24 relative /
2^-25 absolute).  ReLU is 1-Lipschitz, so |got - relu(z64)| <= bound(z) holds for every element, also where z64 lies
within the bound of zero (there it only says that |got| is within the bound).

A second source (cv_conv_desc.in2: out += in2 @ W2 on the output rows, conv64_two) adds Cin2 / 32 units to the same
accumulator and its terms to mag and wabs; nothing else changes.  BatchNorm scales folded into the packed weights are
restated exactly (folded_weights): the packers form w * (col_scale * 2^k) with one fp32 rounding, so the reference uses
the rounded product as ITS weight and the fold adds no term to the bound.

The weight gradient dW[j, ci, co] = sum_u x[nbr[u, j], ci] * dy[u, co] follows the same model with the rows as the
reduction axis: units of 16 rows (the k of one 32x32x16 instruction; 8 instructions of k = 2 for "f32"), plus the row
splits of the plan (at most WGRAD_SPLIT_CAP = 1024) and the reduce launch.
"""
U24 = 2.0 ** -24
SPLIT_CAP = 64
WGRAD_SPLIT_CAP = 1024
PATHS = {"f32": (0.0, 16), "x6": (2.0 ** -22, 12), "h2": (2.0 ** -22, 6), "bf16": (0.0, 2)}
WGRAD_STEPS_PER_16_ROWS = {"f32": 8, "x6": 6, "bf16": 1}


def bf16_round(a):
    """float32 array rounded to the nearest bf16 (ties to even), returned as float32"""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def conv64(x, w, nbr, j_begin=0, j_end=None):
    """float64 sparse convolution on any map.  x [N_in, Cin], w [K, Cin, Cout] (or [Cin, Cout]), nbr [N_out, K] (None:
    K = 1 and the identity map).  Returns (y64, mag, wabs): y64 [N_out, Cout]; mag = sum |x| |w| over the same terms;
    wabs = sum |w| over the same terms (the fp16-pair floor)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    if w.ndim == 2:
        w = w[None]
    if nbr is None:
        nbr = np.arange(x.shape[0], dtype=np.int64)[:, None]
    nbr = np.asarray(nbr)
    j_end = w.shape[0] if j_end is None else j_end
    n_out, cout = nbr.shape[0], w.shape[2]
    y = np.zeros((n_out, cout))
    mag = np.zeros((n_out, cout))
    wabs = np.zeros((n_out, cout))
    for j in range(j_begin, j_end):
        src = nbr[:, j]
        sel = np.nonzero(src >= 0)[0]
        if sel.size:
            xs = x[src[sel]]
            y[sel] += xs @ w[j]
            mag[sel] += np.abs(xs) @ np.abs(w[j])
            wabs[sel] += np.abs(w[j]).sum(0)[None]
    return y, mag, wabs


def conv_bound(mag, wabs, path, units, hl_out=False, y=None):
    """per-element bound of |got - y64| for a convolution on `path` (see the model above) of `units` 32-channel units"""
    u_prod, steps = PATHS[path]
    n_seq = steps * units + SPLIT_CAP + 4
    b = (u_prod + (n_seq + 2) * U24) * mag
    if path == "h2":
        b = b + 2.0 ** -25 * wabs
    if hl_out:
        b = b + U24 * np.abs(y) + 2.0 ** -25
    return b


def conv_units(K, cin):
    return K * ((cin + 31) // 32)


def folded_weights(w, col_scale=None, bf16=False):
    """the weights a packer splits, exactly: w * (col_scale * 2^k) is ONE fp32 rounding (the power of two is exact and
    leaves the accumulator again through acc_scale = 2^-k), so w_eff = float32(w * col_scale), widened; bf16: the
    pieces = 1 packer then rounds that to bf16"""
    w = np.asarray(w, np.float32)
    if col_scale is not None:
        w = (w * np.asarray(col_scale, np.float32)).astype(np.float32)
    return (bf16_round(w) if bf16 else w).astype(np.float64)


def conv64_two(x, w, nbr, x2, w2, j_begin=0, j_end=None):
    """the two-source convolution (cv_conv_desc.in2): y64 = conv64(x, w, nbr, j_begin, j_end) + x2 @ w2 on the output
    rows; x2 [N_out, Cin2], w2 [Cin2, Cout] or [1, Cin2, Cout].  mag and wabs are the sums of both sources' terms."""
    y, mag, wabs = conv64(x, w, nbr, j_begin, j_end)
    x2 = np.asarray(x2, np.float64)
    w2 = np.asarray(w2, np.float64).reshape(x2.shape[1], -1)
    return y + x2 @ w2, mag + np.abs(x2) @ np.abs(w2), wabs + np.abs(w2).sum(0)[None]


def conv_units_two(nj, cin, cin2):
    """units of a two-source launch: nj offsets x ceil(Cin / 32) chunks, then the Cin2 / 32 chunks of the second source"""
    return conv_units(nj, cin) + cin2 // 32


def epilogue64(y, b, acc_in=None, b_acc=None, scale=None, shift=None, res=None, res_hl=False, relu=False,
               hl_out=False, roundings=3):
    """float64 epilogue z = relu((y + acc_in) * scale + shift + res) with its propagated bound (b: bound of y);
    roundings: the multiple of 2^-24 * (|y * scale| + |shift| + |res|) charged for the three fp32 operations"""
    y = np.asarray(y, np.float64)
    if acc_in is not None:
        y = y + acc_in
        b = b + b_acc + U24 * np.abs(y)
    sc = np.ones(y.shape[1]) if scale is None else np.asarray(scale, np.float64)
    sh = np.zeros(y.shape[1]) if shift is None else np.asarray(shift, np.float64)
    r = np.zeros_like(y) if res is None else np.asarray(res, np.float64)
    z = y * sc + sh + r
    bz = np.abs(sc) * b + roundings * U24 * (np.abs(y * sc) + np.abs(sh) + np.abs(r))
    if res is not None and res_hl:
        bz = bz + U24 * np.abs(r) + 2.0 ** -25
    if relu:
        z = np.maximum(z, 0.0)
    if hl_out:
        bz = bz + U24 * np.abs(z) + 2.0 ** -25
    return z, bz


def wgrad64(x, dy, nbr, K):
    """float64 weight gradient dW [K, Cin, Cout] = sum_u x[nbr[u, j]]^T dy[u] and mag = sum_u |x| |dy|"""
    x = np.asarray(x, np.float64)
    dy = np.asarray(dy, np.float64)
    if nbr is None:
        nbr = np.arange(dy.shape[0], dtype=np.int64)[:, None]
    dw = np.zeros((K, x.shape[1], dy.shape[1]))
    mag = np.zeros_like(dw)
    for j in range(K):
        sel = np.nonzero(nbr[:, j] >= 0)[0]
        if sel.size:
            xs = x[nbr[sel, j]]
            dw[j] = xs.T @ dy[sel]
            mag[j] = np.abs(xs).T @ np.abs(dy[sel])
    return dw, mag


def wgrad_bound(mag, path, n_out):
    u_prod = PATHS["x6"][0] if path == "x6" else 0.0
    n_seq = WGRAD_STEPS_PER_16_ROWS[path] * ((n_out + 15) // 16) + WGRAD_SPLIT_CAP + 4
    return (u_prod + (n_seq + 2) * U24) * mag


def within(got, ref, bound):
    """(ok, worst index, worst excess ratio) of |got - ref| <= bound, element by element"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = err / np.maximum(bound, 1e-300)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return bool((err <= bound).all()) and bool(np.isfinite(got).all()), i, float(ratio[i])


# ---- float64 row kernels with per-element error bounds (tests/test_row_kernels_gpu.py) --------------------------------
ROW_ERROR_MODEL = """Error model of the row kernels (affine, BatchNorm fold / statistics / backward, column sums, the hl
format, the heads), per output element.  u = 2^-24 (U24).  Every function below takes the fp32 arrays the kernel receives,
computes in float64 and returns (value, bound) pairs for within().  The constants are forward-error counts of the fp32
operations in the kernel source with about 2x margin; tests/test_row_bound.py pins each of them on the CPU (a numpy fp32
restatement of the kernel's operation order stays at a ratio <= 0.6 of the bound; named wrong results are >= 10 x outside).

  affine       z = relu?(x * scale + shift + res): one product, two additions (or an fma and an addition):
               4u (|x * scale| + |shift| + |res|) - epilogue64 with b = 0 and one more u of margin; the hl twin adds
               u |z| + 2^-25 (ERROR_MODEL).  ReLU is 1-Lipschitz.
  bn_fold      scale = gamma / sqrt(var + eps): addition, square root, division: 6u |scale|.
               shift = beta - mean * scale (+ bias * scale):
               2u (|beta| + 2 |mean * scale| + 2 |bias * scale|) + (|mean| + |bias|) * bound(scale)
  bn_stats     sums of x and x^2 in double, one rounding to fp32 at the end:
               mean        2u |mean| + 2^-50 * mean(|x|)
               biased var  2u * var + 2^-48 * mean(x^2)       (E[x^2] - mu^2 is formed in double: the second term is the
                           cancellation; a negative difference is clamped to 0)
               running     r' = (1 - m) * r + m * s (s = mean, or the unbiased variance var * n / (n - 1); n = 1 keeps
                           var): m * bound(s) + 2u of each fp32 result of the update, the two products and their sum:
                           2u (|(1 - m) * r| + |m * s| + |r'|)   (1 - m is itself rounded: three roundings against 4u)
               scale       gamma / sqrtf((float) var + eps): |scale| (4u + 0.5 (bound(var) + u (var + eps)) / (var + eps))
               shift       beta - (float) mean * scale: u (|beta| + 2 |mean * scale|) + |mean| bound(scale) + |scale| bound(mean)
  bn_backward  mean32 / var32 are exact inputs (arguments of the call).  g = dy * open, istd = 1 / sqrt(var32 + eps),
               xh = (x - mean32) * istd.
               dbeta  = sum g (double accumulator, one rounding):   2u |dbeta| + 2^-50 * sum |g|
               dgamma = sum g * xh (fp32 products: subtraction, istd's three operations, two products; double
                        accumulator):                               8u * sum |g * xh| + u |dgamma|
               dx     = gamma * istd * (g - dbeta / n - xh * dgamma / n):
                        |gamma * istd| * (16u (|g| + |dbeta| / n + |xh * dgamma| / n) + (bound(dbeta) + |xh| bound(dgamma)) / n)
               dres   = g, exact
  col_sum      fp32 throughout: a thread adds every 8th row of its chunk, 8 partial sums meet in LDS, `chunks` partial
               sums per column are added (in chunk order, or by fp32 atomics in any order):
               (ceil(n / 8 / chunks) + 8 + chunks + 2) * u * sum |x|
  hl format    bit-exact model hl_bits(): h = RNE16(x), l = RNE16(x - float32(h)); per 32-channel chunk 64 bytes of h,
               then 64 bytes of l (sparse_conv_common.h).  h + l is x to 2u |x| (the remainder x - h has up to 12
               significant bits, l keeps 11) plus 2^-25 absolute where l is subnormal; the u |z| + 2^-25 that epilogue64 charges
               an hl output is the typical case, and the affine's spare u covers the rest
  heads        exact selection semantics in float64 (first index on ties, class `nclasses` -> head 0); exp / softmax
               outputs are held to the tolerances the project holds expf to (tests/test_decode_gpu.py)
"""


def affine64(x, scale=None, shift=None, res=None, relu=False, hl_out=False):
    """(z, bound) of cv_sp_affine_f32 / cv_sp_affine_hl_f32: relu?(x * scale + shift + res).  Without a scale the
    kernel applies no shift either."""
    assert scale is not None or shift is None
    x = np.asarray(x, np.float64)
    return epilogue64(x, np.zeros_like(x), scale=scale, shift=shift, res=res, relu=relu, hl_out=hl_out, roundings=4)


def bn_fold64(gamma, beta, mean, var, bias=None, eps=1e-5):
    """((scale, bound), (shift, bound)) of cv_sp_bn_fold_f32"""
    gamma, beta, mean, var = (np.asarray(a, np.float64) for a in (gamma, beta, mean, var))
    eps = float(np.float32(eps))
    bias = np.zeros_like(mean) if bias is None else np.asarray(bias, np.float64)
    scale = gamma / np.sqrt(var + eps)
    b_scale = 6 * U24 * np.abs(scale)
    shift = beta - mean * scale + bias * scale
    b_shift = 2 * U24 * (np.abs(beta) + 2 * np.abs(mean * scale) + 2 * np.abs(bias * scale)) + \
        (np.abs(mean) + np.abs(bias)) * b_scale
    return (scale, b_scale), (shift, b_shift)


def bn_stats64(x, n=None, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """cv_sp_bn_stats_f32 on the first n rows of x: dict of (value, bound) for "mean", "var" (biased), "scale", "shift"
    and, with starting values, "running_mean" / "running_var" """
    x = np.asarray(x, np.float64)
    n = x.shape[0] if n is None else n
    x = x[:n]
    eps, m = float(np.float32(eps)), float(np.float32(momentum))
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)                  # the centred form: no cancellation of its own
    b_mean = 2 * U24 * np.abs(mean) + 2.0 ** -50 * np.abs(x).mean(0)
    b_var = 2 * U24 * var + 2.0 ** -48 * (x * x).mean(0)
    out = {"mean": (mean, b_mean), "var": (var, b_var)}
    if gamma is not None:
        gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
        scale = gamma / np.sqrt(var + eps)
        b_scale = np.abs(scale) * (4 * U24 + 0.5 * (b_var + U24 * (var + eps)) / (var + eps))
        shift = beta - mean * scale
        b_shift = U24 * (np.abs(beta) + 2 * np.abs(mean * scale)) + np.abs(mean) * b_scale + np.abs(scale) * b_mean
        out["scale"], out["shift"] = (scale, b_scale), (shift, b_shift)
    if running_mean is not None:
        f = n / (n - 1.0) if n > 1 else 1.0
        for name, r0, s, bs in (("running_mean", running_mean, mean, b_mean), ("running_var", running_var, var * f, b_var * f)):
            t1, t2 = (1.0 - m) * np.asarray(r0, np.float64), m * s
            out[name] = (t1 + t2, m * bs + 2 * U24 * (np.abs(t1) + np.abs(t2) + np.abs(t1 + t2)))
    return out


def bn_backward64(x, dy, open_mask, mean32, var32, gamma, n=None, eps=1e-5):
    """cv_sp_bn_backward_f32 given the fp32 mean / variance the call receives: dict of (value, bound) for "dbeta",
    "dgamma", "dx", "dres".  open_mask: where the ReLU behind the normalisation was open (None: no ReLU)"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.shape[0] if n is None else n
    x, dy = x[:n], dy[:n]
    eps = float(np.float32(eps))
    mean, var, gamma = (np.asarray(a, np.float64) for a in (mean32, var32, gamma))
    g = dy if open_mask is None else dy * np.asarray(open_mask[:n], np.float64)
    istd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * istd
    dbeta = g.sum(0)
    b_dbeta = 2 * U24 * np.abs(dbeta) + 2.0 ** -50 * np.abs(g).sum(0)
    dgamma = (g * xh).sum(0)
    b_dgamma = 8 * U24 * np.abs(g * xh).sum(0) + U24 * np.abs(dgamma)
    dx = gamma * istd * (g - dbeta / n - xh * dgamma / n)
    b_dx = np.abs(gamma * istd) * (16 * U24 * (np.abs(g) + np.abs(dbeta) / n + np.abs(xh * dgamma) / n) +
                                   (b_dbeta + np.abs(xh) * b_dgamma) / n)
    return {"dbeta": (dbeta, b_dbeta), "dgamma": (dgamma, b_dgamma), "dx": (dx, b_dx), "dres": (g, np.zeros_like(g))}


def col_sum64(x, chunks):
    """(sums, bound) of cv_sp_col_sum_det_f32 / cv_sp_col_sum_f32 launched with `chunks` row chunks"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    steps = -(-n // (8 * chunks)) + 8 + chunks + 2
    return x.sum(0), steps * U24 * np.abs(x).sum(0)


def hl_bits(x):
    """the hl format of fp32 rows x [n, c] (c % 32 == 0), bit for bit: uint32 words [n, c]"""
    x = np.ascontiguousarray(x, np.float32)
    n, c = x.shape
    assert c % 32 == 0
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
        l = (x - h.astype(np.float32)).astype(np.float16)
    words = np.stack([h.reshape(n, c // 32, 32), l.reshape(n, c // 32, 32)], 2)        # [n, chunk, h | l, 32] fp16
    return np.ascontiguousarray(words).view(np.uint32).reshape(n, c)


def hl_decode(bits):
    """float32(h) + float32(l) of hl words [n, c] (what cv_sp_from_hl_f32 returns)"""
    n, c = bits.shape
    p = np.ascontiguousarray(bits, np.uint32).view(np.float16).reshape(n, c // 32, 2, 32).astype(np.float32)
    return (p[:, :, 0] + p[:, :, 1]).reshape(n, c)


def head_joint64(out, nclasses=9, log_scale=True):
    """cv_head_joint_f32 in float64 (eval_joint.py:173-190): xyz, scale, prob, class; arg-max takes the first index
    on ties, class `nclasses` (background) selects head 0"""
    out = np.asarray(out, np.float64)
    n = out.shape[0]
    logit = out[:, 6 * nclasses:7 * nclasses + 1]
    am = logit.argmax(1)
    h = np.where(am == nclasses, 0, am)
    rows = np.arange(n)
    xyz = out[:, :3 * nclasses].reshape(n, nclasses, 3)[rows, h]
    scale = out[:, 3 * nclasses:6 * nclasses].reshape(n, nclasses, 3)[rows, h]
    if log_scale:
        scale = np.exp(scale)
    cls = logit[:, :nclasses].argmax(1)
    e = np.exp(logit - logit.max(1, keepdims=True))
    prob = (e[:, :nclasses] / e.sum(1, keepdims=True)).max(1)
    return xyz, scale, prob, cls


def head_separate64(out, log_scale=True):
    """cv_head_separate_f32 in float64 (eval_separate.py:170-181): xyz, scale, prob = softmax(out[6:8])[1]"""
    out = np.asarray(out, np.float64)
    scale = np.exp(out[:, 3:6]) if log_scale else out[:, 3:6]
    mx = np.maximum(out[:, 6], out[:, 7])
    e0, e1 = np.exp(out[:, 6] - mx), np.exp(out[:, 7] - mx)
    return out[:, :3], scale, e1 / (e0 + e1)


def row_case(n, c, seed=0):
    """inputs of the row-kernel tests (fp32): x [n, c] with rows of 1e-3 and 30 times the unit scale and channel means
    of up to 3 sigma, channel c // 2 with a variance below 1e-6 (c >= 2), channel c - 1 constant (c >= 3: its variance
    is exactly 0 and eps decides); dy, res [n, c]; gamma, beta, bias, running_mean, running_var [c]"""
    rng = np.random.default_rng(seed * 1000003 + n * 7 + c * 131)
    x = rng.normal(0, 1, (n, c))
    x[::7] *= 1e-3
    x[::11] *= 30.0
    x += rng.uniform(-3, 3, c)
    if c >= 2:
        x[:, c // 2] = 0.7 + 3e-4 * rng.normal(0, 1, n)
    if c >= 3:
        x[:, c - 1] = rng.uniform(0.5, 2.0)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f(x), dy=f(rng.normal(0, 1, (n, c))), res=f(rng.normal(0, 1, (n, c))),
                gamma=f(rng.uniform(0.5, 1.5, c)), beta=f(rng.normal(0, 0.2, c)), bias=f(rng.normal(0, 0.5, c)),
                running_mean=f(rng.normal(0, 0.5, c)), running_var=f(rng.uniform(0.5, 2.0, c)))
