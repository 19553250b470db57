"""Inputs, float64 references and case lists shared by the second-source and network-program tests
(tests/test_conv_second_source_gpu.py, tests/test_net_program_gpu.py) and by the CPU check that their bounds separate the
defects they exist for (tests/test_conv_bound.py).  Nothing here touches a device."""
import functools
import zlib

import numpy as np

from oracle import sparse_oracle as so
from tests.test_conv_paths_gpu import coords_n, operands

PATH = {3: "x6", 2: "h2", 1: "bf16"}
WP_NPRE = 10                # offsets a conv_hl / conv_rows_wp workgroup keeps (sparse_conv_common.h)


def ksize(k):
    return 1 if k == 1 else 8 if k in ("down", "up") else k ** 3


@functools.lru_cache(maxsize=None)
def ref_map(n, kind, k):
    """(CPU kernel map or None, n_in, n_out): what test_conv_paths_gpu.maps checks the device maps against"""
    c1 = coords_n(n, kind)
    if k == 1:
        return None, n, n
    if k in ("down", "up"):
        ref = so.kernel_map(c1, so.downsample_coords(c1, 1), 2, 1, 2)
        if k == "down":
            return ref, n, ref.shape[0]
        ref_up = np.full((n, 8), -1, np.int64)
        cidx, j = np.nonzero(ref >= 0)
        ref_up[ref[cidx, j], j] = cidx
        return ref_up, ref.shape[0], n
    return so.kernel_map(c1, c1, k, 1, 1), n, n


@functools.lru_cache(maxsize=None)
def second_operands(n_out, cin2, cout, seed=0):
    """x2 [n_out, cin2] (rows of 1e-3 and 8 times the unit scale; its neighbours in memory are 1000 times larger, so no
    30x rows: everything stays in the fp16 range), w2 [1, cin2, cout], scale2 [cout]"""
    rng = np.random.default_rng(seed * 7919 + n_out * 13 + cin2 * 101 + cout)
    x2 = rng.normal(0, 1, (n_out, cin2)).astype(np.float32)
    x2[::5] *= 1e-3
    x2[::9] *= 8.0
    w2 = (rng.normal(0, 1, (1, cin2, cout)) / np.sqrt(cin2)).astype(np.float32)
    scale2 = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    return x2, w2, scale2


def group_orders(ref, groups):
    """a CPU stand-in for the mask orders: per contiguous offset group the rows sorted (stably) by the bit mask of their
    valid neighbours in the group.  Used only to state defect (iii) without a device."""
    n, K = ref.shape
    out = []
    for g in range(groups):
        jb, je = K * g // groups, K * (g + 1) // groups
        key = ((ref[:, jb:je] >= 0).astype(np.int64) << np.arange(je - jb)).sum(1)
        out.append(np.argsort(key, kind="stable"))
    return out


@functools.lru_cache(maxsize=None)
def two_source(n, kind, k, cin, cin2, cout, pieces, j_begin=0, j_end=None, folded=True):
    """the float64 pieces of one two-source case: dict(y, mag, wabs, bound, x2, w2e, ref) - y before the epilogue, with
    the BatchNorm scales folded into both weight sets as the packers do (folded) or left to the epilogue"""
    ref, n_in, n_out = ref_map(n, kind, k)
    K = ksize(k)
    x, w, scale = operands(n_in, n_out, cin, cout, K)[:3]
    x2, w2, scale2 = second_operands(n_out, cin2, cout)
    bf = pieces == 1
    we = so.folded_weights(w, scale if folded else None, bf)
    w2e = so.folded_weights(w2, scale2 if folded else None, bf)[0]
    xs, x2s = (so.bf16_round(x), so.bf16_round(x2)) if bf else (x, x2)
    y, mag, wabs = so.conv64_two(xs, we, ref, x2s, w2e, j_begin, j_end)
    nj = (j_end or K) - j_begin
    bound = so.conv_bound(mag, wabs, PATH[pieces], so.conv_units_two(nj, cin, cin2))
    return dict(y=y, mag=mag, wabs=wabs, bound=bound, x2=np.asarray(x2s, np.float64), w2e=w2e, ref=ref, n_out=n_out)


def defects(case, groups=0):
    """[(name, y_defect)] of a two_source() case: (i) the second source absent, (ii) its last 32-channel chunk dropped
    (Cin2 >= 64), (iii) with mask groups: the chunks of group 1 read x2 at the tile position t instead of the row
    order[t] the tile position stands for"""
    y, x2, w2e = case["y"], case["x2"], case["w2e"]
    out = [("absent", y - x2 @ w2e)]
    if x2.shape[1] >= 64:
        out.append(("last chunk dropped", y - x2[:, -32:] @ w2e[-32:]))
    if groups > 1 and case["ref"] is not None:
        g = 1 if x2.shape[1] // 32 > 1 else 0
        order = group_orders(case["ref"], groups)[g]
        bad = y.copy()
        for c in range(g, x2.shape[1] // 32, groups):
            part = x2[:, 32 * c:32 * c + 32] @ w2e[32 * c:32 * c + 32]
            bad -= part
            bad[order] += part          # output row order[t] gets the product of x2[t]
        out.append(("tile position instead of the permuted row", bad))
    return out


# ---- section 1: the (kernel family, shape) cases of tests/test_conv_second_source_gpu.py -------------------------------
# (n, kind, k, cin, cin2, cout, j_range, groups); the kernel families each one runs on are chosen by the tests
TAIL_ROWS = (1, 127, 128, 129, 257)
HD_TAIL_ROWS = TAIL_ROWS + (255, 256)
DEAL_CASES = [          # (splits, chunks) -> shape, split target
    ((1, 1), (300, "mixed", "down", 32, 32, 32, None), 1),
    ((1, 3), (300, "mixed", "down", 32, 96, 32, None), 1),
    ((1, 1), (300, "mixed", 3, 32, 32, 32, (0, 10)), 1),
    ((1, 3), (300, "mixed", 3, 32, 96, 32, (0, 10)), 1),
    ((3, 1), (129, "mixed", 3, 32, 32, 32, None), 6),
    ((3, 2), (129, "mixed", 3, 32, 64, 32, None), 6),
    ((3, 4), (129, "mixed", 3, 32, 128, 32, None), 6),
    ((27, 2), (300, "mixed", 3, 32, 64, 32, None), 0),
]
GROUP_CHUNKS = (1, 2, 4)
WIDTHS = (32, 64, 96, 128, 256)


def section1_shapes():
    """every (n, kind, k, cin, cin2, cout, j_range, groups) the second-source module runs (pieces aside)"""
    s = set()
    for n in HD_TAIL_ROWS:
        s.add((n, "mixed", 3, 32, 64, 64, None, 0))
    for _, shape, _ in DEAL_CASES:
        s.add(shape + (0,))
    for ch in GROUP_CHUNKS:
        s.add((300, "mixed", 3, 32, 32 * ch, 64, None, 3))
    for g in (2, 4):
        s.add((300, "mixed", 3, 32, 64, 64, None, g))
    for cout in WIDTHS:
        s.add((129, "mixed", 3, 64, 64, cout, None, 0))
    return sorted(s, key=str)


def restated_splits(n_out, cout, nj, cin, target):
    """pick_splits (sparse_conv.hip) for a flavour-0 vector-path launch with a workspace, then conv_dispatch's raise that
    keeps a conv_hl / conv_rows_wp workgroup at WP_NPRE offsets or fewer"""
    nb = 1 if cout <= 32 else 2 if cout <= 64 else 3 if cout <= 96 else 2
    tiles = -(-n_out // 128) * -(-cout // (nb * 32))
    units = nj * (cin // 32)
    if tiles >= 384 or units <= 1:
        sp = 1
    else:
        sp = max(min(-(-target // tiles), units, max((24 << 20) // (n_out * cout * 4), 2), 64), 1)
    per_wg = nj if sp <= 1 else -(-nj // sp) + 1
    if per_wg > WP_NPRE:
        sp = max(sp, (nj + WP_NPRE - 2) // (WP_NPRE - 1))
    return sp


# ---- section 2: the per-model parameters of tests/test_net_program_gpu.py -----------------------------------------------
@functools.lru_cache(maxsize=None)
def model_params(m, tag, K, cin, cout, cin2=0):
    """weights, scale and shift of op `tag` of model m.  Weight magnitudes differ by powers of four between models and
    the scale takes half of it back, so the power of two of the fp16-pair packing (acc_scale) differs per model, folded
    or not, while the activations stay in the fp16 range."""
    rng = np.random.default_rng(m * 10007 + zlib.crc32(tag.encode()) % 100003)
    p = m % 3
    w = (rng.normal(0, 1, (K, cin, cout)) / np.sqrt(cin * min(K, 27)) * 4.0 ** p).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, cout) / 2.0 ** p).astype(np.float32)
    shift = rng.normal(0, 0.2, cout).astype(np.float32)
    out = dict(w=w, scale=scale, shift=shift)
    if cin2:
        out["w2"] = (rng.normal(0, 1, (1, cin2, cout)) / np.sqrt(cin2) * 4.0 ** p).astype(np.float32)
        out["scale2"] = (rng.uniform(0.5, 1.5, cout) / 2.0 ** p).astype(np.float32)
    return out
