"""cv_sp_voxel_rows_f32 (ME.utils.voxel_rows) alone against torch indexing: the gathered rows and the world points are
compared byte for byte through int32 views.  The expected side is torch only: ``column[index]``, ``x * 2.0 - 1.0`` and
``(coords4[:, 1:] * res).float()``."""
import numpy as np
import pytest
import torch

from canonicalvoting_amd.me import utils as me_utils

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1000]
SENTINEL = 0x5A5A5A5A


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def voxel_like(n, m, cuda, seed):
    """an ascending first-point index into m raw rows (rows 0 and m - 1 included when n >= 2) and coordinates with 0,
    negatives and the ends of the key window"""
    g = torch.Generator().manual_seed(seed)
    index = torch.sort(torch.randperm(m, generator=g)[:n])[0].int()
    if n >= 2:
        index[0], index[-1] = 0, m - 1
    c = torch.randint(-300, 300, (n, 4), generator=g, dtype=torch.int32)
    c[:, 0] = 0
    c[:, 1:] = with_edges(c[:, 1:], [0, -1, 1, 32703, -32703, -32704, 7])
    return c.to(cuda), index.to(cuda)


def with_edges(xyz, edge):
    """[n, 3] coordinates with the first words replaced by ``edge`` (as many as fit)"""
    flat = xyz.contiguous().reshape(-1).clone()
    k = min(len(edge), flat.numel())
    flat[:k] = torch.tensor(edge[:k], dtype=flat.dtype)
    return flat.view(-1, 3)


def special_floats(m, w, seed):
    """fp32 payloads that an arithmetic copy would change or a comparison would miss: NaNs with payloads, +-inf, -0.0, denormals"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2 ** 32, (m, w), dtype=np.uint64).astype(np.uint32)          # every bit pattern, NaNs among them
    pool = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000],
                    np.uint32)
    words.reshape(-1)[:min(pool.size, m * w)] = pool[:m * w]
    return torch.from_numpy(words.view(np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_gathers_of_three_widths_from_column_blocks_into_padded_windows(cuda, built_lib, n):
    m = 3 * n + 5
    c4, index = voxel_like(n, m, cuda, n)
    gi = index.long()
    wide = special_floats(m, 12, 100 + n).to(cuda)                       # the sources are column blocks of one wider tensor
    srcs = [wide[:, 0:1], wide[:, 2:5], wide[:, 6:12]]
    ids = torch.randint(-2 ** 31, 2 ** 31 - 1, (m, 2), dtype=torch.int64).int().to(cuda)      # int32 ids, negative ones among them
    ids[0, 0], ids[m - 1, 1] = -1, -2 ** 31
    dst_wide = torch.full((n, 16), SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)
    outs = [dst_wide[:, 1:2], dst_wide[:, 3:6], dst_wide[:, 8:14], None, None]
    assert all(not s.is_contiguous() or s.shape[0] == 1 for s in srcs)
    pts, got = me_utils.voxel_rows(c4, index, 0.03, *srcs, ids, ids[:, 1], out=outs)
    for s, g in zip(srcs, got[:3]):
        assert same_bits(s[gi], g), "width %d" % s.shape[1]
    assert got[3].dtype == torch.int32 and torch.equal(got[3], ids[gi]) and torch.equal(got[4], ids[:, 1][gi])
    assert got[4].shape == (n,)
    # destination words outside the three windows still hold the sentinel
    touched = torch.zeros(16, dtype=torch.bool)
    touched[1:2] = touched[3:6] = touched[8:14] = True
    assert bool((dst_wide.view(torch.int32)[:, ~touched] == SENTINEL).all())
    assert same_bits(pts, (c4[:, 1:] * 0.03).float())
    # the payload really holds what a value comparison cannot see
    w = bits(wide[gi])
    assert n < 2 or (np.isnan(w.view(np.float32)).any() and (w == np.int32(-2 ** 31)).any())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rf", [0, 3])
def test_recentre(cuda, built_lib, n, rf):
    m = 2 * n + 3
    c4, index = voxel_like(n, m, cuda, 7 * n + rf)
    g = torch.Generator().manual_seed(n)
    x = torch.rand((m, 6), generator=g)
    x[0] = torch.tensor([0.0, 1.0, 0.5, 2.0 ** -149, float("nan"), -0.0])
    x[m - 1] = torch.tensor([1e-30, 0.1, 0.7, 1 - 2.0 ** -24, float("inf"), 3.0e38])
    x = x.to(cuda)
    want = x[index.long()].clone()
    want[:, rf:] = want[:, rf:] * 2.0 - 1.0
    _, (got,) = me_utils.voxel_rows(c4, index, 0.05, x, recentre_from=rf, points=False)
    # (x * 2 is exact: the one rounding of x * 2 - 1 is the same as the two torch ops'; NaN payloads pass through both the same way)
    nan = torch.isnan(want)
    assert torch.equal(nan, torch.isnan(got))
    assert same_bits(torch.where(nan, torch.zeros_like(want), want), torch.where(nan, torch.zeros_like(got), got))
    assert same_bits(want[:, :rf], got[:, :rf])


@pytest.mark.parametrize("n", SIZES)
def test_eight_jobs_at_once_and_a_ninth_is_refused(cuda, built_lib, n):
    m = n + 17
    c4, index = voxel_like(n, m, cuda, 11 * n)
    gi = index.long()
    cols = [special_floats(m, w, 200 + w + n).to(cuda) for w in (1, 2, 3, 4, 5, 6, 7)] + \
           [torch.arange(m, dtype=torch.int32, device=cuda) - 5]
    pts, got = me_utils.voxel_rows(c4, index, 0.06, *cols)
    assert len(got) == 8 and all(same_bits(c[gi], g) for c, g in zip(cols, got))
    assert same_bits(pts, (c4[:, 1:] * 0.06).float())
    with pytest.raises(ValueError, match="at most 8"):
        me_utils.voxel_rows(c4, index, 0.06, *(cols + cols[:1]))


@pytest.mark.parametrize("res", [0.03, 0.05, 0.06])
@pytest.mark.parametrize("n", SIZES)
def test_world_points_are_the_bits_of_the_torch_expression(cuda, built_lib, n, res):
    g = torch.Generator().manual_seed(n)
    c = torch.randint(-32704, 32704, (n, 4), generator=g, dtype=torch.int32)
    c[:, 1:] = with_edges(c[:, 1:], [0, 32703, -32703, -1, 1, -32704])
    c = c.to(cuda)
    index = torch.arange(n, dtype=torch.int32, device=cuda)
    want = (c[:, 1:] * res).float()
    pts, got = me_utils.voxel_rows(c, index, res)
    assert got == [] and same_bits(pts, want)
    if n >= 2:
        assert {0, 32703, -32703} <= set(c[:, 1:].reshape(-1).tolist())


@pytest.mark.parametrize("n", SIZES)
def test_without_world_points(cuda, built_lib, n):
    m = n + 1
    _, index = voxel_like(n, m, cuda, 13 * n)
    x = special_floats(m, 3, 300 + n).to(cuda)
    pts, (got,) = me_utils.voxel_rows(None, index, None, x, points=False)
    assert pts is None and same_bits(x[index.long()], got)
