"""CPU checks of tests/coord_ref.py: every adversarial coordinate set has the properties it claims, the suite's oracle
(oracle/sparse_oracle.py, which packs its keys into the kernel's bit fields) equals the unpacked dict reference on all of them,
and the exact comparison rejects each named wrong result on a named case.  The wrong results are mutations of the expected
arrays or of the table restatement, never of a kernel.

Measured on the cases as seeded (the tests below assert the bounds, not these figures).  Rows per level 0..4, and for the
tail-chain cases the occupied run of the named level's table through the wrap, the absent keys a map of the network asks for
that are homed inside the run, and how many of those are homed in its tail, so that the miss walks through slot 0:

  tail_chain_1024      500/341/213/98/31      level 0, 1024 slots: [1020, 1024) + [0, 251)   absent in run 5507, wrapping 21
  tail_chain_8192      2400/1187/475/248/104  level 0, 8192 slots: [8188, 8192) + [0, 214)   absent in run 1286, wrapping 8
  tail_chain_coarse_1  410/270/246/191/100    level 1, 1024 slots: [1020, 1024) + [0, 168)   absent in run 893, wrapping 9
  tail_chain_coarse_2  415/399/270/209/162    level 2, 1024 slots: [1020, 1024) + [0, 166)   absent in run 792, wrapping 8
  tail_chain_coarse_3  410/407/385/270/255    level 3, 1024 slots: [1020, 1024) + [0, 172)   absent in run 950, wrapping 10
  tail_chain_coarse_4  415/415/413/391/270    level 4, 1024 slots: [1020, 1024) + [0, 165)   absent in run 879, wrapping 8
  negative_floor 2500/2073/810/190/52   window_edge 155/32/8/4/4   batches 600/260/40/40/40   first_child_late 1536/673/146/45/20
  wave_run 400/236/66/12/12   dense_full 729/125/27/8/8   isolated 216 at every level   sort_one_cube 52/20/6/4/4
  sizes_N: N rows, 8 at level 4 from N = 63 on (2049: 2049/891/213/62/8)   sort_extent_E: 600 rows, shift 0/1/1/1/2 for E = 63..128

Named wrong results and the cases that reject them: coarse set in sorted-key order - negative_floor, first_child_late;
truncating division - negative_floor; a neighbour across batches - batches; octant bits z fastest - negative_floor, dense_full,
tail_chain_coarse_2; probing that stops at the last slot - every tail_chain case; unclamped batch in the sort key - batches."""
import numpy as np
import pytest

from oracle import sparse_oracle as so
from tests import coord_ref as cr

TAIL_CASES = ["tail_chain_1024", "tail_chain_8192"] + ["tail_chain_coarse_%d" % L for L in (1, 2, 3, 4)]


def level_key(coords, L):
    c = np.asarray(coords, np.int64).copy()
    c[:, 1:] = c[:, 1:] // (1 << L) * (1 << L)
    return [tuple(r) for r in c.tolist()]


# ------------------------------------------------------------------------------------------------------ what the cases claim
@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_case_is_a_valid_small_coordinate_set(name):
    c = cr.case(name).coords
    assert c.dtype == np.int64 and c.ndim == 2 and c.shape[1] == 4 and 1 <= len(c) <= 2500
    assert len({tuple(r) for r in c.tolist()}) == len(c)                                # unique
    assert c[:, 1:].min() >= cr.WINDOW_LO and c[:, 1:].max() <= cr.WINDOW_HI and c[:, 0].min() >= 0 and c[:, 0].max() <= 65535


def test_mix64_restatement_equals_python_integer_arithmetic():
    M = (1 << 64) - 1
    keys = [0, 1, M - 1, 0x0000800080008000, 0xffff7fff7fff7fff, 0x0123456789abcdef]
    for k, got in zip(keys, cr.mix64(np.array(keys, np.uint64)).tolist()):
        k ^= k >> 33
        k = k * 0xff51afd7ed558ccd & M
        k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 & M
        k ^= k >> 33
        assert got == k
    assert cr.packed_key([[65535, -32768, 0, 32767]]).tolist() == [0xffff00008000ffff]
    assert [cr.table_capacity(n) for n in (1, 512, 513, 2048, 2049, 4096, 4097)] == [1024, 1024, 2048, 4096, 8192, 8192, 16384]


@pytest.mark.parametrize("name", TAIL_CASES)
def test_tail_chain_runs_through_the_wrap_with_an_absent_key_inside(name):
    case = cr.case(name)
    (L, t), = case.claims["tables"].items()
    cap = t["cap"]
    assert cr.table_capacity(case.n) == cap and (case.n <= 512 if cap == 1024 else 2049 <= case.n <= 4096)
    assert len(case.claims["chain"]) >= 150 and (cr.home_slots(case.claims["chain"], cap) >= cap - 4).all()
    lv = cr.case_reference(name)["levels"][L]
    have = {tuple(r) for r in lv.tolist()}
    assert all(tuple(r) in have for r in case.claims["chain"].tolist())
    # the occupied run starts in the last 4 slots and continues past slot 0 for at least 100 slots
    assert cap - 4 <= t["run_start"] < cap and t["run_past_zero"] >= 100
    # absent keys that a map of the network asks for, homed inside the run; those homed in its tail must walk the wrap
    assert t["absent_in_run"] >= 1 and t["absent_wrapping"] >= 1
    ghosts = case.claims["ghosts"]
    assert (cr.home_slots(ghosts, cap) >= cap - 4).all() and not any(tuple(r) in have for r in ghosts.tolist())
    s = 1 << L
    assert all(any((g[0], g[1] + dx * s, g[2] + dy * s, g[3] + dz * s) in have for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                   for dz in (-1, 0, 1)) for g in ghosts.tolist())                      # a 3x3x3 map at this level asks for each
    # the line path of the level-0 job needs the box to fit the bitmap (tail_chain_coarse_4 cannot: see COARSE_RADIUS)
    assert case.claims["fits_bitmap"] == (name != "tail_chain_coarse_4")
    assert case.claims["fits_bitmap"] == (cr.box_cells(case.coords) <= cr.BITMAP_BITS)
    print(name, "N per level", [len(x) for x in cr.case_reference(name)["levels"]], t)


def test_negative_floor_straddles_the_origin():
    c = cr.case("negative_floor").coords
    assert (c[:, 1:].min(0) == -17).all() and (c[:, 1:].max(0) == 17).all() and len(c) == 2500
    assert not np.array_equal(c, c[np.lexsort(c.T[::-1])])                              # rows are not in sorted order


def test_window_edge_touches_both_ends_on_different_axes_in_different_batches():
    c = cr.case("window_edge").coords
    lo, hi = c[(c[:, 1:] == cr.WINDOW_LO).any(1)], c[(c[:, 1:] == cr.WINDOW_HI).any(1)]
    assert len(lo) and len(hi)
    assert {0, 3} == set(c[:, 0].tolist()) and 0 in lo[:, 0] and 3 in hi[:, 0]
    assert (c[c[:, 0] == 0][:, 1] == cr.WINDOW_LO).any() and (c[c[:, 0] == 3][:, 2] == cr.WINDOW_HI).any() and \
        (c[c[:, 0] == 3][:, 3] == cr.WINDOW_LO).any()


def test_batches_hold_the_same_clump():
    c = cr.case("batches").coords
    assert tuple(sorted(set(c[:, 0].tolist()))) == cr.BATCHES == (0, 7, 511, 512, 65535)
    clumps = [sorted(map(tuple, c[c[:, 0] == b][:, 1:].tolist())) for b in cr.BATCHES]
    assert all(cl == clumps[0] for cl in clumps)
    assert (np.diff(c[:, 0]) != 0).sum() > len(c) // 2                                  # interleaved


def test_first_child_late_rows_are_far_from_their_siblings():
    case = cr.case("first_child_late")
    seen = set()
    for L, cell, early, late in case.claims["marked"]:
        rows = [i for i, k in enumerate(level_key(case.coords, L)) if k == cell]
        assert rows[0] == early < 100 and rows[1] == late and late - early >= 900 and len(rows) == 3
        assert len(set(level_key(case.coords[rows], L - 1))) == 3                       # three different children at L - 1
        seen.add(L)
    assert seen == {1, 2, 3, 4} and len(case.claims["marked"]) == 12


def test_wave_run_crosses_the_wave_and_the_block_boundary():
    case = cr.case("wave_run")
    assert case.n == 400
    for first, last, edge in case.claims["runs"]:
        assert edge % 64 == 63 and first < edge < last
        for L in (1, 2, 3, 4):
            k = level_key(case.coords, L)
            assert k[edge] == k[edge + 1] and k[first - 1] != k[first] and k[last] != k[last + 1]
            if L >= 2:
                assert len(set(k[first:last + 1])) == 1
            assert k.index(k[edge]) == first                                            # the run holds the voxel's first row
    assert [e for _, _, e in case.claims["runs"]] == [63, 255]
    for r in case.claims["lane0_starts"]:                                               # a voxel that first appears at lane 0
        for L in (1, 2, 3, 4):
            k = level_key(case.coords, L)
            assert r % 64 == 0 and k.index(k[r]) == r
    k1 = level_key(case.coords, 1)
    assert k1[128] == k1[129] == k1[131] and k1.count(k1[192]) == 1


def test_dense_full_hits_everywhere_inside():
    case, ref = cr.case("dense_full"), cr.case_reference("dense_full")
    c = case.coords
    assert len(c) == 729 and (c[:, 1:].min(0) == -4).all() and (c[:, 1:].max(0) == 4).all()
    inner2, inner1 = (np.abs(c[:, 1:]) <= 2).all(1), (np.abs(c[:, 1:]) <= 3).all(1)
    assert inner2.sum() == 125 and (ref["maps"][(5, 1, 1)][inner2] >= 0).all()
    assert (cr.mask_key(ref["maps"][(3, 1, 1)], 0, 27)[inner1] == (1 << 27) - 1).all()


def test_isolated_voxels_only_hit_themselves():
    case, ref = cr.case("isolated"), cr.case_reference("isolated")
    d = np.abs(case.coords[:, None, 1:] - case.coords[None, :, 1:]).max(-1)
    assert d[~np.eye(case.n, dtype=bool)].min() >= 40
    assert [len(x) for x in ref["levels"]] == [case.n] * 5 and case.n > 192
    for (k, ts, stride), m in ref["maps"].items():
        if stride == 2:                 # the only child, in the column of its octant
            assert ((m >= 0).sum(1) == 1).all() and cr.same(m.max(1), np.arange(case.n)), (k, ts, stride)
            continue
        want = np.full_like(m, -1)
        want[:, (k ** 3) // 2] = np.arange(case.n)
        assert cr.same(m, want), (k, ts, stride)


def test_sizes_cut_one_block():
    assert cr.SIZES == (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
    big = cr.case("sizes_2049").coords
    for n in cr.SIZES:
        assert cr.same(cr.case("sizes_%d" % n).coords, big[:n])


@pytest.mark.parametrize("e,shift", [(63, 0), (64, 1), (65, 1), (127, 1), (128, 2)])
def test_sort_extents_sit_on_the_shift_boundaries(e, shift):
    c = cr.case("sort_extent_%d" % e).coords
    assert int((c[:, 1:].max(0) - c[:, 1:].min(0)).max()) == e == cr.case("sort_extent_%d" % e).claims["extent"]
    assert cr.sort_shift(c) == shift and set(c[:, 0].tolist()) == {0, 1}
    q = (c[:, 1:] - c[:, 1:].min(0)) >> shift
    assert q.max() == e >> shift and q.max() < 64 and (shift == 0 or (e >> (shift - 1)) >= 64)
    perm, _ = cr.sort_perm(c)
    assert not np.array_equal(perm, np.arange(len(c)))


def test_sort_one_cube_stays_in_place():
    c = cr.case("sort_one_cube").coords
    key = cr.sort_key(c)
    assert cr.sort_shift(c) == 2 and key[0] < key[1] and key[-2] < key[-1] and len(set(key[1:-1].tolist())) == 1
    assert len(c) == 52 and not np.array_equal(c[1:-1], c[1:-1][np.lexsort(c[1:-1].T[::-1])])       # shuffled inside the cube
    assert cr.same(cr.sort_perm(c)[0], np.arange(len(c)))


# --------------------------------------------------------------------------------------- the suite's oracle on every case
@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_packed_oracle_equals_the_unpacked_reference(name):
    ref = cr.case_reference(name)
    ocm = so.CoordinateManager(cr.case(name).coords)
    for i in range(cr.NUM_LEVELS):
        assert cr.same(ocm.coords[1 << i], ref["levels"][i]), i                          # order included
    for k, ts, stride in cr.NET_MAPS:
        assert cr.same(ocm.map(k, ts, stride), ref["maps"][(k, ts, stride)]), (k, ts, stride)
    for ts_c in (2, 4, 8, 16):          # the up map against the strided map, independently of up_map's own octant arithmetic
        up, down = ref["up"][ts_c], ref["maps"][(2, ts_c // 2, 2)]
        assert ((up >= 0).sum(1) == 1).all()
        f, j = np.nonzero(up >= 0)
        assert np.array_equal(down[up[f, j], j], f)
        assert cr.same(cr.transposed(down, len(up)), up)                                 # and it IS the transposed strided map


def test_transposed_and_mask_key_on_a_hand_made_map():
    nbr = np.array([[0, -1, 2], [-1, 0, -1], [1, 2, 0]])
    assert cr.same(cr.transposed(nbr, 4), [[0, 1, 2], [2, -1, -1], [-1, 2, 0], [-1, -1, -1]])
    assert cr.mask_key(nbr, 0, 3).tolist() == [5 | 2 << 7, 2 | 1 << 7, 7 | 3 << 7]      # narrow group: popcount above bit 7
    wide = np.concatenate([nbr, np.full((3, 6), -1)], 1)
    assert cr.mask_key(wide, 0, 9).tolist() == [5, 2, 7] and cr.mask_key(wide, 1, 3).tolist() == [2 | 1 << 7, 1 | 1 << 7, 3 | 2 << 7]


# ------------------------------------------------------------------------------------------------------ named wrong results
def test_rejects_coarse_set_in_sorted_key_order():
    for name in ("negative_floor", "first_child_late"):
        ref = cr.case_reference(name)
        for i in (1, 2, 3, 4):
            lv = ref["levels"][i]
            wrong = lv[np.argsort(so._keys(lv), kind="stable")]
            assert sorted(map(tuple, wrong.tolist())) == sorted(map(tuple, lv.tolist())) and not cr.same(wrong, lv), (name, i)


def test_rejects_truncating_division_of_negative_coordinates():
    trunc = lambda v, s: int(v / s) * s
    c = cr.case("negative_floor").coords
    wrong, ref = cr.levels(c, floor=trunc), cr.case_reference("negative_floor")["levels"]
    for i in (1, 2, 3, 4):
        assert not cr.same(wrong[i], ref[i]), i
    assert cr.same(cr.levels(np.abs(c[:50]), floor=trunc)[1], cr.levels(np.abs(c[:50]))[1])       # (equal where nothing is negative)


def test_rejects_a_neighbour_found_across_batches():
    ref = cr.case_reference("batches")
    for k, ts, stride in ((5, 1, 1), (3, 1, 1), (3, 4, 1), (2, 1, 2)):
        i = ts.bit_length() - 1
        wrong = cr.kernel_map(ref["levels"][i], ref["levels"][i + (stride == 2)], k, ts, same_batch=False)
        assert not cr.same(wrong, ref["maps"][(k, ts, stride)]), (k, ts, stride)
        assert ((wrong >= 0) == (ref["maps"][(k, ts, stride)] >= 0)).all()              # same hits, rows of another batch
    lv0, m = ref["levels"][0], ref["maps"][(5, 1, 1)]                                    # and the reference never crosses
    u, j = np.nonzero(m >= 0)
    assert (lv0[m[u, j], 0] == lv0[u, 0]).all()


def test_rejects_octant_bits_in_z_fastest_order():
    for name in ("negative_floor", "dense_full", "tail_chain_coarse_2"):
        ref = cr.case_reference(name)
        for i in range(4):
            wrong = cr.up_map(ref["levels"][i], ref["levels"][i + 1], 2 << i, octant=lambda ox, oy, oz: oz + 2 * oy + 4 * ox)
            assert not cr.same(wrong, ref["up"][2 << i]), (name, i)


@pytest.mark.parametrize("name", TAIL_CASES)
def test_rejects_probing_that_stops_at_the_last_slot(name):
    case = cr.case(name)
    (L, t), = case.claims["tables"].items()
    lv = cr.case_reference(name)["levels"][L]
    table = cr.occupancy(lv, t["cap"])
    found = cr.table_find(table, lv)
    assert (found >= 0).all()
    chain_found = cr.table_find(table, case.claims["chain"])
    assert (chain_found < t["run_past_zero"]).sum() >= 100                               # chain keys stored behind the wrap
    wrong = cr.table_find(table, lv, wrap=False)                                         # the same table, a lookup that does not wrap
    assert not cr.same(wrong >= 0, found >= 0) and (wrong < 0).sum() >= 100
    dropped = cr.occupancy(lv, t["cap"], wrap=False)                                     # an insert that does not wrap loses keys
    assert sum(k is not None for k in dropped) < sum(k is not None for k in table) == len(lv)


def test_rejects_unclamped_batch_in_the_sort_key():
    c = cr.case("batches").coords
    good, wrong = np.argsort(cr.sort_key(c), kind="stable"), np.argsort(cr.sort_key(c, clamp=False), kind="stable")
    assert not cr.same(wrong, good)
    low = c[c[:, 0] < 512]                                                               # (equal where no batch index is clamped)
    assert cr.same(np.argsort(cr.sort_key(low, clamp=False), kind="stable"), np.argsort(cr.sort_key(low), kind="stable"))
