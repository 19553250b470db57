"""An independent reference of the coordinate manager and hand-made adversarial coordinate sets, numpy and Python only.

Three parts, shared by tests/test_coord_ref.py (CPU: the cases' claims, the suite's oracle against this reference, named wrong
results) and tests/test_coords_edge_gpu.py (the kernels of csrc/sparse_coords.hip, the mask orders of csrc/conv_prep.hip and
transpose_map of csrc/sparse_train.hip against this reference):

  1. Reference.  Coordinates are never packed into bit fields here: sets are dicts keyed by (b, x, y, z) tuples, so an
     aliasing mistake of the kernel's 16-bit key fields (which oracle/sparse_oracle.py shares through _keys) is not shared.
  2. Table restatement.  mix64, the packed key and linear-probing occupancy of the kernel's hash table for a given capacity.
     It is used ONLY to construct collision cases and to verify what they claim, never as the expected value of a map.  The set
     of occupied slots under linear probing does not depend on the insertion order, so these claims hold for the device's
     table whatever order its atomics ran in.
  3. Cases.  Each is a function of no arguments returning a Case: int64 [N, 4] coordinates (batch, x, y, z), all valid (unique,
     inside the key window), with the properties it claims in `.claims`.  N stays <= about 3000 (<= 2500 for the 5x5x5 map).
"""
import functools

import numpy as np

NUM_LEVELS = 5
BITMAP_BITS = (1 << 20) * 32          # CV_BITMAP_WORDS * 32 (csrc/cv_common.h): cells of the occupancy bitmap
WINDOW_LO, WINDOW_HI = -32704, 32703  # the key window CoordinateManager documents
NET_MAPS = ((5, 1, 1), (3, 1, 1), (3, 2, 1), (3, 4, 1), (3, 8, 1), (3, 16, 1), (2, 1, 2), (2, 2, 2), (2, 4, 2), (2, 8, 2))


# ====================================================================================================== 1. reference
def _rows(a):
    return [tuple(r) for r in np.asarray(a, np.int64).reshape(-1, 4).tolist()]


def floor_to(v, s):
    """floor(v / s) * s with Python floor division (negative coordinates round down)"""
    return v // s * s


def levels(coords, floor=floor_to):
    """the coordinate sets of tensor strides 1, 2, 4, 8, 16: level L = floor(c / 2^L) * 2^L, duplicates removed, in the
    order of the first appearance of a child in the next finer set"""
    out = [np.asarray(coords, np.int64).reshape(-1, 4)]
    for L in range(1, NUM_LEVELS):
        s = 1 << L
        seen = {}
        for b, x, y, z in _rows(out[-1]):
            seen.setdefault((b, floor(x, s), floor(y, s), floor(z, s)), None)
        out.append(np.array(list(seen), np.int64).reshape(-1, 4))
    return out


def kernel_offset(k, j):
    """offset j of a k^3 kernel, x fastest; odd kernels are centred, even kernels start at 0 (build_kernel_map)"""
    lo = -(k // 2) if k % 2 else 0
    return lo + j % k, lo + j // k % k, lo + j // (k * k)


def kernel_map(in_set, out_set, k, ts, same_batch=True):
    """nbr [N_out, k^3]: row of (out + offset_j * ts) in in_set, or -1.  same_batch=False is a named wrong result: the
    batch index is ignored (the first row with the same x, y, z in ANY batch is found)"""
    key = (lambda t: t) if same_batch else (lambda t: t[1:])
    table = {}
    for i, t in enumerate(_rows(in_set)):
        table.setdefault(key(t), i)
    out = np.asarray(out_set, np.int64).reshape(-1, 4)
    nbr = np.empty((len(out), k ** 3), np.int64)
    for j in range(k ** 3):
        ox, oy, oz = kernel_offset(k, j)
        q = out + np.array([0, ox * ts, oy * ts, oz * ts], np.int64)
        nbr[:, j] = [table.get(key(t), -1) for t in _rows(q)]
    return nbr


def up_map(fine, coarse, ts, octant=lambda ox, oy, oz: ox + 2 * oy + 4 * oz):
    """[N_fine, 8] map of the transposed k2s2 convolution onto the set of stride ts / 2: the parent's row (in `coarse`, stride
    ts) in the octant column ox + 2 oy + 4 oz, -1 elsewhere"""
    table = {t: i for i, t in enumerate(_rows(coarse))}
    h = ts // 2
    up = np.full((len(fine), 8), -1, np.int64)
    for f, (b, x, y, z) in enumerate(_rows(fine)):
        px, py, pz = floor_to(x, ts), floor_to(y, ts), floor_to(z, ts)
        up[f, octant((x - px) // h, (y - py) // h, (z - pz) // h)] = table[(b, px, py, pz)]
    return up


def transposed(nbr, n_in):
    """[n_in, K]: t[i, j] = u where nbr[u, j] == i, -1 where no output row reads input row i through offset j"""
    nbr = np.asarray(nbr, np.int64)
    t = np.full((n_in, nbr.shape[1]), -1, np.int64)
    u, j = np.nonzero(nbr >= 0)
    t[nbr[u, j], j] = u
    return t


def mask_key(nbr, jb, je):
    """sort key of the mask orders over offsets [jb, je): bit (j - jb) = entry j >= 0; groups of at most 7 offsets carry the
    number of valid offsets above bit 7 (group_mask, csrc/conv_prep.hip)"""
    v = np.asarray(nbr)[:, jb:je] >= 0
    m = np.zeros(len(v), np.int64)
    for j in range(je - jb):
        m |= v[:, j].astype(np.int64) << j
    if je - jb <= 7:
        m |= v.sum(1).astype(np.int64) << 7
    return m


def _interleave3(x, y, z, bits):
    k = np.zeros(len(x), np.int64)
    for bit in range(bits):
        for ax, v in enumerate((x, y, z)):
            k |= ((v >> bit) & 1) << (3 * bit + ax)
    return k


def sort_shift(coords):
    c = np.asarray(coords, np.int64)
    ext = int((c[:, 1:].max(0) - c[:, 1:].min(0)).max())
    shift = 0
    while (ext >> shift) >= 64:
        shift += 1
    return shift


def sort_key(coords, clamp=True):
    """key of the spatial row sort: batch index clamped to [0, 511] above bit 18, below it the Morton code (6 bits per axis,
    x lowest) of (c - min) >> shift, shift = the smallest that brings the largest extent (max - min) under 64.
    clamp=False is a named wrong result."""
    c = np.asarray(coords, np.int64)
    q = (c[:, 1:] - c[:, 1:].min(0)) >> sort_shift(c)
    b = np.clip(c[:, 0], 0, 511) if clamp else c[:, 0]
    return (b << 18) | _interleave3(q[:, 0], q[:, 1], q[:, 2], 6)


def sort_perm(coords):
    """(perm, inv) of the stable sort by sort_key: perm[s] = original row of sorted row s"""
    perm = np.argsort(sort_key(coords), kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return perm, inv


def morton_key(coords):
    """cv_sp_morton_keys: the low 15 bits of the batch index above bit 48, the 16-bit Morton code of c + 32768 below"""
    c = np.asarray(coords, np.int64)
    u = c[:, 1:] + 32768
    return ((c[:, 0] & 0x7fff) << 48) | _interleave3(u[:, 0], u[:, 1], u[:, 2], 16)


def reference(coords, stem=True):
    """every set and map of one forward on `coords`: dict(levels=[5 sets], maps={(k, ts, stride): nbr}, up={ts_coarse: up});
    stem=False leaves the 5x5x5 map out"""
    lv = levels(coords)
    maps = {}
    for k, ts, stride in NET_MAPS[0 if stem else 1:]:
        i = ts.bit_length() - 1
        maps[(k, ts, stride)] = kernel_map(lv[i], lv[i + (stride == 2)], k, ts)
    up = {2 << i: up_map(lv[i], lv[i + 1], 2 << i) for i in range(4)}
    return dict(levels=lv, maps=maps, up=up)


def same(got, want):
    """the comparison of these tests: exact equality of integer arrays, shape and row order included"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype.kind in "iu" and want.dtype.kind in "iu" and bool(np.array_equal(got, want))


# ============================================================================================ 2. table restatement
def mix64(k):
    k = np.atleast_1d(np.asarray(k, np.uint64)).copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def packed_key(coords):
    """pack_key of csrc/sparse_coords.hip: 16 bits per field, spatial fields biased by 32768"""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    f = [(c[:, 0] & 0xffff).astype(np.uint64)] + [((c[:, a] + 32768) & 0xffff).astype(np.uint64) for a in (1, 2, 3)]
    return (f[0] << np.uint64(48)) | (f[1] << np.uint64(32)) | (f[2] << np.uint64(16)) | f[3]


def table_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def home_slots(coords, cap):
    return (mix64(packed_key(coords)) & np.uint64(cap - 1)).astype(np.int64)


def occupancy(coords, cap, wrap=True):
    """the table after inserting every key with linear probing: list of cap entries, a packed key or None.  wrap=False is a
    named wrong result: probing stops at the last slot (the key is dropped) instead of going on at slot 0"""
    table = [None] * cap
    for key, s in zip(packed_key(coords).tolist(), home_slots(coords, cap).tolist()):
        while s < cap and table[s] is not None and table[s] != key:
            s += 1
            if s == cap and wrap:
                s = 0
        if s < cap:
            table[s] = key
    return table


def table_find(table, coords, wrap=True):
    """slot of every key in the table or -1 (probing to the first empty slot); wrap=False stops behind the last slot"""
    cap = len(table)
    out = []
    for key, s in zip(packed_key(coords).tolist(), home_slots(coords, cap).tolist()):
        while s < cap and table[s] is not None and table[s] != key:
            s += 1
            if s == cap and wrap:
                s = 0
        out.append(s if s < cap and table[s] == key else -1)
    return np.array(out, np.int64)


def wrapped_run(table):
    """(start, end): slots [start, cap) and [0, end) are occupied, start - 1 and end are empty: the run through the wrap"""
    cap = len(table)
    start, end = cap, 0
    while start > 0 and table[start - 1] is not None:
        start -= 1
    while end < cap and table[end] is not None:
        end += 1
    return start, end


def absent_queries(in_set, out_set, k, ts):
    """distinct coordinates that the (k, ts) map of out_set asks in_set for and does not find"""
    have = set(_rows(in_set))
    out = np.asarray(out_set, np.int64).reshape(-1, 4)
    q = set()
    for j in range(k ** 3):
        ox, oy, oz = kernel_offset(k, j)
        q.update(_rows(out + np.array([0, ox * ts, oy * ts, oz * ts], np.int64)))
    return np.array(sorted(q - have), np.int64).reshape(-1, 4)


def chain_claims(level_set, cap, queries):
    """what a tail-chain case claims of one level's table: the occupied run through the wrap and the absent queried keys
    whose home slot lies in it.  Those homed in the tail part [start, cap) must walk through the wrap to the first empty slot."""
    start, end = wrapped_run(occupancy(level_set, cap))
    h = home_slots(queries, cap) if len(queries) else np.zeros(0, np.int64)
    return dict(cap=cap, run_start=start, run_past_zero=end, absent_in_run=int(((h >= start) | (h < end)).sum()),
                absent_wrapping=int((h >= start).sum()))


# ================================================================================================================ 3. cases
class Case:
    def __init__(self, name, coords, **claims):
        self.name, self.coords, self.claims = name, np.ascontiguousarray(coords, np.int64).reshape(-1, 4), claims
        self.n = len(self.coords)

    def __repr__(self):
        return self.name


def box_cells(coords):
    """cells of the occupancy bitmap over the set's bounding box: extents times (largest batch index + 1)"""
    c = np.asarray(coords, np.int64)
    ext = c[:, 1:].max(0) - c[:, 1:].min(0) + 1
    return int(ext[0]) * int(ext[1]) * int(ext[2]) * int(c[:, 0].max() + 1)


def _grid(lo, hi):
    r = np.arange(lo, hi)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def _with_batch(xyz, b=0):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], 1)


def _thinned_block(lo, hi, n, seed):
    """n voxels of the block [lo, hi)^3 in shuffled order"""
    g = _grid(lo, hi)
    rng = np.random.default_rng(seed)
    return _with_batch(g[rng.permutation(len(g))[:n]])


def _tail_cells(L, cap, radius, count):
    """the `count` level-L cells nearest the origin, within +-radius cells, whose key's home slot is one of the last 4 slots"""
    cells = _with_batch(_grid(-radius, radius + 1) << L)
    tail = cells[home_slots(cells, cap) >= cap - 4]
    order = np.argsort((tail[:, 1:] ** 2).sum(1), kind="stable")
    assert len(order) >= count, (L, cap, len(order))
    return tail[order[:count]]


GUARD = 128      # fillers are not homed in the GUARD slots in front of the tail: the run must START in the last 4 slots


def _fillers(chosen, ghosts, L, cap, n_fill, reach=1):
    """level-L cells homed outside the guard zone: first one neighbour of every ghost (a cell homed in the last 4 slots that
    stays OUT of the set, so that a map asks for it and must walk the wrap to miss it), then cells next to the chosen ones,
    round robin over the offsets"""
    s = 1 << L
    have = set(_rows(chosen)) | set(_rows(ghosts))
    out = []
    offs = _grid(-reach, reach + 1) * s
    offs = offs[np.random.default_rng(L).permutation(len(offs))]
    for base, each in ((ghosts, True), (chosen, False)):
        todo = np.ones(len(base), bool)
        for o in offs:
            cand = base + np.array([0, o[0], o[1], o[2]], np.int64)
            h = home_slots(cand, cap)
            ok = ((h < cap - 4 - GUARD) | (h >= cap - 4)) & todo
            for i, t in enumerate(_rows(cand)):
                if ok[i] and t not in have and len(out) < n_fill:
                    have.add(t)
                    out.append(t)
                    todo[i] = not each
    return np.array(out, np.int64).reshape(-1, 4)


N_GHOSTS = 8


def _tail_chain(name, cap, radius, n_chain, n_total, seed):
    tail = _tail_cells(0, cap, radius, n_chain + N_GHOSTS)
    chain, ghosts = tail[:n_chain], tail[n_chain:]
    c = np.concatenate([chain, _fillers(chain, ghosts, 0, cap, n_total - n_chain, reach=1)])
    c = c[np.random.default_rng(seed).permutation(len(c))]
    assert table_capacity(len(c)) == cap
    return Case(name, c, chain=chain, ghosts=ghosts, tables={0: chain_claims(c, cap, absent_queries(c, c, 5, 1))},
                fits_bitmap=box_cells(c) <= BITMAP_BITS)


def tail_chain_1024():
    """capacity 1024: 160 voxels homed in the last 4 slots, neighbours around them, 500 rows"""
    return _tail_chain("tail_chain_1024", 1024, 20, 160, 500, 1)


def tail_chain_8192():
    """capacity 8192: 160 voxels homed in the last 4 slots, neighbours around them, 2400 rows"""
    return _tail_chain("tail_chain_8192", 8192, 44, 160, 2400, 2)


# cells are searched within +-radius cells.  L = 1, 2, 3: the box of the case fits the occupancy bitmap (L = 3: 37 cells of 8
# and a filler cell on either side, 312^3 < 2^25).  L = 4 cannot: 2^25 bits hold 8192 level-4 cells, of which about 32 are
# homed in the last 4 of 1024 slots - no run of 100 - so that case's level-0 job takes its per-entry path; its level-4 table
# is probed by the coarse jobs, which never use the bitmap
COARSE_RADIUS = {1: 32, 2: 32, 3: 18, 4: 32}


def tail_chain_coarse(L):
    """the level-L table (capacity 1024) holds 150 cells homed in its last 4 slots, each with 1 to 3 children, and cells next
    to them with one child each"""
    cap, s = 1024, 1 << L
    tail = _tail_cells(L, cap, COARSE_RADIUS[L], 150 + N_GHOSTS)
    chosen, ghosts = tail[:150], tail[150:]
    cells = np.concatenate([chosen, _fillers(chosen, ghosts, L, cap, 120)])
    rng = np.random.default_rng(10 + L)
    rows = []
    for i, cell in enumerate(cells):
        kids = rng.permutation(s ** 3)[:int(rng.integers(1, 4)) if i < len(chosen) else 1]
        for kid in kids:
            rows.append(cell + np.array([0, kid % s, kid // s % s, kid // (s * s)], np.int64))
    c = np.array(rows, np.int64)
    c = c[rng.permutation(len(c))]
    assert table_capacity(len(c)) == cap
    lv = levels(c)
    q = [absent_queries(lv[L], lv[L], 3, s)]
    if L < 4:
        q.append(absent_queries(lv[L], lv[L + 1], 2, s))
    q = np.unique(np.concatenate(q), axis=0)
    return Case("tail_chain_coarse_%d" % L, c, chain=chosen, ghosts=ghosts, tables={L: chain_claims(lv[L], cap, q)},
                fits_bitmap=box_cells(c) <= BITMAP_BITS)


def negative_floor():
    """a block straddling the origin on every axis, thinned, rows shuffled"""
    return Case("negative_floor", _thinned_block(-17, 18, 2500, 3))


def window_edge():
    """two dense clumps touching -32704 and +32703 on different axes, in different batches"""
    a = _with_batch(_grid(0, 4) + np.array([WINDOW_LO, 3, -2]), 0)
    b = _with_batch(_grid(-3, 1) + np.array([12, WINDOW_HI, 7]), 3)
    d = _with_batch(_grid(0, 3) + np.array([-5, 40, WINDOW_LO]), 3)
    c = np.concatenate([a, b, d])
    return Case("window_edge", c[np.random.default_rng(4).permutation(len(c))])


BATCHES = (0, 7, 511, 512, 65535)


def batches():
    """the same xyz clump in five batches, rows interleaved: neighbours never cross a batch, the sort clamps at 511"""
    clump = _thinned_block(-3, 4, 120, 5)[:, 1:]
    c = np.concatenate([_with_batch(clump, b) for b in BATCHES])
    return Case("batches", c[np.random.default_rng(6).permutation(len(c))], batch_set=BATCHES)


def _placed(background, inserts):
    """rows `inserts` {row: (b, x, y, z)} at their rows, the background's rows in order everywhere else"""
    n = len(background) + len(inserts)
    out = np.empty((n, 4), np.int64)
    it = iter(background)
    for r in range(n):
        out[r] = inserts[r] if r in inserts else next(it)
    assert len(set(_rows(out))) == n
    return out


def first_child_late():
    """for three coarse voxels at every level L, one child sits at an early row and the siblings 1000 rows later"""
    inserts, marked = {}, []
    early, late = 5, 1000
    for L in range(1, 5):
        s, h = 1 << L, 1 << (L - 1)
        for i in range(3):
            cell = np.array([0, 64 + 32 * i, 64 * L, -64 - 32 * i], np.int64)        # far from the background and from each other
            assert (cell[1:] % 16 == 0).all()
            inserts[early] = cell + np.array([0, h, 0, h])                             # children in three different sub-cells
            inserts[late] = cell + np.array([0, 0, h, 0])
            inserts[late + 1] = cell + np.array([0, s - 1, s - 1, s - 1])
            marked.append((L, tuple(cell.tolist()), early, late))
            early, late = early + 7, late + 13
    return Case("first_child_late", _placed(_thinned_block(-8, 9, 1500, 7), inserts), marked=marked)


def wave_run():
    """rows 60..67 are the eight children of one level-1 voxel and rows 68..70 children of a sibling in the same level-2
    voxel: a run of equal coarse keys crosses lanes 63|64 at every level; the same at rows 250..260 across the 256-thread
    block; row 128 starts a voxel whose siblings follow (a run beginning at lane 0) and row 192 is alone in its level-4 voxel"""
    inserts = {}
    for first, cell in ((60, (0, 96, -48, 32)), (250, (0, -96, 64, -80))):
        kids = [(cell[0], cell[1] + (j & 1), cell[2] + (j >> 1 & 1), cell[3] + (j >> 2)) for j in range(8)]
        kids += [(cell[0], cell[1] + 2, cell[2] + 3, cell[3] + j) for j in range(3)]
        for r, t in enumerate(kids):
            inserts[first + r] = t
    for r in range(4):
        inserts[128 + r] = (0, 160 + (r & 1), 160, 160 + (r >> 1))
    inserts[192] = (0, -160, -160, 163)
    return Case("wave_run", _placed(_thinned_block(-6, 7, 400 - len(inserts), 8), inserts), runs=((60, 70, 63), (250, 260, 255)),
                lane0_starts=(128, 192))


def dense_full():
    """a full 9x9x9 block, rows shuffled"""
    return Case("dense_full", _thinned_block(-4, 5, 729, 9))


def isolated():
    """216 voxels 48 apart: only the centre offset hits, every coarse level keeps N rows"""
    g = _with_batch(_grid(0, 6) * 48 + np.array([-131, -7, 5]))
    return Case("isolated", g[np.random.default_rng(11).permutation(len(g))])


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)


def sized(n):
    """the first n rows of one thinned, shuffled block (n <= 3000)"""
    return Case("sizes_%d" % n, _thinned_block(-9, 10, 3000, 12)[:n])


SORT_EXTENTS = (63, 64, 65, 127, 128)


def sort_extent(e):
    """600 rows in two batches whose largest extent (max - min) is exactly e on the y axis, smaller on x and z"""
    rng = np.random.default_rng(e)
    lo = np.array([-20, -e // 2, 3])
    span = np.array([min(e, 40) - 1, e, min(e, 50) - 1])
    xyz = np.unique(rng.integers(0, span + 1, (700, 3)), axis=0)
    xyz = xyz[rng.permutation(len(xyz))[:598]]
    xyz = np.concatenate([xyz, [[0, 0, 0]], [span]])
    xyz = np.unique(xyz, axis=0)
    xyz = xyz[rng.permutation(len(xyz))] + lo
    c = _with_batch(xyz)
    c[::3, 0] = 1
    return Case("sort_extent_%d" % e, c, extent=e)


def sort_one_cube():
    """extent 200 (shift 2): row 0 in the cube of the smallest key, the last row in the cube of the largest, every other row
    inside ONE 4x4x4 cube in shuffled order: the stable sort leaves the identity permutation"""
    cube = _grid(0, 4)[np.random.default_rng(13).permutation(64)[:50]] + np.array([100, 52, 24])
    xyz = np.concatenate([[[0, 0, 0]], cube, [[200, 200, 200]]]) + np.array([-7, -100, 9])
    return Case("sort_one_cube", _with_batch(xyz), extent=200)


CASES = {f.__name__: f for f in (tail_chain_1024, tail_chain_8192, negative_floor, window_edge, batches, first_child_late,
                                 wave_run, dense_full, isolated, sort_one_cube)}
CASES.update({"tail_chain_coarse_%d" % L: functools.partial(tail_chain_coarse, L) for L in (1, 2, 3, 4)})
CASES.update({"sizes_%d" % n: functools.partial(sized, n) for n in SIZES})
CASES.update({"sort_extent_%d" % e: functools.partial(sort_extent, e) for e in SORT_EXTENTS})
CASE_NAMES = sorted(CASES)
SORT_CASE_NAMES = ["sort_extent_%d" % e for e in SORT_EXTENTS] + ["sort_one_cube", "batches"] + ["sizes_%d" % n for n in SIZES]


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and its reference, computed once per process and shared (callers must not write into the arrays)"""
    c = CASES[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name):
    return reference(case(name).coords)


@functools.lru_cache(maxsize=None)
def case_sorted_reference(name):
    """(perm, inv, reference of the rows in the order of the spatial sort, without the 5x5x5 map)"""
    perm, inv = sort_perm(case(name).coords)
    return perm, inv, reference(case(name).coords[perm], stem=False)
