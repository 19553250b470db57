"""MinkowskiEngine-compatible facade over the gfx950 sparse-voxel engine (libcvhip.so).

Only the subset the reference touches: ``SparseTensor`` (``.F``, ``.C``,
``decomposed_coordinates_and_features``), ``MinkowskiConvolution``,
``MinkowskiConvolutionTranspose``, ``MinkowskiBatchNorm`` (sub-module ``.bn``),
``MinkowskiReLU``, ``cat``, ``modules.resnet_block.BasicBlock``,
``utils.batched_coordinates / sparse_quantize / kaiming_normal_``.
Call sites: utils/minkunet.py:53-180, utils/resnet.py:109-154, train_joint.py:82,250,
eval_joint.py:64,169, utils/dataloader.py:197.

Parameter names and shapes follow MinkowskiEngine 0.5.x so reference checkpoints keep their
keys: conv weight ``kernel`` [K^3, Cin, Cout] ([Cin, Cout] when K = 1), ``bias`` [1, Cout],
``MinkowskiBatchNorm.bn`` = ``nn.BatchNorm1d``.

Row-order invariant relied on by the reference (train_joint.py:256-272): row i of a
stride-1 output corresponds to row i of the input coordinates.
"""
import ctypes
import math
import os
import threading
import weakref

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._lib import ptr as _ptr, stream as _stream, vp
from . import utils  # noqa: F401

__version__ = "0.5.3-cvhip"


class _NoSwitch:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(dev):
    """`with torch.cuda.device(dev)` that costs nothing when dev is the current device already (one process per GPU: always)"""
    if dev.index is None or torch.cuda.current_device() == dev.index:
        return _NO_SWITCH
    return torch.cuda.device(dev)


class _FusedPlan:
    """what CoordinateManager.fused_fast() returns"""
    __slots__ = ("keep", "counts", "cap", "stem_k", "groups", "off", "layout", "map_ptrs", "perm_ptrs", "views")


class CoordinateManager:
    """Coordinate sets per tensor stride, their hash tables and the cached kernel maps."""

    NUM_LEVELS = 5

    def __init__(self, coords, num_levels=NUM_LEVELS, check=True, lazy=False):
        """check=False with num_levels=1 builds the level-0 hash without any host sync (the
        duplicate count stays on the device).  lazy=True (what SparseTensor passes): nothing is built until a map,
        a coarser level or the coordinates of this (caller-order) set are asked for - the fused network never does,
        it runs on the spatially sorted twin from fused_plan()."""
        assert coords.is_cuda and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
        self.device = coords.device
        if coords.shape[0] == 0:
            raise RuntimeError("SparseTensor: empty coordinate set")
        self.cap = int(_lib.lib().cv_sp_table_capacity(coords.shape[0]))
        self._input = coords.contiguous()
        self._fused = None
        self._lazy = (num_levels, check) if lazy else None
        if not lazy:
            self._build(num_levels, check)

    def __getattr__(self, name):
        # attributes created by _build(): a lazy manager builds on first use
        if name in ("coords", "counts", "_level", "_keys", "_vals", "_coords_buf", "_counts_d", "_verified", "_maps",
                    "num_levels") and self.__dict__.get("_lazy") is not None:
            lazy, self._lazy = self._lazy, None
            self._build(*lazy)
            return self.__dict__[name]
        raise AttributeError(name)

    @classmethod
    def _from_levels(cls, coords_buf, keys, vals, counts_d, counts, cap):
        """manager over levels built elsewhere (cv_sp_scene_plan)"""
        self = object.__new__(cls)
        self.device = coords_buf[0].device
        self.cap = cap
        self._input = coords_buf[0]
        self._fused = None
        self._lazy = None
        self.num_levels = len(coords_buf)
        self._coords_buf, self._keys, self._vals, self._counts_d = coords_buf, keys, vals, counts_d
        self._verified = True
        self.counts = counts
        self.coords = {1 << i: coords_buf[i][:counts[i]] for i in range(self.num_levels)}
        self._level = {1 << i: i for i in range(self.num_levels)}
        self._maps = {}
        return self

    def _build(self, num_levels, check):
        L = _lib.lib()
        dev = self.device
        n = self._input.shape[0]
        self.num_levels = num_levels
        self._coords_buf = [self._input] + [torch.empty((n, 4), dtype=torch.int32, device=dev)
                                            for _ in range(num_levels - 1)]
        self._keys = [torch.empty(self.cap, dtype=torch.int64, device=dev) for _ in range(num_levels)]
        self._vals = [torch.empty(self.cap, dtype=torch.int32, device=dev) for _ in range(num_levels)]
        self._counts_d = torch.empty(8, dtype=torch.int32, device=dev)
        counts_h = (ctypes.c_int32 * 8)()
        ws = torch.empty(int(L.cv_sp_levels_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        sync = check or num_levels > 1
        with _on(dev):
            _lib.check(L.cv_sp_build_levels(arr(self._coords_buf), arr(self._keys), arr(self._vals), n,
                                            self.cap, num_levels, _ptr(self._counts_d),
                                            counts_h if sync else None, _ptr(ws), ws.numel(), _stream(dev)),
                       "cv_sp_build_levels")
        self._verified = sync
        if sync:
            self._raise_on_dups(counts_h[5], counts_h[6])
            self.counts = [int(counts_h[i]) for i in range(num_levels)]
        else:
            self.counts = [n]
        self.coords = {1 << i: self._coords_buf[i][:self.counts[i]] for i in range(num_levels)}
        self._level = {1 << i: i for i in range(num_levels)}
        self._maps = {}

    @staticmethod
    def _raise_on_dups(count, out_of_range=0):
        if out_of_range != 0:
            raise RuntimeError("SparseTensor: %d coordinates outside the supported window (spatial coordinates in "
                               "[-32704, 32703], batch index < 65536)" % out_of_range)
        if count != 0:
            raise RuntimeError("SparseTensor: %d duplicate coordinates (quantise with "
                               "utils.sparse_quantize first, as utils/dataloader.py:197 does)" % count)

    def _verify(self):
        """deferred duplicate check of a set built without a host sync (first map request pays it)"""
        if not self._verified:
            c = self._counts_d[5:7].tolist()
            self._raise_on_dups(int(c[0]), int(c[1]))
            self._verified = True

    def ensure_levels(self, num_levels=NUM_LEVELS):
        if self.num_levels < num_levels:
            self._build(num_levels, True)

    def mask_perms(self, k, ts, groups=2):
        """int32 [groups, n]: for each contiguous group of the k^3 offsets, the row order sorted by the
        bit mask of valid neighbours within that group (stride-1 map at tensor stride ts, cached)."""
        key = ("mp", k, ts, groups)
        m = self._maps.get(key)
        if m is None:
            L = _lib.lib()
            nbr = self.kernel_map(k, ts)
            n, K = nbr.shape
            if (K + groups - 1) // groups <= 10:
                m = _perms_with_map(nbr, groups)
            else:       # wide groups: generic key + device sort
                m = torch.empty((groups, n), dtype=torch.int32, device=self.device)
                keys = torch.empty(n, dtype=torch.int64, device=self.device)
                for g in range(groups):
                    jb, je = K * g // groups, K * (g + 1) // groups      # same split as the kernel
                    with torch.cuda.device(self.device):
                        _lib.check(L.cv_sp_mask_keys(_ptr(nbr), n, K, jb, je, _ptr(keys), _stream(self.device)),
                                   "cv_sp_mask_keys")
                    m[g] = torch.argsort(keys).to(torch.int32)
            self._maps[key] = m
        return m

    def up_perm(self, ts_coarse):
        """row order of the fine set sorted by octant (the 8-bit mask of the transposed-conv map): tiles of
        128 rows then share one kernel offset and the other seven are skipped."""
        key = ("upperm", ts_coarse)
        m = self._maps.get(key)
        if m is None:
            L = _lib.lib()
            up = self.up_map(ts_coarse)
            m = torch.empty((1, up.shape[0]), dtype=torch.int32, device=self.device)
            ws = torch.empty(4096, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(L.cv_sp_mask_perms(_ptr(up), up.shape[0], 8, 1, _ptr(m), _ptr(ws), ws.numel(), 0,
                                              _stream(self.device)), "cv_sp_mask_perms")
            m = m[0]
            self._maps[key] = m
        return m

    # mask-sorted offset groups of the 3x3x3 convs: levels with at least MASKED_MIN_ROWS rows get MASK_GROUPS orders.
    # Three groups since the hl-format kernels (round 2): 3 / 4 / 5 groups = net 2.44 / 2.47 / 2.53 ms, 507 / 486 / 476
    # scenes/s six in flight - a quarter less partial-sum traffic is worth more than the 4 % more MFMA blocks (four groups
    # were better with the round-1 kernels: 2.99 vs 3.20 ms)
    MASK_GROUPS = int(os.environ.get("CV_NET_MASK_GROUPS", "3"))
    MASKED_MIN_ROWS = int(os.environ.get("CV_MASKED_MIN_ROWS", "16384"))      # process-wide; a thread's own: masked_min_rows()
    LIB_MASKED_MIN_ROWS = MASKED_MIN_ROWS          # the one-scene-at-a-time default (pipeline.policy_for_scenes_in_flight)

    @classmethod
    def plan_mask_groups(cls):
        """mask groups the scene plan builds orders for (0: groups too wide for its counting sort - built lazily, mask_perms)"""
        return cls.MASK_GROUPS if (27 + cls.MASK_GROUPS - 1) // cls.MASK_GROUPS <= 10 else 0

    def fused_fast(self, stem_k=5):
        """The coordinate plan of the fused network as raw device pointers (what MinkUNet.program_forward hands to the
        C executor): .counts rows per level, .map_ptrs [stem, down 0-3, k3 0-4, up 0-3, out], .perm_ptrs [mask orders of
        levels 0-4 (None where a level is not mask-sorted), octant orders of the four transposed convs].
        ONE C call (cv_sp_scene_plan: spatial row sort, the five levels of the sorted set, every map and order) into
        three allocations; the tensor views of the plan (fused_plan) are only made when somebody asks for them."""
        cache = self.__dict__.setdefault("_fused_cache", {})
        mmr = masked_min_rows()                # (part of the key: a plan built under another launch policy has other orders)
        if (stem_k, mmr) in cache:
            return cache[(stem_k, mmr)]
        L = _lib.lib()
        dev = self.device
        n = self._input.shape[0]
        NL = CoordinateManager.NUM_LEVELS
        G = self.plan_mask_groups()
        # int32 buffer perm | inv | coords of 5 levels | table values of 5 levels | counts | arena (cv_sp_scene_plan_layout)
        lay = _lib.ScenePlanLayout()
        _lib.check(L.cv_sp_scene_plan_layout(n, stem_k, G, mmr, ctypes.byref(lay)), "cv_sp_scene_plan_layout")
        ibuf = torch.empty(lay.int_words, dtype=torch.int32, device=dev)
        kbuf = torch.empty(lay.key_words, dtype=torch.int64, device=dev)
        sws_b, lws_b = lay.sort_ws_bytes, lay.levels_ws_bytes
        o_lws = (sws_b + 63) & ~63
        wbuf = _lib.scratch(dev, "scene_plan", o_lws + lws_b)      # sort + level workspaces: dead when the call returns
        ib, kb, wb = ibuf.data_ptr(), kbuf.data_ptr(), wbuf.data_ptr()
        c_coords = (vp * NL)(*[ib + 4 * o for o in lay.coords])
        c_keys = (vp * NL)(*[kb + 8 * lay.cap * i for i in range(NL)])
        c_vals = (vp * NL)(*[ib + 4 * o for o in lay.vals])
        counts_h = (ctypes.c_int32 * 8)()
        off = _lib.SceneMaps()
        with _on(dev):
            _lib.check(L.cv_sp_scene_plan(_ptr(self._input), n, vp(ib + 4 * lay.perm), vp(ib + 4 * lay.inv), c_coords, c_keys,
                                          c_vals, lay.cap, vp(ib + 4 * lay.counts), counts_h, stem_k, G, mmr,
                                          vp(ib + 4 * lay.arena), lay.int_words - lay.arena, ctypes.byref(off), vp(wb), sws_b,
                                          vp(wb + o_lws), lws_b, _stream(dev)), "cv_sp_scene_plan")
        self._raise_on_dups(counts_h[5], counts_h[6])
        plan = _FusedPlan()
        plan.keep = (ibuf, kbuf)
        plan.counts = [int(counts_h[i]) for i in range(NL)]
        plan.cap, plan.stem_k, plan.groups, plan.off, plan.layout = lay.cap, stem_k, G, off, lay
        maps, perms = (vp * _lib.NET_MAP_SLOTS)(), (vp * _lib.NET_PERM_SLOTS)()
        # (every mask order the plan has: the per-model row threshold is applied by MinkUNet.program_forward)
        _lib.check(L.cv_sp_scene_plan_slots(ctypes.byref(lay), ctypes.byref(off), (ctypes.c_int64 * NL)(*plan.counts), 0, vp(ib),
                                            maps, perms), "cv_sp_scene_plan_slots")
        plan.map_ptrs, plan.perm_ptrs = list(maps), list(perms)
        plan.views = None
        cache[(stem_k, mmr)] = plan
        self._fused = plan
        return plan

    def fused_plan(self, stem_k=5):
        """Spatially sorted twin of this coordinate set for the fused network:
        (sorted manager with all levels, stem map sorted<-original rows, final map original<-sorted) as tensors -
        views of the buffers fused_fast() filled, every kernel map / processing order pre-seeded into the sorted
        manager's cache."""
        plan = self.fused_fast(stem_k)
        if plan.views is None:
            ibuf, kbuf = plan.keep
            n, cap, G, off = self._input.shape[0], plan.cap, plan.groups, plan.off
            lay, o_inv, o_counts, o_arena = plan.layout, plan.layout.inv, plan.layout.counts, plan.layout.arena
            c = plan.counts
            NL = len(c)
            coords_buf = [ibuf[o:o + 4 * n].view(n, 4) for o in lay.coords]
            keys = [kbuf[i * cap:(i + 1) * cap] for i in range(NL)]
            vals = [ibuf[o:o + cap] for o in lay.vals]
            cm_s = CoordinateManager._from_levels(coords_buf, keys, vals, ibuf[o_counts:o_counts + 8], c, cap)
            arena = ibuf[o_arena:]
            view = lambda o, r, k: arena[o:o + r * k].view(r, k)
            stem_map = view(off.stem, c[0], stem_k ** 3)
            out_map = ibuf[o_inv:o_inv + n].view(n, 1)   # original row <- sorted row: the final 1x1 conv's "kernel map"
            for i in range(4):
                cm_s._maps[("k", 2, 1 << i, 2)] = view(off.down[i], c[i + 1], 8)
                cm_s._maps[("up", 16 >> i)] = view(off.up[i], c[3 - i], 8)
                cm_s._maps[("upperm", 16 >> i)] = arena[off.up_perm[i]:off.up_perm[i] + c[3 - i]]
            for i in range(5):
                cm_s._maps[("k", 3, 1 << i, 1)] = view(off.k3[i], c[i], 27)
                if i == 0 or off.mask_perm[i] >= 0:     # the map builder's validity words lie behind these maps (map_valid_words)
                    cm_s._maps[("k", 3, 1 << i, 1)]._cv_valid_words = arena[off.k3[i] + 27 * c[i]:off.k3[i] + 28 * c[i]]
                if off.mask_perm[i] >= 0:
                    mp = view(off.mask_perm[i], G, c[i])
                    mp._cv_has_map = True              # the map rows in processing order follow in the arena
                    mp._cv_from_plan = True
                    cm_s._maps[("mp", 3, 1 << i, G)] = mp
                    cm_s._maps[("k", 3, 1 << i, 1)]._cv_mask_perms = mp      # the generic conv path finds the orders on the map
            plan.views = (cm_s, stem_map, out_map)
        return plan.views

    def num_rows(self, ts):
        if ts == 1:
            return self._input.shape[0]
        if ts not in self._level:
            self.ensure_levels()
        return self.counts[self._level[ts]]

    def kernel_map(self, k, ts_in, stride=1):
        """int32 [n_out, k^3]: rows of the ts_in set feeding each row of the ts_in*stride set."""
        if ts_in * stride not in self._level:
            self.ensure_levels()
        self._verify()
        key = ("k", k, ts_in, stride)
        m = self._maps.get(key)
        if m is None:
            L = _lib.lib()
            li = self._level[ts_in]
            out = self.coords[ts_in * stride]
            m = torch.empty((out.shape[0], k ** 3), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(L.cv_sp_kernel_map(_ptr(out), out.shape[0], _ptr(self._keys[li]),
                                              _ptr(self._vals[li]), self.cap, k, ts_in, _ptr(m),
                                              _stream(self.device)), "cv_sp_kernel_map")
            self._maps[key] = m
        return m

    def up_map(self, ts_coarse):
        """int32 [n_fine, 8] map of the transposed k2s2 conv ts_coarse -> ts_coarse/2."""
        key = ("up", ts_coarse)
        m = self._maps.get(key)
        if m is None:
            L = _lib.lib()
            down = self.kernel_map(2, ts_coarse // 2, 2)
            n_fine = self.num_rows(ts_coarse // 2)
            m = torch.empty((n_fine, 8), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(L.cv_sp_up_map(_ptr(down), down.shape[0], n_fine, _ptr(m), _stream(self.device)),
                           "cv_sp_up_map")
            self._maps[key] = m
        return m


class SparseTensor:
    """``ME.SparseTensor(features, coordinates, device=...)`` (train_joint.py:250)."""

    def __init__(self, features, coordinates=None, device=None, coordinate_manager=None, tensor_stride=1,
                 **_):
        if device is None:
            device = features.device if coordinates is None else (
                features.device if features.is_cuda else torch.device("cuda"))
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("canonicalvoting_amd SparseTensor runs on the GPU only (no CPU engine); "
                               "pass device='cuda'")
        self.F = features.to(device=device, dtype=torch.float32)
        self.F_hl = None        # training forward: the same rows in the hl format (written by the producing BatchNorm pass)
        if coordinate_manager is None:
            if coordinates is None:
                raise ValueError("coordinates or coordinate_manager required")
            c = coordinates
            if c.is_floating_point():
                c = torch.floor(c)
            coordinate_manager = CoordinateManager(c.to(device=device, dtype=torch.int32).contiguous(),
                                                   num_levels=1, check=False, lazy=True)
        self.coordinate_manager = coordinate_manager
        self.tensor_stride = tensor_stride if isinstance(tensor_stride, int) else int(tensor_stride[0])
        if self.F.shape[0] != coordinate_manager.num_rows(self.tensor_stride):
            raise RuntimeError("features have %d rows, coordinate set has %d" % (
                self.F.shape[0], coordinate_manager.num_rows(self.tensor_stride)))

    @property
    def C(self):
        cm = self.coordinate_manager
        if self.tensor_stride not in cm.coords:
            cm.ensure_levels()
        return cm.coords[self.tensor_stride]

    @property
    def coordinates(self):
        return self.C

    @property
    def features(self):
        return self.F

    @property
    def device(self):
        return self.F.device

    @property
    def shape(self):
        return self.F.shape

    def __len__(self):
        return self.F.shape[0]

    @property
    def decomposed_coordinates_and_features(self):
        """per-batch (coords[:, 1:], feats) lists (sunrgbd/brnetcanon.py:227)"""
        C, Fm = self.C, self.F
        nb = int(C[:, 0].max().item()) + 1
        cs, fs = [], []
        for b in range(nb):
            m = C[:, 0] == b
            cs.append(C[m][:, 1:])
            fs.append(Fm[m])
        return cs, fs

    def _like(self, F, tensor_stride=None, F_hl=None):
        t = SparseTensor(F, coordinate_manager=self.coordinate_manager,
                         tensor_stride=self.tensor_stride if tensor_stride is None else tensor_stride)
        t.F_hl = F_hl
        return t


def _workspace(dev, nbytes):
    """one persistent split-K workspace per (device, stream), grown on demand; stream-ordered reuse is safe
    because every conv of a stream finishes reading it before the next one starts."""
    return _lib.scratch(dev, "conv_ws", nbytes)


_range_flags = {}
_range_lock = threading.Lock()


def range_flag(dev):
    """one int32 word of pinned (device-visible) host memory per (device, stream): fp16-pair convolutions set it when
    an input magnitude leaves the fp16 range (cv_conv_desc.range_flag); read it after synchronising the stream"""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    with _range_lock:
        f = _range_flags.get(key)
        if f is None:
            f = _range_flags[key] = torch.zeros(1, dtype=torch.int32).pin_memory()
    return f


def _piece_path(cin, cout, flavour=0):
    """the convolution runs on packed 16-bit weight pieces (conv_rows_wp / conv_hl / conv_hd), not on v_mfma_f32_32x32x2_f32"""
    return CONV_X6 and flavour in (0, 1) and cin % 32 == 0 and cout % 4 == 0


def conv_forward(x_feats, weight, nbr, n_out, scale=None, shift=None, residual=None, relu=False,
                 out=None, flavour=0, row_perm=None, j_begin=0, j_end=0, acc_in=None, perm_groups=0,
                 cache_weights=True, pieces=None, in_hl=False, out_hl=False, res_hl=False, stem_mfma=False,
                 split_tickets=None, weight_t=False, acc_scale_dev=None, step=None):
    """Low-level call into cv_sp_conv_f32 (fused epilogue).  weight [K,Cin,Cout] or [Cin,Cout].
    in_hl / out_hl / res_hl: the operand is in the hl format (to_hl / from_hl; cv_conv_desc.in_hl), pieces=2 only.
    pieces=2: fp16-pair products (the caller reads range_flag(dev) after synchronising);
    pieces=1: single bf16 products (the opt-in bf16 compute mode); None: 1 under COMPUTE_DTYPE == "bf16", else 3.
    weight_t: the TRANSPOSED convolution of `weight` ([K, Cout', Cin'] = a layer's forward kernel; the input gradient).
    step: the training step whose weight scales and pre-packed weights apply (None: the calling thread's, if any)."""
    if pieces is None:
        pieces = 1 if COMPUTE_DTYPE == "bf16" else 3
    L = _lib.lib()
    dev = x_feats.device
    # 1. the operands
    w = weight if weight.dim() == 3 else weight[None]
    if weight_t and not _piece_path(w.shape[2], w.shape[1], flavour):
        w, weight_t = w.permute(0, 2, 1), False       # (packed straight from the forward layout only where the pieces run)
    w = w.contiguous()
    K, cin, cout = (w.shape[0], w.shape[2], w.shape[1]) if weight_t else w.shape
    assert x_feats.shape[1] == cin and x_feats.stride(1) == 1
    if out is None:
        out = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    # 2. generic (module-by-module / training) path: mask-sorted offset groups, orders cached on the map
    if (AUTO_MASK_GROUPS > 1 and row_perm is None and perm_groups == 0 and flavour == 0 and nbr is not None
            and K == 27 and n_out >= AUTO_MASK_MIN_ROWS and cin % 32 == 0 and j_begin == 0 and j_end == 0
            and acc_in is None):
        row_perm = map_mask_perms(nbr, AUTO_MASK_GROUPS)
        perm_groups = row_perm.shape[0]
    # 3. the weights as the kernel reads them
    wp, _, weight_pieces, acc_scale, folded = resolve_weights(
        weight, w, pieces, flavour=flavour, transposed=weight_t, stem=stem_mfma and nbr is not None and flavour == 0,
        col_scale=scale, cache=cache_weights, step=step if step is not None else current_step())
    if folded:
        scale = None
    # 4. the descriptor
    ws = None
    if perm_groups > 1:
        ws = _workspace(dev, 4 * perm_groups * n_out * cout + 256)
    elif flavour == 0 and n_out < 128 * 384:
        ws = _workspace(dev, int(L.cv_sp_conv_workspace_bytes(n_out, cout, K)))
    # (only what is set: ctypes zero-fills the rest, the three reserved fields among them, and every keyword costs host time)
    d = _lib.ConvDesc(in_=x_feats.data_ptr(), n_in=x_feats.shape[0], in_ld=x_feats.stride(0), cin=cin, weight=w.data_ptr(),
                      K=K, cout=cout, n_out=n_out, relu=bool(relu), out=out.data_ptr(), out_ld=out.stride(0), flavour=flavour,
                      perm_groups=perm_groups, weight_pieces=weight_pieces, acc_scale=acc_scale, in_hl=bool(in_hl),
                      out_hl=bool(out_hl), res_hl=bool(res_hl))
    if nbr is not None:
        d.nbr = nbr.data_ptr()
    if scale is not None:
        d.scale = scale.data_ptr()
    if shift is not None:
        d.shift = shift.data_ptr()
    if residual is not None:
        d.residual, d.res_ld = residual.data_ptr(), residual.stride(0)
    if ws is not None:
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    if row_perm is not None:
        d.row_perm, d.perm_has_map = row_perm.data_ptr(), bool(perm_groups > 1 and getattr(row_perm, "_cv_has_map", False))
        if d.perm_has_map and nbr is not None and K <= 32 and option("zskip"):
            d.valid_words = map_valid_words(nbr).data_ptr()
    if j_begin or j_end:
        d.j_begin, d.j_end = j_begin, j_end
    if acc_in is not None:
        d.acc_in, d.acc_ld = acc_in.data_ptr(), acc_in.stride(0)
    if wp is not None:
        d.weight_x6 = wp.data_ptr()
    if weight_pieces == 2:
        d.range_flag = range_flag(dev).data_ptr()
    if split_tickets is not None:
        d.split_tickets = split_tickets.data_ptr()
    if acc_scale_dev is not None:
        d.acc_scale_dev = acc_scale_dev.data_ptr()
    with _on(dev):
        _lib.check(L.cv_sp_conv_f32(ctypes.byref(d), _stream(dev)), "cv_sp_conv_f32")
    return out


_policy_tls = threading.local()


def masked_min_rows():
    """Rows from which a level's 3x3x3 convolutions run mask-sorted: the CALLING THREAD's value while it is inside
    pipeline.scene_policy(...) (launch sizing per call: two hosts with different policies in one process do not see each
    other), else the process-wide CoordinateManager.MASKED_MIN_ROWS."""
    v = getattr(_policy_tls, "masked_min_rows", None)
    return CoordinateManager.MASKED_MIN_ROWS if v is None else v


def set_masked_min_rows_thread(rows):
    """the calling thread's masked_min_rows() (None: follow the process-wide value); returns the previous thread value"""
    before = getattr(_policy_tls, "masked_min_rows", None)
    _policy_tls.masked_min_rows = None if rows is None else int(rows)
    return before


def set_split_target(workgroups):
    """cv_sp_set_split_target: workgroups a split convolution launch aims at (0: the library default, 768 - best for one
    scene in flight; 256 pays from about four scenes in flight).  Returns the previous value."""
    return int(_lib.lib().cv_sp_set_split_target(int(workgroups)))


def set_option(name, value):
    """cv_sp_set_option: kernel selection knobs of the convolutions ("hd_mask", "hd_min_rows"); returns the previous value"""
    prev = ctypes.c_longlong(0)
    _lib.check(_lib.lib().cv_sp_set_option(name.encode(), int(value), ctypes.byref(prev)), "cv_sp_set_option")
    return int(prev.value)


def option(name):
    """current value of a cv_sp_set_option knob"""
    v = ctypes.c_longlong(0)
    _lib.check(_lib.lib().cv_sp_get_option(name.encode(), ctypes.byref(v)), "cv_sp_get_option")
    return int(v.value)


def to_hl(x):
    """fp32 rows [n, C] (C % 32 == 0) -> the hl format (same shape and dtype, the bytes hold the fp16 pairs)"""
    y = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.check(_lib.lib().cv_sp_to_hl_f32(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.data_ptr(), y.stride(0),
                                              range_flag(x.device).data_ptr(), _stream(x.device)), "cv_sp_to_hl_f32")
    return y


def from_hl(x):
    y = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.check(_lib.lib().cv_sp_from_hl_f32(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), y.data_ptr(),
                                                y.stride(0), _stream(x.device)), "cv_sp_from_hl_f32")
    return y


# conv_forward applies mask-sorted offset groups to big 3x3x3 maps on its own (0 = off)
AUTO_MASK_GROUPS = int(os.environ.get("CV_MASK_GROUPS", "4"))
AUTO_MASK_MIN_ROWS = int(os.environ.get("CV_AUTO_MASK_MIN_ROWS", "16384"))


def map_mask_perms(nbr, groups):
    """[groups, n] processing orders of a kernel map (see CoordinateManager.mask_perms), cached on the map."""
    hit = getattr(nbr, "_cv_mask_perms", None)
    if hit is not None and getattr(hit, "_cv_from_plan", False):
        return hit          # built with the scene's coordinate plan (its own group count): no second sort of the same map
    if hit is None or hit.shape[0] != groups:
        hit = nbr._cv_mask_perms = _perms_with_map(nbr, groups)
    return hit


def map_valid_words(nbr):
    """int32 [n]: bit j of word i = nbr[i, j] >= 0 (K <= 32) - cv_conv_desc.valid_words, cached on the map.  A map of the
    scene plan carries the words its builder left behind it; for any other map they are made here, once."""
    hit = getattr(nbr, "_cv_valid_words", None)
    if hit is None:
        bits = torch.ones(nbr.shape[1], dtype=torch.int64, device=nbr.device) << torch.arange(nbr.shape[1], device=nbr.device)
        hit = nbr._cv_valid_words = ((nbr >= 0) * bits).sum(1).to(torch.int32)
    return hit


def _perms_with_map(nbr, groups):
    """[groups, n] orders (a view) followed, in the same buffer, by the kernel map rows of every group in processing
    order [groups, n, W] (cv_sp_mask_perms with_map = 1); the view carries `_cv_has_map` for conv_forward."""
    L = _lib.lib()
    n, K = nbr.shape
    W = (K + groups - 1) // groups
    # orders, the map rows in processing order, then one validity byte per (group, row) (cv_sp_mask_perms with_map = 1)
    flat = torch.empty(groups * n * (1 + W) + (groups * n + 3) // 4, dtype=torch.int32, device=nbr.device)
    ws = torch.empty(groups * 4096, dtype=torch.uint8, device=nbr.device)
    with _on(nbr.device):
        _lib.check(L.cv_sp_mask_perms(_ptr(nbr), n, K, groups, _ptr(flat), _ptr(ws), ws.numel(), 1,
                                      _stream(nbr.device)), "cv_sp_mask_perms")
    m = flat[:groups * n].view(groups, n)
    m._cv_has_map = True
    m._cv_flat = flat
    return m


# 1 (default): vector-path convs run their fp32 products as six bf16 piece products on the bf16 matrix cores
# (conv_rows_wp); 0: v_mfma_f32_32x32x2_f32
CONV_X6 = os.environ.get("CV_CONV_X6", "1") != "0"


# Product precision of the vector-path convolutions (forward, input gradient, weight gradient):
#   "fp32" (default): fp32-level products (bf16 triples / fp16 pairs, see conv_rows_wp.hip) - the parity path;
#   "bf16": operands rounded to bf16, one bf16 x bf16 product, fp32 accumulation and fp32 storage - the opt-in
#           compute mode BASELINE configs 3-4 name for training (bench.py --dtype bf16); NOT within the 1e-4 bar.
COMPUTE_DTYPE = "bf16" if os.environ.get("CV_COMPUTE_DTYPE", "fp32") == "bf16" else "fp32"


def set_compute_dtype(dtype):
    """"fp32" or "bf16" (see COMPUTE_DTYPE); returns the previous setting.  Cached eval programs are keyed by it."""
    global COMPUTE_DTYPE
    assert dtype in ("fp32", "bf16"), dtype
    prev, COMPUTE_DTYPE = COMPUTE_DTYPE, dtype
    return prev


def pack_weights(w3, pieces, col_scale=None, scale_log2=0, transposed=False, stem=False):
    """uncached: w3 [K, Cin, Cout] (times an optional per-output-column scale - a folded BatchNorm - and 2^scale_log2) as the
    int16 words one of the piece kernels reads: pieces = 3 bf16 triples (conv_rows_wp; cv_sp_pack_weights_x6_f32), 2 fp16
    pairs (cv_sp_pack_weights_h2_f32), 1 one bf16 (cv_sp_pack_weights_bf16_f32).  transposed: the weights of the transposed
    convolution, packed straight from the forward layout (cv_sp_pack_weights_t_f32; no column scale).  stem: [K, 3|6, 32] as
    fp16 pairs in the B-operand order of conv_stem_mfma (cv_sp_pack_weights_stem_h2_f32)."""
    L = _lib.lib()
    dev = w3.device
    K, c1, c2 = w3.shape
    assert not (transposed and col_scale is not None) and not (stem and (pieces != 2 or c2 != 32))
    wp = torch.empty(8 * c1 * 1024 if stem else pieces * w3.numel(), dtype=torch.int16, device=dev)
    args, k, st = (_ptr(w3), K, c1, c2), int(scale_log2), _stream(dev)
    with _on(dev):
        if stem:
            _lib.check(L.cv_sp_pack_weights_stem_h2_f32(_ptr(w3), K, c1, _ptr(col_scale), k, _ptr(wp), st),
                       "cv_sp_pack_weights_stem_h2_f32")
        elif transposed:
            _lib.check(L.cv_sp_pack_weights_t_f32(*args, pieces, k, _ptr(wp), st), "cv_sp_pack_weights_t_f32")
        elif pieces == 2:
            _lib.check(L.cv_sp_pack_weights_h2_f32(*args, _ptr(col_scale), k, _ptr(wp), st), "cv_sp_pack_weights_h2_f32")
        elif pieces == 1:
            _lib.check(L.cv_sp_pack_weights_bf16_f32(*args, _ptr(col_scale), _ptr(wp), st), "cv_sp_pack_weights_bf16_f32")
        else:
            _lib.check(L.cv_sp_pack_weights_x6_f32(*args, _ptr(col_scale), _ptr(wp), st), "cv_sp_pack_weights_x6_f32")
    return wp


def h2_scale_log2(*scaled_weights):
    """power of two that brings the largest magnitude of the given (weight [K,Cin,Cout], column scale or None) sets
    to about 2^13 (cv_sp_pack_weights_h2_f32); one host sync, at pack time only"""
    amax = 0.0
    for w3, col_scale in scaled_weights:
        a = w3.abs().amax(dim=(0, 1)) if col_scale is not None else w3.abs().max()
        amax = max(amax, float((a * col_scale.abs()).max()) if col_scale is not None else float(a))
    if not math.isfinite(amax) or amax <= 0.0:
        return 0
    return max(-60, min(60, 13 - math.ceil(math.log2(amax))))


# eval-time cache of packed weights, every format: id(weight) -> (weak reference, (data_ptr, _version, shape), {format: (words,
# scale_log2)}).  A hit is the SAME live tensor object, unmodified: the weak reference drops the entry when the tensor dies,
# so neither a recycled id nor a recycled allocation of the same shape can meet the packing of a dead tensor.
_pack_cache = {}


def invalidate_weight_caches():
    """Drop every cached re-packing of a weight tensor.  The cache is keyed by tensor version, and fused optimizers
    (torch.optim.Adam(fused=True)) update parameters WITHOUT bumping it: modules call this when they switch between train and
    eval mode, and the training path never caches."""
    _pack_cache.clear()


def _cached_packings(weight):
    """the {format: (words, scale_log2)} table of this tensor object as it is now"""
    key = id(weight)
    ver = (weight.data_ptr(), weight._version, tuple(weight.shape))
    hit = _pack_cache.get(key)
    if hit is None or hit[1] != ver or hit[0]() is not weight:
        hit = _pack_cache[key] = (weakref.ref(weight, lambda _r, k=key: _pack_cache.pop(k, None)), ver, {})
    return hit[2]


def resolve_weights(weight, w3, pieces, flavour=0, transposed=False, stem=False, col_scale=None, second=None, cache=False,
                    step=None):
    """How a convolution's weights reach the kernel - the one place that decides it, for conv_forward and the eval program:
    (packed words, packed words of the second source, cv_conv_desc.weight_pieces, acc_scale, BatchNorm scale folded in).
    weight: the caller's tensor (the cache and a step's scales go by it); w3: the same as contiguous [K, Cin, Cout]
    (transposed: the forward kernel [K, Cout', Cin'] of the layer whose input gradient this is).
    pieces: 1 / 2 / 3 as in pack_weights, where the shape allows the piece kernels (_piece_path) - else (None, None, 3, 1, False):
    fp32 products on the unpacked weights.  stem: the caller allows conv_stem_mfma (fp16 pairs, [K <= 128, 3|6, 32]).
    col_scale: the BatchNorm scale of the epilogue; folded into the packed weights (the caller then drops it) for the stem and
    with a second source.  second = (w2 [1, Cin2, Cout], scale2): out += scale2 * (src2 @ w2), one accumulator - one common
    power of two for the fp16 pairs.
    fp16 pairs take their power of two (acc_scale = 2^-k) from, in this order: the step's pre-packed arena (not with cache),
    the step's per-weight exponents (nothing folded in), one readback of the maximum (h2_scale_log2).
    cache: keep / take the packing in the eval-time cache (never a folded or a transposed one)."""
    K, cin, cout = (w3.shape[0], w3.shape[2], w3.shape[1]) if transposed else w3.shape
    stem = stem and pieces == 2 and cin in (3, 6) and cout == 32 and K <= 128
    if not stem and not _piece_path(cin, cout, flavour):
        return None, None, 3, 1.0, False
    folded = stem or second is not None
    fold = col_scale if folded else None
    k = None
    if pieces == 2 and step is not None and fold is None and second is None:
        pre = step.packed.get((w3.data_ptr(), int(transposed))) if (step.packed and not cache and not stem) else None
        if pre is not None and pre[0].numel() == 2 * w3.numel():
            TRAIN_COUNTERS["prepacked"] += 1              # packed at the start of the step (_ModuleState.prepack)
            return pre[0], None, 2, 2.0 ** -pre[1], folded
        k = step.scales.get(weight.data_ptr())
    table = _cached_packings(weight) if (cache and fold is None and second is None and not transposed) else None
    hit = table.get((pieces, stem)) if table is not None else None
    wp2 = None
    if hit is None:
        sets = [(w3, fold)] + ([second] if second is not None else [])
        if pieces != 2:
            k = 0
        elif k is None:
            k = h2_scale_log2(*sets)                     # (one host wait: a training step hands the scales over instead)
        hit = (pack_weights(w3, pieces, fold, k, transposed, stem), k)
        if second is not None:
            wp2 = pack_weights(second[0], pieces, second[1], k)
        if table is not None:
            table[(pieces, stem)] = hit
    return hit[0], wp2, pieces, (2.0 ** -hit[1] if pieces == 2 else 1.0), folded


def conv_forward_masked(x_feats, weight, nbr, perms, n_out, **epilogue):
    """k^3 conv with the kernel offsets split into G groups, each group processed with the rows in the
    order sorted by that group's neighbour mask (see sparse_conv.hip); one launch + one reduce.
    perms: int32 [G, n_out] from CoordinateManager.mask_perms."""
    return conv_forward(x_feats, weight, nbr, n_out, row_perm=perms, perm_groups=perms.shape[0],
                        flavour=epilogue.pop("flavour", 0), **epilogue)


def transposed_map(nbr, n_in):
    """nbr_t [n_in, K] with nbr_t[i][j] = u iff nbr[u][j] == i (cached on the map tensor)."""
    hit = getattr(nbr, "_cv_transposed", None)
    if hit is None or hit.shape[0] != n_in:
        L = _lib.lib()
        hit = torch.empty((n_in, nbr.shape[1]), dtype=torch.int32, device=nbr.device)
        with _on(nbr.device):
            _lib.check(L.cv_sp_transpose_map(_ptr(nbr), nbr.shape[0], nbr.shape[1], n_in, _ptr(hit),
                                             _stream(nbr.device)), "cv_sp_transpose_map")
        nbr._cv_transposed = hit
    return hit


def conv_wgrad(x_feats, grad_out, nbr, K):
    """dW [K, Cin, Cout] = sum_u x[nbr[u][j]]^T dy[u]  (cv_sp_conv_wgrad_f32)."""
    L = _lib.lib()
    dev = x_feats.device
    cin, cout, n_out = x_feats.shape[1], grad_out.shape[1], grad_out.shape[0]
    dw = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    ws = _workspace(dev, int(L.cv_sp_wgrad_workspace_bytes(n_out, cin, cout, K)))
    with _on(dev):
        if COMPUTE_DTYPE == "bf16":
            _lib.check(L.cv_sp_conv_wgrad_px_f32(_ptr(x_feats), x_feats.stride(0), cin, _ptr(grad_out),
                                                 grad_out.stride(0), cout, _ptr(nbr), K, n_out, _ptr(dw), _ptr(ws),
                                                 ws.numel(), 1, _stream(dev)), "cv_sp_conv_wgrad_px_f32")
        else:
            _lib.check(L.cv_sp_conv_wgrad_f32(_ptr(x_feats), x_feats.stride(0), cin, _ptr(grad_out),
                                              grad_out.stride(0), cout, _ptr(nbr), K, n_out, _ptr(dw), _ptr(ws),
                                              ws.numel(), _stream(dev)), "cv_sp_conv_wgrad_f32")
    return dw


def col_sum(x):
    """column sums (bias gradient) in a fixed summation order: cv_sp_col_sum_det_f32"""
    L = _lib.lib()
    out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    ws = _lib.scratch(x.device, "col_sum", int(L.cv_sp_col_sum_workspace_bytes(x.shape[0], x.shape[1])))
    with _on(x.device):
        _lib.check(L.cv_sp_col_sum_det_f32(_ptr(x), x.shape[0], x.shape[1], x.stride(0), _ptr(out), _ptr(ws), ws.numel(),
                                           _stream(x.device)), "cv_sp_col_sum_det_f32")
    return out


# training: weight gradient of a layer on a side stream next to its input gradient.
#   CV_BACKWARD_OVERLAP=0: one stream; 1: the layer's stream waits for the side stream before backward() returns;
#   2 (default): that wait moves to the end of the backward pass (the side stream works through the weight gradients
#   while the layer's stream goes on with the BatchNorm backward and the next input gradient) whenever nothing can
#   touch the gradient earlier - see _ConvFn.backward.
BACKWARD_OVERLAP = int(os.environ.get("CV_BACKWARD_OVERLAP", "2"))
LATE_GRAD_LOG = None        # tests: a list that receives (kernel parameter, data_ptr of d_kernel) of every late-joined layer
_wgrad_streams = {}
_wgrad_lock = threading.Lock()
_wgrad_pending = threading.local()


def _wgrad_stream(dev):
    """the side stream of (device, current stream) for _ConvFn.backward"""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    with _wgrad_lock:
        s = _wgrad_streams.get(key)
        if s is None:
            s = _wgrad_streams[key] = torch.cuda.Stream(device=dev)
    return s


def _join_at_end_of_backward(cur, side):
    """queue ONE callback per backward pass and (stream, side stream) pair: the stream waits for the side stream when
    the autograd engine has run the last node (before it hands the gradients to the caller's stream)"""
    pend = getattr(_wgrad_pending, "pairs", None)
    if pend is None:
        pend = _wgrad_pending.pairs = {}
    # (the pass is part of the key: two backward passes interleaved on one engine thread each get their own join)
    key = (torch._C._current_graph_task_id(), cur.cuda_stream, side.cuda_stream)
    if key in pend:
        return
    pend[key] = (cur, side)

    def join():
        pend.pop(key, None)
        cur.wait_stream(side)
        torch.cuda.current_stream(cur.device).wait_stream(side)

    torch.autograd.Variable._execution_engine.queue_callback(join)


def _gradient_untouched_until_end(kernel):
    """True when nothing reads or writes the weight gradient between _ConvFn.backward and the end of the backward pass:
    no gradient to accumulate into (AccumulateGrad then keeps the tensor itself, no kernel), no hooks on the parameter,
    no process group with more than one rank (DDP's reducer copies gradients into its buckets as they arrive), no
    anomaly / graph-building mode.  Code that hooks the gradient accumulators by other means sets
    CV_BACKWARD_OVERLAP=1."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return False          # (DDP's reducer hooks sit on the gradient accumulators, invisible from here - also with ONE rank,
                              #  where the bucket copy still runs on the layer's stream as the gradient arrives)
    # (AccumulateGrad keeps a gradient tensor as it is - no kernel on the layer's stream - only when its layout is the
    # parameter's: a non-contiguous kernel parameter would make it clone d_kernel on the main stream, racing the side stream)
    return (kernel.is_leaf and kernel.grad is None and kernel.is_contiguous() and not kernel._backward_hooks
            and not getattr(kernel, "_post_accumulate_grad_hooks", None)
            and not torch.is_grad_enabled() and not torch.is_anomaly_enabled())


# 1 (default): the training forward's convolutions run on the eval path's hl-format kernels (conv_hl / conv_hd: fp16 pairs, operands
# split once by the producing BatchNorm pass instead of once per gather) wherever the input has an hl twin; the range flag guards
# it (train.train_step redoes the step on the bf16 triples).  0: conv_rows_wp on the fp32 rows.
TRAIN_FWD_HL = int(os.environ.get("CV_TRAIN_FWD_HL", "1"))
# 1 (default): the input gradients run on the hl-format kernels too.  The BatchNorm backward writes dx a second time as fp16 pairs
# times a per-layer power of two taken from the PREVIOUS step's largest |dx| of that layer (three words per layer that live on
# the device: cv_sp_bn_backward_hl_f32) - inside train.train_step only (pair_scale_hints rotates the maxima between steps);
# a layer's first step, and every backward outside a step, takes the bf16 triples.
TRAIN_BWD_HL = int(os.environ.get("CV_TRAIN_BWD_HL", "1"))
# 1 (default): train.train_step packs the fp16-pair weights of all convolutions (both directions) by one launch per step
TRAIN_PREPACK = int(os.environ.get("CV_TRAIN_PREPACK", "1"))
TRAIN_COUNTERS = {"hl_dgrad": 0, "prepacked": 0}           # (tests: how many input gradients took the hl path)
# of the calling thread: .step, the training step in progress (pair_scale_hints); .triples, inside on_bf16_triples()
_train_state = threading.local()


def current_step():
    """the training step the calling thread is in (a pair_scale_hints), or None"""
    return getattr(_train_state, "step", None)


class on_bf16_triples:
    """`with on_bf16_triples():` the calling thread's training forwards stay off the fp16 pairs (train.train_step redoes a step
    that left the fp16 range this way)"""

    def __enter__(self):
        self.outer = getattr(_train_state, "triples", False)
        _train_state.triples = True
        return self

    def __exit__(self, *exc):
        _train_state.triples = self.outer
        return False


def train_forward_hl():
    return TRAIN_FWD_HL != 0 and COMPUTE_DTYPE != "bf16" and not getattr(_train_state, "triples", False)


def train_uses_pairs():
    """the training forward multiplies fp16 pairs somewhere (range flag to check, weight scales to hand over)"""
    return train_forward_hl()


class _GradSlots:
    """per-layer words of the hl-format gradient twins (keyed by the BatchNorm gain's storage), one device buffer per module tree"""

    def __init__(self, dev):
        self.buf = torch.zeros((128, 8200), dtype=torch.int32, device=dev)  # [layer][4096 x this step's maxima | 4096 x last step's | 1 / s] (CV_BN_SLOT_WORDS)
        self.index = {}
        self.seen = set()                    # layers whose slot[1] holds a maximum (they ran a backward in the step before)
        self.running = set()

    def rotate(self):
        with torch.no_grad():
            self.buf[:, 4096:8192].copy_(self.buf[:, 0:4096])
            self.buf[:, 0:4096].zero_()
        self.seen, self.running = self.running, set()

    def take(self, key):
        """(slot tensor, usable) for the layer; usable = last step left a maximum"""
        i = self.index.get(key)
        if i is None:
            if len(self.index) >= self.buf.shape[0]:
                return None, False
            i = self.index[key] = len(self.index)
        self.running.add(key)
        return self.buf[i], key in self.seen


class _ModuleState:
    """What a module tree keeps from one training step to the next, for the convolution kernels `ks` it had when this was
    built (pair_scale_hints builds another when `sig` no longer matches): the weight maxima on their way to the host, the
    arena of the pre-packed weights, the gradient slots."""

    def __init__(self, sig, ks, dev):
        self.sig, self.dev = sig, dev
        self.host = torch.empty(len(ks), dtype=torch.float32).pin_memory()
        self.request(ks)
        self.slots = None
        self.meta = None

    @staticmethod
    def signature(ks):
        return tuple((k.data_ptr(), tuple(k.shape), k.is_contiguous()) for k in ks) + (str(ks[0].device), bool(TRAIN_BWD_HL))

    def request(self, ks):
        """the max-norms of the weights as they are now (ONE multi-tensor launch) travel to pinned memory"""
        with torch.no_grad():
            self.host.copy_(torch.stack(torch._foreach_norm([k.detach() for k in ks], float("inf"))), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self.dev))

    def scales(self, ks):
        """{kernel.data_ptr(): scale_log2} from the maxima requested a step ago; requests the next step's"""
        self.event.synchronize()                 # (already passed in the steady state: it was recorded a step ago)
        amax = self.host.tolist()
        self.request(ks)
        return {k.data_ptr(): (max(-60, min(60, 13 - math.ceil(math.log2(a)))) if (math.isfinite(a) and a > 0) else 0)
                for k, a in zip(ks, amax)}

    def grad_slots(self):
        if self.slots is None:
            self.slots = _GradSlots(self.dev)
        self.slots.rotate()
        return self.slots

    def prepack(self, ks, scales):
        """fp16-pair weights of every convolution of a training step - forward layout and, for the input gradients, transposed
        - packed by ONE launch in front of the step's forward (cv_sp_pack_weights_h2_batch_f32) into an arena that lives with
        the module: {(kernel.data_ptr(), transposed): (packed words, scale_log2)} for resolve_weights.  Per layer and direction
        this was a launch of its own (117 per MinkUNet34C step) with the stream idle in front of most of them."""
        if self.meta is None:
            meta, off = [], 0
            for k in ks:
                if not k.is_contiguous():
                    continue
                K, cin, cout = (k.shape if k.dim() == 3 else (1,) + tuple(k.shape))
                words = 2 * K * cin * cout
                if cin % 32 == 0 and cout % 4 == 0:
                    meta.append((k.data_ptr(), 0, K, cin, cout, off, words))
                    off += (words + 63) // 64 * 64
                if TRAIN_BWD_HL and cout % 32 == 0 and cin % 4 == 0:      # the transposed convolution: Cin' = cout, Cout' = cin
                    meta.append((k.data_ptr(), 1, K, cout, cin, off, words))
                    off += (words + 63) // 64 * 64
            self.arena = torch.empty(max(off, 64), dtype=torch.int16, device=self.dev)
            self.jobs = (_lib.PackJob * max(len(meta), 1))()
            for j, (ptr, trans, K, cin, cout, o, words) in zip(self.jobs, meta):
                j.w, j.wp, j.K, j.cin, j.cout, j.trans = ptr, self.arena.data_ptr() + 2 * o, K, cin, cout, trans
            self.d_jobs = torch.empty(max(len(meta), 1) * ctypes.sizeof(_lib.PackJob), dtype=torch.uint8, device=self.dev)
            self.meta = meta
        packed = {}
        for j, (ptr, trans, K, cin, cout, o, words) in zip(self.jobs, self.meta):
            j.scale_log2 = int(scales.get(ptr, 0))
            packed[(ptr, trans)] = (self.arena[o:o + words], j.scale_log2)
        if self.meta:
            with _on(self.dev):
                _lib.check(_lib.lib().cv_sp_pack_weights_h2_batch_f32(self.jobs, len(self.meta), _ptr(self.d_jobs),
                                                                      _stream(self.dev)), "cv_sp_pack_weights_h2_batch_f32")
        return packed


class pair_scale_hints:
    """`with pair_scale_hints(module):` ONE TRAINING STEP of `module` on the calling thread (the weights do not move between its
    forward and its optimizer step).  The object is what the step's autograd nodes share; _ConvFn and _BNTrainFn find it
    through the calling thread in their forward and keep it on their ctx, for the backward on the autograd engine's thread:
        scales      {kernel.data_ptr(): power of two of the fp16-pair products}.  Without it every fp16-pair convolution reads
                    its own maximum back (63 host waits per MinkUNet34C forward).  No host wait in the steady state: the
                    max-norms travel to pinned memory behind the step that computed them and the NEXT step reads them - an
                    optimizer step moves a weight maximum by a fraction of a percent and the scale leaves a factor of 8 to
                    the fp16 range.  The first step of a module (or a changed parameter list) waits once.
        packed      the pre-packed weights of the step (TRAIN_PREPACK; _ModuleState.prepack), or None
        slots       the gradient slots (TRAIN_BWD_HL; _GradSlots), or None
        twins       {dx.data_ptr(): (hl twin, 1 / factor on the device, shape, dx)} from a BatchNorm backward to the input
                    gradient of the convolution below it
        used_pairs  a forward of the step multiplied fp16 pairs: there is a range flag to read
    A node built outside a step has none: bf16 triples for its input gradient, its own scale readback for a pair forward.
    When the block is left the step is closed: a backward that runs later finds it empty."""

    def __init__(self, module):
        self.module = module
        self.scales, self.packed, self.slots, self.twins, self.used_pairs = {}, None, None, {}, False

    def __enter__(self):
        self.outer = current_step()
        ks = [m.kernel for m in self.module.modules() if isinstance(m, MinkowskiConvolutionBase) and m.kernel.is_cuda]
        if ks and train_forward_hl():
            sig = _ModuleState.signature(ks)
            st = self.module.__dict__.get("_cv_train_state")
            if st is None or st.sig != sig:
                st = self.module.__dict__["_cv_train_state"] = _ModuleState(sig, ks, ks[0].device)
            self.scales = st.scales(ks)
            if TRAIN_PREPACK:
                self.packed = st.prepack(ks, self.scales)
            if TRAIN_BWD_HL:
                self.slots = st.grad_slots()
        _train_state.step = self
        return self

    def __exit__(self, *exc):
        _train_state.step = self.outer
        self.scales, self.packed, self.slots, self.twins = {}, None, None, {}
        return False

    def range_flag_device(self, dev):
        """the range flag of this thread's stream as a float32 device scalar (1.0 = a training forward since the last reset left
        the fp16 range), read in stream order behind the kernels that may raise it: hand it to a fused optimizer as `found_inf`
        and the update is skipped on the device without a host wait (train.train_step).  None when no forward of the step used
        the fp16 pairs."""
        if not self.used_pairs:
            return None
        return range_flag(dev).to(dev, non_blocking=True).to(torch.float32).reshape(())

    def left_fp16_range(self, dev, group=None):
        """True when a convolution of this step's forward staged an input beyond the fp16 range on the current stream
        (synchronises the stream; the flag is reset).  False without a wait when no forward used the fp16 pairs.  group: a
        process group whose ranks step together (DDP) - the answer is then the MAXIMUM over the ranks (what GradScaler does
        with found_inf): every rank redoes the step, or none does."""
        if not self.used_pairs and group is None:
            return False
        self.used_pairs = False
        torch.cuda.current_stream(dev).synchronize()
        flag = range_flag(dev)
        raised = int(flag[0]) != 0
        if group is not None:
            import torch.distributed as dist
            t = torch.tensor([1.0 if raised else 0.0], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            raised = float(t[0]) != 0.0
        if not raised:
            return False
        flag.zero_()
        return True


def copy_unless_flag(srcs, dsts, dev, flag=None):
    """dsts[i].copy_(srcs[i]) for lists of same-shaped device tensors in ceil(n / 96) launches, skipped ON THE DEVICE while
    `flag` (a device-visible int32 tensor, e.g. range_flag(dev); None: always copy) is non-zero: cv_sp_copy_unless_flag."""
    n = len(srcs)
    if n == 0:
        return
    a_src = (vp * n)(*[t.data_ptr() for t in srcs])
    a_dst = (vp * n)(*[t.data_ptr() for t in dsts])
    a_len = (ctypes.c_longlong * n)(*[t.numel() * t.element_size() for t in srcs])
    with _on(dev):
        _lib.check(_lib.lib().cv_sp_copy_unless_flag(a_src, a_dst, a_len, n, vp(flag.data_ptr()) if flag is not None else None,
                                                     _stream(dev)), "cv_sp_copy_unless_flag")


class _ConvFn(torch.autograd.Function):
    """Sparse convolution with HIP forward, input-gradient (the same kernel on the transposed map with
    transposed weights) and weight-gradient kernels."""

    @staticmethod
    def forward(ctx, feats, kernel, bias, nbr, n_out, feats_hl=None):
        feats = feats.contiguous()
        ctx.save_for_backward(feats, kernel, nbr if nbr is not None else torch.empty(0))
        ctx.has_nbr = nbr is not None
        ctx.has_bias = bias is not None
        shift = bias.reshape(-1).contiguous() if bias is not None else None
        step = ctx.step = current_step()
        # fp32-level products of the training FORWARD: fp16 pairs (three piece products) while the activations are inside
        # the fp16 range - they sit behind BatchNorm - with the range flag as the guard (train.train_step reads it once per
        # step and redoes the step on the bf16 triples)
        if feats_hl is not None and train_forward_hl() and feats.shape[1] % 32 == 0 and feats_hl.stride(0) % 32 == 0:
            # the eval path's kernels on the hl twin (the fp32 rows stay saved for the weight gradient)
            if step is not None:
                step.used_pairs = True
            return conv_forward(feats_hl, kernel, nbr, n_out, shift=shift, cache_weights=False, pieces=2, in_hl=True, step=step)
        k3 = kernel if kernel.dim() == 3 else kernel[None]
        if (train_forward_hl() and nbr is not None and feats.shape[1] in (3, 6) and k3.shape[2] == 32 and k3.shape[0] <= 128):
            # the stem (conv0p1s1: 5x5x5, 3 or 6 -> 32 channels) on the matrix cores, like the eval program's (conv_stem_mfma)
            if step is not None:
                step.used_pairs = True
            return conv_forward(feats, kernel, nbr, n_out, shift=shift, cache_weights=False, pieces=2, stem_mfma=True, step=step)
        return conv_forward(feats, kernel, nbr, n_out, shift=shift, cache_weights=False, step=step)

    @staticmethod
    def backward(ctx, grad):
        feats, kernel, nbr = ctx.saved_tensors
        nbr = nbr if ctx.has_nbr else None
        grad = grad.contiguous()
        k3 = kernel if kernel.dim() == 3 else kernel[None]
        d_feats = d_kernel = d_bias = None
        # The two gradients of a layer read the same dy and write different tensors: the weight gradient goes to a
        # side stream next to the input gradient (each alone leaves most SIMDs with one or two waves and a tail of
        # long tasks).  Either the layer's own stream waits for the side stream before backward returns (everything
        # that consumes d_kernel, frees x / dy or reuses their memory is then ordered behind both), or - when nothing
        # can touch the gradient before the end of the pass - that wait is queued for the end of the backward pass and
        # x / dy are marked as in use by the side stream.  The same kernels on the same inputs: results bit for bit.
        side = _wgrad_stream(grad.device) if (BACKWARD_OVERLAP and ctx.needs_input_grad[0] and
                                              ctx.needs_input_grad[1]) else None
        late = False
        if side is not None:
            cur = torch.cuda.current_stream(grad.device)
            late = BACKWARD_OVERLAP >= 2 and _gradient_untouched_until_end(kernel)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                d_kernel = conv_wgrad(feats, grad, nbr, k3.shape[0]).reshape(kernel.shape)
            if late:
                # the side stream still reads x and dy after this node has released them: their blocks go back to the
                # allocator only when the side stream has passed this point
                feats.record_stream(side)
                grad.record_stream(side)
                if nbr is not None:
                    nbr.record_stream(side)
                _join_at_end_of_backward(cur, side)
                if LATE_GRAD_LOG is not None:
                    LATE_GRAD_LOG.append((kernel, d_kernel.data_ptr()))
        step = ctx.step
        twin = step.twins.pop(grad.data_ptr(), None) if step is not None else None     # (taken out whether or not it is used)
        if ctx.needs_input_grad[0]:
            nbr_t = transposed_map(nbr, feats.shape[0]) if nbr is not None else None
            if (twin is not None and twin[2] == grad.shape and COMPUTE_DTYPE != "bf16" and k3.shape[2] % 32 == 0
                    and k3.shape[1] % 4 == 0):
                # the eval path's kernels on the gradient's hl twin (written by the BatchNorm backward above this layer)
                d_feats = conv_forward(twin[0], k3.detach(), nbr_t, feats.shape[0], cache_weights=False, weight_t=True,
                                       pieces=2, in_hl=True, acc_scale_dev=twin[1], step=step)
                TRAIN_COUNTERS["hl_dgrad"] += 1
            else:
                d_feats = conv_forward(grad, k3.detach(), nbr_t, feats.shape[0], cache_weights=False, weight_t=True, step=step)
        if side is not None:
            if not late:
                cur.wait_stream(side)
        elif ctx.needs_input_grad[1]:
            d_kernel = conv_wgrad(feats, grad, nbr, k3.shape[0]).reshape(kernel.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            d_bias = col_sum(grad).reshape(1, -1)
        return d_feats, d_kernel, d_bias, None, None, None


class MinkowskiConvolutionBase(nn.Module):
    TRANSPOSED = False

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, dimension=3, **_):
        super().__init__()
        assert dimension == 3, "only D=3 is built"
        assert dilation == 1, "dilation is not used by the reference network"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = kernel_size if isinstance(kernel_size, int) else int(kernel_size[0])
        self.stride = stride if isinstance(stride, int) else int(stride[0])
        self.dimension = dimension
        K = self.kernel_size ** 3
        shape = (in_channels, out_channels) if K == 1 else (K, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty((1, out_channels), dtype=torch.float32)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        K = self.kernel_size ** 3
        n = (self.out_channels if self.TRANSPOSED else self.in_channels) * K
        stdv = 1.0 / math.sqrt(n)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def train(self, mode=True):
        invalidate_weight_caches()
        return super().train(mode)

    def _map(self, x):
        cm, ts = x.coordinate_manager, x.tensor_stride
        if self.TRANSPOSED:
            assert self.kernel_size == 2 and self.stride == 2, "only k2s2 transposed conv is built"
            return cm.up_map(ts), ts // 2
        if self.kernel_size == 1 and self.stride == 1:
            return None, ts
        return cm.kernel_map(self.kernel_size, ts, self.stride), ts * self.stride

    def forward(self, x):
        nbr, ts_out = self._map(x)
        n_out = x.coordinate_manager.num_rows(ts_out)
        F = _ConvFn.apply(x.F, self.kernel, self.bias, nbr, n_out, getattr(x, "F_hl", None))
        return x._like(F, ts_out)

    def extra_repr(self):
        return "in=%d, out=%d, kernel_size=%d, stride=%d" % (self.in_channels, self.out_channels,
                                                             self.kernel_size, self.stride)


class MinkowskiConvolution(MinkowskiConvolutionBase):
    TRANSPOSED = False


class MinkowskiConvolutionTranspose(MinkowskiConvolutionBase):
    TRANSPOSED = True


def bn_affine(bn):
    """(scale, shift) of an eval-mode BatchNorm1d, computed on the device."""
    L = _lib.lib()
    c = bn.num_features
    dev = bn.weight.device
    out = torch.empty((2, c), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(L.cv_sp_bn_fold_f32(_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean),
                                       _ptr(bn.running_var), _ptr(None), float(bn.eps), c, _ptr(out[0]),
                                       _ptr(out[1]), _stream(dev)), "cv_sp_bn_fold_f32")
    return out[0], out[1]


def affine_forward(F, scale, shift, relu, out=None, residual=None, out_hl=None, relu_bits=None):
    """relu?(F * scale + shift + residual); out_hl: a second output in the hl format (cv_sp_affine_hl_f32)"""
    L = _lib.lib()
    dev = F.device
    if out is None:
        out = torch.empty_like(F)
    if out_hl is not None:
        with _on(dev):
            _lib.check(L.cv_sp_affine_hl_f32(_ptr(F), F.shape[0], F.shape[1], F.stride(0), _ptr(scale), _ptr(shift),
                                             _ptr(residual), residual.stride(0) if residual is not None else 0,
                                             1 if relu else 0, _ptr(out), out.stride(0), _ptr(out_hl), out_hl.stride(0),
                                             _ptr(relu_bits), range_flag(dev).data_ptr(), _stream(dev)), "cv_sp_affine_hl_f32")
        return out
    with _on(dev):
        _lib.check(L.cv_sp_affine_f32(_ptr(F), F.shape[0], F.shape[1], F.stride(0), _ptr(scale), _ptr(shift),
                                      _ptr(residual), residual.stride(0) if residual is not None else 0,
                                      1 if relu else 0, _ptr(out), out.stride(0), _stream(dev)),
                   "cv_sp_affine_f32")
    return out


class _BNTrainFn(torch.autograd.Function):
    """Training-mode BatchNorm1d over feature rows on the HIP kernels (statistics, apply, backward), with the
    residual add and ReLU that follow it in BasicBlock folded into the same passes."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, residual, relu, want_hl=False):
        L = _lib.lib()
        x = x.contiguous()
        n, c = x.shape
        dev = x.device
        stats = torch.empty((4, c), dtype=torch.float32, device=dev)          # mean, var, scale, shift
        ws = torch.empty(int(L.cv_sp_bn_workspace_bytes(c)), dtype=torch.uint8, device=dev)
        with _on(dev):
            _lib.check(L.cv_sp_bn_stats_f32(_ptr(x), n, c, x.stride(0), _ptr(gamma), _ptr(beta), float(eps),
                                            float(momentum), _ptr(running_mean), _ptr(running_var), _ptr(stats[0]),
                                            _ptr(stats[1]), _ptr(stats[2]), _ptr(stats[3]), _ptr(ws), ws.numel(),
                                            _stream(dev)), "cv_sp_bn_stats_f32")
        if residual is not None and residual.stride(1) != 1:
            residual = residual.contiguous()
        # want_hl: the output once more as fp16 pairs for the convolution that reads it (TRAIN_FWD_HL; c % 32 == 0)
        y_hl = torch.empty_like(x) if want_hl else None
        # ... and where its ReLU is open as one bit per element: what the backward reads instead of y (a 32nd of the bytes)
        bits = torch.empty((n, c // 32), dtype=torch.int32, device=dev) if (want_hl and relu) else None
        y = affine_forward(x, stats[2], stats[3], relu, residual=residual, out_hl=y_hl, relu_bits=bits)
        ctx.save_for_backward(x, gamma, stats, bits if bits is not None else (y if relu else None))
        ctx.bits = bits is not None
        ctx.eps = float(eps)
        ctx.has_res = residual is not None
        ctx.two = want_hl
        ctx.step = current_step()
        ctx.set_materialize_grads(False)         # (no zero tensor for the twin's "gradient": it was a fill of N x C per layer)
        if want_hl:
            if ctx.step is not None:
                ctx.step.used_pairs = True
            ctx.mark_non_differentiable(y_hl)
            return y, y_hl
        return y

    @staticmethod
    def backward(ctx, dy, *_unused):
        L = _lib.lib()
        x, gamma, stats, y = ctx.saved_tensors
        dy = dy.contiguous()
        n, c = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        dg = torch.empty((2, c), dtype=torch.float32, device=dev)
        dres = None
        if ctx.has_res and ctx.needs_input_grad[7]:
            dres = torch.empty_like(x) if y is not None else dy
        ws = torch.empty(int(L.cv_sp_bn_workspace_bytes(c)), dtype=torch.uint8, device=dev)
        bits = y if ctx.bits else None
        y_rows = None if ctx.bits else y
        step = ctx.step
        slots = step.slots if step is not None else None
        slot, usable, dx_hl = None, False, None
        if slots is not None and c % 32 == 0 and x.stride(0) % 32 == 0 and x.stride(0) == dx.stride(0):
            slot, usable = slots.take(gamma.data_ptr())
            if slot is not None:
                # dx leaves with its hl twin for the input gradient of the convolution that produced x (usable from the layer's
                # second step on: the factor comes from the maximum the step before left in the slot)
                dx_hl = torch.empty_like(dx)
        with _on(dev):
            # (without a twin and without ReLU bits the trailing arguments are NULL: cv_sp_bn_backward_f32)
            _lib.check(L.cv_sp_bn_backward_hl_f32(_ptr(x), _ptr(dy), _ptr(y_rows), n, c, x.stride(0), _ptr(stats[0]),
                                                  _ptr(stats[1]), ctx.eps, _ptr(gamma), _ptr(dg[0]), _ptr(dg[1]),
                                                  _ptr(dx), _ptr(dres) if y is not None else None, _ptr(ws), ws.numel(),
                                                  _ptr(dx_hl), _ptr(slot) if dx_hl is not None else None,
                                                  range_flag(dev).data_ptr() if dx_hl is not None or bits is not None else None,
                                                  _ptr(bits),
                                                  _stream(dev)), "cv_sp_bn_backward_hl_f32")
        if dx_hl is not None and usable:
            # (the entry holds dx itself: while it is in the table the allocator cannot hand dx's address to another gradient
            # tensor, so a twin whose consumer is not a _ConvFn - it then stays until the step's table is dropped - can never be
            # taken for a later tensor at the same address: ADVICE r5)
            step.twins[dx.data_ptr()] = (dx_hl, slot[8192:8193].view(torch.float32), dx.shape, dx)
        return dx, dg[0], dg[1], None, None, None, None, dres, None, None


# `num_batches_tracked += 1` of every BatchNorm of a training forward (62 one-element launches per MinkUNet34C step) as ONE
# multi-tensor add: a network forward opens the batch (batched_counter_updates), the modules append their counters
_nbt_pending = threading.local()


class batched_counter_updates:
    def __enter__(self):
        self.outer = getattr(_nbt_pending, "tensors", None)
        if self.outer is None:
            _nbt_pending.tensors = []
        return self

    def __exit__(self, *exc):
        if self.outer is None:
            pend, _nbt_pending.tensors = _nbt_pending.tensors, None
            if pend:
                with torch.no_grad():
                    torch._foreach_add_(pend, 1)
        return False


class MinkowskiBatchNorm(nn.Module):
    """``nn.BatchNorm1d`` over the feature rows; sub-module name ``bn`` (utils/resnet.py:115-116)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    def forward(self, x):
        return self.forward_fused(x)

    def forward_fused(self, x, residual=None, relu=False):
        """relu?(bn(x) + residual) in one pass (BasicBlock's tail, resnet_block.py forward)."""
        bn = self.bn
        if self.training and bn.affine and bn.track_running_stats and bn.momentum is not None and x.F.shape[0] > 1:
            pend = getattr(_nbt_pending, "tensors", None)
            if pend is not None:
                pend.append(bn.num_batches_tracked)         # one multi-tensor add at the end of the network forward
            else:
                with torch.no_grad():
                    bn.num_batches_tracked += 1
            if relu and train_forward_hl() and x.F.shape[1] % 32 == 0:
                # every convolution input of the network is the output of such a pass (or a concat of two): it leaves with
                # its hl twin
                y, y_hl = _BNTrainFn.apply(x.F, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                           residual, True, True)
                return x._like(y, F_hl=y_hl)
            return x._like(_BNTrainFn.apply(x.F, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                            bn.momentum, bn.eps, residual, bool(relu)))
        if self.training or torch.is_grad_enabled() and (x.F.requires_grad or residual is not None and
                                                         residual.requires_grad):
            y = self.bn(x.F)                      # unusual configurations / eval with autograd: torch's kernels
            if residual is not None:
                y = y + residual
            return x._like(torch.relu(y) if relu else y)
        scale, shift = bn_affine(self.bn)
        return x._like(affine_forward(x.F.contiguous(), scale, shift, relu, residual=residual))


class _SyncBNFn(torch.autograd.Function):
    """Training-mode BatchNorm over the rows of ALL ranks (scene-parallel DDP gives every rank its own scenes; the
    reference's statistics are over the batch of 3 scans on one GPU, config/config.yaml:15, train_joint.py:244-251).
    One all-reduce of [2C + 1] sums (count, sum x, sum x^2) in the forward, one of [2C] (sum dy, sum dy * xhat) in the
    backward; everything else is row-local.  Plain torch ops on purpose: the same code runs over gloo on CPU (the
    2-rank test) and over RCCL on the GPUs, and it is an option next to the per-GPU HIP BatchNorm, not the default."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, group):
        import torch.distributed as dist
        n, c = x.shape
        xd = x.double()
        pack = torch.cat([xd.new_full((1,), float(n)), xd.sum(0), (xd * xd).sum(0)])
        dist.all_reduce(pack, group=group)
        total = pack[0]
        mean = pack[1:1 + c] / total
        var = (pack[1 + c:] / total - mean * mean).clamp_(min=0.0)           # biased (normalisation) variance
        with torch.no_grad():
            running_mean.mul_(1 - momentum).add_(momentum * mean.to(running_mean.dtype))
            unbiased = var * (total / (total - 1).clamp(min=1.0))
            running_var.mul_(1 - momentum).add_(momentum * unbiased.to(running_var.dtype))
        invstd = torch.rsqrt(var + eps)
        xhat = ((xd - mean) * invstd).to(x.dtype)
        ctx.save_for_backward(xhat, gamma, invstd.to(x.dtype))
        ctx.total = total
        ctx.group = group
        return xhat * gamma + beta

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        xhat, gamma, invstd = ctx.saved_tensors
        c = dy.shape[1]
        dyd = dy.double()
        sums = torch.cat([dyd.sum(0), (dyd * xhat.double()).sum(0)])
        dgamma, dbeta = sums[c:].to(dy.dtype), sums[:c].to(dy.dtype)          # local: DDP averages parameter grads
        dist.all_reduce(sums, group=ctx.group)
        m_dy = (sums[:c] / ctx.total).to(dy.dtype)
        m_dyx = (sums[c:] / ctx.total).to(dy.dtype)
        dx = (dy - m_dy - xhat * m_dyx) * (gamma * invstd)
        return dx, dgamma, dbeta, None, None, None, None, None


class MinkowskiSyncBatchNorm(MinkowskiBatchNorm):
    """MinkowskiBatchNorm whose training-mode statistics span all ranks (ME.MinkowskiSyncBatchNorm); same ``bn``
    sub-module, same state-dict keys.  Eval mode and single-process runs are the base class."""
    process_group = None

    def forward_fused(self, x, residual=None, relu=False):
        import torch.distributed as dist
        bn = self.bn
        if not (self.training and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1):
            return super().forward_fused(x, residual, relu)
        with torch.no_grad():
            bn.num_batches_tracked += 1
        y = _SyncBNFn.apply(x.F, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                            self.process_group)
        if residual is not None:
            y = y + residual
        return x._like(torch.relu(y) if relu else y)


def convert_sync_batchnorm(module, process_group=None):
    """every MinkowskiBatchNorm of ``module`` becomes a MinkowskiSyncBatchNorm in place (parameters, buffers and
    state-dict names untouched) - the counterpart of ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm"""
    for m in module.modules():
        if type(m) is MinkowskiBatchNorm:
            m.__class__ = MinkowskiSyncBatchNorm
            m.process_group = process_group
    return module


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        if x.F.requires_grad:
            return x._like(torch.relu(x.F))
        F = x.F.contiguous()
        return x._like(affine_forward(F, None, None, True, out=F if self.inplace else None))


def cat(*tensors):
    """Channel concat of tensors on the same coordinate map (utils/minkunet.py:153)."""
    if len(tensors) == 1 and isinstance(tensors[0], (list, tuple)):
        tensors = tuple(tensors[0])
    t0 = tensors[0]
    for t in tensors[1:]:
        assert t.coordinate_manager is t0.coordinate_manager and t.tensor_stride == t0.tensor_stride
    hl = None
    if all(getattr(t, "F_hl", None) is not None and t.F.shape[1] % 32 == 0 for t in tensors):
        hl = torch.cat([t.F_hl for t in tensors], dim=1)       # 32-channel chunks keep their bytes: the concat of hl rows is hl
    return t0._like(torch.cat([t.F for t in tensors], dim=1), F_hl=hl)


from . import modules  # noqa: E402,F401
