"""SUN RGB-D proposal sampler of the reference's BRNet plug-in:
``HoughVotingModule`` of sunrgbd/brnetcanon.py:104-162 with the same constructor, forward signature and
return values.  The vote is the 7-argument ``hv_cuda.forward(..., corners)`` (brnetcanon.py:99).

Two paths behind it.  ``forward`` is the reference's statement-for-statement transliteration in torch ops (max / argmax
over the up axis, power, multinomial sampling of 1.5 x num_proposal cells, rejection by distance to the seed votes,
truncation): the call-by-call reference, with about eight host waits per sample and loop trip.  BRNet calls the sampler once
per SAMPLE of every training and test iteration, so ``propose`` runs the same steps as two HIP entry points
(cv_prop_columns_f32, cv_prop_select_f32; csrc/hv_proposals.hip) behind ONE host wait, and
``propose_clouds`` is the caller's per-batch front (brnetcanon.py:213-249: voxelise, network, head, corners, sampler per
cloud) behind three.  mmdet3d / BRNet themselves are out of scope (absent dependencies)."""
import ctypes
import threading

import numpy as np
import torch
import torch.nn as nn

from . import _lib, hv_cuda
from .hough import HVFunction

SEED_RADIUS = 0.3                                  # brnetcanon.py:145


def unravel_index(index, shape):
    """sunrgbd/brnetcanon.py:86-91"""
    out = []
    for dim in reversed(shape):
        out.append(index % dim)
        index = torch.div(index, dim, rounding_mode="floor")
    return tuple(reversed(out))


_pinned_lock = threading.Lock()
_pinned_free = {}


def _pinned_i32(count):
    """a page-locked int32 landing buffer (recycled: allocating page-locked memory costs about a millisecond)"""
    with _pinned_lock:
        free = _pinned_free.get(count)
        if free:
            return free.pop()
    return torch.empty(count, dtype=torch.int32).pin_memory()


def _recycle_i32(buf):
    """hand a landing buffer back once the copy into it has been waited for"""
    with _pinned_lock:
        free = _pinned_free.setdefault(buf.numel(), [])
        if len(free) < 16:
            free.append(buf)


def _wait_here(dev):
    """block the host until everything queued on torch's current stream of ``dev`` has run (an event wait)"""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ev.synchronize()


class _Sample:
    """one sample between the enqueue of its launches and the wait for its fill count"""
    __slots__ = ("grid_scale", "dims", "corner", "res", "seeds", "yidx", "cdf", "flags", "cand", "scales", "info_d", "info_h",
                 "pinned_draws", "rounds_used")


class HoughVotingModule(nn.Module):
    def __init__(self, res=0.03, num_rots=36, nms_size=0.15, thresh=0, num_proposal=256, no_grad=True):
        super().__init__()
        self.res = torch.tensor(res, dtype=torch.float32, device="cuda")
        self.num_rots = torch.tensor(num_rots, dtype=torch.int32, device="cuda")
        # the launch geometry needs both on the host: known here, so no vote has to read them back
        hv_cuda.prime_scalar(self.res, float(np.float32(res)))
        hv_cuda.prime_scalar(self.num_rots, int(num_rots))
        self.no_grad = no_grad
        self.nms_size_grid = int(nms_size // res)
        self.num_proposal = num_proposal
        self.thresh = thresh

    def _sample(self, dist, n):
        """the one stochastic step (brnetcanon.py:137); a method so tests can pin the draws"""
        return torch.multinomial(dist, n, replacement=True)

    def forward(self, pc, xyz, scale, prob, corners, vote_points, pow=0.5):
        with torch.set_grad_enabled(not self.no_grad):
            hv_map, _, hv_scale = HVFunction.apply(pc.contiguous(), xyz.contiguous(), scale.contiguous(),
                                                   prob.contiguous(), self.res, self.num_rots, corners)
        hv_map_y = hv_map.max(1)[0] + 1e-7                                   # :124
        hv_map_y = torch.pow(hv_map_y, pow)
        hv_map_yidx = torch.argmax(hv_map, 1)
        dist = hv_map_y.reshape(-1)
        if (not torch.all(torch.isfinite(dist))) or (dist.sum() < 1e-7):     # :129-130
            dist = torch.ones_like(dist)
        cnt = 0
        loc, sample_vals, scales = [], [], []
        while cnt < self.num_proposal:                                       # :135-153
            sample = self._sample(dist, int(self.num_proposal * 1.5))
            sample_val = dist[sample]
            ix, iz = unravel_index(sample, hv_map_y.shape)
            iy = hv_map_yidx[ix, iz]
            world_loc = torch.stack([ix, iy, iz], -1) * self.res + corners[0]
            sc = hv_scale[ix, iy, iz, :]
            dist2seed = torch.min(torch.cdist(world_loc, vote_points), -1)[0]
            near = dist2seed < 0.3
            if torch.sum(near) == 0:
                loc.append(world_loc); sample_vals.append(sample_val); scales.append(sc)
            else:
                loc.append(world_loc[near]); sample_vals.append(sample_val[near]); scales.append(sc[near])
            cnt += loc[-1].shape[0]
        candidates = torch.cat(loc)[:self.num_proposal]
        scales = torch.cat(scales)[:self.num_proposal]
        probs = torch.zeros_like(candidates)[..., 0]                         # :160 (the reference returns zeros)
        return candidates, probs, scales

    # ------------------------------------------------------------------ the device path
    @property
    def per_round(self):
        """draws of one loop trip (brnetcanon.py:136)"""
        return int(self.num_proposal * 1.5)

    def _select(self, s, start, rounds, draws=None, uniform=None):
        """enqueue cv_prop_select_f32 on sample ``s`` from row ``start`` (no wait)"""
        L = _lib.lib()
        dev = s.cand.device
        ws = _lib.scratch(dev, "prop_select", int(L.cv_prop_workspace_bytes(self.per_round)))
        d = _lib.PropSelectDesc()
        d.d_grid_scale, d.d_yidx, d.d_cdf = _lib.ptr(s.grid_scale), _lib.ptr(s.yidx), _lib.ptr(s.cdf)
        d.dims = (ctypes.c_int * 3)(*s.dims)
        d.res, d.corner = s.res, (ctypes.c_float * 3)(*s.corner)
        d.d_seeds, d.n_seeds, d.radius = _lib.ptr(s.seeds), s.seeds.shape[0], SEED_RADIUS
        d.d_draws, d.d_uniform = _lib.ptr(draws), _lib.ptr(uniform)
        d.rounds, d.per_round, d.num_proposal, d.start = rounds, self.per_round, self.num_proposal, start
        d.d_cand, d.d_scale, d.d_info, d.h_info = _lib.ptr(s.cand), _lib.ptr(s.scales), _lib.ptr(s.info_d), _lib.ptr(s.info_h)
        d.d_ws, d.ws_bytes = _lib.ptr(ws), ws.numel()
        with torch.cuda.device(dev):
            _lib.check(L.cv_prop_select_f32(ctypes.byref(d), _lib.stream(dev)), "cv_prop_select_f32")

    def _enqueue(self, pc, xyz, scale, prob, corners, vote_points, pow, draws, rounds, generator, info_h):
        """vote, columns and the first select of one sample on torch's current stream, without a wait; ``info_h``: a pinned
        int32 [2] view that receives {filled, rounds_used}"""
        L = _lib.lib()
        dev = pc.device
        pc, xyz, scale, prob = pc.contiguous(), xyz.contiguous(), scale.contiguous(), prob.contiguous()
        _, res_v, nrot, _ = hv_cuda._checked_inputs(pc, xyz, scale, prob, self.res, self.num_rots)
        seeds = vote_points.detach().to(torch.float32).contiguous()
        if not seeds.is_cuda or seeds.dim() != 2 or seeds.shape[1] != 3 or seeds.shape[0] < 1:
            raise RuntimeError("vote_points must be a CUDA tensor [V >= 1, 3]")
        c = corners.detach().to("cpu", torch.float32)               # (a CPU tensor stays where it is: no device read)
        mn = [float(v) for v in c[0]]
        dims = hv_cuda._grid_dims(hv_cuda._f3(mn), hv_cuda._f3(c[1]), res_v)
        with torch.no_grad():
            grid_obj, _, grid_scale = hv_cuda._vote(pc, xyz, scale, prob, res_v, nrot, mn, dims)
        n = dims[0] * dims[2]
        s = _Sample()
        s.grid_scale, s.dims, s.corner, s.res, s.seeds = grid_scale, dims, mn, res_v, seeds
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        s.yidx = torch.empty(n, dtype=torch.int32, device=dev)
        s.cdf = torch.empty(n, dtype=torch.float64, device=dev)
        s.flags = torch.empty(2, dtype=torch.int32, device=dev)
        s.cand = torch.empty((self.num_proposal, 3), dtype=torch.float32, device=dev)
        s.scales = torch.empty((self.num_proposal, 3), dtype=torch.float32, device=dev)
        s.info_d = torch.empty(2, dtype=torch.int32, device=dev)
        s.info_h, s.rounds_used = info_h, 0
        with torch.cuda.device(dev):
            _lib.check(L.cv_prop_columns_f32(_lib.ptr(grid_obj), (ctypes.c_int * 3)(*dims), float(pow), _lib.ptr(dist),
                                             _lib.ptr(s.yidx), _lib.ptr(s.cdf), _lib.ptr(s.flags), _lib.stream(dev)),
                       "cv_prop_columns_f32")
        s.pinned_draws = draws is not None
        if draws is not None:
            table = self._draw_table(draws, n, dev)
            self._select(s, 0, table.shape[0], draws=table)
        else:
            self._select(s, 0, rounds, uniform=torch.rand(rounds * self.per_round, generator=generator, device=dev))
        return s

    def _draw_table(self, draws, n_cells, dev):
        """pinned draws (one index array per loop trip) as the int64 [trips][per_round] table of cv_prop_select_f32"""
        if len(draws) < 1:
            raise ValueError("propose: an empty list of pinned draws")
        if all(torch.is_tensor(t) and t.is_cuda for t in draws):
            table = torch.stack([t.reshape(-1) for t in draws]).to(torch.int64)
        else:
            host = np.stack([np.asarray(t.cpu() if torch.is_tensor(t) else t).reshape(-1) for t in draws]).astype(np.int64)
            if host.size and (host.min() < 0 or host.max() >= n_cells):
                raise IndexError("propose: a pinned draw outside the %d cells of the map" % n_cells)
            table = torch.from_numpy(host).to(dev)
        if table.shape[1] != self.per_round:
            raise ValueError("propose: %d draws per trip, the sampler takes int(num_proposal * 1.5) = %d"
                             % (table.shape[1], self.per_round))
        return table.contiguous()

    def _finish(self, samples, rounds, generator):
        """ONE wait for the fill counts of ``samples``; a sample whose budget ended short draws another one and continues
        (uniform draws) or raises (pinned draws).  Returns [(candidates, probs, scales)]."""
        dev = samples[0].cand.device
        _wait_here(dev)
        out = []
        for s in samples:
            filled, used = int(s.info_h[0]), int(s.info_h[1])
            s.rounds_used += used
            while filled < self.num_proposal:
                if s.pinned_draws:
                    raise RuntimeError("propose: the pinned draws ran out after %d trips with %d of %d proposals"
                                       % (s.rounds_used, filled, self.num_proposal))
                self._select(s, filled, rounds, uniform=torch.rand(rounds * self.per_round, generator=generator, device=dev))
                _wait_here(dev)
                filled, used = int(s.info_h[0]), int(s.info_h[1])
                s.rounds_used += used
            out.append((s.cand, torch.zeros(self.num_proposal, dtype=torch.float32, device=dev), s.scales))
        self.last_rounds_used = [s.rounds_used for s in samples]
        return out

    def propose(self, pc, xyz, scale, prob, corners, vote_points, pow=0.5, draws=None, rounds=4, generator=None):
        """``forward`` on the device path: vote, cv_prop_columns_f32, cv_prop_select_f32 and ONE host wait, for the fill
        count.  Same arguments, and (candidates [P, 3], probs [P] of zeros, scales [P, 3]) as ``forward`` returns them.

        corners: preferably a CPU tensor [2, 3] - the vote then needs no device read; a device tensor costs its one copy.
        draws: None, or the pinned per-trip index arrays ([int(1.5 P)] each, numpy or torch) - the result is then, bit for
        bit, what the numpy oracle computes from the same grids, and ``forward`` with the same draws wherever the nearest
        seed is not within rounding of the 0.3 m radius (``forward`` measures it with torch's matrix-product cdist).  A list
        that runs out before P proposals exist raises.
        draws=None: a budget of ``rounds`` trips of uniforms is drawn up front with ``torch.rand(..., generator=generator)``
        on the device and each is inverted through the fp64 prefix sums of the map; a budget that ends short is followed by
        another one.  THE ONE SEMANTIC DIFFERENCE from ``forward``: torch's generator state afterwards differs from the
        reference's (which calls torch.multinomial once per trip it needs); the distribution of the draws does not.
        ``last_rounds_used`` holds the trips the last call evaluated."""
        if rounds < 1:
            raise ValueError("propose: rounds must be at least 1")
        info_h = _pinned_i32(2)
        s = self._enqueue(pc, xyz, scale, prob, corners, vote_points, pow, draws, rounds, generator, info_h)
        out = self._finish([s], rounds, generator)[0]
        _recycle_i32(info_h)
        return out


def cloud_corners(coords4, n_clouds, quantization_size, border=0.0):
    """Row ranges and grid corners of every cloud of a batched coordinate set, from ONE launch (cv_prop_cloud_ranges_i32) and one
    host wait: coords4 [N, 4] int32 (batch, x, y, z) with the batch column non-decreasing, as quantize_batch returns it.
    Returns (ranges [(first row, end row)], corners [B] of CPU float32 [2, 3]): brnetcanon.py:235-240, where
    ``torch.min(coord * q)`` is ``float32(min coord) * float32(q)`` because the rounded product is monotone, and ``border``
    widens x and z."""
    L = _lib.lib()
    dev = coords4.device
    assert coords4.is_cuda and coords4.dtype == torch.int32 and coords4.is_contiguous() and coords4.dim() == 2 \
        and coords4.shape[1] == 4, "coords4: contiguous int32 [N, 4] on the device"
    out_d = torch.empty((n_clouds, 8), dtype=torch.int32, device=dev)
    out_h = _pinned_i32(n_clouds * 8)
    with torch.cuda.device(dev):
        _lib.check(L.cv_prop_cloud_ranges_i32(_lib.ptr(coords4), coords4.shape[0], n_clouds, _lib.ptr(out_d), _lib.ptr(out_h),
                                              _lib.stream(dev)), "cv_prop_cloud_ranges_i32")
    _wait_here(dev)
    table = out_h.numpy().reshape(n_clouds, 8).copy()
    _recycle_i32(out_h)
    q, b = np.float32(quantization_size), np.float32(border)
    ranges, corners = [], []
    for row in table:
        if row[0] >= row[1]:
            raise RuntimeError("propose_clouds: cloud %d has no voxel" % len(ranges))
        c = np.stack([row[2:5].astype(np.float32) * q, row[5:8].astype(np.float32) * q]).astype(np.float32)
        c[0, 0] -= b; c[0, 2] -= b
        c[1, 0] += b; c[1, 2] += b
        ranges.append((int(row[0]), int(row[1])))
        corners.append(torch.from_numpy(c))
    return ranges, corners


def propose_clouds(model, hvm, clouds, vote_points, quantization_size=0.03, border=0.0, pow=0.5, draws=None, rounds=4,
                   generator=None):
    """sunrgbd/brnetcanon.py:213-249 for a batch of B clouds with three host waits (voxel count, row ranges and bounds, fill
    counts) instead of a dozen per sample.

    clouds: B device tensors [Mi, 3], already in the network's axis order (the caller's ``points[i][..., [0, 2, 1]]``);
    vote_points: B device tensors [V, 3] (or one [B, V, 3]) in the same order; model: the 8-channel per-category network
    (MinkUNet34C(3, 8) there); hvm: a HoughVotingModule.  draws: None, or one list of pinned per-trip draws per cloud.
    Steps: quantize_batch; ONE voxel_rows launch (world points ``float(coord) * q``, the first point's xyz as the three input
    features); one batched network forward; one head_separate over all rows; cloud_corners; per sample the vote into views
    of its row range (a cloud's rows are contiguous: nothing is copied), columns and select; one wait for all B fill counts.
    Returns (proposals [B, P, 3], probs [B, P], scales [B, P, 3]), sample b bit for bit ``hvm.propose`` on cloud b's rows."""
    from . import me as ME
    from .me import utils as ME_utils
    from .pipeline import head_separate
    B = len(clouds)
    if B < 1 or len(vote_points) != B or (draws is not None and len(draws) != B):
        raise ValueError("propose_clouds: one vote_points entry (and draws list) per cloud")
    if rounds < 1:
        raise ValueError("propose_clouds: rounds must be at least 1")
    dev = clouds[0].device
    with torch.no_grad():
        offsets = [0]
        for c in clouds[:-1]:
            offsets.append(offsets[-1] + c.shape[0])
        raw = torch.cat([c.to(torch.float32) for c in clouds], 0).contiguous()
        coords4, index = ME_utils.quantize_batch(raw, quantization_size, offsets=offsets)             # wait 1: voxel count
        pts, (feats,) = ME_utils.voxel_rows(coords4, index, np.float32(quantization_size), raw)
        x = ME.SparseTensor(feats, coords4, device=dev)
        deferred = hasattr(model, "check_range")
        y = model(x, defer_check=True) if deferred else model(x)
        xyz, scale, prob = head_separate(y.F, log_scale=True)
        ranges, corners = cloud_corners(coords4, B, quantization_size, border)                        # wait 2
        if deferred:
            # the stream has been waited for: the fp16-range flag of the network's convolutions is final
            y2 = model.check_range(x, y)
            if y2 is not y:
                xyz, scale, prob = head_separate(y2.F, log_scale=True)
        info_h = _pinned_i32(2 * B)
        samples = []
        for b, (r0, r1) in enumerate(ranges):
            samples.append(hvm._enqueue(pts[r0:r1], xyz[r0:r1], scale[r0:r1], prob[r0:r1], corners[b], vote_points[b], pow,
                                        None if draws is None else draws[b], rounds, generator, info_h[2 * b:2 * b + 2]))
        out = hvm._finish(samples, rounds, generator)                                                 # wait 3
        _recycle_i32(info_h)
    return tuple(torch.stack([o[k] for o in out]) for k in range(3))
