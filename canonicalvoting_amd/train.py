"""Training step of the joint model as functions (train_joint.py:244-288):

    joint_loss          head gather by ground-truth class + masked MSE(xyz) + MSE(log scale) + CE(class)
                        (train_joint.py:253-283; defaults from config/config.yaml)
    separate_loss       the per-category model's loss with the minimum over symmetry-equivalent poses
                        (train_separate.py:247-287)
    separate_loss_packed the same over data.collate_sym's packed labels: the pose loss on the device, no host wait
    train_step          zero_grad -> forward -> loss -> backward -> optimizer.step (:246-288)
    train_step_separate the same for the per-category model (train_separate.py:236-292); both run through _run_step
    adjust_learning_rate step LR decay (:128-138, config.yaml:32-36)
    make_ddp            scene-parallel data parallelism: torch DDP (bucketed gradient all-reduce over
                        RCCL, overlapped with backward) around the model (the reference
                        itself is single-GPU)

The sparse convolutions run forward / input-gradient / weight-gradient on the HIP kernels
(canonicalvoting_amd.me._ConvFn), batch-statistics BatchNorm with the residual add and ReLU folded in on
bn_col_reduce4 / bn_backward_apply4 (me._BNTrainFn).  The losses are torch ops by default; the packed pose loss always runs on
sym_loss.hip, and with ``device_loss=True`` (train_step, train_step_separate; ``device_rows=True`` of separate_loss_packed) the
per-row terms - head gather, masked squared errors, cross entropy and their backward - run on row_loss.hip instead
(joint_loss_device: two launches forward, one backward, no host wait).

    joint_loss_device   joint_loss on the row-loss kernels, the same arguments and keys
    joint_loss_val      the validation form (train_joint.py:311-340): head by the predicted class, NaN without object rows
    validate_joint      the trainer's validation pass (train_joint.py:293-430): losses, detections and mAP per scan list
    validate_separate   the per-category trainer's (train_separate.py:301-458): separate_loss_packed, head_separate, vote,
                        the separate-variant decode and NMS of the one category, AP and recall
    finish_pending      act on a range flag the lagged read has not reached yet (restore BatchNorm statistics, go to the
                        triples) in front of a validation pass or a checkpoint

The reference's stale-loss bug (`losses` persists across iterations) is not
reproduced: a batch without object points contributes only the classification loss.
"""
import torch
import torch.nn.functional as F

from . import me as ME


def joint_loss(out_feats, xyz_labels, scale_labels, class_labels, nclasses=9, log_scale=True,
               xyz_factor=1.0, scale_factor=1.0, xyz_component_weights=(1.0, 1.0, 1.0)):
    """out_feats [N, 7*nclasses+1]; labels as utils/dataloader.py:170-188 (class 9 / -1 = background)."""
    labels = class_labels.long()
    idx = labels.clamp(min=0)
    idx = torch.where(idx == nclasses, torch.zeros_like(idx), idx)             # :254-256
    g = idx[:, None, None].expand(-1, 1, 3)
    out_xyz = torch.gather(out_feats[:, :3 * nclasses].reshape(-1, nclasses, 3), 1, g)[:, 0]       # :257
    out_scale = torch.gather(out_feats[:, 3 * nclasses:6 * nclasses].reshape(-1, nclasses, 3), 1, g)[:, 0]
    out_class = out_feats[:, 6 * nclasses:]
    mask = (labels < nclasses) & (labels >= 0)                                  # :261
    w = torch.as_tensor(xyz_component_weights, dtype=out_feats.dtype, device=out_feats.device)
    # :262-272 without a host wait.  The reference indexes with the boolean mask (`if torch.any(mask)`, `x[mask]`): every such
    # line makes the host wait for the forward, and the backward is only queued once the chip has run dry (3-4 ms of a 27 ms
    # step, profiles/r5/train_gaps.txt).  The same means as sums over all rows times the mask, divided by the object rows on
    # the device: equal up to summation order; no object row: both terms are zero, as the reference's `if` leaves them.
    # Background rows are SELECTED away in front of the arithmetic (prediction and target both become 0 there), not multiplied by
    # zero behind it: a non-finite prediction in a row the reference never touches (:262-272 index with the mask) reaches
    # neither the loss nor - through 0 * inf in a backward formula - a gradient.
    m = mask[:, None]
    cnt = mask.sum()
    denom = (cnt * 3).clamp(min=1).to(out_feats.dtype)
    zero = torch.zeros((), dtype=out_feats.dtype, device=out_feats.device)
    safe_scale = torch.where(m, scale_labels, torch.ones_like(scale_labels))
    tgt_scale = torch.where(m, torch.log(safe_scale) if log_scale else safe_scale, zero)       # :266-269
    tgt_xyz = torch.where(m, xyz_labels, zero)
    out_scale = torch.where(m, out_scale, zero)
    out_xyz = torch.where(m, out_xyz, zero)
    losses = {"loss_scale": torch.sum((out_scale - tgt_scale) ** 2 * w) / denom * scale_factor,
              "loss_xyz": torch.sum((out_xyz - tgt_xyz) ** 2 * w) / denom * xyz_factor}
    # :273; the reference's labels are 0..9 (9 = background, utils/dataloader.py:172) - a negative label would make its
    # CrossEntropyLoss raise, here it counts as background
    losses["loss_class"] = F.cross_entropy(out_class, torch.where(labels < 0, torch.full_like(labels, nclasses), labels))
    return sum(losses.values()), losses


def joint_loss_device(out_feats, xyz_labels, scale_labels, class_labels, nclasses=9, log_scale=True,
                      xyz_factor=1.0, scale_factor=1.0, xyz_component_weights=(1.0, 1.0, 1.0)):
    """joint_loss on the device (ME.utils.row_loss, cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32): the same arguments, the same
    ``(total, {"loss_scale", "loss_xyz", "loss_class"})``; fp64 terms and sums rounded once, the same bytes on every run, no
    host wait.  The gradient flows through ``total``; the three parts are reported values without one."""
    loss_xyz, loss_scale, loss_class, total = ME.utils.row_loss(
        out_feats, class_labels, xyz_labels, scale_labels, layout="joint", gather="label", empty="zero", nclasses=nclasses,
        log_scale=log_scale, weights=xyz_component_weights, xyz_factor=xyz_factor, scale_factor=scale_factor)
    return total, {"loss_scale": loss_scale, "loss_xyz": loss_xyz, "loss_class": loss_class}


def joint_loss_val(out_feats, xyz_labels, scale_labels, class_labels, nclasses=9, log_scale=True,
                   xyz_factor=1.0, scale_factor=1.0, xyz_component_weights=(1.0, 1.0, 1.0)):
    """The validation losses of train_joint.py:311-340 on the device, without a gradient: the head is chosen by the PREDICTED
    class (argmax of the logits, class ``nclasses`` -> head 0, :315-316), not by the label, and a scan without an object row
    gives NaN for loss_xyz and loss_scale - the reference's mean over nothing (:331-332).  Same return form as joint_loss."""
    with torch.no_grad():
        loss_xyz, loss_scale, loss_class, total = ME.utils.row_loss(
            out_feats, class_labels, xyz_labels, scale_labels, layout="joint", gather="argmax", empty="nan", nclasses=nclasses,
            log_scale=log_scale, weights=xyz_component_weights, xyz_factor=xyz_factor, scale_factor=scale_factor)
    return total, {"loss_scale": loss_scale, "loss_xyz": loss_xyz, "loss_class": loss_class}


def separate_loss(out_feats, xyz_labels, scale_labels, obj_labels, coords4=None, log_scale=True, xyz_factor=1.0,
                  scale_factor=1.0, xyz_component_weights=(1.0, 1.0, 1.0), reference_indexing=True):
    """Loss of the per-category model (train_separate.py:247-287): out_feats [N, 8] = xyz, (log) scale, 2 objectness
    logits; ``xyz_labels`` per scan a list of [rows, [xyz under each symmetry-equivalent pose]]
    (data.collate_fn_separate); the coordinate loss of a model is the MINIMUM over its poses (:271-275), averaged
    over models.  ``reference_indexing``: the reference indexes the BATCH output with each scan's own row numbers
    (:270, `batch_idx` is computed and never used), which is only right for the first scan of a batch; True keeps
    that, False offsets the rows of scan j by the rows of scans < j (needs ``coords4``)."""
    obj = obj_labels.long()
    mask = obj == 1
    w = torch.as_tensor(xyz_component_weights, dtype=out_feats.dtype, device=out_feats.device)
    losses = {"loss_obj": F.cross_entropy(out_feats[:, 6:8], obj)}
    tgt = torch.log(scale_labels[mask]) if log_scale else scale_labels[mask]
    losses["loss_scale"] = torch.mean((out_feats[:, 3:6][mask] - tgt) ** 2 * w) * scale_factor
    out_xyz = out_feats[:, :3]
    first_row = None
    if not reference_indexing:
        counts = torch.bincount(coords4[:, 0].long(), minlength=len(xyz_labels))
        first_row = torch.cumsum(counts, 0) - counts
    per_model = []
    for j, per_scan in enumerate(xyz_labels):
        for rows, xyzs in per_scan:
            rows = rows.to(out_feats.device)
            if first_row is not None:
                rows = rows + first_row[j]
            pred = out_xyz[rows]
            per_model.append(torch.stack([torch.mean((pred - x.to(out_feats.device)) ** 2 * w) for x in xyzs]).min())
    losses["loss_xyz"] = torch.mean(torch.stack(per_model)) * xyz_factor
    return sum(losses.values()), losses


def separate_loss_packed(out_feats, sym, scale_labels, obj_labels, log_scale=True, xyz_factor=1.0, scale_factor=1.0,
                         xyz_component_weights=(1.0, 1.0, 1.0), device_rows=False):
    """separate_loss - the same three terms under the same keys - over packed symmetry labels, without a host wait.
    ``sym``: a data.SymBatch on the output's device (data.collate_sym + data.sym_to_device; which indexing its rows follow
    was decided in the collate).  Its largest row is compared with the output's rows here, from the host int, before anything
    is launched.  loss_xyz: ME.utils.sym_loss (HIP: minimum over the symmetry-equivalent poses per model, mean over the
    models; two launches forward, one backward).  loss_obj: the same cross entropy.  loss_scale: in joint_loss's form - the
    object count stays on the device as the denominator and background rows are selected away in front of the arithmetic,
    so a non-finite background prediction reaches neither the loss nor a gradient, and a batch without an object row gives
    a zero term where separate_loss's mean over nothing gives NaN.
    ``device_rows``: loss_scale and loss_obj come from ME.utils.row_loss(layout='separate') (row_loss.hip) instead of torch
    ops, loss_xyz still from sym_loss; the two gradients stay two autograd outputs that torch adds.  The gradient of the row
    terms then flows through the total only (the two parts are reported values)."""
    if sym.max_row >= out_feats.shape[0]:
        raise ValueError("separate_loss_packed: label row %d outside the %d output rows" % (sym.max_row, out_feats.shape[0]))
    if device_rows:
        _, loss_scale, loss_obj, rows_total = ME.utils.row_loss(
            out_feats, obj_labels, None, scale_labels, layout="separate", gather="label", empty="zero", log_scale=log_scale,
            weights=xyz_component_weights, scale_factor=scale_factor)
        loss_xyz = ME.utils.sym_loss(out_feats, sym, xyz_component_weights, xyz_factor)
        return rows_total + loss_xyz, {"loss_obj": loss_obj, "loss_scale": loss_scale, "loss_xyz": loss_xyz}
    obj = obj_labels.long()
    m = (obj == 1)[:, None]
    w = torch.as_tensor(xyz_component_weights, dtype=out_feats.dtype, device=out_feats.device)
    losses = {"loss_obj": F.cross_entropy(out_feats[:, 6:8], obj)}
    denom = (m.sum() * 3).clamp(min=1).to(out_feats.dtype)
    zero = torch.zeros((), dtype=out_feats.dtype, device=out_feats.device)
    safe_scale = torch.where(m, scale_labels, torch.ones_like(scale_labels))
    tgt = torch.where(m, torch.log(safe_scale) if log_scale else safe_scale, zero)
    out_scale = torch.where(m, out_feats[:, 3:6], zero)
    losses["loss_scale"] = torch.sum((out_scale - tgt) ** 2 * w) / denom * scale_factor
    losses["loss_xyz"] = ME.utils.sym_loss(out_feats, sym, xyz_component_weights, xyz_factor)
    return sum(losses.values()), losses


def _skips_on_device(optimizer):
    """a fused torch Adam / AdamW takes `found_inf` (what torch.cuda.amp.GradScaler hands it): the update is skipped on the device"""
    return isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)) and all(g.get("fused") for g in optimizer.param_groups)


FLAG_LAG = 2        # train_step reads the range flag of the step this many calls ago (all ranks the same one)


def _step_group(model):
    """the process group whose ranks step together with this model (DDP), or None"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = getattr(model, "process_group", None)
    if group is None and not isinstance(model, torch.nn.parallel.DistributedDataParallel):
        return None
    return group if dist.get_world_size(group) > 1 else None


class _FlagRing:
    """The range flag of the step FLAG_LAG calls ago - the SAME step on every rank, after an all-reduce (MAX) over the group:
    ranks that step together act on one value at one step (skip / restore / redo / switch to the triples together; a rank
    acting on its own flag, or on a live peek that lands at another step, leaves the others with diverged parameters or in a
    collective nobody joins: ADVICE r5).  push() stores this step's flag behind the step's work (pinned memory + event, no
    host wait); noticed() reads the oldest stored one, whose event passed long ago."""

    def __init__(self, dev, lag=FLAG_LAG):
        self.dev, self.lag, self.k, self.slots = dev, lag, 0, [None] * lag

    def noticed(self):
        slot = self.slots[self.k % self.lag]
        if slot is None or not slot["valid"]:
            return False
        if slot["event"] is not None:
            slot["event"].synchronize()
        return float(slot["host"][0]) != 0.0

    def pending(self):
        """whether ANY stored flag is raised, the youngest included: waits for the event of every valid slot (finish_pending)"""
        raised = False
        for slot in self.slots:
            if slot is None or not slot["valid"]:
                continue
            if slot["event"] is not None:
                slot["event"].synchronize()
            raised = raised or float(slot["host"][0]) != 0.0
        return raised

    def push(self, found, group=None):
        """found: float scalar tensor on the step's device (None: the step used no fp16 pairs); returns the group's value"""
        i = self.k % self.lag
        self.k += 1
        slot = self.slots[i]
        if slot is None:
            cuda = self.dev.type == "cuda"
            host = torch.zeros(1, dtype=torch.float32)
            slot = self.slots[i] = {"host": host.pin_memory() if cuda else host, "event": torch.cuda.Event() if cuda else None,
                                    "valid": False}
        slot["valid"] = found is not None
        if found is None:
            return None
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(found, op=dist.ReduceOp.MAX, group=group)
        slot["host"].copy_(found.reshape(1), non_blocking=True)
        if slot["event"] is not None:
            slot["event"].record(torch.cuda.current_stream(self.dev))
        return found


class _StepState:
    """what train_step keeps with a model between its calls: the lagged range flags, the BatchNorm snapshot buffers, and
    whether a flagged step has sent the model to the bf16 triples for good"""
    ring, snapshot, pairs_off = None, None, False


def _step_state(model):
    st = model.__dict__.get("_cv_step_state")
    if st is None:
        st = model.__dict__["_cv_step_state"] = _StepState()
    return st


def _bn_state(model):
    """(the BatchNorm running statistics and counters of `model`, a snapshot buffer for each that lives with the model)"""
    bufs = [b for m in model.modules() for b in (getattr(m, "running_mean", None), getattr(m, "running_var", None),
                                                 getattr(m, "num_batches_tracked", None)) if b is not None]
    st = _step_state(model)
    saved = st.snapshot
    if saved is None or len(saved) != len(bufs) or any(a.shape != b.shape or a.device != b.device or a.dtype != b.dtype
                                                       for a, b in zip(saved, bufs)):
        saved = st.snapshot = [torch.empty_like(b) for b in bufs]
    return bufs, saved


def _drop_flagged_steps(model, st, dev, bufs, saved):
    """What follows a noticed range flag: the flagged steps' updates were skipped on the device and the BatchNorm snapshot still
    holds the statistics and counters of before the first of them - wait for the stream, put them back, clear the flag, count
    the fallback and send the model to the bf16 triples for good (no ring from here on)."""
    torch.cuda.current_stream(dev).synchronize()
    with torch.no_grad():
        torch._foreach_copy_(bufs, saved)
    ME.range_flag(dev).zero_()
    model.train_range_fallbacks = getattr(model, "train_range_fallbacks", 0) + 1
    st.pairs_off, st.ring = True, None


def finish_pending(model):
    """Act NOW on a range flag that train_step / train_step_separate would only notice FLAG_LAG calls later - in front of
    anything that reads the model between two steps: a validation pass, a checkpoint.  ``model``: the object that was handed to
    the step (under DDP the wrapper: the step state lives on it).
    No ring (the model never stepped, the optimizer cannot skip on the device, or the model is on the bf16 triples already):
    returns False and launches nothing.  Otherwise waits for the event of every stored flag and reads them all; all zero:
    returns False and nothing changes.  Any non-zero: what the step's own lagged read does - stream synchronised, BatchNorm
    running statistics and counters restored from the snapshot of before the first flagged step, ME.range_flag zeroed,
    ``model.train_range_fallbacks`` counted, the model on the triples from here on - and returns True.  It runs no step: the
    flagged batches stay dropped, as train_step documents.
    Under DDP the stored flags are the all-reduced ones (push reduces before it stores), so every rank reads the same values
    and no collective is needed here - but EVERY rank must call this at the same point between the same two steps, or the
    ranks leave the fp16 pairs at different steps."""
    st = model.__dict__.get("_cv_step_state")
    ring = st.ring if st is not None else None
    if ring is None:
        return False
    if not ring.pending():
        return False
    _drop_flagged_steps(model, st, ring.dev, *_bn_state(model))
    return True


def _run_step(model, optimizer, dev, forward_loss):
    """The core of train_step and train_step_separate: zero_grad -> ``forward_loss()`` (a closure: forward and loss, returns
    ``(loss, parts)``) -> backward -> optimizer.step, inside the one training-step state a model keeps (_StepState): the
    pair-scale hints and the batched weight pack, the range-flag ring with `found_inf`, the BatchNorm snapshot guard, the
    bf16-triples fallback and the agreement of the flag over DDP ranks - as train_step's docstring describes them."""
    group = _step_group(model)

    def fwd_bwd():
        optimizer.zero_grad(set_to_none=True)
        loss, parts = forward_loss()
        loss.backward()
        return loss, parts

    def on_triples(fn):
        with ME.on_bf16_triples():
            return fn()

    st = _step_state(model)
    if not ME.train_uses_pairs() or st.pairs_off:
        loss, parts = on_triples(fwd_bwd)
        optimizer.step()
        return loss.detach(), {k: v.detach() for k, v in parts.items()}

    bufs, saved = _bn_state(model)
    if _skips_on_device(optimizer):
        if st.ring is None or st.ring.dev != dev:
            st.ring = _FlagRing(dev)
        ring = st.ring
        if ring.noticed():
            # the step FLAG_LAG calls ago left the fp16 range (on this rank or, under DDP, on any rank): its update and that
            # of every step queued since was skipped on the device, and the BatchNorm snapshot still holds the statistics and
            # counters of before it
            _drop_flagged_steps(model, st, dev, bufs, saved)
            return _run_step(model, optimizer, dev, forward_loss)
        # BatchNorm statistics of before this step, kept ON THE DEVICE only while no step has raised the flag
        ME.copy_unless_flag(bufs, saved, dev, ME.range_flag(dev))
        with ME.pair_scale_hints(model) as step:
            loss, parts = fwd_bwd()
        found = ring.push(step.range_flag_device(dev), group)
        if found is not None and group is not None:
            # the local flag follows the group's: every rank's later steps skip too, and every rank's snapshot guard closes
            ME.range_flag(dev).copy_(found.reshape(1).to(torch.int32), non_blocking=True)
        optimizer.found_inf = found
        try:
            optimizer.step()
        finally:
            optimizer.found_inf = None
        return loss.detach(), {k: v.detach() for k, v in parts.items()}

    # the step may have to be redone: keep the BatchNorm running statistics of before the step, so that the redo does not count
    # the batch twice (one momentum update and one num_batches_tracked increment per iteration, as train_joint.py:250-283 gives)
    # (one multi-tensor copy into buffers that live with the model: 186 one-element clones per step were 186 launches)
    with torch.no_grad():
        torch._foreach_copy_(saved, bufs)
    with ME.pair_scale_hints(model) as step:
        loss, parts = fwd_bwd()
    if step.left_fp16_range(dev, group):
        with torch.no_grad():
            torch._foreach_copy_(bufs, saved)
        loss, parts = on_triples(fwd_bwd)
        model.train_range_fallbacks = getattr(model, "train_range_fallbacks", 0) + 1
    optimizer.step()
    return loss.detach(), {k: v.detach() for k, v in parts.items()}


def train_step(model, optimizer, coords4, feats, xyz_labels, scale_labels, class_labels, device_loss=False, **loss_kw):
    """one iteration of train_joint.py:246-288; feats already recentred (:248-249).  ``device_loss``: joint_loss_device (the
    row-loss kernels) instead of joint_loss (torch ops).

    The forward multiplies fp16 pairs on the eval path's kernels (ME.TRAIN_FWD_HL); an activation beyond the fp16 range - never
    behind a healthy BatchNorm - raises the range flag.  With a fused Adam the flag rides to the optimizer as `found_inf`: the
    update of such a step is skipped ON THE DEVICE (no host wait in the step).  The host reads the flag of the step FLAG_LAG
    calls ago (pinned memory + an event that has long passed): it then restores the BatchNorm running statistics and counters
    from a snapshot that a device-side guard has kept at the state before the FIRST flagged step (cv_sp_copy_unless_flag: the
    flagged batches are dropped as a whole - no update, no statistics, exactly as if they had not been drawn), counts the
    fallback (model.train_range_fallbacks) and runs this and the following steps on the bf16 triples.  Other optimizers: the host
    waits for the flag and redoes the step on the triples before the optimizer sees a gradient.
    Under DDP the flag is all-reduced (MAX) over the ranks of the model's process group before anybody acts on it, and the
    lagged read looks at the same step on every rank: all ranks skip, restore, redo and switch to the triples together."""
    dev = feats.device

    def forward_loss():
        out = model(ME.SparseTensor(feats, coords4, device=dev))
        return (joint_loss_device if device_loss else joint_loss)(out.F, xyz_labels, scale_labels, class_labels, **loss_kw)

    return _run_step(model, optimizer, dev, forward_loss)


def _is_sym_batch(labels):
    return isinstance(labels, tuple) and hasattr(labels, "seg_ptr") and hasattr(labels, "n_segments")


def train_step_separate(model, optimizer, coords4, feats, xyz_labels, scale_labels, obj_labels, device_loss=False, **loss_kw):
    """one iteration of train_separate.py:236-292 (8-channel per-category model); feats already recentred (:241-242).
    Returns None for a batch without object points, which the reference skips (:238-240).

    ``xyz_labels`` a data.SymBatch (data.collate_sym): the step of train_step - one _StepState per model with the pair-scale
    hints, the batched weight pack, the range flag as `found_inf`, the BatchNorm snapshot guard, the bf16-triples fallback and
    the DDP flag agreement (_run_step) - around separate_loss_packed, with no host wait: the skip is ``n_segments == 0``, a
    host int.  The labels may still be on the host (copied non-blocking here) or already on the device (data.sym_to_device).
    ``device_loss`` (packed labels only): separate_loss_packed(device_rows=True).
    ``xyz_labels`` the nested lists of data.collate_fn_separate: the plain forward -> separate_loss -> backward -> step."""
    dev = feats.device
    if _is_sym_batch(xyz_labels):
        sym = xyz_labels
        if sym.n_segments == 0:
            return None
        if sym.rows.device != dev:
            from .data import sym_to_device
            sym = sym_to_device(sym, dev)
        scale_dev, obj_dev = scale_labels.to(dev, non_blocking=True), obj_labels.to(dev, non_blocking=True)

        def forward_loss():
            out = model(ME.SparseTensor(feats, coords4, device=dev))
            return separate_loss_packed(out.F, sym, scale_dev, obj_dev, device_rows=device_loss, **loss_kw)

        return _run_step(model, optimizer, dev, forward_loss)
    if device_loss:
        raise ValueError("train_step_separate: device_loss needs packed labels (data.collate_sym)")
    if not bool((obj_labels == 1).any()):
        return None
    optimizer.zero_grad(set_to_none=True)
    out = model(ME.SparseTensor(feats, coords4, device=feats.device))
    loss, parts = separate_loss(out.F, xyz_labels, scale_labels.to(dev), obj_labels.to(dev), coords4=coords4, **loss_kw)
    loss.backward()
    optimizer.step()
    return loss.detach(), {k: v.detach() for k, v in parts.items()}


def validate_joint(model, hv, batches, res, gt_boxes=None, nclasses=9, log_scale=True, xyz_factor=1.0, scale_factor=1.0,
                   xyz_component_weights=(1.0, 1.0, 1.0), **decode_kw):
    """The validation pass of train_joint.py:293-430.  ``batches`` yields one scan at a time (batch size 1):
    ``(id_scan, coords4, feats, xyz_labels, scale_labels, class_labels)`` on the model's device, feats already recentred
    (:305-306).  Per scan ONE eval-mode forward under no_grad (pipeline.detect_scene's, its fp16-range check included),
    joint_loss_val on that output (:311-340), then pipeline.head_joint and vote, decode and per-class NMS on the same output
    (decode.detect, :342-439); the detections go into ``pred_map_cls[id_scan]``.
    Returns a dict: ``losses`` = the mean of loss / loss_xyz / loss_scale / loss_class over the scans (the per-scan values
    stay on the device and are read once at the end; a scan without an object row makes the two means NaN, as the
    reference's values are), ``pred_map_cls``, ``n_scans`` and - with ``gt_boxes`` {id_scan: lines ``tx ty tz ry sx sy sz ...
    category`` as in cfg.data.gt_path} - ``map`` = {0.25: ..., 0.5: ...} from calc_map.compute_map.
    The model is put back into the mode it was in; eval-mode BatchNorm leaves the running statistics untouched."""
    from . import decode, hv_cuda, pipeline
    was_training = model.training
    model.eval()
    kw = dict(nclasses=nclasses, log_scale=log_scale, xyz_factor=xyz_factor, scale_factor=scale_factor,
              xyz_component_weights=xyz_component_weights)
    pred_map_cls, per_scan = {}, []
    try:
        with torch.no_grad():
            for id_scan, coords4, feats, xyz_labels, scale_labels, class_labels in batches:
                dev = feats.device
                scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
                hv_cuda.prefetch_geometry(scan_points)
                x = ME.SparseTensor(feats, coords4, device=dev)
                deferred = hasattr(model, "check_range")
                y = model(x, defer_check=True) if deferred else model(x)
                for attempt in range(2):
                    total, parts = joint_loss_val(y.F, xyz_labels.to(dev), scale_labels.to(dev), class_labels.to(dev), **kw)
                    xyz, scale, prob, cls = pipeline.head_joint(y.F, nclasses, log_scale)
                    dets, _ = decode.detect(hv, coords4[:, 1:], xyz, scale, prob, cls, res, nclasses, scan_points=scan_points,
                                            **decode_kw)
                    y2 = model.check_range(x, y) if (deferred and attempt == 0) else y
                    if y2 is y:
                        break
                    y = y2
                pred_map_cls[id_scan] = dets
                per_scan.append(torch.stack([total, parts["loss_xyz"], parts["loss_scale"], parts["loss_class"]]))
    finally:
        model.train(was_training)
    return _validation_result(per_scan, ("loss", "loss_xyz", "loss_scale", "loss_class"), pred_map_cls, gt_boxes)


def _validation_result(per_scan, keys, pred_map_cls, gt_boxes):
    """what validate_joint and validate_separate return: the means of the per-scan loss rows (the pass's one host read), the
    detections, the scan count and - with ground truth - the mAP dicts over the scans that ran"""
    from . import calc_map
    from .data import parse_gt_lines
    out = {"pred_map_cls": pred_map_cls, "n_scans": len(per_scan)}
    mean = torch.stack(per_scan).mean(0).tolist() if per_scan else [float("nan")] * len(keys)
    out["losses"] = dict(zip(keys, mean))
    if gt_boxes is not None:
        gt_map_cls = {i: [(c, calc_map.gt_box(*p)) for c, p in parse_gt_lines(gt_boxes[i])] for i in pred_map_cls}
        out["map"] = {thr: calc_map.compute_map(pred_map_cls, gt_map_cls, thr) for thr in (0.25, 0.5)}
    return out


def validate_separate(model, hv, batches, res, category=0, gt_boxes=None, log_scale=True, xyz_factor=1.0, scale_factor=1.0,
                      xyz_component_weights=(1.0, 1.0, 1.0), device_loss=False, overlap_threshold=0.3, **decode_kw):
    """The validation pass of train_separate.py:301-458, validate_joint's twin for the 8-channel model of ONE category.
    ``batches`` yields one scan at a time: ``(id_scan, coords4, feats, sym, scale_labels, obj_labels)``, feats already
    recentred (:316-317), ``sym`` the data.SymBatch of that one scan on the host or on the device.  A scan without a segment
    (``sym.n_segments == 0``, a host int) is skipped as the reference skips it (:310-312): not counted, no entry in
    ``pred_map_cls``, its ground truth unused.  Per scan ONE eval-mode forward under no_grad (its fp16-range check deferred
    behind the decode, as validate_joint's), separate_loss_packed on that output (:322-357; ``device_loss``: its
    ``device_rows``), then pipeline.head_separate and vote, decode and NMS of the one category on the same output - the decode
    of eval_separate.py (its elimination slice and float32 error threshold), which train_separate.py:386,420 shares; the
    detections go into ``pred_map_cls[id_scan]`` as ``(category, box[8,3], score)``.
    Returns validate_joint's dict: ``losses`` = the mean of loss / loss_obj / loss_scale / loss_xyz over the scans that ran
    (read once at the end; NaN without a scan), ``pred_map_cls``, ``n_scans`` and - with ``gt_boxes`` {id_scan: lines} -
    ``map`` = {0.25: ..., 0.5: ...} from calc_map.compute_map over the scans that ran, ground-truth classes from
    data.parse_gt_lines (the reference logs the 0.5 entry's '<category> Average Precision' and '<category> Recall', :455-458).
    The model is put back into the mode it was in; eval-mode BatchNorm leaves the running statistics untouched.  In the middle
    of a training run call finish_pending first: a range flag nobody has read yet means non-finite statistics."""
    from . import hv_cuda, pipeline
    from .data import sym_to_device
    was_training = model.training
    model.eval()
    kw = dict(log_scale=log_scale, xyz_factor=xyz_factor, scale_factor=scale_factor, xyz_component_weights=xyz_component_weights,
              device_rows=device_loss)
    pipeline._separate_defaults(decode_kw)
    pred_map_cls, per_scan = {}, []
    try:
        with torch.no_grad():
            for id_scan, coords4, feats, sym, scale_labels, obj_labels in batches:
                if sym.n_segments == 0:
                    continue
                dev = feats.device
                if sym.rows.device != dev:
                    sym = sym_to_device(sym, dev)
                scale_dev, obj_dev = scale_labels.to(dev, non_blocking=True), obj_labels.to(dev, non_blocking=True)
                scan_points = (coords4[:, 1:].to(dev) * res).float().contiguous()
                hv_cuda.prefetch_geometry(scan_points)
                x = ME.SparseTensor(feats, coords4, device=dev)
                deferred = hasattr(model, "check_range")
                y = model(x, defer_check=True) if deferred else model(x)
                for attempt in range(2):
                    total, parts = separate_loss_packed(y.F, sym, scale_dev, obj_dev, **kw)
                    dets = pipeline._separate_by_calls(hv, scan_points, [pipeline.head_separate(y.F, log_scale)], res, [category],
                                                       overlap_threshold, **decode_kw)
                    # the decode has waited for the stream: the fp16-range flag of the network's convolutions is final now
                    y2 = model.check_range(x, y) if (deferred and attempt == 0) else y
                    if y2 is y:
                        break
                    y = y2
                pred_map_cls[id_scan] = dets
                per_scan.append(torch.stack([total, parts["loss_obj"], parts["loss_scale"], parts["loss_xyz"]]))
    finally:
        model.train(was_training)
    return _validation_result(per_scan, ("loss", "loss_obj", "loss_scale", "loss_xyz"), pred_map_cls, gt_boxes)


def adjust_learning_rate(optimizer, epoch, base_lr=1e-3, decay_steps=(80, 120, 160), decay_rates=(0.1, 0.1, 0.1)):
    lr = base_lr
    for s, r in zip(decay_steps, decay_rates):
        if epoch >= s:
            lr *= r
    for g in optimizer.param_groups:
        g["lr"] = lr
    return lr


def bn_momentum(epoch, decay_step, decay_rate, init=0.5, floor=0.001):
    """train_joint.py:200-201,224: max(0.5 * rate ** (epoch // step), 0.001)"""
    return max(init * decay_rate ** int(epoch / decay_step), floor)


def set_bn_momentum(model, momentum, effective=False):
    """BNMomentumScheduler.step (train_joint.py:86-125).  The reference's setter assigns ``m.momentum`` on every
    ``ME.MinkowskiBatchNorm`` (:94-98) - the WRAPPER, whose forward runs its ``.bn`` (an nn.BatchNorm1d created with
    momentum 0.1): the running statistics of the reference therefore keep updating with 0.1 whatever the schedule
    says.  Default here = the same observable behaviour (the attribute is set on the wrapper, ``.bn`` is untouched);
    ``effective=True`` applies the schedule to ``.bn.momentum`` as its authors presumably intended.  Returns the
    number of modules touched."""
    k = 0
    for m in model.modules():
        if isinstance(m, ME.MinkowskiBatchNorm):
            m.momentum = momentum
            if effective:
                m.bn.momentum = momentum
            k += 1
    return k


def make_optimizer(model, lr=1e-3, weight_decay=0.0):
    """torch.optim.Adam as train_joint.py:219-223 (fused multi-tensor implementation on the GPU)."""
    params = [p for p in model.parameters() if p.requires_grad]
    fused = all(p.is_cuda for p in params)
    return torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, fused=fused)


def make_ddp(model, device, bucket_cap_mb=48):
    """One process per GPU; 37.9 M fp32 gradients = 151 MB per step in ~48 MB buckets so the
    all-reduce of the decoder's gradients overlaps the encoder's backward."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    return DDP(model, device_ids=[device.index], bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True)
