"""Losses, criteria and evaluator records on the logits (heatmap.hip): the soft-argmax decode, ExpectedLandmarkMSE, the weighted
BCE on logits or probabilities, the step's criteria as one autograd node, and the device-side evaluators' record kernels."""
from __future__ import annotations

import ctypes as ct
from typing import Optional

import torch

from ._core import _check, _check_rows, _hm_workspace, _level_arrays, _on_current_device, call, raw


def heatmap_expect_fwd(logits: torch.Tensor, batch: int, levels, labels: Optional[torch.Tensor] = None,
                       valid: Optional[torch.Tensor] = None, want_argmax: bool = False):
    """Per (frame, level, channel): softmax-expected (h, w), (max, sum-exp), first arg max, label (h, w), mean(valid).

    levels: [(first row inside a frame's rows, side)]; logits [batch * n_rows, 4].
    Returns dict(expect [B,L,4,2], stats [B,L,4,2], argmax [B,L,4] | None, gt [B,L,4,2] | None, vmean [B,L,4] | None)."""
    if logits.shape[0] % batch:
        raise RuntimeError("logit rows are not a multiple of the batch size")
    n_rows = logits.shape[0] // batch
    _check_rows(logits, "logits", None, 4)
    _check_rows(labels, "labels", logits.shape[0], 4, optional=True)
    _check_rows(valid, "valid", logits.shape[0], 4, optional=True)
    start, side, n = _level_arrays(levels)
    dev = logits.device
    ws = _hm_workspace(dev, "eg_heatmap_workspace_bytes", batch, side, n)
    expect = torch.empty(batch, n, 4, 2, dtype=torch.float32, device=dev)
    stats = torch.empty(batch, n, 4, 2, dtype=torch.float32, device=dev)
    argmax = torch.empty(batch, n, 4, dtype=torch.int64, device=dev) if want_argmax else None
    gt = torch.empty(batch, n, 4, 2, dtype=torch.float32, device=dev) if labels is not None else None
    vmean = torch.empty(batch, n, 4, dtype=torch.float32, device=dev) if valid is not None else None
    call("eg_heatmap_expect_fwd", logits, labels, valid, batch, n_rows, start, side, n, ws, expect, stats, argmax, gt, vmean)
    return {"expect": expect, "stats": stats, "argmax": argmax, "gt": gt, "vmean": vmean}


def heatmap_expect_bwd(logits, expect, stats, d_expect, batch: int, levels) -> torch.Tensor:
    n_rows = logits.shape[0] // batch
    start, side, n = _level_arrays(levels)
    d_logits = torch.empty_like(logits)
    call("eg_heatmap_expect_bwd", logits, expect, stats, d_expect.contiguous(), batch, n_rows, start, side, n, d_logits)
    return d_logits


class _HeatmapExpectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, batch, levels, labels, valid):
        r = heatmap_expect_fwd(logits, batch, levels, labels, valid)
        ctx.save_for_backward(logits, r["expect"], r["stats"])
        ctx.batch, ctx.levels = batch, levels
        gt = r["gt"] if r["gt"] is not None else logits.new_zeros(0)
        vm = r["vmean"] if r["vmean"] is not None else logits.new_zeros(0)
        ctx.mark_non_differentiable(gt, vm)
        return r["expect"], gt, vm

    @staticmethod
    def backward(ctx, d_expect, _dgt, _dvm):
        logits, expect, stats = ctx.saved_tensors
        return heatmap_expect_bwd(logits, expect, stats, d_expect, ctx.batch, ctx.levels), None, None, None, None


def heatmap_expect(logits, batch: int, levels, labels=None, valid=None):
    """(expect, gt, vmean) with autograd through `expect` (d/d logits)."""
    return _HeatmapExpectFn.apply(logits, batch, tuple(levels), labels, valid)


HEATMAP_RENDER_OUTPUTS = ("heat", "pred", "gt", "base")


def heatmap_render(logits: torch.Tensor, batch: int, level, first: int = 0, count: int = 1, labels: Optional[torch.Tensor] = None,
                   image: Optional[torch.Tensor] = None, want=HEATMAP_RENDER_OUTPUTS):
    """The pictures of one level (first row inside a frame's rows, side) of frames first .. first + count - 1 (eg_heatmap_render):
    dict of device tensors, one per name in `want`:
      "heat" float32 [count, side, side, 4]: softmax over the level's rows, exp(x - M) / S;
      "pred" / "gt" / "base" uint8 [count, side, side, 3] (HWC): the frame (0.8 * image, black without one) under the per-channel
      normalised heat maps exp(x - M) / under the labels / alone, in the reference's colours and operation order
      (create_overlay_image + ToPILImage, evaluators.py:595-616), saturating at 255 where the reference's .byte() would wrap.
    logits (and labels: "gt" needs them) float32 [batch * n_rows, 4]; image float32 [batch, C, side, side] (channel 0 is drawn).
    The frames' rows are sliced, not copied; eg_heatmap_expect_fwd on that slice gives the level's
    (M, S), then ONE launch renders: nothing is read back."""
    if logits.shape[0] % batch:
        raise RuntimeError("logit rows are not a multiple of the batch size")
    n_rows = logits.shape[0] // batch
    _check_rows(logits, "logits", None, 4)
    _check_rows(labels, "labels", logits.shape[0], 4, optional=True)
    start, side = int(level[0]), int(level[1])
    first, count = int(first), int(count)
    want = tuple(want)
    if not want or any(w not in HEATMAP_RENDER_OUTPUTS for w in want):
        raise RuntimeError(f"want must name at least one of {HEATMAP_RENDER_OUTPUTS}, got {want}")
    if "gt" in want and labels is None:
        raise RuntimeError('the "gt" image needs labels')
    if count < 1 or first < 0 or first + count > batch:
        raise RuntimeError(f"frames {first} .. {first + count - 1} are not inside a batch of {batch}")
    if side < 1 or start < 0 or start + side * side > n_rows:
        raise RuntimeError(f"level (start {start}, side {side}) is outside the frame's {n_rows} rows")
    dev = logits.device
    stride = 0
    if image is not None:
        if image.dim() != 4 or image.shape[0] != batch or tuple(image.shape[-2:]) != (side, side):
            raise RuntimeError(f"image must be [{batch}, C, {side}, {side}], got {tuple(image.shape)}")
        _check(image, "image", device=dev)
        stride = image.numel() // batch
        image = image[first:first + count]                    # (a view: channel 0 of frame i starts at i * stride)
    lg = logits[first * n_rows:(first + count) * n_rows]
    lb = None if labels is None else labels[first * n_rows:(first + count) * n_rows]
    lg, lb = _aligned16(lg, lb)
    stats = heatmap_expect_fwd(lg, count, [(start, side)])["stats"]
    out = {}
    if "heat" in want:
        out["heat"] = torch.empty(count, side, side, 4, dtype=torch.float32, device=dev)
    for name in ("pred", "gt", "base"):
        if name in want:
            out[name] = torch.empty(count, side, side, 3, dtype=torch.uint8, device=dev)
    call("eg_heatmap_render", lg, lb if "gt" in want else None, image, stride, stats, count, n_rows, start, side,
         out.get("heat"), out.get("pred"), out.get("gt"), out.get("base"))
    return out


def elm_reduce(expect, gt, vmean, inv_side, weight: float):
    """ExpectedLandmarkMSE's combination of the per-(frame, level, channel) expectations and its gradient in one launch
    (eg_elm_reduce) -> (loss [1], d loss / d expect [B, L, 4, 2])."""
    B, L = int(expect.shape[0]), int(expect.shape[1])
    _check(expect, "expect", (B, L, 4, 2))
    _check(gt, "gt", (B, L, 4, 2))
    _check(vmean, "vmean", (B, L, 4))
    _check(inv_side, "inv_side", numel=L)           # one value per level
    loss = torch.empty(1, dtype=torch.float32, device=expect.device)
    d = torch.empty_like(expect)
    call("eg_elm_reduce", expect, gt, vmean, inv_side, B, L, weight, loss, d)
    return loss, d


def bce_logits_fwd(logits, labels, valid, ones_weight: float) -> torch.Tensor:
    """[sum(w * bce * valid), sum(valid), ratio] as a float32 device tensor (no host sync)."""
    return _bce_fwd(logits, labels, valid, ones_weight, False)


def bce_probs_fwd(probs, labels, valid, ones_weight: float) -> torch.Tensor:
    """bce_logits_fwd for probabilities (nn.BCELoss's element formula; an element outside [0, 1] makes the loss NaN)."""
    return _bce_fwd(probs, labels, valid, ones_weight, True)


def _aligned16(*tensors):
    """The kernels read 16 bytes per lane: a contiguous view at an odd element offset (flat[1:], a slice of a packed buffer) is copied."""
    return tuple(t if t is None or t.data_ptr() % 16 == 0 else t.clone() for t in tensors)


def _bce_fwd(logits, labels, valid, ones_weight: float, probs: bool) -> torch.Tensor:
    _check(logits, "probs" if probs else "logits")
    _check(labels, "labels")
    if labels.numel() != logits.numel() or (valid is not None and valid.numel() != logits.numel()):
        raise RuntimeError("logits, labels and valid must have the same number of elements")
    logits, labels, valid = _aligned16(logits, labels, valid)
    ws = _hm_workspace(logits.device, "eg_heatmap_workspace_bytes", 1, (ct.c_int * 1)(1), 1)
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    call("eg_bce_probs_fwd" if probs else "eg_bce_logits_fwd", logits, labels, valid, logits.numel(), ones_weight, ws, out)
    return out


class _BCELogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, valid, ones_weight, probs=False):
        out = _bce_fwd(logits, labels, valid, ones_weight, probs)
        ctx.save_for_backward(logits, labels, valid if valid is not None else logits.new_zeros(0), out)
        ctx.ones_weight, ctx.has_valid, ctx.probs = ones_weight, valid is not None, probs
        return out[2]

    @staticmethod
    def backward(ctx, g):
        logits, labels, valid, out = ctx.saved_tensors
        scale = (g / out[1]).reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(logits)
        call("eg_bce_probs_bwd" if ctx.probs else "eg_bce_logits_bwd", logits, labels, valid if ctx.has_valid else None,
             logits.numel(), ctx.ones_weight, scale, dx)
        return dx, None, None, None, None


def bce_logits(logits, labels, valid=None, ones_weight: float = 1.0) -> torch.Tensor:
    """sum(w * bce_with_logits(x, y) * valid) / sum(valid), w = ones_weight where y == 1 (autograd wrt logits)."""
    return _BCELogitsFn.apply(logits, labels, valid, float(ones_weight))


def bce_probs(probs, labels, valid=None, ones_weight: float = 1.0) -> torch.Tensor:
    """sum(w * bce(p, y) * valid) / sum(valid) on probabilities (nn.BCELoss's element formula: log clamped at -100, gradient
    (p - y) / max((1 - p) p, 1e-12)), w = ones_weight where y == 1 (autograd wrt probs).  torch raises for p outside [0, 1]; the
    kernel cannot (it may be captured into a graph): such an element makes the result NaN, whatever its valid."""
    return _BCELogitsFn.apply(probs, labels, valid, float(ones_weight), True)


# ---------------------------------------------------------------------------
# the device-side evaluators' records
# ---------------------------------------------------------------------------
CONFUSION_MAX_CHANNELS = 8
CONFUSION_WORKSPACE_BYTES = 512 * CONFUSION_MAX_CHANNELS * 32      # the full grid of eg_confusion_counts at any channel count


def _check_counter(counter, device) -> None:
    _check(counter, "counter", dtype=torch.int64, numel=1, device=device)


def confusion_counts(pred: torch.Tensor, y: torch.Tensor, valid: torch.Tensor, history: torch.Tensor, counter: torch.Tensor,
                     workspace: torch.Tensor) -> None:
    """Append one record of per-channel confusion counts {TP, FN, FP, TN} over the rows with valid > 0 (prediction positive iff
    pred > 0.5, label positive iff y != 0) to ``history[counter]`` and advance ``counter`` -- ONE launch on the current stream, no
    host synchronisation, no allocation.  pred / y / valid: contiguous CUDA float32 [rows, C], 1 <= C <= 8; history: int64
    [capacity, C, 4]; counter: int64 [1]; workspace: CONFUSION_WORKSPACE_BYTES bytes, not shared with another stream's launch.
    Past capacity nothing is written but the counter still advances."""
    _check(pred, "pred", (None, None))
    _on_current_device(pred, "pred")
    if not 1 <= pred.shape[1] <= CONFUSION_MAX_CHANNELS or pred.shape[0] < 1:
        raise RuntimeError(f"pred must be [rows >= 1, 1..{CONFUSION_MAX_CHANNELS}], got {tuple(pred.shape)}")
    rows, ch = pred.shape
    dev = pred.device
    _check(y, "y", (rows, ch), device=dev)
    _check(valid, "valid", (rows, ch), device=dev)
    _check(history, "history", (None, ch, 4), dtype=torch.int64, device=dev)
    if history.shape[0] < 1:
        raise RuntimeError("history must hold at least one record")
    _check_counter(counter, dev)
    _check(workspace, "workspace", dtype=torch.uint8, device=dev)
    if workspace.numel() < CONFUSION_WORKSPACE_BYTES:
        raise RuntimeError(f"workspace must be uint8 with at least {CONFUSION_WORKSPACE_BYTES} bytes")
    call("eg_confusion_counts", pred, y, valid, rows, ch, workspace, workspace.numel(), history, history.shape[0], counter)


LANDMARK_RECORD_FLOATS = 16         # eg_landmark_record_*: one record of the history
LANDMARK_DETAIL_FLOATS = 24         # ... and one frame of its detail block


def landmark_record_workspace_bytes(batch: int, frame: int) -> int:
    return int(raw("eg_landmark_record_workspace_bytes", int(batch), int(frame)))


def _check_record_buffers(device, batch: int, pix2mm_x, pix2mm_y, history, detail, counter) -> None:
    _check(pix2mm_x, "pix2mm_x", numel=batch, device=device)           # one value per frame
    _check(pix2mm_y, "pix2mm_y", numel=batch, device=device)
    _check(history, "history", (None, LANDMARK_RECORD_FLOATS), device=device)
    if history.shape[0] < 1:
        raise RuntimeError("history must hold at least one record")
    _check(detail, "detail", (history.shape[0], batch, LANDMARK_DETAIL_FLOATS), device=device)
    _check_counter(counter, device)


def landmark_record_hm(logits, labels, valid, batch: int, frame: int, pix2mm_x, pix2mm_y, history, detail, counter, workspace) -> None:
    """Append one landmark-evaluator record (the main grid's decode -> coordinate errors, valid flags, width MAE / MPE, per-frame
    detail) of a heat-map model to ``history[counter]`` / ``detail[counter]`` and advance ``counter`` -- two launches on the current
    stream (eg_landmark_record_hm), no host synchronisation, no allocation.  logits / labels / valid: contiguous CUDA float32
    [batch * n_rows, 4]; pix2mm_x / pix2mm_y: CUDA float32 [batch]; history float32 [capacity, 16]; detail float32
    [capacity, batch, 24]; counter int64 [1]; workspace: uint8, ``landmark_record_workspace_bytes(batch, frame)`` bytes or more,
    not shared with another stream's launch.  Past capacity nothing is written but the counter still advances."""
    if logits.shape[0] % batch:
        raise RuntimeError(f"{logits.shape[0]} logit rows is not a multiple of the batch size {batch}")
    _check_rows(logits, "logits", None, 4)
    _check_rows(labels, "labels", logits.shape[0], 4)
    _check_rows(valid, "valid", logits.shape[0], 4)
    _check_record_buffers(logits.device, batch, pix2mm_x, pix2mm_y, history, detail, counter)
    _check(workspace, "workspace", dtype=torch.uint8, device=logits.device)
    call("eg_landmark_record_hm", logits, labels, valid, batch, logits.shape[0] // batch, frame, pix2mm_x, pix2mm_y, workspace,
         workspace.numel(), history, detail, history.shape[0], counter)


def landmark_record_coord(coord_pred, coord_y, batch: int, pix2mm_x, pix2mm_y, history, detail, counter) -> None:
    """landmark_record_hm for a coordinate-graph model: the record from the predicted and labelled (h, w) of the 4 landmarks of every
    frame (contiguous CUDA float32 [batch * 4, 2]), every landmark valid -- one launch (eg_landmark_record_coord)."""
    _check(coord_pred, "coord_pred", numel=batch * 8)           # batch x 4 (h, w) pairs
    _check(coord_y, "coord_y", numel=batch * 8)
    _on_current_device(coord_pred, "coord_pred")
    _check_record_buffers(coord_pred.device, batch, pix2mm_x, pix2mm_y, history, detail, counter)
    call("eg_landmark_record_coord", coord_pred, coord_y, batch, pix2mm_x, pix2mm_y, history, detail, history.shape[0], counter)


# ---------------------------------------------------------------------------
# the step's criteria as one autograd node
# ---------------------------------------------------------------------------
class _CriteriaFn(torch.autograd.Function):
    """WeightedBCEWithLogitsLoss or WeightedBCE + ExpectedLandmarkMSE (+ MSE or MAE on the landmark coordinates) of one training step
    as ONE autograd node over eg_criteria_ex_fwd / eg_criteria_ex_bwd: (logits [B*n,4], coord_pred [R,2] | None) -> (total, bce, elm,
    coord | None), every output a 0-d tensor that can be backpropagated on its own or summed (engine.py:582-600, :271)."""

    @staticmethod
    def forward(ctx, logits, coord_pred, labels, valid, coord_y, batch, levels, inv_side, ones_weight, w_bce, w_elm, w_coord, bce_on_probs,
                coord_l1):
        dev = logits.device
        n_rows = logits.shape[0] // batch
        start, side, n = _level_arrays(levels)
        ws = _hm_workspace(dev, "eg_criteria_workspace_bytes", batch, side, n)
        expect = torch.empty(batch, n, 4, 2, dtype=torch.float32, device=dev)
        stats = torch.empty_like(expect)
        d_expect = torch.empty_like(expect)
        has_coord = coord_pred is not None
        cp = coord_pred.contiguous() if has_coord else None
        cy = coord_y.to(torch.float32).contiguous() if has_coord else None
        d_coord = torch.empty_like(cp) if has_coord else None
        bce_scale = torch.empty(1, dtype=torch.float32, device=dev)
        total, vb, ve = (torch.empty((), dtype=torch.float32, device=dev) for _ in range(3))
        vc = torch.empty((), dtype=torch.float32, device=dev) if has_coord else None
        call("eg_criteria_ex_fwd", logits, labels, valid, batch, n_rows, start, side, n, inv_side, ones_weight, w_bce, w_elm, cp, cy,
             cp.numel() if has_coord else 0, w_coord, ws, expect, stats, d_expect, d_coord, bce_scale, total, vb, ve, vc,
             bce_on_probs, coord_l1)
        ctx.meta = (batch, levels, ones_weight, has_coord, int(bce_on_probs), int(coord_l1))
        ctx.save_for_backward(logits, labels, valid, expect, stats, d_expect, bce_scale, d_coord if has_coord else logits.new_zeros(0))
        ctx.set_materialize_grads(False)
        return total, vb, ve, vc

    @staticmethod
    def backward(ctx, g_total, g_bce, g_elm, g_coord):
        logits, labels, valid, expect, stats, d_expect, bce_scale, d_coord = ctx.saved_tensors
        batch, levels, ones_weight, has_coord, bce_on_probs, coord_l1 = ctx.meta
        start, side, n = _level_arrays(levels)
        gs = [None if g is None else g.to(torch.float32).reshape(1).contiguous() for g in (g_total, g_bce, g_elm, g_coord)]
        d_logits = torch.empty_like(logits)
        want_coord = has_coord and ctx.needs_input_grad[1]
        d_coord_out = torch.empty_like(d_coord) if want_coord else None
        call("eg_criteria_ex_bwd", logits, labels, valid, batch, logits.shape[0] // batch, start, side, n, ones_weight, expect, stats,
             d_expect, bce_scale, d_coord if want_coord else None, d_coord.numel() if want_coord else 0, *gs, d_logits, d_coord_out,
             bce_on_probs, coord_l1)
        return (d_logits, d_coord_out) + (None,) * 12


def landmark_criteria(logits, labels, valid, batch: int, levels, inv_side, ones_weight: float, w_bce: float, w_elm: float,
                      coord_pred=None, coord_y=None, w_coord: float = 1.0, bce_on_probs: bool = False, coord_l1: bool = False):
    """-> (total, bce, elm, coord | None): the step's criteria as one autograd node (5 launches forward + backward).
    bce_on_probs: the BCE term is WeightedBCE's on probabilities (bce_probs) instead of WeightedBCEWithLogitsLoss's; coord_l1: the
    coordinate term is MAE (w_coord * mean|coord_pred - coord_y|) instead of MSE."""
    for name, t in (("logits", logits), ("labels", labels), ("valid", valid)):
        _check_rows(t, name, logits.shape[0], 4)
    logits, labels, valid = _aligned16(logits, labels, valid)
    return _CriteriaFn.apply(logits, coord_pred, labels, valid, coord_y, int(batch), levels, inv_side, float(ones_weight), float(w_bce),
                             float(w_elm), float(w_coord), bool(bce_on_probs), bool(coord_l1))
