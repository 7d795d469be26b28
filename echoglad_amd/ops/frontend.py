"""The UNet front-end's operators: conv3x3 -> ReLU -> BatchNorm, whose input may be a nearest-resized map concatenated with a second
one, and the adaptive max pool.  `conv3x3_relu_bn` / `adaptive_max_pool` are the eval-mode forward, one launch each, inference only;
`conv3x3_relu_bn_train` / `adaptive_max_pool_train` are the training-mode block with batch statistics and the pool, each with a
backward.  Both modes check their arguments with the same helpers (`_conv_args`, `_bn_parts`, `_on_device`, `_pool_args`)."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from ._core import _check, _on_current_device, _scratch, call, raw

MAX_SIDE = 512
MAX_CHANNELS = 512
MAX_ENLARGEMENT = 16        # training mode: the resize backward adds a source pixel's destination block in one chain: <= 16 x 16 terms


def _no_grad_needed(what: str, *tensors) -> None:
    """Inference only: with autograd recording, no input may ask for a gradient (there is no backward to give it)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is inference-only and has no backward: call it under torch.no_grad(), or detach the inputs "
                           "and parameters that require grad")


def _square_map(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[2] != t.shape[3] or t.shape[2] < 1:
        raise RuntimeError(f"{name} must be a square NCHW map [batch, channels, side, side], got "
                           f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor, got {t.dtype}, contiguous = {t.is_contiguous()}")


def _conv_args(x0, weight, bias, side, x1):
    """The shape, dtype and limit checks both convolution operators make -> (batch, c0, side0, side, c1, c_out)."""
    _square_map(x0, "x0")
    batch, c0, side0 = int(x0.shape[0]), int(x0.shape[1]), int(x0.shape[2])
    side = side0 if side is None else int(side)
    c1 = 0
    if x1 is not None:
        _square_map(x1, "x1")
        if x1.shape[0] != batch or x1.shape[2] != side:
            raise RuntimeError(f"x1 must be [{batch}, *, {side}, {side}] next to x0 {tuple(x0.shape)} at side {side}, got {tuple(x1.shape)}")
        c1 = int(x1.shape[1])
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise RuntimeError(f"weight must be [c_out, c_in, 3, 3], got {tuple(weight.shape)}")
    if weight.dtype != torch.float32 or not weight.is_contiguous():
        raise RuntimeError(f"weight must be a contiguous float32 tensor, got {weight.dtype}")
    c_out = int(weight.shape[0])
    if weight.shape[1] != c0 + c1:
        raise RuntimeError(f"weight takes {weight.shape[1]} input channels but the sources bring c0 + c1 = {c0} + {c1}")
    if batch < 1 or not 1 <= side <= MAX_SIDE or side0 > MAX_SIDE or not 1 <= c0 + c1 <= MAX_CHANNELS or not 1 <= c_out <= MAX_CHANNELS:
        raise RuntimeError(f"batch >= 1, sides 1 .. {MAX_SIDE} and channels 1 .. {MAX_CHANNELS} are covered, got batch {batch}, "
                           f"sides {side0} -> {side}, channels {c0} + {c1} -> {c_out}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != c_out):
        raise RuntimeError(f"bias must be float32 with {c_out} elements, got {tuple(bias.shape)} {bias.dtype}")
    return batch, c0, side0, side, c1, c_out


def _bn_parts(bn, c_out: int, training: bool):
    """(weight, bias, running_mean, running_var, eps, momentum, module or None) of an nn.BatchNorm2d that is in the mode asked for,
    or of a tuple as it is: 5 entries in eval mode (momentum comes back None), 6 with the momentum in training mode."""
    module = None
    if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        if training:
            if not bn.training:
                raise RuntimeError("bn is in eval mode (running statistics): conv3x3_relu_bn_train takes a BatchNorm in training mode; "
                                   "conv3x3_relu_bn is the eval-mode operator")
            if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
                raise NotImplementedError("conv3x3_relu_bn_train: a BatchNorm with track_running_stats=False is not covered")
        else:
            if bn.running_mean is None or bn.running_var is None:
                raise RuntimeError("bn has no running statistics (track_running_stats=False): the eval-mode front-end needs them")
            if bn.training:
                raise RuntimeError("bn is in training mode (batch statistics): conv3x3_relu_bn is inference-only")
        parts = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps) + ((bn.momentum,) if training else ())
        module = bn
    else:
        parts = tuple(bn)
        if len(parts) != (6 if training else 5):
            raise RuntimeError("bn must be an nn.BatchNorm2d or a " + ("6-tuple (weight, bias, running_mean, running_var, eps, momentum)"
                                                                       if training else "5-tuple (weight, bias, running_mean, running_var, eps)"))
    if training and parts[5] is None:
        raise NotImplementedError("conv3x3_relu_bn_train: momentum=None (a cumulative moving average) is not covered")
    gamma, beta, mean, var, eps = parts[:5]
    if not training and (mean is None or var is None):
        raise RuntimeError("bn needs running_mean and running_var")
    for t, name in ((gamma, "bn weight"), (beta, "bn bias"), (mean, "bn running_mean"), (var, "bn running_var")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != c_out):
            raise RuntimeError(f"{name} must be float32 with {c_out} elements, got {tuple(t.shape)} {t.dtype}")
    return gamma, beta, mean, var, float(eps), float(parts[5]) if training else None, module


def _on_device(first, name: str, *others) -> None:
    """`first` is a tensor of the current device the kernels take; every (tensor, name) after it that is given sits there with it."""
    _check(first, name)
    _on_current_device(first, name)
    for t, other in others:
        if t is not None:
            _check(t, other, device=first.device)


def _conv_on_device(x0, x1, weight, bias, gamma, beta, mean, var) -> None:
    _on_device(x0, "x0", (x1, "x1"), (weight, "weight"), (bias, "bias"), (gamma, "bn weight"), (beta, "bn bias"),
               (mean, "bn running_mean"), (var, "bn running_var"))


def _pool_args(x, side_out) -> int:
    """The checks both pools make -> side_out."""
    _square_map(x, "x")
    side_out, side_in = int(side_out), int(x.shape[2])
    if not 1 <= side_out <= side_in <= MAX_SIDE:
        raise RuntimeError(f"side_out must be in 1 .. side_in = {side_in} <= {MAX_SIDE}, got {side_out}")
    if int(x.shape[0]) * int(x.shape[1]) < 1:
        raise RuntimeError("x has no planes")
    return side_out


def conv3x3_relu_bn(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], bn, side: Optional[int] = None,
                    x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BatchNorm_eval(relu(conv3x3(cat([nearest_resize(x0, side), x1], dim=1)) + bias)) -> [batch, c_out, side, side]
    (eg_conv3x3_relu_bn_fwd; zero padding 1).  x0 [batch, c0, side0, side0]; side None: side0 (no resize); x1 [batch, c1, side,
    side] or None; weight [c_out, c0 + c1, 3, 3] as nn.Conv2d holds it; bias [c_out] or None; bn an nn.BatchNorm2d in eval mode
    or (weight, bias, running_mean, running_var, eps) with weight / bias possibly None.  Parameters are read at the call."""
    batch, c0, side0, side, c1, c_out = _conv_args(x0, weight, bias, side, x1)
    gamma, beta, mean, var, eps, _, _ = _bn_parts(bn, c_out, training=False)
    _no_grad_needed("conv3x3_relu_bn", x0, x1, weight, bias, gamma, beta)
    _conv_on_device(x0, x1, weight, bias, gamma, beta, mean, var)
    out = torch.empty((batch, c_out, side, side), dtype=torch.float32, device=x0.device)
    call("eg_conv3x3_relu_bn_fwd", x0.detach(), c0, side0, None if x1 is None else x1.detach(), c1, batch, side, weight.detach(),
         None if bias is None else bias.detach(), None if gamma is None else gamma.detach(),
         None if beta is None else beta.detach(), mean, var, eps, c_out, out)
    return out


def adaptive_max_pool(x: torch.Tensor, side_out: int) -> torch.Tensor:
    """nn.AdaptiveMaxPool2d(side_out) of a square NCHW map -> [batch, channels, side_out, side_out] (eg_adaptive_max_pool_fwd)."""
    side_out = _pool_args(x, side_out)
    _no_grad_needed("adaptive_max_pool", x)
    _on_device(x, "x")
    out = torch.empty((x.shape[0], x.shape[1], side_out, side_out), dtype=torch.float32, device=x.device)
    call("eg_adaptive_max_pool_fwd", x.detach(), int(x.shape[0]) * int(x.shape[1]), int(x.shape[2]), side_out, out)
    return out


# ---------------------------------------------------------------------------
# training mode
# ---------------------------------------------------------------------------
def _train_workspace(device, batch: int, c_in: int, c_out: int, side: int) -> torch.Tensor:
    """The block's workspace (eg_frontend_train_workspace_bytes): chunk statistics and the weight gradient's slices."""
    return _scratch("frontend_train", device, max(int(raw("eg_frontend_train_workspace_bytes", batch, c_in, c_out, side)), 256))


class _Conv3x3ReluBnTrain(torch.autograd.Function):
    """y = BatchNorm_train(relu(conv3x3(cat([resize(x0), x1])) + bias)).  Saved: r = relu(...), the batch mean and 1 / std, and
    references to x0, x1, weight and gamma -- never y, never an upsampled or concatenated map."""

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, gamma, beta, stats, eps, momentum, side):
        batch, c0, side0 = int(x0.shape[0]), int(x0.shape[1]), int(x0.shape[2])
        c1 = 0 if x1 is None else int(x1.shape[1])
        c_out = int(weight.shape[0])
        dev = x0.device
        r = torch.empty((batch, c_out, side, side), dtype=torch.float32, device=dev)
        y = torch.empty_like(r)
        save_mean = torch.empty(c_out, dtype=torch.float32, device=dev)
        save_invstd = torch.empty(c_out, dtype=torch.float32, device=dev)
        ws = _train_workspace(dev, batch, c0 + c1, c_out, side)
        det = lambda t: None if t is None else t.detach()
        call("eg_conv3x3_relu_fwd", det(x0), c0, side0, det(x1), c1, batch, side, det(weight), det(bias), c_out, r)
        call("eg_bn2d_train_fwd", r, batch, c_out, side, det(gamma), det(beta), eps, momentum, stats[0], stats[1], ws, y, save_mean,
             save_invstd)
        ctx.save_for_backward(x0, x1, weight, gamma, r, save_mean, save_invstd)
        ctx.has_bias, ctx.has_beta, ctx.side = bias is not None, beta is not None, side
        return y

    @staticmethod
    @once_differentiable                    # a double backward raises
    def backward(ctx, dy):
        x0, x1, weight, gamma, r, save_mean, save_invstd = ctx.saved_tensors
        need_x0, need_x1, need_w, need_b, need_g, need_be = ctx.needs_input_grad[:6]
        batch, c0, side0 = int(x0.shape[0]), int(x0.shape[1]), int(x0.shape[2])
        c1 = 0 if x1 is None else int(x1.shape[1])
        c_out, side, dev = int(weight.shape[0]), ctx.side, x0.device
        dy = dy.contiguous()
        if dy.dtype != torch.float32 or dy.shape != r.shape:
            raise RuntimeError(f"conv3x3_relu_bn_train backward: dy must be float32 {tuple(r.shape)}, got {dy.dtype} {tuple(dy.shape)}")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ws = _train_workspace(dev, batch, c0 + c1, c_out, side)
        dz = torch.empty_like(r)
        dgamma = new(c_out) if need_g and gamma is not None else None
        dbeta = new(c_out) if need_be and ctx.has_beta else None
        dbias = new(c_out) if need_b and ctx.has_bias else None
        call("eg_relu_bn2d_bwd", dy, r, save_mean, save_invstd, gamma, batch, c_out, side, ws, dz, dgamma, dbeta, dbias)
        dx0 = dx1 = dw = None
        need_x1 = need_x1 and x1 is not None
        if need_x0 or need_x1:
            dx0 = torch.empty_like(x0) if need_x0 else None
            dx1 = torch.empty_like(x1) if need_x1 else None
            full = new(batch, c0, side, side) if need_x0 and side0 != side else None
            call("eg_conv3x3_bwd_data", dz, weight, batch, c_out, side, c0, side0, c1, dx0, dx1, full)
        if need_w:
            dw = torch.empty_like(weight)
            call("eg_conv3x3_bwd_weight", x0, c0, side0, x1, c1, batch, side, dz, c_out, ws, dw)
        return dx0, dx1, dw, dbias, dgamma, dbeta, None, None, None, None


def conv3x3_relu_bn_train(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], bn, side: Optional[int] = None,
                          x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BatchNorm_train(relu(conv3x3(cat([nearest_resize(x0, side), x1], dim=1)) + bias)) -> [batch, c_out, side, side], with a
    backward (gradients of x0, x1, weight, bias and the BatchNorm's weight and bias, each only where it is asked for).  The
    arguments are `conv3x3_relu_bn`'s; bn is an nn.BatchNorm2d in TRAINING mode -- its running statistics and
    num_batches_tracked move as nn.BatchNorm2d moves them -- or (weight, bias, running_mean | None, running_var | None, eps,
    momentum).  3 launches forward (eg_conv3x3_relu_fwd, eg_bn2d_train_fwd), up to 7 backward; bit-reproducible, capturable."""
    batch, c0, side0, side, c1, c_out = _conv_args(x0, weight, bias, side, x1)
    if -(-side // side0) > MAX_ENLARGEMENT:
        raise RuntimeError(f"enlargements above {MAX_ENLARGEMENT} x are not covered in training mode, got {side0} -> {side}")
    gamma, beta, mean, var, eps, momentum, module = _bn_parts(bn, c_out, training=True)
    if batch * side * side == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(batch, c_out, side, side)}")
    _conv_on_device(x0, x1, weight, bias, gamma, beta, mean, var)
    y = _Conv3x3ReluBnTrain.apply(x0, x1, weight, bias, gamma, beta, (mean, var), eps, momentum, side)
    if module is not None and module.num_batches_tracked is not None:
        module.num_batches_tracked.add_(1)
    return y


class _AdaptiveMaxPoolTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, side_out):
        planes, side_in = int(x.shape[0]) * int(x.shape[1]), int(x.shape[2])
        out = torch.empty((x.shape[0], x.shape[1], side_out, side_out), dtype=torch.float32, device=x.device)
        idx = torch.empty(out.shape, dtype=torch.int32, device=x.device)
        call("eg_adaptive_max_pool_idx_fwd", x.detach(), planes, side_in, side_out, out, idx)
        ctx.save_for_backward(idx)
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype != torch.float32 or dy.shape != idx.shape:
            raise RuntimeError(f"adaptive_max_pool_train backward: dy must be float32 {tuple(idx.shape)}, got {dy.dtype} {tuple(dy.shape)}")
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        call("eg_adaptive_max_pool_bwd", dy, idx, ctx.shape[0] * ctx.shape[1], ctx.shape[2], int(idx.shape[2]), dx)
        return dx, None


def adaptive_max_pool_train(x: torch.Tensor, side_out: int) -> torch.Tensor:
    """`adaptive_max_pool` (the same kernel, the same bits) with a backward: the forward also writes every window's first maximum
    in row-major order (eg_adaptive_max_pool_idx_fwd), the backward gathers (eg_adaptive_max_pool_bwd)."""
    side_out = _pool_args(x, side_out)
    _on_device(x, "x")
    return _AdaptiveMaxPoolTrain.apply(x, side_out)
