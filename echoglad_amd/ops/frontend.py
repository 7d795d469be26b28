"""The UNet front-end's operators in eval mode (frontend.hip): conv3x3 -> ReLU -> BatchNorm as one launch, whose input may be a
nearest-resized map concatenated with a second one, and the adaptive max pool.  Inference only: neither has a backward."""
from __future__ import annotations

from typing import Optional

import torch

from ._core import _check, _on_current_device, call

MAX_SIDE = 512
MAX_CHANNELS = 512


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


def _bn_parts(bn, c_out: int):
    """(weight, bias, running_mean, running_var, eps) of an nn.BatchNorm2d in eval mode, or of a 5-tuple as it is."""
    if isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        if bn.running_mean is None or bn.running_var is None:
            raise RuntimeError("bn has no running statistics (track_running_stats=False): the eval-mode front-end needs them")
        if bn.training:
            raise RuntimeError("bn is in training mode (batch statistics): conv3x3_relu_bn is inference-only")
        parts = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    else:
        parts = tuple(bn)
        if len(parts) != 5:
            raise RuntimeError("bn must be an nn.BatchNorm2d or a 5-tuple (weight, bias, running_mean, running_var, eps)")
    gamma, beta, mean, var, eps = parts
    if mean is None or var is None:
        raise RuntimeError("bn needs running_mean and running_var")
    for t, name in ((gamma, "bn weight"), (beta, "bn bias"), (mean, "bn running_mean"), (var, "bn running_var")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != c_out):
            raise RuntimeError(f"{name} must be float32 with {c_out} elements, got {tuple(t.shape)} {t.dtype}")
    return gamma, beta, mean, var, float(eps)


def conv3x3_relu_bn(x0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], bn, side: Optional[int] = None,
                    x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BatchNorm_eval(relu(conv3x3(cat([nearest_resize(x0, side), x1], dim=1)) + bias)) -> [batch, c_out, side, side]
    (eg_conv3x3_relu_bn_fwd; zero padding 1).  x0 [batch, c0, side0, side0]; side None: side0 (no resize); x1 [batch, c1, side,
    side] or None; weight [c_out, c0 + c1, 3, 3] as nn.Conv2d holds it; bias [c_out] or None; bn an nn.BatchNorm2d in eval mode
    or (weight, bias, running_mean, running_var, eps) with weight / bias possibly None.  Parameters are read at the call."""
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
    gamma, beta, mean, var, eps = _bn_parts(bn, c_out)
    _no_grad_needed("conv3x3_relu_bn", x0, x1, weight, bias, gamma, beta)
    _check(x0, "x0")
    _on_current_device(x0, "x0")
    for t, name in ((x1, "x1"), (weight, "weight"), (bias, "bias"), (gamma, "bn weight"), (beta, "bn bias"),
                    (mean, "bn running_mean"), (var, "bn running_var")):
        if t is not None:
            _check(t, name, device=x0.device)
    out = torch.empty((batch, c_out, side, side), dtype=torch.float32, device=x0.device)
    call("eg_conv3x3_relu_bn_fwd", x0.detach(), c0, side0, None if x1 is None else x1.detach(), c1, batch, side, weight.detach(),
         None if bias is None else bias.detach(), None if gamma is None else gamma.detach(),
         None if beta is None else beta.detach(), mean, var, eps, c_out, out)
    return out


def adaptive_max_pool(x: torch.Tensor, side_out: int) -> torch.Tensor:
    """nn.AdaptiveMaxPool2d(side_out) of a square NCHW map -> [batch, channels, side_out, side_out] (eg_adaptive_max_pool_fwd)."""
    _square_map(x, "x")
    side_out = int(side_out)
    side_in = int(x.shape[2])
    if not 1 <= side_out <= side_in <= MAX_SIDE:
        raise RuntimeError(f"side_out must be in 1 .. side_in = {side_in} <= {MAX_SIDE}, got {side_out}")
    planes = int(x.shape[0]) * int(x.shape[1])
    if planes < 1:
        raise RuntimeError("x has no planes")
    _no_grad_needed("adaptive_max_pool", x)
    _check(x, "x")
    _on_current_device(x, "x")
    out = torch.empty((x.shape[0], x.shape[1], side_out, side_out), dtype=torch.float32, device=x.device)
    call("eg_adaptive_max_pool_fwd", x.detach(), planes, side_in, side_out, out)
    return out
