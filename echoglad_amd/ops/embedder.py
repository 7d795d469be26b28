"""The CNN embedder's residual block (the reference's CNNResBlock with kernel 3 and pool 1): conv3x3 -> BatchNorm2d -> + residual
(1 x 1 convolution, or the input itself) -> ReLU -> Dropout2d.  `embed_block` is the eval-mode forward, one launch, inference only;
`embed_block_train` is the training-mode block with batch statistics, a plane mask and a backward; `pyramid_block` is the
CNN-pyramid variant's eval-mode block (128 -> 128 channels, identity residual, an adaptive max pool behind it) and
`pyramid_block_train` that block in training mode with its backward.  Arguments are checked with the
front-end's helpers (`_conv_args`, `_bn_parts`, `_on_device`)."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from ._core import _scratch, _seed, call, raw
from .frontend import _bn_parts, _conv_args, _no_grad_needed, _on_device, _train_workspace

MAX_CHANNELS = 128


def _block_args(x, conv_w, conv_b, one_w, one_b):
    """The checks both modes make -> (batch, c_in, c_out, side)."""
    batch, c_in, _, side, _, c_out = _conv_args(x, conv_w, conv_b, None, None)
    if c_in > MAX_CHANNELS or c_out > MAX_CHANNELS:
        raise RuntimeError(f"the embedder block covers channels 1 .. {MAX_CHANNELS}, got {c_in} -> {c_out}")
    if one_w is None:
        if c_in != c_out:
            raise RuntimeError(f"one_w must be given where c_in != c_out ({c_in} -> {c_out}): there is no identity residual")
        if one_b is not None:
            raise RuntimeError("one_b without one_w")
    else:
        if not isinstance(one_w, torch.Tensor) or one_w.dtype != torch.float32 or not one_w.is_contiguous() or \
                one_w.numel() != c_out * c_in or tuple(one_w.shape[:2]) != (c_out, c_in):
            raise RuntimeError(f"one_w must be a contiguous float32 [{c_out}, {c_in}, 1, 1], got {tuple(one_w.shape)} {one_w.dtype}")
        if one_b is not None and (one_b.dtype != torch.float32 or one_b.numel() != c_out):
            raise RuntimeError(f"one_b must be float32 with {c_out} elements, got {tuple(one_b.shape)} {one_b.dtype}")
    return batch, c_in, c_out, side


def _block_on_device(x, conv_w, conv_b, one_w, one_b, gamma, beta, mean, var) -> None:
    _on_device(x, "x", (conv_w, "conv_w"), (conv_b, "conv_b"), (one_w, "one_w"), (one_b, "one_b"), (gamma, "bn weight"),
               (beta, "bn bias"), (mean, "bn running_mean"), (var, "bn running_var"))


def _det(t):
    return None if t is None else t.detach()


def embed_block(x: torch.Tensor, conv_w: torch.Tensor, conv_b: Optional[torch.Tensor], bn, one_w: Optional[torch.Tensor] = None,
                one_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu(BatchNorm_eval(conv3x3(x) + conv_b) + r) -> [batch, c_out, side, side] in ONE launch (eg_embed_block_fwd), r = the 1 x 1
    convolution (one_w [c_out, c_in, 1, 1], one_b) of x, or x itself where one_w is None (c_in == c_out).  x [batch, c_in, side, side];
    conv_w [c_out, c_in, 3, 3] as nn.Conv2d holds it; bn an nn.BatchNorm2d in eval mode or (weight, bias, running_mean, running_var,
    eps).  Dropout2d is the identity in eval mode.  Parameters are read at the call."""
    batch, c_in, c_out, side = _block_args(x, conv_w, conv_b, one_w, one_b)
    gamma, beta, mean, var, eps, _, _ = _bn_parts(bn, c_out, training=False)
    _no_grad_needed("embed_block", x, conv_w, conv_b, one_w, one_b, gamma, beta)
    _block_on_device(x, conv_w, conv_b, one_w, one_b, gamma, beta, mean, var)
    out = torch.empty((batch, c_out, side, side), dtype=torch.float32, device=x.device)
    call("eg_embed_block_fwd", x.detach(), batch, c_in, side, conv_w.detach(), _det(conv_b), _det(gamma), _det(beta), mean, var, eps,
         _det(one_w), _det(one_b), c_out, out)
    return out


def pyramid_block(x: torch.Tensor, conv_w: torch.Tensor, conv_b: Optional[torch.Tensor], bn, side_out: int) -> torch.Tensor:
    """relu(AdaptiveMaxPool2d(side_out)(BatchNorm_eval(conv3x3(x) + conv_b) + x)) -> [batch, 128, side_out, side_out]
    (eg_pyramid_block_fwd): the CNN-pyramid variant's block, 128 -> 128 channels with the input itself as the residual.  The
    arguments are `embed_block`'s and are checked the same way; 1 <= side_out <= side.  Sides from 4 on run the convolution on the
    f32-input matrix instruction, smaller ones on `embed_block`'s kernel; the result equals
    adaptive_max_pool(embed_block(x, conv_w, conv_b, bn), side_out) bit for bit at every side.  Where side_out != side the full-size
    map goes through a scratch buffer of its own kind ("pyramid": batch * 128 * side^2 floats, grown, never shrunk)."""
    batch, side, side_out = _pyramid_args(x, conv_w, conv_b, side_out)
    c_out = MAX_CHANNELS
    gamma, beta, mean, var, eps, _, _ = _bn_parts(bn, c_out, training=False)
    _no_grad_needed("pyramid_block", x, conv_w, conv_b, gamma, beta)
    _block_on_device(x, conv_w, conv_b, None, None, gamma, beta, mean, var)
    nbytes = int(raw("eg_pyramid_block_scratch_bytes", batch, side, side_out))
    scratch = _scratch("pyramid", x.device, nbytes) if nbytes else None
    out = torch.empty((batch, c_out, side_out, side_out), dtype=torch.float32, device=x.device)
    call("eg_pyramid_block_fwd", x.detach(), batch, side, conv_w.detach(), _det(conv_b), _det(gamma), _det(beta), mean, var, eps,
         side_out, scratch, out)
    return out


def _pyramid_args(x, conv_w, conv_b, side_out):
    """The checks both pyramid blocks make -> (batch, side, side_out)."""
    batch, c_in, c_out, side = _block_args(x, conv_w, conv_b, None, None)
    if c_in != MAX_CHANNELS or c_out != MAX_CHANNELS:
        raise RuntimeError(f"the pyramid block covers {MAX_CHANNELS} -> {MAX_CHANNELS} channels, got {c_in} -> {c_out}")
    side_out = int(side_out)
    if not 1 <= side_out <= side:
        raise RuntimeError(f"side_out must be in 1 .. side = {side}, got {side_out}")
    return batch, side, side_out


def _pyramid_workspace(device, batch: int, side: int, side_out: int) -> torch.Tensor:
    """One workspace for a training-mode pyramid block (eg_pyramid_train_workspace_bytes): the chunk sums of the BatchNorm in both
    directions and the weight gradient's slices, at most 64 of them whatever the batch and the side."""
    return _scratch("pyramid_train", device, max(int(raw("eg_pyramid_train_workspace_bytes", batch, side, side_out)), 256))


class _PyramidBlockTrain(torch.autograd.Function):
    """Saved: x, z, idx and out (pooled), keep, the batch mean and 1 / std, and references to the parameters -- never y, never
    v = y + x or any other full-size map."""

    @staticmethod
    def forward(ctx, x, conv_w, conv_b, gamma, beta, stats, eps, momentum, side_out, p, seed):
        batch, side, dev, C = int(x.shape[0]), int(x.shape[2]), x.device, MAX_CHANNELS
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        z, y, out = new(batch, C, side, side), new(batch, C, side, side), new(batch, C, side_out, side_out)
        idx = torch.empty((batch, C, side_out, side_out), dtype=torch.int32, device=dev)
        save_mean, save_invstd, keep = new(C), new(C), new(batch * C)
        call("eg_pyramid_conv_fwd", x.detach(), batch, side, conv_w.detach(), _det(conv_b), z)
        call("eg_bn2d_train_fwd", z, batch, C, side, _det(gamma), _det(beta), eps, momentum, stats[0], stats[1],
             _pyramid_workspace(dev, batch, side, side_out), y, save_mean, save_invstd)
        call("eg_pyramid_act_fwd", y, x.detach(), batch, side, side_out, p, seed, keep, idx, out)
        ctx.save_for_backward(x, conv_w, gamma, out, z, idx, keep, save_mean, save_invstd)
        ctx.has = (conv_b is not None, beta is not None)
        ctx.mark_non_differentiable(keep)
        return out, keep

    @staticmethod
    @once_differentiable                    # a double backward raises
    def backward(ctx, dout, _dkeep):
        x, conv_w, gamma, out, z, idx, keep, save_mean, save_invstd = ctx.saved_tensors
        need_x, need_w3, need_b3, need_g, need_be = ctx.needs_input_grad[:5]
        has_b3, has_beta = ctx.has
        batch, side, side_out, dev, C = int(x.shape[0]), int(x.shape[2]), int(out.shape[2]), x.device, MAX_CHANNELS
        dout = dout.contiguous()
        if dout.dtype != torch.float32 or dout.shape != out.shape:
            raise RuntimeError(f"pyramid_block_train backward: dout must be float32 {tuple(out.shape)}, got {dout.dtype} {tuple(dout.shape)}")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ds, dz = torch.empty_like(z), torch.empty_like(z)
        dgamma = new(C) if need_g and gamma is not None else None
        dbeta = new(C) if need_be and has_beta else None
        db3 = new(C) if need_b3 and has_b3 else None
        ws = _pyramid_workspace(dev, batch, side, side_out)
        call("eg_pyramid_act_bwd", dout, out, keep, idx, z, save_mean, save_invstd, gamma, batch, side, side_out, ws, ds, dz, dgamma,
             dbeta, db3)
        dw3 = dx = None
        if need_w3:
            dw3 = torch.empty_like(conv_w)
            call("eg_pyramid_conv_bwd_weight", x, dz, batch, side, ws, dw3)
        if need_x:                          # the chain, then the residual's share in the epilogue: always this order
            dx = torch.empty_like(x)
            call("eg_pyramid_conv_bwd_data", dz, conv_w, ds, batch, side, dx)
        return dx, dw3, db3, dgamma, dbeta, None, None, None, None, None, None


def pyramid_block_train(x: torch.Tensor, conv_w: torch.Tensor, conv_b: Optional[torch.Tensor], bn, side_out: int, p: float, seed: int,
                        return_keep: bool = False):
    """Dropout2d_p(relu(AdaptiveMaxPool2d(side_out)(BatchNorm_train(conv3x3(x) + conv_b) + x))) -> [batch, 128, side_out, side_out],
    with a backward (gradients of x, conv_w, conv_b and the BatchNorm's weight and bias, each only where it is asked for): the
    CNN-pyramid block in training mode, pool, then ReLU, then dropout as in the reference.  The arguments are `pyramid_block`'s and
    are checked the same way; bn is an nn.BatchNorm2d in TRAINING mode -- its running statistics and num_batches_tracked move as
    nn.BatchNorm2d moves them -- or (weight, bias, running_mean | None, running_var | None, eps, momentum).  The plane mask is
    `embed_block_train`'s (seed + the device's dropout epoch, b * 128 + o); return_keep: also return it [batch * 128].  All three
    convolutions run on the f32-input matrix instruction (the data gradient from side 17 on); the weight gradient's workspace is at
    most 64 slices whatever the batch and the side (scratch kind "pyramid_train").  Bit-reproducible, capturable; CUDA tensors only."""
    batch, side, side_out = _pyramid_args(x, conv_w, conv_b, side_out)
    gamma, beta, mean, var, eps, momentum, module = _bn_parts(bn, MAX_CHANNELS, training=True)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), but got {p}")
    if batch * side * side == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(batch, MAX_CHANNELS, side, side)}")
    _block_on_device(x, conv_w, conv_b, None, None, gamma, beta, mean, var)
    out, keep = _PyramidBlockTrain.apply(x, conv_w, conv_b, gamma, beta, (mean, var), eps, momentum, side_out, p, _seed(seed))
    if module is not None and module.num_batches_tracked is not None:
        module.num_batches_tracked.add_(1)
    return (out, keep) if return_keep else out


def _workspace(device, batch: int, c_in: int, c_out: int, side: int) -> torch.Tensor:
    """The backward's workspace (eg_embed_workspace_bytes): chunk sums of the BatchNorm, of dz and of the 1 x 1 weight gradient."""
    return _scratch("embedder", device, max(int(raw("eg_embed_workspace_bytes", batch, c_in, c_out, side)), 256))


class _EmbedBlockTrain(torch.autograd.Function):
    """Saved: x, out, z, keep, the batch mean and 1 / std, and references to the parameters -- never y, never the residual."""

    @staticmethod
    def forward(ctx, x, conv_w, conv_b, gamma, beta, one_w, one_b, stats, eps, momentum, p, seed):
        batch, c_in, side, c_out, dev = int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(conv_w.shape[0]), x.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        z, y, out = new(batch, c_out, side, side), new(batch, c_out, side, side), new(batch, c_out, side, side)
        save_mean, save_invstd, keep = new(c_out), new(c_out), new(batch * c_out)
        call("eg_embed_conv_fwd", x.detach(), batch, c_in, side, conv_w.detach(), _det(conv_b), c_out, z)
        call("eg_bn2d_train_fwd", z, batch, c_out, side, _det(gamma), _det(beta), eps, momentum, stats[0], stats[1],
             _train_workspace(dev, batch, c_in, c_out, side), y, save_mean, save_invstd)
        call("eg_embed_act_fwd", y, x.detach(), batch, c_in, side, _det(one_w), _det(one_b), c_out, p, seed, keep, out)
        ctx.save_for_backward(x, conv_w, gamma, one_w, out, z, keep, save_mean, save_invstd)
        ctx.has = (conv_b is not None, beta is not None, one_b is not None)
        ctx.mark_non_differentiable(keep)
        return out, keep

    @staticmethod
    @once_differentiable                    # a double backward raises
    def backward(ctx, dout, _dkeep):
        x, conv_w, gamma, one_w, out, z, keep, save_mean, save_invstd = ctx.saved_tensors
        need_x, need_w3, need_b3, need_g, need_be, need_w1, need_b1 = ctx.needs_input_grad[:7]
        has_b3, has_beta, has_b1 = ctx.has
        batch, c_in, side, c_out, dev = int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(conv_w.shape[0]), x.device
        dout = dout.contiguous()
        if dout.dtype != torch.float32 or dout.shape != out.shape:
            raise RuntimeError(f"embed_block_train backward: dout must be float32 {tuple(out.shape)}, got {dout.dtype} {tuple(dout.shape)}")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        ds, dz = torch.empty_like(out), torch.empty_like(out)
        dgamma = new(c_out) if need_g and gamma is not None else None
        dbeta = new(c_out) if need_be and has_beta else None
        db3 = new(c_out) if need_b3 and has_b3 else None
        db1 = new(c_out) if need_b1 and has_b1 else None
        dw1 = torch.empty_like(one_w) if need_w1 and one_w is not None else None
        call("eg_embed_act_bwd", dout, out, keep, x, z, save_mean, save_invstd, gamma, batch, c_in, c_out, side,
             _workspace(dev, batch, c_in, c_out, side), ds, dz, dgamma, dbeta, db3, db1, dw1)
        dw3 = dx = None
        if need_w3:
            dw3 = torch.empty_like(conv_w)
            call("eg_conv3x3_bwd_weight", x, c_in, side, None, 0, batch, side, dz, c_out, _train_workspace(dev, batch, c_in, c_out, side), dw3)
        if need_x:                          # the data gradient first, the residual's share added in place after it: always this order
            dx = torch.empty_like(x)
            call("eg_conv3x3_bwd_data", dz, conv_w, batch, c_out, side, c_in, side, 0, dx, None, None)
            call("eg_embed_res_bwd_input", ds, one_w, batch, c_in, c_out, side, dx)
        return dx, dw3, db3, dgamma, dbeta, dw1, db1, None, None, None, None, None


def embed_block_train(x: torch.Tensor, conv_w: torch.Tensor, conv_b: Optional[torch.Tensor], bn, one_w: Optional[torch.Tensor],
                      one_b: Optional[torch.Tensor], p: float, seed: int, return_keep: bool = False):
    """Dropout2d_p(relu(BatchNorm_train(conv3x3(x) + conv_b) + r)) -> [batch, c_out, side, side], with a backward (gradients of x,
    conv_w, conv_b, the BatchNorm's weight and bias, one_w and one_b, each only where it is asked for).  The arguments are
    `embed_block`'s; bn is an nn.BatchNorm2d in TRAINING mode -- its running statistics and num_batches_tracked move as
    nn.BatchNorm2d moves them -- or (weight, bias, running_mean | None, running_var | None, eps, momentum).  Plane (b, o) is kept
    (and scaled by 1 / (1 - p)) or zeroed by the counter-based mask of (seed + the device's dropout epoch, b * c_out + o);
    return_keep: also return that mask [batch * c_out] as the kernel wrote it.  4 launches forward, 5 backward and 7 where x asks
    for a gradient; bit-reproducible, capturable."""
    batch, c_in, c_out, side = _block_args(x, conv_w, conv_b, one_w, one_b)
    gamma, beta, mean, var, eps, momentum, module = _bn_parts(bn, c_out, training=True)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), but got {p}")
    if batch * side * side == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(batch, c_out, side, side)}")
    _block_on_device(x, conv_w, conv_b, one_w, one_b, gamma, beta, mean, var)
    out, keep = _EmbedBlockTrain.apply(x, conv_w, conv_b, gamma, beta, one_w, one_b, (mean, var), eps, momentum, p, _seed(seed))
    if module is not None and module.num_batches_tracked is not None:
        module.num_batches_tracked.add_(1)
    return (out, keep) if return_keep else out
