"""Parameter tables of the Linear-BN-ReLU-Drop-Linear-BN-ReLU-Drop-Linear networks (the 4 classifier heads, the coordinate
MLPs) and the stacked layout the kernels take them in."""
from __future__ import annotations

from math import prod

import torch
import torch.nn as nn

from .. import ops

C = ops.C

# the 10 parameters of such a network: where they sit in the nn.Sequential, and what the kernels call them
_HEAD_PARAM_IDX = ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias"), (4, "weight"), (4, "bias"), (5, "weight"),
                   (5, "bias"), (8, "weight"), (8, "bias"))
_MLP_NAMES = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")

# one classifier head (128-32-16-1): the shapes of its parameters, their sizes, and the shapes of the four heads' stacked arrays.
# In one flat buffer the stacked arrays follow each other in this order: the layout of _stack_head_params' bank and of
# eg_classifier_bwd's packed gradients (include/echoglad_hip.h)
_HEAD_PARAM_SHAPES = ((32, C), (32,), (32,), (32,), (16, 32), (16,), (16,), (16,), (1, 16), (1,))
_HEAD_SIZES = tuple(prod(s) for s in _HEAD_PARAM_SHAPES)
_HEAD_SHAPES = ((4 * 32, C), (128,), (128,), (128,), (4, 16, 32), (64,), (64,), (64,), (64,), (4,))
# one coordinate MLP (136-32-16-2); eg_coord_mlp_bwd packs its gradients in this order
_MLP_SHAPES = ((32, C + 8), (32,), (32,), (32,), (16, 32), (16,), (16,), (16,), (2, 16), (2,))
_MLP_SIZES = tuple(prod(s) for s in _MLP_SHAPES)


def _seq_params(seq: nn.Sequential):
    """The 10 parameters of a Linear-BN-ReLU-Drop-Linear-BN-ReLU-Drop-Linear head in _HEAD_PARAM_IDX order (plain dict lookups:
    this runs for 7 heads several times per training step, and at batch 1 the step is bound by the host)."""
    m = seq._modules
    return [m[str(j)]._parameters[name] for j, name in _HEAD_PARAM_IDX]


def _mlp_stats_cfg(m) -> dict:
    """Epsilons, dropout rates, running statistics of such a network (``m`` = its ``_modules``) under the kernels' names;
    seeds 0 until a train-mode forward draws them."""
    bn1, bn2 = m["1"], m["5"]
    return dict(eps1=bn1.eps, eps2=bn2.eps, p1=float(m["3"].p), p2=float(m["7"].p), seed1=0, seed2=0,
                running_mean1=bn1.running_mean, running_var1=bn1.running_var, running_mean2=bn2.running_mean,
                running_var2=bn2.running_var)


def _mlp_kernel_params(cfg: dict, params) -> dict:
    """cfg + the 10 parameters under the kernels' names, detached and contiguous."""
    P = dict(cfg)
    P.update({k: p.detach().contiguous() for k, p in zip(_MLP_NAMES, params)})
    return P


def _without_running(P: dict) -> dict:
    """What a backward needs of P: everything but the running statistics (the forward has updated them)."""
    return {k: v for k, v in P.items() if not k.startswith("running")}


def _head_param_offsets():
    """Element offset of parameter (head k, array j) = params[10 * k + j] in the flat buffer of _stack_head_params."""
    offs, start = [0] * 40, 0
    for j, size in enumerate(_HEAD_SIZES):
        for k in range(4):
            offs[10 * k + j] = start + k * size
        start += 4 * size
    return offs


def _views_of(bank: torch.Tensor, tensors, offsets) -> bool:
    """Is tensors[i] the contiguous float32 slice of ``bank`` that starts at element offsets[i]?"""
    base, dev = bank.data_ptr(), bank.device
    for t, o in zip(tensors, offsets):
        if t.data_ptr() != base + 4 * o or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            return False
    return True


def _move_into(bank: torch.Tensor, tensors, offsets, assign) -> None:
    """Copies tensors[i] into bank[offsets[i] : + numel] and re-points it there (assign(i, view)): once, not per step."""
    with torch.no_grad():
        for i, (t, o) in enumerate(zip(tensors, offsets)):
            view = bank[o:o + t.numel()].view(t.shape)
            view.copy_(t)
            assign(i, view)


def _stack_head_params(params, cfg):
    """The 4 x 10 head parameters as the stacked arrays the kernels take: ONE flat buffer filled by one multi-tensor copy (a
    torch.cat / stack per array was 10 launches per step), the arrays are views of it."""
    bank = cfg.get("_param_bank")
    if bank is not None and _views_of(bank, params, _head_param_offsets()):
        P, start = dict(cfg), 0                   # the parameters ARE the stacked arrays (HierarchicalPatchModel._heads_in_place): nothing to copy
        for size, name, shape in zip(_HEAD_SIZES, _MLP_NAMES, _HEAD_SHAPES):
            P[name] = bank[start:start + 4 * size].view(shape)
            start += 4 * size
        return P
    flat = torch.empty(4 * sum(_HEAD_SIZES), dtype=torch.float32, device=params[0].device)
    dst, src, start = [], [], 0
    P = dict(cfg)
    for j, (size, name, shape) in enumerate(zip(_HEAD_SIZES, _MLP_NAMES, _HEAD_SHAPES)):
        P[name] = flat[start:start + 4 * size].view(shape)
        for k in range(4):
            dst.append(flat[start + k * size:start + (k + 1) * size])
            src.append(params[10 * k + j].detach().reshape(-1))
        start += 4 * size
    torch._foreach_copy_(dst, src)
    return P


def fold_last_into_heads(weight, scale, shift, w1, s1, t1, residual: bool):
    """The last GCN layer (no ReLU) folded into the heads' first Linear + eval-mode BatchNorm.  With
    h3 = scale * ((A_hat h) weight^T) + shift + r h  and  u = s1 * (h3 w1^T) + t1:

        u = (A_hat h) m1^T + r h w1s^T + c1,   m1 = diag(s1) w1 diag(scale) weight,  w1s = diag(s1) w1,  c1 = s1 * (w1 shift) + t1

    scale / shift of None mean 1 and 0.  Computed in float64 on the parameters' device, rounded once -> (m1 [128,128],
    w1s [128,128], c1 [128]), float32 and contiguous.  ``residual`` enters no value (r multiplies the input in the kernel,
    eg_gcn_layer_cls_fold_fwd, which skips the second product without it); the argument is there so that the call names
    everything the launch depends on."""
    with torch.no_grad():
        w1d, s1d = w1.double(), s1.double()
        w = weight.double() if scale is None else scale.double()[:, None] * weight.double()
        w1s = s1d[:, None] * w1d
        m1 = w1s @ w
        c1 = t1.double() if shift is None else s1d * (w1d @ shift.double()) + t1.double()
        return tuple(t.float().contiguous() for t in (m1, w1s, c1))


def _unstack_head_grads(g):
    """eg_classifier_bwd's packed gradients [4 * sum(_HEAD_SIZES)] -> 40 views, one per parameter, in the order of the ``params``
    of _stack_head_params (head k, array j at 10 * k + j)."""
    arrays = [a.view(4, *shape) for a, shape in zip(torch.split(g, [4 * s for s in _HEAD_SIZES]), _HEAD_PARAM_SHAPES)]
    return tuple(a[k] for k in range(4) for a in arrays)


def _mlp_grads(g):
    """eg_coord_mlp_bwd's packed gradients -> 10 views in _HEAD_PARAM_IDX order."""
    return tuple(a.view(shape) for a, shape in zip(torch.split(g, _MLP_SIZES), _MLP_SHAPES))
