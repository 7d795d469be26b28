"""What the embedder's CPU and GPU tests share: the plane mask of csrc/train_common.h restated in Python integers, the seeded
fixture of one residual block, and the same block from torch modules on the CPU in any dtype (the reference of every GPU case)."""
from __future__ import annotations

import numpy as np
import torch

from echoglad_amd.nn import CNNResBlock

M64 = (1 << 64) - 1


def mask_word(seed: int, group: int) -> int:
    """The splitmix64 finaliser of seed + group * golden ratio (train_common.h mask_word)."""
    z = (seed + group * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def plane_keep(seed: int, planes: int, p: float) -> torch.Tensor:
    """keep[i] = 0 or 1 / (1 - p) for i < planes: the 16-bit field i & 3 of mask_word(seed, i >> 2) against floor(65536 p), in the
    float32 arithmetic of the kernel (keep_scale).  `seed` is the caller's seed PLUS the device's dropout epoch."""
    threshold = int(np.float32(p) * np.float32(65536.0))
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    seed &= M64
    return torch.tensor([inv_keep if ((mask_word(seed, i >> 2) >> (16 * (i & 3))) & 0xFFFF) >= threshold else 0.0 for i in range(planes)],
                        dtype=torch.float32)


def block_fixture(B, c_in, c_out, side, seed, one_by_one=None, all_on=False):
    """x randn, W3 randn / sqrt(9 c_in), W1 randn / sqrt(c_in), biases 0.05 randn, |gamma| in [0.5, 1.5] with alternating sign,
    beta 0.3 randn, running statistics away from (0, 1), dout randn.  one_by_one None: a 1 x 1 residual exactly where c_in != c_out.
    all_on: x = |randn|, W1 = |randn|, b1 >= 0, beta = 8, so that every s is far above zero."""
    g = torch.Generator().manual_seed(seed)
    one_by_one = c_in != c_out if one_by_one is None else one_by_one
    fx = dict(B=B, c_in=c_in, c_out=c_out, side=side)
    fx["x"] = torch.randn(B, c_in, side, side, generator=g)
    fx["w3"] = torch.randn(c_out, c_in, 3, 3, generator=g) / (9 * c_in) ** 0.5
    fx["b3"] = 0.05 * torch.randn(c_out, generator=g)
    fx["w1"] = torch.randn(c_out, c_in, 1, 1, generator=g) / c_in ** 0.5 if one_by_one else None
    fx["b1"] = 0.05 * torch.randn(c_out, generator=g) if one_by_one else None
    sign = torch.tensor([1.0 if o % 2 == 0 else -1.0 for o in range(c_out)])
    fx["gamma"] = sign * (0.5 + torch.rand(c_out, generator=g))
    fx["beta"] = 0.3 * torch.randn(c_out, generator=g)
    fx["rm"] = 0.3 * torch.randn(c_out, generator=g)
    fx["rv"] = 0.5 + torch.rand(c_out, generator=g)
    fx["dout"] = torch.randn(B, c_out, side, side, generator=g)
    if all_on:
        fx["x"] = fx["x"].abs()
        fx["beta"] = torch.full((c_out,), 8.0)
        if one_by_one:
            fx["w1"], fx["b1"] = fx["w1"].abs(), fx["b1"].abs()
    return fx


def block_module(fx, dtype=torch.float32, device="cpu", training=True) -> CNNResBlock:
    """The fixture's block as a CNNResBlock of torch modules (dropout 0: the tests inject their own plane mask)."""
    blk = CNNResBlock(in_channels=fx["c_in"], padding=1, out_channels=fx["c_out"], kernel_size=3, pool_size=1, cnn_dropout_p=0.0)
    if fx["w1"] is not None and blk.one_by_one_cnn is None:             # a 1 x 1 residual between equal channel counts
        blk.one_by_one_cnn = torch.nn.Conv2d(fx["c_in"], fx["c_out"], kernel_size=1)
    with torch.no_grad():
        blk.conv.weight.copy_(fx["w3"])
        blk.conv.bias.copy_(fx["b3"])
        blk.bn.weight.copy_(fx["gamma"])
        blk.bn.bias.copy_(fx["beta"])
        blk.bn.running_mean.copy_(fx["rm"])
        blk.bn.running_var.copy_(fx["rv"])
        if fx["w1"] is not None:
            blk.one_by_one_cnn.weight.copy_(fx["w1"])
            blk.one_by_one_cnn.bias.copy_(fx["b1"])
    return blk.to(device=device, dtype=dtype).train(training)


def block_reference(fx, dtype, training=True, keep=None):
    """The block on the CPU in `dtype` -> outputs, statistics, every gradient, the pre-activation s and dz.  keep [B * c_out]: the
    plane mask, applied after the ReLU."""
    blk = block_module(fx, dtype, training=training)
    got = {}
    blk.pool.register_forward_pre_hook(lambda m, inp: got.__setitem__("s", inp[0].detach()))
    if training:
        blk.conv.register_forward_hook(lambda m, inp, out: out.register_hook(lambda g: got.__setitem__("dz", g.detach())) and None)
    x = fx["x"].to(dtype).requires_grad_(training)
    out = blk(x)
    if keep is not None:
        out = out * keep.to(dtype).view(fx["B"], fx["c_out"], 1, 1)
    got["out"] = out.detach()
    if not training:
        return got
    (out * fx["dout"].to(dtype)).sum().backward()
    one = blk.one_by_one_cnn
    got.update(rm=blk.bn.running_mean.clone(), rv=blk.bn.running_var.clone(), nbt=int(blk.bn.num_batches_tracked), dx=x.grad,
               dw3=blk.conv.weight.grad, db3=blk.conv.bias.grad, dgamma=blk.bn.weight.grad, dbeta=blk.bn.bias.grad,
               dw1=None if one is None else one.weight.grad, db1=None if one is None else one.bias.grad)
    return got


def relu_margin(r64, r32):
    """(the float32 mask is the float64 mask, min|s64| / max|s32 - s64|) of the two references' pre-activations."""
    s64, s32 = r64["s"], r32["s"].double()
    err = float((s32 - s64).abs().max())
    return torch.equal(s32 > 0, s64 > 0), float(s64.abs().min()) / max(err, 1e-300)
