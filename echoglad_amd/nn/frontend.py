"""The reference's UNet encoder / decoder (DownConv / UpConv, src/core/models.py:841-876) on the HIP front-end operators, no
upsampled or concatenated intermediate.  `unet_decoder_maps`: eval mode, 3 launches (conv, conv, pool) per DownConv and 2 per UpConv.
`unet_decoder_maps_train`: training mode (batch statistics) with a backward, 7 launches per DownConv and 6 per UpConv forward."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from ..ops import frontend as F_ops


def _refuse(where: str, why: str):
    raise NotImplementedError(f"unet_decoder_maps: {where}: {why} (the HIP front-end covers Conv2d(kernel 3, padding 1, stride 1, "
                              "dilation 1, groups 1, zero padding) -> ReLU -> BatchNorm2d with running statistics, "
                              "AdaptiveMaxPool2d and nearest Upsample(size=) on square maps)")


def _square(value, where: str) -> int:
    """An int or an (s, s) pair -> s."""
    if isinstance(value, (tuple, list)):
        if len(value) != 2 or value[0] != value[1] or value[0] is None:
            _refuse(where, f"size {tuple(value)} is not square")
        value = value[0]
    if value is None or int(value) != value or int(value) < 1:
        _refuse(where, f"size {value!r} is not a positive integer")
    return int(value)


def _check_conv(conv, where: str) -> None:
    if not isinstance(conv, nn.Conv2d):
        _refuse(where, f"{type(conv).__name__} is not an nn.Conv2d")
    pad = conv.padding if not isinstance(conv.padding, str) else None
    for got, want, what in ((tuple(conv.kernel_size), (3, 3), "kernel_size"), (None if pad is None else tuple(pad), (1, 1), "padding"),
                            (tuple(conv.stride), (1, 1), "stride"), (tuple(conv.dilation), (1, 1), "dilation"),
                            (conv.groups, 1, "groups"), (conv.padding_mode, "zeros", "padding_mode")):
        if got != want:
            _refuse(where, f"{what} = {conv.padding if what == 'padding' else got}, not {want}")


def _check_bn(bn, where: str, training: bool = False) -> None:
    if not isinstance(bn, nn.BatchNorm2d):
        _refuse(where, f"{type(bn).__name__} is not an nn.BatchNorm2d")
    if bn.running_mean is None or bn.running_var is None:
        _refuse(where, "the BatchNorm keeps no running statistics")
    if bn.training and not training:
        _refuse(where, "the BatchNorm is in training mode (batch statistics)")
    if training and not bn.training:
        _refuse(where, "the BatchNorm is in eval mode (running statistics): unet_decoder_maps is the eval-mode route")
    if training and bn.momentum is None:
        _refuse(where, "the BatchNorm has momentum=None (a cumulative moving average)")


def _check_block(block, where: str, training: bool = False) -> None:
    for conv, bn in (("conv1", "BN1"), ("conv2", "BN2")):
        if not hasattr(block, conv) or not hasattr(block, bn):
            _refuse(where, f"no {conv} / {bn}")
        _check_conv(getattr(block, conv), f"{where}.{conv}")
        _check_bn(getattr(block, bn), f"{where}.{bn}", training)


def _structure(down_convs, up_convs, frames, training: bool):
    """The structure checks both routes share -> (down blocks, up blocks, pool sides, upsample sides)."""
    down_convs, up_convs = list(down_convs), list(up_convs)
    if len(down_convs) != len(up_convs):
        _refuse("blocks", f"{len(down_convs)} down blocks against {len(up_convs)} up blocks")
    if frames.dim() != 4 or frames.shape[2] != frames.shape[3]:
        _refuse("frames", f"shape {tuple(frames.shape)} is not a square NCHW batch")
    pools, sizes = [], []
    for i, down in enumerate(down_convs):
        _check_block(down, f"down_convs[{i}]", training)
        if not isinstance(getattr(down, "pool", None), nn.AdaptiveMaxPool2d) or down.pool.return_indices:
            _refuse(f"down_convs[{i}].pool", "not an nn.AdaptiveMaxPool2d without indices")
        pools.append(_square(down.pool.output_size, f"down_convs[{i}].pool.output_size"))
    for i, up in enumerate(up_convs):
        _check_block(up, f"up_convs[{i}]", training)
        ups = getattr(up, "upsample", None)
        if not isinstance(ups, nn.Upsample) or ups.mode != "nearest" or ups.size is None:
            _refuse(f"up_convs[{i}].upsample", "not a nearest nn.Upsample(size=)")
        sizes.append(_square(ups.size, f"up_convs[{i}].upsample.size"))
    return down_convs, up_convs, pools, sizes


def _walk(down_convs, up_convs, frames, conv, pool, training: bool) -> List[torch.Tensor]:
    """The walk over the blocks both routes make, on the convolution and pool operators of one mode."""
    down_convs, up_convs, pools, sizes = _structure(down_convs, up_convs, frames, training)
    x, skips = frames.contiguous(), []
    for down, side_out in zip(down_convs, pools):
        skips.append(x)
        x = conv(x, down.conv1.weight, down.conv1.bias, down.BN1)
        x = conv(x, down.conv2.weight, down.conv2.bias, down.BN2)
        x = pool(x, side_out)
    feats = [x]
    for up, side in zip(up_convs, sizes):
        skip = skips.pop()
        if skip.shape[2] != side:
            _refuse("up_convs", f"upsample.size {side} does not meet the skip map's side {skip.shape[2]}")
        x = conv(x, up.conv1.weight, up.conv1.bias, up.BN1, side=side)                                  # upsample + conv1
        x = conv(x, up.conv2.weight, up.conv2.bias, up.BN2, x1=skip)                                    # cat([x, skip]) + conv2
        feats.append(x)
    return feats


def unet_decoder_maps(down_convs, up_convs, frames: torch.Tensor) -> List[torch.Tensor]:
    """The decoder's maps, coarse to fine, of the reference's UNet front-end in eval mode: what

        x, skips = frames, []
        for down in down_convs: skips.append(x); x = down(x)
        feats = [x]
        for up in up_convs: x = up(x, skips.pop()); feats.append(x)

    returns, on eg_conv3x3_relu_bn_fwd and eg_adaptive_max_pool_fwd: 3 launches per down block, 2 per up block (35 for the default
    7 + 7).  Blocks are anything with the reference's attribute names: down.conv1 / BN1 / conv2 / BN2 / pool.output_size,
    up.upsample.size / conv1 / BN1 / conv2 / BN2.  Parameters and running statistics are read at the call: nothing is cached.
    Inference only; NotImplementedError for a block outside this structure."""
    return _walk(down_convs, up_convs, frames, F_ops.conv3x3_relu_bn, F_ops.adaptive_max_pool, training=False)


def unet_decoder_maps_train(down_convs, up_convs, frames: torch.Tensor) -> List[torch.Tensor]:
    """`unet_decoder_maps` in TRAINING mode, with a backward: the same blocks with batch statistics (every BatchNorm must be in
    training mode; running statistics and num_batches_tracked move as torch moves them) on ops.conv3x3_relu_bn_train and
    ops.adaptive_max_pool_train.  Skips, the upsample and the concatenation are passed as sources, as in eval: autograd saves the
    ReLU outputs, the batch statistics and the pools' indices, never an upsampled or concatenated map.  91 launches forward for
    the default 7 + 7; bit-reproducible; capturable.  NotImplementedError for a block outside the structure."""
    return _walk(down_convs, up_convs, frames, F_ops.conv3x3_relu_bn_train, F_ops.adaptive_max_pool_train, training=True)
