"""The reference's CNN embedder (CNNResBlock / CNN, src/core/models.py:71-260): constructor signatures, attribute names and
state_dict keys are the reference's, so a checkpoint's `embedder_state_dict` loads ``strict=True``:

    conv.{i}.0.conv.{weight,bias}    conv.{i}.0.bn.{weight,bias,running_mean,running_var,num_batches_tracked}
    conv.{i}.0.one_by_one_cnn.{weight,bias}        (only where the block changes the channel count)

The default route is built from torch modules, covers every argument of the reference and runs on the CPU.  `CNN.enable_hip`
switches blocks of kernel 3 and pool 1 to ops.embed_block (eval, one launch per block) and ops.embed_block_train (training:
bit-reproducible, capturable, the plane mask drawn from the device's dropout epoch)."""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn

from ..ops import embedder as E_ops


def _refuse(where: str, why: str):
    raise NotImplementedError(f"CNN.enable_hip: {where}: {why} (the HIP embedder covers Conv2d(kernel 3, padding 1, stride 1, "
                              "dilation 1, groups 1, zero padding) -> BatchNorm2d with running statistics -> + residual -> "
                              "MaxPool2d(1) -> ReLU -> Dropout2d on square maps, without an output FC)")


class CNNResBlock(nn.Module):
    """conv -> bn -> + residual (one_by_one_cnn(x) where the channel counts differ, else x) -> pool -> ReLU -> Dropout2d."""

    def __init__(self, in_channels: int, padding: int, out_channels: int = 128, kernel_size: int = 3, pool_size: int = 2,
                 out_size: int = None, cnn_dropout_p: float = 0.0):
        super().__init__()
        # registration order is the state_dict's order: the residual's 1 x 1 convolution (only where the channel count changes) first
        self.one_by_one_cnn = nn.Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=(padding, padding))
        self.bn = nn.BatchNorm2d(out_channels)
        self.pool = nn.MaxPool2d((pool_size, pool_size)) if out_size is None else nn.AdaptiveMaxPool2d((out_size, out_size))
        self.activation = nn.ReLU()
        self.dropout = nn.Dropout2d(cnn_dropout_p)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        residual = x if self.one_by_one_cnn is None else self.one_by_one_cnn(x)
        x = self.bn(self.conv(x)) + residual
        return self.dropout(self.activation(self.pool(x)))

    # ---- the HIP route -----------------------------------------------------------------------------------------------------
    def check_hip(self, where: str, training: bool) -> None:
        """NotImplementedError, naming `where` and the reason, unless the block is one the HIP embedder covers in that mode."""
        conv = self.conv
        for got, want, what in ((tuple(conv.kernel_size), (3, 3), "kernel_size"), (tuple(conv.padding), (1, 1), "padding"),
                                (tuple(conv.stride), (1, 1), "stride"), (tuple(conv.dilation), (1, 1), "dilation"),
                                (conv.groups, 1, "groups"), (conv.padding_mode, "zeros", "padding_mode")):
            if got != want:
                _refuse(f"{where}.conv", f"{what} = {got}, not {want}")
        if not isinstance(self.pool, nn.MaxPool2d):
            _refuse(f"{where}.pool", f"{type(self.pool).__name__} (an adaptive pool) is not covered")
        size = self.pool.kernel_size
        if (tuple(size) if isinstance(size, (tuple, list)) else (size, size)) != (1, 1):
            _refuse(f"{where}.pool", f"pool_size = {size}, not 1")
        bn = self.bn
        if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
            _refuse(f"{where}.bn", "the BatchNorm keeps no running statistics")
        if bn.momentum is None:
            _refuse(f"{where}.bn", "the BatchNorm has momentum=None (a cumulative moving average)")
        if bn.training != training:
            _refuse(f"{where}.bn", f"the BatchNorm is in {'training' if bn.training else 'eval'} mode, the module in "
                                   f"{'training' if training else 'eval'} mode")

    def forward_hip(self, x: torch.Tensor, seed: int = 0) -> torch.Tensor:
        """The block on ops.embed_block (eval) or ops.embed_block_train (training, `seed` for the plane mask)."""
        one = self.one_by_one_cnn
        one_w, one_b = (None, None) if one is None else (one.weight, one.bias)
        if self.training:
            return E_ops.embed_block_train(x, self.conv.weight, self.conv.bias, self.bn, one_w, one_b, self.dropout.p, seed)
        return E_ops.embed_block(x, self.conv.weight, self.conv.bias, self.bn, one_w, one_b)


class CNN(nn.Module):
    """A stack of CNNResBlocks, the first one on 1 channel, and an optional output FC."""

    def __init__(self, out_channels: list, kernel_sizes: list = None, pool_sizes: list = None, fc_output_dim: list = None,
                 cnn_dropout_p: float = 0.0):
        super().__init__()
        n = len(out_channels)
        per_layer = lambda v, default: [default] * n if v is None else (list(v) if isinstance(v, (list, tuple)) else [v] * n)
        kernel_sizes, pool_sizes = per_layer(kernel_sizes, 3), per_layer(pool_sizes, 1)
        if len(kernel_sizes) != n or len(pool_sizes) != n:
            raise ValueError("kernel_sizes and pool_sizes need one entry per layer of out_channels")
        widths = [1] + list(out_channels)                 # the frames have one channel
        # every block sits in a Sequential of its own: the keys are conv.{i}.0.*
        self.conv = nn.Sequential(*[nn.Sequential(CNNResBlock(widths[i], (kernel_sizes[i] - 1) // 2, widths[i + 1], kernel_sizes[i],
                                                              pool_sizes[i], cnn_dropout_p=cnn_dropout_p)) for i in range(n)])
        self.output_fc = None
        if fc_output_dim is not None:                     # mean over the map, then Linear + ReLU on [batch, channels] rows
            self.output_fc = nn.Sequential(nn.AdaptiveAvgPool3d((None, 1, 1)), nn.Flatten(2), nn.Linear(widths[-1], fc_output_dim),
                                           nn.ReLU(inplace=True))
        # plain attributes: no parameter, no buffer, the state_dict does not know them
        self._hip = False
        self._hip_train = False
        self.dropout_seed_hook: Optional[Callable] = None

    def enable_hip(self, flag: bool = True, train: bool = False) -> "CNN":
        """Route the blocks through the HIP embedder: in eval mode under torch.no_grad() one launch per block (ops.embed_block);
        with train=True also in training mode with autograd on (ops.embed_block_train).  Every other combination stays on the torch
        modules.  NotImplementedError, naming the block, for a structure the kernels do not cover.  Returns self."""
        if flag:
            if self.output_fc is not None:
                _refuse("output_fc", "fc_output_dim is not covered")
            for i, seq in enumerate(self.conv):
                seq[0].check_hip(f"conv[{i}][0]", self.training)
        self._hip, self._hip_train = bool(flag), bool(flag and train)
        return self

    def _route(self) -> Optional[str]:
        if self._hip and not self.training and not torch.is_grad_enabled():
            return "eval"
        if self._hip_train and self.training and torch.is_grad_enabled():
            return "train"
        return None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        route = self._route()
        if route is None:
            x = self.conv(x)
            return x if self.output_fc is None else self.output_fc(x)
        for i, seq in enumerate(self.conv):
            block = seq[0]
            block.check_hip(f"conv[{i}][0]", self.training)
            seed = 0
            if route == "train" and block.dropout.p > 0:
                # drawn on the host, as the model draws its seeds; the kernel adds the device's epoch, so a replayed capture moves on
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            if route == "train" and self.dropout_seed_hook is not None:
                self.dropout_seed_hook("embedder", i, (seed,))
            x = block.forward_hip(x.contiguous(), seed)
        return x
