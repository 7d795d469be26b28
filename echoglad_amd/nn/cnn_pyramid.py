"""The reference's CNN-pyramid variant (CNNHierarchicalPatchModel, src/core/models.py:556-636; `cnn_hierarchical_patch` in
src/builders/model_builder.py): a stack of CNNResBlock(128 -> 128, kernel 3, AdaptiveMaxPool2d(width)) in front of the GNN whose
last `num_aux_graphs` outputs are the node features of the aux levels, coarse to fine; the frame embedding itself is the main
level.  Constructor signature, attribute names and state_dict keys are the reference's, so a checkpoint loads ``strict=True``:

    conv.{i}.conv.{weight,bias}    conv.{i}.bn.{weight,bias,running_mean,running_var,num_batches_tracked}
    conv_hierarchical_grids.{i}.*  the same block objects once more (the reference's IntermediateLayerGetter is a ModuleDict over them)

The default route is the torch modules and runs on the CPU.  `enable_hip_pyramid` switches the blocks to ops.pyramid_block in eval
mode under torch.no_grad() (csrc/pyramid_conv.hip: the convolution on the f32-input matrix instruction, then the adaptive max pool),
and with ``train=True`` to ops.pyramid_block_train in training mode with autograd on (bit-reproducible, capturable, all three
convolutions on the matrix instruction, the plane masks drawn from the device's dropout epoch); the tail is the base class's `pack_node_features` (one packing launch) on every route."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from ..ops import embedder as E_ops
from .embedder import CNNResBlock
from .model import C, HierarchicalPatchModel


def _refuse(where: str, why: str):
    raise NotImplementedError(f"CNNHierarchicalPatchModel.enable_hip_pyramid: {where}: {why} (the HIP pyramid covers Conv2d(128, 128, "
                              "kernel 3, padding 1, stride 1, dilation 1, groups 1, zero padding) -> BatchNorm2d with running "
                              "statistics -> + input -> AdaptiveMaxPool2d(square) -> ReLU -> Dropout2d on square maps)")


class CNNHierarchicalPatchModel(HierarchicalPatchModel):
    """``HierarchicalPatchModel`` whose aux-level node features come from a down-sampling CNN (same constructor as the reference
    class: ``cnn_layers_out_width`` / ``cnn_dropout_p`` + the base class's keyword arguments; ``forward`` takes the embedder's
    ``[B, 128, F, F]`` frames).  Level g (side 2^(g+1), g = 0 .. num_aux_graphs - 1) is the output of block L - 1 - g."""

    def __init__(self, cnn_layers_out_width: Optional[List[int]] = None, cnn_dropout_p: float = 0.0, **kwargs):
        super().__init__(**kwargs)
        widths = [128, 64, 32, 16, 8, 4, 2] if cnn_layers_out_width is None else [int(w) for w in cnn_layers_out_width]
        L, naux = len(widths), self.num_aux_graphs
        if L < 1:
            raise ValueError("cnn_layers_out_width needs at least one layer")
        if naux > L:
            raise ValueError(f"the CNN yields {L} maps (sides {widths}); num_aux_graphs={naux} levels need at least that many layers")
        if not self.use_main_graph_only and [widths[L - 1 - g] for g in range(naux)] != [2 ** (g + 1) for g in range(naux)]:
            raise ValueError(f"level g of the graph is a 2^(g+1) x 2^(g+1) grid: the last {naux} widths of cnn_layers_out_width must be "
                             f"{[2 ** (g + 1) for g in reversed(range(naux))]}, got {widths[L - naux:]}")
        dim = self.node_embedding_dim
        self.conv = nn.Sequential(*[CNNResBlock(in_channels=dim, padding=1, out_channels=dim, kernel_size=3, out_size=w,
                                                cnn_dropout_p=cnn_dropout_p) for w in widths])
        # the reference's IntermediateLayerGetter(self.conv, {L-1-g: g}): a ModuleDict of conv's children up to the last one a level
        # is taken from (all of them; only the first where there is no aux level), registered a second time under this name
        last = L - 1 if naux > 0 else 0
        self.conv_hierarchical_grids = nn.ModuleDict({str(i): self.conv[i] for i in range(last + 1)})
        self.cnn_layers_out_width = widths
        self.hip_pyramid = False            # plain attributes: no parameter, no buffer, not in the state_dict
        self.hip_pyramid_train = False

    # ---- the HIP route ---------------------------------------------------------------------------------------------------------
    def _check_block(self, i: int) -> int:
        """NotImplementedError naming block i and the reason unless it is one ops.pyramid_block covers -> its output side."""
        blk, where = self.conv[i], f"conv[{i}]"
        conv = blk.conv
        for got, want, what in ((conv.in_channels, C, "in_channels"), (conv.out_channels, C, "out_channels"),
                                (tuple(conv.kernel_size), (3, 3), "kernel_size"), (tuple(conv.padding), (1, 1), "padding"),
                                (tuple(conv.stride), (1, 1), "stride"), (tuple(conv.dilation), (1, 1), "dilation"),
                                (conv.groups, 1, "groups"), (conv.padding_mode, "zeros", "padding_mode")):
            if got != want:
                _refuse(f"{where}.conv", f"{what} = {got}, not {want}")
        if blk.one_by_one_cnn is not None:
            _refuse(f"{where}.one_by_one_cnn", "a 1 x 1 residual convolution is not covered")
        if not isinstance(blk.pool, nn.AdaptiveMaxPool2d):
            _refuse(f"{where}.pool", f"{type(blk.pool).__name__} is not an AdaptiveMaxPool2d")
        size = blk.pool.output_size
        size = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
        if len(size) != 2 or size[0] != size[1] or not isinstance(size[0], int) or size[0] < 1:
            _refuse(f"{where}.pool", f"output_size = {blk.pool.output_size} is not a square size")
        bn = blk.bn
        if not isinstance(bn, nn.BatchNorm2d) or not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
            _refuse(f"{where}.bn", "the BatchNorm keeps no running statistics")
        if bn.momentum is None:
            _refuse(f"{where}.bn", "the BatchNorm has momentum=None (a cumulative moving average)")
        if bn.training != self.training:
            _refuse(f"{where}.bn", f"the BatchNorm is in {'training' if bn.training else 'eval'} mode, the module in "
                                   f"{'training' if self.training else 'eval'} mode")
        return int(size[0])

    def enable_hip_pyramid(self, flag: bool = True, train: bool = False) -> "CNNHierarchicalPatchModel":
        """Opt in: in eval mode under torch.no_grad(), with CUDA float32 frames, the blocks run on ops.pyramid_block (one
        convolution launch on the matrix unit and one pool launch per block, bit-reproducible, capturable).  With train=True also
        in training mode with autograd on: ops.pyramid_block_train (batch statistics, the plane masks of Dropout2d from a host seed
        per block plus the device's dropout epoch, a backward with all three convolutions on the matrix unit; the seeds go to
        ``dropout_seed_hook`` as ("pyramid", block, (seed,))).  Every other combination, and CPU tensors, stay on the torch
        modules.  NotImplementedError, naming the block, for a structure the kernels do not cover.  Works together with
        ``enable_hip_graph()``: the packing behind the pyramid writes the static node-feature buffer, so one captured graph serves
        every batch.  Returns self."""
        if flag:
            for i in range(len(self.conv)):
                self._check_block(i)
        self.hip_pyramid, self.hip_pyramid_train = bool(flag), bool(flag and train)
        return self

    def _hip_route(self, frames: torch.Tensor) -> Optional[str]:
        if not (frames.is_cuda and frames.dtype == torch.float32):
            return None
        if self.hip_pyramid and not self.training and not torch.is_grad_enabled():
            return "eval"
        if self.hip_pyramid_train and self.training and torch.is_grad_enabled():
            return "train"
        return None

    def pyramid_maps(self, frames: torch.Tensor) -> List[torch.Tensor]:
        """[B, 128, F, F] -> the output of every block, in block order (sides cnn_layers_out_width)."""
        outs, x = [], frames
        route = self._hip_route(frames)
        if route is not None:
            x = x.contiguous()
            for i, blk in enumerate(self.conv):
                side_out = self._check_block(i)
                if side_out > x.shape[2]:
                    _refuse(f"conv[{i}].pool", f"output_size {side_out} enlarges the {x.shape[2]} x {x.shape[3]} map")
                if route == "eval":
                    x = E_ops.pyramid_block(x, blk.conv.weight, blk.conv.bias, blk.bn, side_out)
                else:
                    seed = 0
                    if blk.dropout.p > 0:
                        # drawn on the host, as nn.CNN draws its seeds; the kernel adds the device's epoch, so a replayed capture moves on
                        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                    if self.dropout_seed_hook is not None:
                        self.dropout_seed_hook("pyramid", i, (seed,))
                    x = E_ops.pyramid_block_train(x.contiguous(), blk.conv.weight, blk.conv.bias, blk.bn, side_out, blk.dropout.p, seed)
                outs.append(x)
            return outs
        for blk in self.conv:
            x = blk(x)
            outs.append(x)
        return outs

    def create_node_pixels(self, echo_frames: torch.Tensor, num_samples_per_batch: int, node_coords=None):
        """models.py:590-636: the last num_aux_graphs block outputs coarse to fine, then the frame itself; connection nodes start
        from the means of those maps in that order."""
        B = int(num_samples_per_batch)
        if self.use_main_graph_only:
            # the pyramid's outputs are not used; in training mode it runs as in the reference (its BatchNorm statistics move)
            if self.training:
                self.pyramid_maps(echo_frames)
            return self.pack_node_features([echo_frames], B, node_coords, None)
        outs = self.pyramid_maps(echo_frames)
        L = len(outs)
        maps = [outs[L - 1 - g] for g in range(self.num_aux_graphs)] + [echo_frames]
        conn = None
        mode = self._conn_rows_mode("level")
        if self.use_connection_nodes and not mode:
            conn = torch.stack([m.mean(dim=(2, 3)) for m in maps], dim=1)                     # [B, naux + 1, 128]
        return self.pack_node_features(maps, B, node_coords, conn, **mode)
