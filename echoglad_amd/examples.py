"""Route A of INTEGRATION.md for the reference's UNet variant, as a runnable example.

``UNetNodeFeatureModel`` has the shape of the reference's ``UNETHierarchicalPatchModel`` (src/core/models.py:639-756; the class
``configs/default.yml`` names as ``unet_hierarchical_patch``): a convolutional encoder / decoder in front of the GNN whose
decoder maps become the node features of the levels.  The front-end is dense convolution work, written here with plain torch
modules (MIOpen); ``enable_hip_frontend()`` switches its eval-mode forward to the HIP front-end (frontend.hip), and with
``train=True`` its training-mode forward and backward as well (frontend_train.hip).  The
HIP path that is always on begins at the tail of ``create_node_pixels``, where the reference applies a 1x1 convolution + ReLU to
every decoder map and concatenates the permuted maps per sample in a Python loop (models.py:707-756).  That tail is ONE launch
here (``pack_node_features_linear`` -> eg_conv1x1_relu_pack_levels) and writes the GNN's input layout directly; everything
after it is the base class's ``forward_nodes``.  Its backward goes through torch's convolution gradients by default and, with
``enable_hip_frontend(..., tail=True)``, through the fixed-order eg_conv1x1_relu_pack_bwd.

``UNetNoGNN`` / ``UNet`` are the reference's ablations without a GNN (``UNETIntermediateNoGnn`` / ``UNET``, models.py:759-838): the
same front-end and tail, the node-type filter and the four heads; in eval mode everything behind the decoder is one launch
(``ops.conv1x1_relu_heads`` -> eg_conv1x1_relu_heads_fwd).

Module names (``down_convs.{i}.conv1 / BN1 / conv2 / BN2``, ``up_convs.{i}.*``, ``linears.{i}``) are the reference's, so a
reference checkpoint of this variant loads with ``strict=True`` (src/core/checkpointers.py:94-98)."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .nn import C, HierarchicalPatchModel, unet_decoder_maps, unet_decoder_maps_train
from .topology import get_topology


class _Down(nn.Module):
    """(conv3x3 -> ReLU -> BN) x 2 -> adaptive max pool to ``out_side`` (the reference's DownConv, models.py:841-856)."""

    def __init__(self, c_in: int, c_out: int, out_side: int):
        super().__init__()
        self.conv1, self.BN1 = nn.Conv2d(c_in, c_out, 3, padding=1), nn.BatchNorm2d(c_out)
        self.conv2, self.BN2 = nn.Conv2d(c_out, c_out, 3, padding=1), nn.BatchNorm2d(c_out)
        self.pool = nn.AdaptiveMaxPool2d(out_side)

    def forward(self, x):
        x = self.BN1(F.relu(self.conv1(x)))
        return self.pool(self.BN2(F.relu(self.conv2(x))))


class _Up(nn.Module):
    """upsample to ``out_side`` -> conv3x3 (halves the channels) -> cat(skip) -> conv3x3 (models.py:859-876)."""

    def __init__(self, c_in: int, c_out: int, out_side: int):
        super().__init__()
        self.upsample = nn.Upsample(size=out_side)
        self.conv1, self.BN1 = nn.Conv2d(c_in, c_out, 3, padding=1), nn.BatchNorm2d(c_out)
        self.conv2, self.BN2 = nn.Conv2d(c_in, c_out, 3, padding=1), nn.BatchNorm2d(c_out)

    def forward(self, x, skip):
        x = self.BN1(F.relu(self.conv1(self.upsample(x))))
        return self.BN2(F.relu(self.conv2(torch.cat([x, skip], dim=1))))


class UNetNodeFeatureModel(HierarchicalPatchModel):
    """``HierarchicalPatchModel`` whose node features come from a UNet decoder (same constructor as the reference class:
    ``encoder_embedding_widths`` / ``encoder_embedding_dims`` + the base class's keyword arguments; ``forward`` takes the
    embedder's ``[B, dims[0] // 2, F, F]`` frames, engine.py:240)."""

    def __init__(self, encoder_embedding_widths: Optional[List[int]] = None, encoder_embedding_dims: Optional[List[int]] = None,
                 **kwargs):
        super().__init__(**kwargs)
        widths = [128, 64, 32, 16, 8, 4, 2] if encoder_embedding_widths is None else list(encoder_embedding_widths)
        dims = [8, 16, 32, 64, 128, 256, 512] if encoder_embedding_dims is None else list(encoder_embedding_dims)
        if len(widths) != len(dims):
            raise ValueError("encoder_embedding_widths and encoder_embedding_dims must have the same length")
        if not self.use_main_graph_only and self.num_aux_graphs != len(widths):
            raise ValueError(f"the decoder yields {len(widths)} coarse maps (sides {sorted(widths)}) and the frame-sized one; "
                             f"num_aux_graphs={self.num_aux_graphs} levels need exactly that many")
        if not self.use_main_graph_only and sorted(widths) != [2 ** g for g in range(1, self.num_aux_graphs + 1)]:
            raise ValueError("level g of the graph is a 2^g x 2^g grid: the encoder widths must be those sides")
        self.down_convs = nn.ModuleList(_Down(d // 2, d, w) for d, w in zip(dims, widths))
        up_sides = list(reversed(widths))[1:] + [self.frame_size]
        self.up_convs = nn.ModuleList(_Up(d, d // 2, s) for d, s in zip(reversed(dims), up_sides))
        feats_in = list(reversed(dims)) + [dims[0] // 2]
        self.linears = nn.ModuleList(nn.Conv2d(c, self.node_embedding_dim, kernel_size=1) for c in feats_in)
        self.hip_frontend = False           # plain attributes: no parameter, no buffer, not in the state_dict
        self.hip_frontend_train = False
        self.hip_tail = False

    def enable_hip_frontend(self, flag: bool = True, train: bool = False, tail: bool = False) -> "UNetNodeFeatureModel":
        """Opt in: in eval mode with autograd off, ``decoder_maps`` runs on the HIP front-end (``nn.unet_decoder_maps``: 35
        launches, bit-reproducible) instead of torch's modules.  Training and eval with gradients keep the torch path, unless
        ``train=True``: then training mode with autograd on takes ``nn.unet_decoder_maps_train`` (batch statistics, HIP backward,
        bit-reproducible); eval with gradients stays on torch.  ``tail=True``, independent of ``train``: whenever autograd is on,
        the tail (``linears`` + ReLU + packing) takes its fixed-order HIP backward (eg_conv1x1_relu_pack_bwd) instead of torch's
        1 x 1 convolution gradients, the last piece of the step that was not reproducible bit for bit.  With
        ``use_connection_nodes`` only behind ``enable_hip_conn_rows()``: the torch connection-node means below differentiate torch's
        1 x 1 convolutions, so the step would silently stay non-reproducible."""
        if flag and tail and self.use_connection_nodes and not self.hip_conn_rows:
            raise ValueError("enable_hip_frontend(tail=True) with use_connection_nodes=True: the connection-node means of "
                             "create_node_pixels differentiate torch's 1 x 1 convolutions, the step would not be bit-reproducible "
                             "(call enable_hip_conn_rows() first: the means then run in HIP, in a fixed order)")
        self.hip_frontend = bool(flag)
        self.hip_frontend_train = bool(flag) and bool(train)
        self.hip_tail = bool(flag) and bool(tail)
        return self

    def decoder_maps(self, frames: torch.Tensor) -> List[torch.Tensor]:
        """[B, dims[0] // 2, F, F] -> the decoder's maps, coarse to fine: sides 2, 4, ..., 2^naux, F."""
        if self.hip_frontend and not self.training and not torch.is_grad_enabled():
            return unet_decoder_maps(self.down_convs, self.up_convs, frames)
        if self.hip_frontend_train and self.training and torch.is_grad_enabled():
            return unet_decoder_maps_train(self.down_convs, self.up_convs, frames)
        x, skips = frames, []
        for down in self.down_convs:
            skips.append(x)
            x = down(x)
        feats = [x]
        for up in self.up_convs:
            x = up(x, skips.pop())
            feats.append(x)
        return feats

    def create_node_pixels(self, echo_frames: torch.Tensor, num_samples_per_batch: int, node_coords=None):
        B = int(num_samples_per_batch)
        feats = self.decoder_maps(echo_frames)
        lin = list(self.linears)
        if self.use_main_graph_only:
            feats, lin = feats[-1:], lin[-1:]
        conn = None
        mode = self._conn_rows_mode("level")            # enable_hip_conn_rows: means over the packed rows, inside the packing node
        if self.use_connection_nodes and not self.use_main_graph_only and not mode:
            # the connection nodes start from the mean of every level's ACTIVATED map (models.py:737-752): activated here, once
            # more, on the coarse maps only -- they are a few percent of the frame-sized one -- and on the frame-sized map's mean
            with torch.set_grad_enabled(torch.is_grad_enabled()):
                conn = torch.stack([F.relu(m(f)).mean(dim=(2, 3)) for f, m in zip(feats, lin)], dim=1)        # [B, naux + 1, 128]
        return self.pack_node_features_linear(feats, lin, B, node_coords, conn, backward="hip" if self.hip_tail else "torch", **mode)


class UNetNoGNN(UNetNodeFeatureModel):
    """The reference's ablation ``UNETIntermediateNoGnn`` (src/core/models.py:759-799; ``unet_noGNN`` in its model registry): the
    UNet's ``create_node_pixels``, the rows with ``node_type != 0`` dropped, the four classifier heads -- no GNN layer in between.
    Constructor and state_dict keys are ``UNetNodeFeatureModel``'s (the reference's ablations construct the unused ``gnn_layers``
    too), so a reference checkpoint loads with ``strict=True``; ``gnn_layers`` never receive a gradient.

    In eval mode with autograd off the whole path behind the decoder is ONE launch (``ops.conv1x1_relu_heads``): the tail's
    128-channel rows go from LDS into the heads and are never written, and the rows the filter drops are never computed -- the
    bilinear samples of the coordinate nodes and the connection-node means, which the reference computes and then discards, are
    skipped.  Same logits, bit for bit, as the composed route ``forward_heads(create_node_pixels(...))`` that every other mode
    takes (and this one with ``fuse_tail = False``).  ``edge_index`` is accepted and never read: no graph handle is resolved."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.fuse_tail = True               # plain attribute, like hip_frontend

    def forward(self, data_batch=None, x=None, node_coords=None, edge_index=None, node_type=None, batch_idx=None):
        if data_batch is not None:
            x = data_batch.x
            if self.use_coordinate_graph:
                node_coords = data_batch.node_coords
        B = x.shape[0]
        if self.fuse_tail and not self.training and not torch.is_grad_enabled() and not self._narrow:
            feats, lin = self.decoder_maps(x), list(self.linears)
            if self.use_main_graph_only:
                feats, lin = feats[-1:], lin[-1:]
            rows, n_valid = sum(int(f.shape[2]) * int(f.shape[3]) for f in feats), self._row_ranges()[2]
            if rows != n_valid:
                raise RuntimeError(f"the decoder's levels give {rows} rows per frame, the topology has {n_valid} valid nodes")
            out = ops.conv1x1_relu_heads([f.float() for f in feats], [m.weight for m in lin], [m.bias for m in lin], B,
                                         self._packed_classifier(), sigmoid=self.output_activation == "sigmoid")
            return out.squeeze(1), None
        nc = node_coords.reshape(B, 4, -1) if self.use_coordinate_graph else None
        return self.forward_heads(self.create_node_pixels(x, B, nc), B).squeeze(1), None


class UNet(UNetNoGNN):
    """The reference's ``UNET`` (src/core/models.py:802-838; ``unet`` in its registry): the same forward under its second name."""


def reference_tail(model: UNetNodeFeatureModel, feats: List[torch.Tensor], B: int) -> torch.Tensor:
    """What the reference's tail computes with torch ops (plain levels, no connection / coordinate nodes): the check of the
    fused launch in tests/test_gpu_pack.py and the `unfused` leg of bench.py's end-to-end context number."""
    maps = [F.relu(m(f)) for f, m in zip(feats, model.linears)]
    rows = []
    for i in range(B):
        rows += [m[i].permute(1, 2, 0).reshape(-1, C) for m in maps]
    return torch.cat(rows, dim=0)
