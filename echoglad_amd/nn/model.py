"""HierarchicalPatchModel: the reference's model on the HIP kernels."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..topology import TopologySpec, get_topology
from ._heads import _HEAD_SIZES, _head_param_offsets, fold_last_into_heads, _mlp_kernel_params, _mlp_stats_cfg, _move_into, _seq_params, _views_of
from ._resolve import GraphResolver
from ._train import ROUTES, CoordCfg, HeadsCfg, LayerCfg, Plan, _CoordMlpFn, _TrainFn, _bn_step, new_box
from .modules import GCNConv, JumpingKnowledge, Sequential, _fold_bn, _versions

C = ops.C


def _mlp_head(in_f, hid, out_f, drop_p, last):
    return nn.Sequential(nn.Linear(in_f, hid), nn.BatchNorm1d(hid), nn.ReLU(inplace=True), nn.Dropout(p=drop_p),
                         nn.Linear(hid, hid // 2), nn.BatchNorm1d(hid // 2), nn.ReLU(inplace=True),
                         nn.Dropout(p=drop_p), nn.Linear(hid // 2, out_f), last)


class HierarchicalPatchModel(nn.Module):
    """Counterpart of the reference ``HierarchicalPatchModel`` (src/core/models.py:262-553).

    ``forward(data_batch=None, x=, node_coords=, edge_index=, node_type=, batch_idx=)``
    -> ``(logits [B*N_valid, n_out] (squeezed), node_coords [4B,2] | None)`` exactly as
    engine.py:248-255 calls it.  ``forward_nodes`` enters at the node features
    ``[B*N, 128]`` — the interval the throughput metric is defined on."""

    def __init__(self, frame_size: int = 32, gnn_dropout_p: float = 0.0, classifier_dropout_p: float = 0.0,
                 node_embedding_dim: int = 128, node_hidden_dim: int = 64, num_output_channels: int = 4,
                 num_gnn_layers: int = 3, num_aux_graphs: int = 4, gnn_jk_mode: str = "last",
                 classifier_hidden_dim: int = 16, residual: bool = True, use_coordinate_graph: bool = False,
                 output_activation: str = "sigmoid", use_connection_nodes=False, use_main_graph_only=False):
        super().__init__()
        if gnn_jk_mode not in ("last", "max", "cat"):
            raise ValueError("Only last, max or cat jumping knowledge mode is supported.")
        if node_embedding_dim != C:
            raise NotImplementedError(f"the HIP path is built for node_embedding_dim = {C} (node-feature packing, models.py:498-537)")
        if not (1 <= node_hidden_dim <= C):
            raise NotImplementedError(f"node_hidden_dim must be in [1, {C}]")
        # Widths other than configs/default.yml's 128 / 32 -- the reference's signature defaults are node_hidden_dim = 64,
        # classifier_hidden_dim = 16 (models.py:286-301) -- take a COMPATIBILITY route: GCNConv on the 128-channel kernels with
        # zero padding, BatchNorm / Dropout / activation / heads as the torch modules they are; none of the fused kernels.
        # With the coordinate graph on that route the landmark MLP (Linear(hidden + 8, cls_hidden) ...) runs as its torch modules and the
        # coordinate rows are resampled by eg_bilinear4_* from the node rows zero-padded to 128 channels.
        self._narrow = node_hidden_dim != C or classifier_hidden_dim != 32
        self.gnn_layers = nn.ModuleList()
        self.node_coordinate_mlp = nn.ModuleList()
        for i in range(num_gnn_layers):
            self.gnn_layers.append(Sequential("x, edge_index", [
                (GCNConv(in_channels=node_embedding_dim if i == 0 else node_hidden_dim,
                         out_channels=node_hidden_dim), "x, edge_index -> x"),
                nn.BatchNorm1d(node_hidden_dim),
                nn.Dropout(p=gnn_dropout_p),
                nn.Identity() if i == num_gnn_layers - 1 else nn.ReLU(inplace=True)]))
            if use_coordinate_graph:
                self.node_coordinate_mlp.append(
                    _mlp_head(node_hidden_dim + 8, classifier_hidden_dim, 2, classifier_dropout_p, nn.Identity()))
        self.output_activation = output_activation
        if output_activation == "sigmoid":
            make_last = nn.Sigmoid
        elif output_activation == "logit":
            make_last = nn.Identity
        else:
            raise ValueError(f"invalid output_activation:{output_activation}")
        self.node_classifiers = nn.ModuleList(
            [_mlp_head(node_hidden_dim, classifier_hidden_dim, 1, classifier_dropout_p, make_last())
             for _ in range(num_output_channels)])
        self.jk = JumpingKnowledge(gnn_jk_mode) if gnn_jk_mode != "last" else None
        self.frame_size = frame_size
        self.residual = residual
        self.num_gnn_layers = num_gnn_layers
        self.node_embedding_dim = node_embedding_dim
        self.num_aux_graphs = num_aux_graphs
        self.use_coordinate_graph = use_coordinate_graph
        self.use_connection_nodes = use_connection_nodes
        self.use_main_graph_only = use_main_graph_only
        self.classifier_hidden_dim = classifier_hidden_dim
        self.num_output_channels = num_output_channels
        # static topology implied by the constructor arguments (datasets.py:1441-1584); the graph
        # *type* ('grid' vs 'grid-diagonal') is dataset config, so it is verified per edge_index.
        self.topology_spec = TopologySpec(frame_size=frame_size, num_aux_graphs=num_aux_graphs,
                                          use_main_graph_only=bool(use_main_graph_only),
                                          use_coordinate_graph=bool(use_coordinate_graph),
                                          use_connection_nodes=bool(use_connection_nodes))
        self._resolver = GraphResolver(self.topology_spec)
        self._fold_cache: Dict[str, tuple] = {}
        self._hip_graphs: Dict[tuple, tuple] = {}
        self._static_feats: Dict[tuple, torch.Tensor] = {}
        self.hip_graph_captures = 0
        self.use_hip_graph = False
        self.hip_conn_rows = False          # a plain attribute: no parameter, no buffer, not in the state_dict (enable_hip_conn_rows)
        # eval path: layer i leaves the child sums of its output in a side buffer for layer i+1
        # (eg_gcn_layer_fwd_chain); False runs every layer on its own
        self.chain_layers = bool(ROUTES.chain_layers)
        # ... and the last layer runs the classifier heads on its output tile inside the kernel (False: separate)
        self.fuse_classifier = bool(ROUTES.fuse_classifier)
        self._kidsum: Dict[tuple, tuple] = {}
        # optional callable (layer index, layer output incl. residual and coordinate rows) -> None, called by forward_nodes
        self.layer_output_hook = None
        # optional callable (kind, module, seeds) -> None, called whenever a train-mode forward draws the seeds of a Dropout site:
        # ("gnn", gnn_layers[i], (seed,)), ("coord_mlp", node_coordinate_mlp[i], (seed1, seed2)), ("heads", node_classifiers,
        # (seed1, seed2)).  The mask of a site is a pure function of (seed, element index) (csrc/train_common.h): a test
        # regenerates the kernels' masks from these seeds and injects them into the oracle
        self.dropout_seed_hook = None

    def enable_hip_graph(self, flag: bool = True) -> "HierarchicalPatchModel":
        """Inference only: capture the kernel sequence of ``forward_nodes`` (3 fused layers + classifier
        + queue resets) into a HIP graph and replay it on later calls.

        Through ``forward()`` -- ``model(x=frames, edge_index=...)`` / ``model(data_batch)``, the calls engine.py:251-255,
        :394-398 make -- the node-feature packing in front of the stack (``pack_node_features`` / ``_linear``) writes into ONE static
        ``[B*N,128]`` buffer per (batch size, device), so every new batch of frames replays the SAME captured graph: the key
        is (that buffer's address, B, the resolved graph handle, parameter versions), never the identity of an input tensor.
        ``forward_nodes`` on a caller-owned buffer is captured once per buffer address (the buffer is kept alive by the entry).
        The returned logits tensor -- and, through ``forward()``, the node features -- are owned by the model and overwritten by
        the next call.  ``hip_graph_captures`` counts captures (a test asserts 1 over many batches)."""
        self.use_hip_graph = bool(flag)
        self._hip_graphs.clear()
        self._static_feats.clear()
        return self

    def enable_hip_conn_rows(self, flag: bool = True) -> "HierarchicalPatchModel":
        """Opt in (models with ``use_connection_nodes``; without them the switch has no effect): the connection rows of the node
        features are column means over the packed level rows themselves, taken in HIP inside the packing call's autograd node
        (``conn_rows=`` of ops.pyramid_pack / pack_levels / conv1x1_relu_pack_levels: eg_conn_rows_fwd / _bwd, a fixed order of
        summation both ways) -- no torch mean, no second pass over the level maps, no clone of the node array.  The values differ
        from the torch route's by the order of an fp32 sum.  Off (the default): nothing changes.  ``enable_hip_conn_rows(False)``
        while a UNet model's ``hip_tail`` is on is a ValueError: that tail is only reproducible with this switch.  Returns self."""
        if not flag and getattr(self, "hip_tail", False) and self.use_connection_nodes:
            raise ValueError("enable_hip_conn_rows(False) while enable_hip_frontend(tail=True) is on with use_connection_nodes=True: "
                             "switch the tail off first (the torch means would make the step non-reproducible)")
        self.hip_conn_rows = bool(flag)
        return self

    def _conn_rows_mode(self, mode: str) -> dict:
        """{"conn_rows": mode} where this model's connection rows come from the packing call (enable_hip_conn_rows), else {}: the
        keyword is passed on only with the switch on, every call with it off is the call it was."""
        return {"conn_rows": mode} if (self.hip_conn_rows and self.use_connection_nodes and not self.use_main_graph_only) else {}

    def _static_node_feats(self, B: int, inputs) -> Optional[torch.Tensor]:
        """The static node-feature buffer ``forward()``'s packing writes into when the call will take the replayed route
        (eval, nothing wants a gradient, no coordinate graph / narrow widths / hook), else None."""
        if not self.use_hip_graph or self.training or self._narrow or self.use_coordinate_graph or self.layer_output_hook is not None:
            return None
        if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in inputs) or
                                        any(p.requires_grad for p in self.parameters())):
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        dev = inputs[0].device
        if dev.type != "cuda":
            return None
        n = self._row_ranges()[0]
        key = (B, n, dev)
        buf = self._static_feats.get(key)
        if buf is None:
            if len(self._static_feats) >= 4:               # (entries of _hip_graphs keep the buffers their graphs read alive)
                self._static_feats.clear()
            buf = torch.empty(B * n, C, dtype=torch.float32, device=dev)
            self._static_feats[key] = buf
        return buf

    # ---- static row ranges (replace the reference's node_type host syncs, models.py:447,456,473,485)
    def _row_ranges(self):
        topo = get_topology(self.topology_spec)
        return topo.num_nodes, topo.n_conn, topo.num_valid_nodes, topo.main.base, topo.coord_base

    def train(self, mode: bool = True):
        """nn.Module.train + a fresh start for everything cached on in-place version counters (folded inference parameters, captured
        inference graphs): a training step replayed from a HIP graph (engine.GraphedTrainStep) runs no host code, so the running
        statistics it updates on the device bump no counter -- the switch to eval() in front of an evaluation is where that shows."""
        if bool(mode) != self.training:                # (a change of mode only: eval() in front of every batch keeps its graphs)
            self.__dict__.get("_fold_cache", {}).clear()
            graphs = self.__dict__.get("_hip_graphs")
            if graphs:
                graphs.clear()
        return super().train(mode)

    # ---- folded inference parameters, cached on parameter versions -------------------------
    def _folded_layers(self):
        key = tuple(_versions(l) for l in self.gnn_layers)
        hit = self._fold_cache.get("layers")
        if hit is None or hit[0] != key:
            with torch.no_grad():
                vals = []
                for l in self.gnn_layers:
                    conv, bn = l.module_0, l.module_1
                    scale, shift = _fold_bn(bn, conv.bias)
                    vals.append((conv.lin.weight.detach().contiguous(), scale, shift))
            hit = (key, vals)
            self._fold_cache["layers"] = hit
        return hit[1]

    def _packed_classifier(self):
        key = tuple(_versions(c) for c in self.node_classifiers)
        hit = self._fold_cache.get("cls")
        if hit is None or hit[0] != key:
            if self.num_output_channels != 4 or self.classifier_hidden_dim != 32:
                raise NotImplementedError("the fused classifier kernel is built for 4 heads of 128-32-16-1")
            with torch.no_grad():
                w1 = torch.cat([c[0].weight for c in self.node_classifiers], dim=0)           # [128,128]
                st1 = [_fold_bn(c[1], c[0].bias) for c in self.node_classifiers]
                w2 = torch.stack([c[4].weight for c in self.node_classifiers], dim=0)          # [4,16,32]
                st2 = [_fold_bn(c[5], c[4].bias) for c in self.node_classifiers]
                w3 = torch.cat([c[8].weight for c in self.node_classifiers], dim=0)            # [4,16]
                b3 = torch.cat([c[8].bias for c in self.node_classifiers], dim=0)              # [4]
                packed = {"w1": w1.contiguous(), "s1": torch.cat([s for s, _ in st1]).contiguous(),
                          "t1": torch.cat([t for _, t in st1]).contiguous(), "w2": w2.contiguous(),
                          "s2": torch.cat([s for s, _ in st2]).contiguous(),
                          "t2": torch.cat([t for _, t in st2]).contiguous(), "w3": w3.contiguous(),
                          "b3": b3.contiguous()}
            hit = (key, packed)
            self._fold_cache["cls"] = hit
        return hit[1]

    def _folded_last(self):
        """(m1, w1s, c1, lo planes) -- _heads.fold_last_into_heads and ops.fold_lo_table: the last layer (it has no ReLU) inside the heads' first Linear, for
        eg_gcn_layer_cls_fold_fwd.  Cached on the versions the two tables above are cached on."""
        key = (tuple(_versions(l) for l in self.gnn_layers), tuple(_versions(c) for c in self.node_classifiers))
        hit = self._fold_cache.get("fold_last")
        if hit is None or hit[0] != key:
            w, scale, shift = self._folded_layers()[-1]
            packed = self._packed_classifier()
            folded = fold_last_into_heads(w, scale, shift, packed["w1"], packed["s1"], packed["t1"], bool(self.residual))
            # ... and the lo planes of m1 and w1s the bf16 body streams (ops.fold_lo_table): held here, so that a captured graph
            # sees stable addresses
            hit = (key, folded + (ops.fold_lo_table(folded[0], folded[1]),))
            self._fold_cache["fold_last"] = hit
        return hit[1]

    # ---- one GNN layer in train mode: one autograd node over eg_gcn_layer_train_fwd / eg_gcn_layer_bwd ------------------
    def _layer_plan(self, i: int, graph: ops.Graph, gb: int, kid=(None, None), boxes=None, counters=None, row_hi: int = 0):
        """(LayerCfg, (weight, bias, gamma, beta)) of layer i for this step -- its dropout seed drawn, its batch counted -- or None
        when its BatchNorm / Dropout are frozen inside a training model.  boxes, row_hi: the hand-down of the BatchNorm-backward sums
        (_sums_down_boxes) over the rows [0, row_hi) of every frame."""
        layer = self.gnn_layers[i]
        conv, bn, drop = layer.module_0, layer.module_1, layer.module_2
        if not (bn.training and bn.affine and drop.training):
            return None
        p = float(drop.p)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0      # host RNG: reproducible under torch.manual_seed
        if self.dropout_seed_hook is not None:
            self.dropout_seed_hook("gnn", layer, (seed,))
        _, momentum = _bn_step(bn, counters)
        last = i == self.num_gnn_layers - 1
        mine, below = (None, None) if boxes is None else (None if last else boxes[i], boxes[i - 1] if i > 0 else None)
        cfg = LayerCfg(graph, gb, not last, p, seed, bool(self.residual), momentum, bn.eps, bn.running_mean, bn.running_var,
                       kid[0], kid[1], mine, below, row_hi)
        return cfg, (conv.lin.weight, conv.bias, bn.weight, bn.bias)

    def _layer_frozen(self, i: int, x_in: torch.Tensor, graph: ops.Graph, gb: int):
        """A frozen (eval-mode) BatchNorm / Dropout inside a training model: GCNConv kernel + the torch modules."""
        h = self.gnn_layers[i].forward_graph(x_in, graph, gb)
        return h + x_in if self.residual else h

    def _layer_train(self, i: int, x_in: torch.Tensor, graph: ops.Graph, gb: int, kid=(None, None)):
        plan = self._layer_plan(i, graph, gb, kid)
        if plan is None:
            return self._layer_frozen(i, x_in, graph, gb)
        return _TrainFn.apply(x_in, None, Plan(layer=plan[0]), *plan[1])[0]

    def _kid_pair(self, kids, i: int):
        """(child sums layer i reads | None, child sums it leaves behind | None) out of the two side buffers of a chained stack."""
        return kids[(i + 1) & 1] if i > 0 else None, kids[i & 1] if i < self.num_gnn_layers - 1 else None

    def _sums_down_boxes(self, graph: ops.Graph):
        """One box per layer for the hand-down of the BatchNorm-backward sums (layer i's forward fills box i, the node of layer
        i + 1 reads it, its dX launch takes layer i's sums and leaves them in the box: _train.new_box), or None where that launch is
        not the producer / consumer kernel's.  EG_SUMS_DOWN=0: every layer takes its own sums (the round-5 step; A/B and fallback)."""
        if not (self.residual and ops.lower_sums_supported(graph.bwd) and os.environ.get("EG_SUMS_DOWN", "1") != "0"):
            return None
        return [new_box() for _ in range(self.num_gnn_layers)]

    # ---- coordinate-graph update (models.py:438-473), explicit form ------------------------------------------------------
    def _coordinate_update(self, i: int, h: torch.Tensor, node_coords: torch.Tensor, batch: int):
        """The update as autograd nodes of its own (eval mode; train mode with hooks, JumpingKnowledge or frozen sub-modules):
        nothing is modified in place under autograd -- the overwrite of the coordinate rows copies h.  The training step's
        route folds the update into the node that consumes h instead (_train.Plan: front / behind)."""
        n, _, _, main_base, coord_base = self._row_ranges()
        fs = self.frame_size
        hd = h.shape[1]
        if hd != C:
            # the compatibility route (node_hidden_dim < 128): the torch modules on the landmark rows, the 4-tap sample on zero-padded rows
            lm = h.view(batch, n, hd)[:, coord_base:, :].reshape(batch * 4, hd)
            shape_feats = (node_coords.unsqueeze(1) - node_coords.unsqueeze(2)).reshape(batch * 4, 8)
            delta = self.node_coordinate_mlp[i](torch.cat((lm, shape_feats), dim=1))
            node_coords = torch.clamp(node_coords + delta.view(batch, 4, 2), min=0, max=fs - 1)
            new_feats = ops.bilinear4(F.pad(h, (0, C - hd)), node_coords, batch, n, main_base, fs)[:, :hd]
            out = h.clone()
            out.view(batch, n, hd)[:, coord_base:coord_base + 4, :] = new_feats.reshape(batch, 4, hd)
            return out, node_coords
        # pairwise (other - self) offsets per frame, flattened to 8 numbers per landmark (:441-444)
        lm = h.view(batch, n, C)[:, coord_base:, :].reshape(batch * 4, C).clone()
        new_coords = self._coord_mlp_kernel(self.node_coordinate_mlp[i], lm, node_coords, batch, fs)
        if new_coords is None:
            # a mix of frozen and training sub-modules, or eval mode with gradients: the torch modules, op by op
            shape_feats = (node_coords.unsqueeze(1) - node_coords.unsqueeze(2)).reshape(batch * 4, 8)
            delta = self.node_coordinate_mlp[i](torch.cat((lm, shape_feats), dim=1))
            new_coords = torch.clamp(node_coords + delta.view(batch, 4, 2), min=0, max=fs - 1)
        node_coords = new_coords
        new_feats = ops.bilinear4(h, node_coords, batch, n, main_base, fs)            # [4B, 128]
        h = ops.scatter_coord_rows(h, new_feats, batch, n, coord_base)
        return h, node_coords

    def _coord_mlp_cfg(self, mlp: nn.Sequential):
        """(cfg, params) of node_coordinate_mlp[i] for the kernels when every sub-module is in plain train state, else None."""
        if self._narrow or self.node_embedding_dim != C or not ROUTES.coord_mlp_kernel:
            return None
        m = mlp._modules                       # (nn.Sequential.__getitem__ walks an islice: ~170 of them per step were 0.2 ms of host time)
        bn1, bn2, d1, d2 = m["1"], m["5"], m["3"], m["7"]
        if not (bn1.affine and bn2.affine and bn1.training and bn2.training and d1.training and d2.training):
            return None
        return _mlp_stats_cfg(m), _seq_params(mlp)

    def _coord_mlp_train_cfg(self, mlp: nn.Sequential, pending: Optional[list] = None):
        """The same with this step's dropout seeds drawn and the BatchNorm batches counted (call once per forward)."""
        cfg, params = self._coord_mlp_cfg(mlp)
        if cfg["p1"] > 0 or cfg["p2"] > 0:
            cfg["seed1"], cfg["seed2"] = torch.randint(0, 2 ** 62, (2,)).tolist()     # host RNG, like the layers
        if self.dropout_seed_hook is not None:
            self.dropout_seed_hook("coord_mlp", mlp, (cfg["seed1"], cfg["seed2"]))
        _, cfg["momentum1"] = _bn_step(mlp[1], pending)
        _, cfg["momentum2"] = _bn_step(mlp[5], pending)
        return cfg, params

    def _coord_mlp_kernel(self, mlp: nn.Sequential, lm: torch.Tensor, node_coords: torch.Tensor, batch: int, frame: int):
        """models.py:441-453 on eg_coord_mlp_fwd / _bwd (one launch each way) -> new coords [B,4,2], or None when the
        module states are not ones the kernel implements."""
        if self._narrow or self.node_embedding_dim != C or node_coords.shape[-1] != 2 or node_coords.dtype != torch.float32 or \
                not ROUTES.coord_mlp_kernel:
            return None
        bn1, bn2, d1, d2 = mlp[1], mlp[5], mlp[3], mlp[7]
        if not (bn1.affine and bn2.affine):
            return None
        if self._coord_mlp_cfg(mlp) is not None:
            cfg, params = self._coord_mlp_train_cfg(mlp)
            return _CoordMlpFn.apply(lm, node_coords, (batch, frame), cfg, *params)
        cfg, params = _mlp_stats_cfg(mlp._modules), _seq_params(mlp)
        frozen = not (bn1.training or bn2.training or d1.training or d2.training)
        needs_grad = torch.is_grad_enabled() and (lm.requires_grad or node_coords.requires_grad or
                                                  any(p.requires_grad for p in params))
        if frozen and not needs_grad and bn1.running_mean is not None and bn2.running_mean is not None:
            P = _mlp_kernel_params(dict(cfg, momentum1=None, momentum2=None), params)
            new, _ = ops.coord_mlp_fwd(lm.contiguous(), node_coords.reshape(batch * 4, 2).contiguous(), batch, P, False, frame,
                                       False)
            return new.view(batch, 4, 2)
        return None

    # ---- the hot path: three routes -------------------------------------------------------------------------------------------
    def forward_nodes(self, node_feats: torch.Tensor, edge_index: torch.Tensor, batch: Optional[int] = None,
                      node_coords: Optional[torch.Tensor] = None):
        """node_feats [B*N,128] -> (logits [B*N_valid, n_out], node_coords | None)."""
        graph, gb = self._resolver.resolve(edge_index, node_feats.shape[0])
        n = self._row_ranges()[0]
        if node_feats.shape[0] % n != 0:
            raise RuntimeError(f"{node_feats.shape[0]} node rows is not a multiple of the {n} nodes per frame")
        B = node_feats.shape[0] // n
        if batch is not None and batch != B:
            raise RuntimeError(f"batch_idx implies {batch} frames but the node rows imply {B}")
        if self.use_coordinate_graph:
            node_coords = node_coords.reshape(B, 4, -1)
        else:
            node_coords = None
        fused = (not self.training) and (not torch.is_grad_enabled() or not node_feats.requires_grad) and not self._narrow
        fused = fused and self.layer_output_hook is None and not any(
            p.requires_grad and torch.is_grad_enabled() for p in self.parameters())
        # JumpingKnowledge('max') stays on the fused path as a running maximum written by the layer kernels
        # (eg_gcn_layer_fwd_jk); where those do not cover the handle the layers run one by one and torch takes the maximum,
        # as before: CSR graphs and pyramids without child sums (fused_classifier_ok is False), coordinate nodes, and the
        # handles with graph.hybrid set -- 'grid-diagonal' levels and connection nodes, which the kernel has no
        # running-maximum instantiation for (eg_launch_layer_ps refuses them)
        jk_fused = (fused and self.jk is not None and graph.fused_classifier_ok and not self.use_coordinate_graph
                    and not graph.hybrid and ROUTES.jk_fused)
        fused = fused and (self.jk is None or jk_fused)
        if fused:
            if self.use_hip_graph and not self.use_coordinate_graph and node_feats.is_contiguous() \
                    and not torch.cuda.is_current_stream_capturing():
                return self._forward_nodes_graphed(node_feats, edge_index, B), None
            return self._forward_eval_fused(node_feats, graph, gb, B, node_coords, jk_fused)
        if self._train_stack_ok(node_coords):
            return self._forward_train(node_feats, graph, gb, B, node_coords)
        return self._forward_stepwise(node_feats, graph, gb, B, node_coords)

    def forward_heads(self, node_feats: torch.Tensor, batch: int) -> torch.Tensor:
        """The last step of ``forward_nodes`` with no layer in front of it: node_feats [B*N, 128] -> the node-type filter (a row
        range per frame) and the four heads -> logits [B*N_valid, n_out].  What the reference's no-GNN baselines run behind
        ``create_node_pixels`` (models.py:791-797).  The heads' existing routes: eg_classifier_fwd in eval mode where nothing wants
        a gradient, the stacked heads node in training mode, the torch modules where neither applies (narrow widths, eval mode
        with gradients, frozen sub-modules)."""
        n, n_conn, n_valid, _, _ = self._row_ranges()
        B = int(batch)
        if node_feats.shape[0] != B * n:
            raise RuntimeError(f"{node_feats.shape[0]} node rows is not {B} frames of {n} nodes")
        h = node_feats.contiguous()
        wants_grad = torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in self.node_classifiers.parameters()))
        if not self.training and not wants_grad and not self._narrow:
            return ops.classifier_fwd(h, B, n, n_conn, n_valid, self._packed_classifier(), sigmoid=self.output_activation == "sigmoid")
        if self.training and self._stacked_heads_ok():
            return self._classifier_train(h, B, n, n_conn, n_valid)
        return self._classifier_modules(h, B, n, n_conn, n_valid)

    # ---- eval: folded layers, one launch each ---------------------------------------------------------------------------------
    def _forward_eval_fused(self, x0: torch.Tensor, graph: ops.Graph, gb: int, B: int, node_coords, jk_fused: bool):
        n, n_conn, n_valid, _, _ = self._row_ranges()
        L, coord = self.num_gnn_layers, self.use_coordinate_graph
        folded = self._folded_layers()
        kids = (None, None)
        # chained layers: each layer leaves the child sums of its output behind for the next one
        if self.chain_layers and not coord and graph.kidsum_rows > 0 and L > 1:
            kids = self._kidsum_buffers(graph, gb)
        # (a chained stack hands the last layer its child sums; a single layer has no layer in front of it that could, and the
        #  kernel pulls the child rows itself -- kidsum_in = NULL -- as the first layer of every stack does; graph.hybrid handles
        #  keep the separate heads there: their fused heads are tested with the child sums handed in only)
        fuse_cls = (self.fuse_classifier and graph.fused_classifier_ok and not coord
                    and (kids[0] is not None or graph.kidsum_rows == 0 or (L == 1 and self.chain_layers and not graph.hybrid))
                    and n_conn == graph.num_conn and n_valid == n - n_conn
                    and self.num_output_channels == 4 and self.classifier_hidden_dim == 32)
        jkb = self._jk_buffers(graph, gb, x0) if jk_fused else None
        sigmoid = self.output_activation == "sigmoid"
        h = x0.contiguous()
        for i in range(L):
            x_in, last = h, i == L - 1
            w, scale, shift = folded[i]
            kid_in, kid_out = self._kid_pair(kids, i)
            jk_prev = None if not jk_fused else (x_in if i == 0 else jkb[(i + 1) & 1])     # max over node features, h_1 .. h_i
            if last and fuse_cls:
                # the last layer hands its output tile to the classifier heads inside the kernel -- or, without the running
                # maximum, is part of their first Linear (it has no ReLU) and no such tile is formed
                if not jk_fused and ROUTES.fold_last:
                    out = ops.gcn_layer_cls_fold_fwd(graph, gb, x_in, self._folded_last(), bool(self.residual), self._packed_classifier(),
                                                     sigmoid=sigmoid, kidsum_in=kid_in)
                    return out.squeeze(1), None
                out = ops.gcn_layer_cls_fwd(graph, gb, x_in, w, scale, shift, x_in if self.residual else None, False,
                                            self._packed_classifier(), sigmoid=sigmoid, kidsum_in=kid_in, jk_in=jk_prev)
                return out.squeeze(1), None
            h = ops.gcn_layer_fwd(graph, gb, x_in, w, scale, shift, x_in if self.residual else None, relu=not last,
                                  kidsum_in=kid_in, kidsum_out=kid_out, jk_in=jk_prev, jk_out=jkb[i & 1] if jk_fused else None)
            if coord:
                h, node_coords = self._coordinate_update(i, h, node_coords, B)
        if jk_fused:
            h = jkb[(L - 1) & 1]
        out = ops.classifier_fwd(h, B, n, n_conn, n_valid, self._packed_classifier(), sigmoid=sigmoid)
        return out.squeeze(1), node_coords.reshape(B * 4, -1) if coord else None

    # ---- train: the stack as autograd nodes that hand straight on to each other -------------------------------------------------
    def _train_coord_fused_ok(self, node_coords) -> bool:
        if not (self.training and self.use_coordinate_graph and self.layer_output_hook is None and self.jk is None):
            return False
        if node_coords is None or node_coords.shape[-1] != 2 or node_coords.dtype != torch.float32:
            return False
        if not ROUTES.coord_fused or not self._stacked_heads_ok():
            return False
        for l in self.gnn_layers:
            if not (l.module_1.training and l.module_1.affine and l.module_2.training):
                return False
        return all(self._coord_mlp_cfg(m) is not None for m in self.node_coordinate_mlp)

    def _train_stack_ok(self, node_coords) -> bool:
        """Does nothing but the next node consume a node's output?  (A hook, JumpingKnowledge or the explicit coordinate update would
        put other gradients or row patches between the dX launch of a layer and the layer below.)"""
        if self.use_coordinate_graph:
            return self._train_coord_fused_ok(node_coords)
        return self.training and not self._narrow and self.layer_output_hook is None and self.jk is None

    def _act_in_heads_ok(self) -> bool:
        """Train mode without the coordinate graph: may the last layer + the heads run as one node?"""
        return (not self._narrow and not self.use_coordinate_graph and self.layer_output_hook is None and self.jk is None
                and self._stacked_heads_ok() and self._layer_cfg_static_ok(self.num_gnn_layers - 1)
                and ROUTES.act_in_heads)

    def _coord_plan(self, i: int, dims, counters):
        """(CoordCfg, the MLP's 10 parameters) of the update behind layer i for this step; dims: CoordCfg's first five fields."""
        mlp_cfg, params = self._coord_mlp_train_cfg(self.node_coordinate_mlp[i], counters)
        return CoordCfg(*dims, mlp_cfg), params

    def _forward_train(self, x0: torch.Tensor, graph: ops.Graph, gb: int, B: int, node_coords):
        """Step i < L: layer i, with the coordinate update of layer i - 1 in front of it; the last step: the heads, with the update of
        the last layer -- as a node of their own (step L), or as one node with the last layer (ROUTES.act_in_heads: the layer's
        activation pass runs inside the heads' first kernel).  A layer with a frozen BatchNorm / Dropout runs as its torch modules."""
        n, n_conn, n_valid, main_base, coord_base = self._row_ranges()
        dims = (B, n, main_base, self.frame_size, coord_base)
        L, coord = self.num_gnn_layers, node_coords is not None
        static = all(self._layer_cfg_static_ok(i) for i in range(L))
        kids = self._train_kidsums(graph, gb) if static else (None, None)
        boxes = self._down_boxes = self._sums_down_boxes(graph) if static else None       # (kept for one step: tests look into them)
        stacked = self._stacked_heads_ok()
        act_in_heads = bool(ROUTES.act_in_heads) if coord else self._act_in_heads_ok()
        # with the coordinate graph the num_batches_tracked of every BatchNorm of the step are bumped together by finish(counters);
        # without it each layer's is bumped as the layer runs
        counters = [] if coord else None
        nothing = (None, ())
        h, coords = x0.contiguous(), node_coords
        for i in range(L + 1):
            layer, params = nothing
            if i < L:
                # (the sums handed down cover the rows in front of the coordinate rows: all of them where there are none, coord_base == n)
                plan = self._layer_plan(i, graph, gb, self._kid_pair(kids, i), boxes, counters, coord_base)
                if plan is None:
                    h = self._layer_frozen(i, h, graph, gb)
                    continue
                layer, params = plan
            with_heads = i == L or (i == L - 1 and act_in_heads)
            if with_heads and not stacked:
                return self._classifier_modules(h, B, n, n_conn, n_valid).squeeze(1), None
            front, front_params = self._coord_plan(i - 1, dims, counters) if coord and i > 0 else nothing
            behind, behind_params = self._coord_plan(i, dims, counters) if coord and with_heads and i < L else nothing
            heads, head_params, finish = self._heads_plan(B, n, n_conn, n_valid) if with_heads else (None, (), None)
            updates = front is not None or behind is not None       # (layer 0 and the stacks without a coordinate graph: the node sees no coordinates)
            h, new_coords = _TrainFn.apply(h, coords if updates else None, Plan(layer, heads, front, behind), *params, *front_params,
                                           *behind_params, *head_params)
            if updates:
                coords = new_coords
            if with_heads:
                finish(counters or ())
                return h.squeeze(1), coords.reshape(B * 4, -1) if coord else None

    def _train_kidsums(self, graph: ops.Graph, gb: int):
        """Child-sum side buffers of the chained train forward (layer i leaves the child sums of its output for layer i + 1:
        eg_gcn_layer_train_fwd), or (None, None)."""
        if graph.kidsum_rows == 0 or self.num_gnn_layers < 2 or not ROUTES.train_chain:
            return None, None
        return self._kidsum_buffers(graph, gb)

    # ---- everything else: something sits between the layers -------------------------------------------------------------------
    def _forward_stepwise(self, x0: torch.Tensor, graph: ops.Graph, gb: int, B: int, node_coords):
        """Narrow widths, hooks, JumpingKnowledge outside the kernels, frozen sub-modules or ROUTES.coord_fused off with the
        coordinate graph (the explicit _coordinate_update), eval mode with gradients.  In train mode a layer is still one node
        (_layer_train) and the heads one stacked network (_classifier_train) where their module states allow it."""
        n, n_conn, n_valid, _, _ = self._row_ranges()
        train = self.training and not self._narrow
        kids = (None, None)
        if train and all(self._layer_cfg_static_ok(i) for i in range(self.num_gnn_layers)):
            kids = self._train_kidsums(graph, gb)
            if self.use_coordinate_graph:
                kids = (None, None)                   # (the explicit coordinate update rewrites rows)
        hidden = [x0.contiguous()]
        for i in range(self.num_gnn_layers):
            x_in = hidden[i]
            if train:
                h = self._layer_train(i, x_in, graph, gb, self._kid_pair(kids, i))
            else:
                h = self.gnn_layers[i].forward_graph(x_in, graph, gb)
                if self.residual and h.shape[1] == x_in.shape[1]:
                    h = h + x_in
            if self.use_coordinate_graph:
                h, node_coords = self._coordinate_update(i, h, node_coords, B)
            if self.layer_output_hook is not None:
                self.layer_output_hook(i, h)              # e.g. h.retain_grad() / h.register_hook(...) in a test
            hidden.append(h)
        h = self.jk(hidden) if self.jk is not None else hidden[-1]
        if self.training and self._stacked_heads_ok():
            out = self._classifier_train(h, B, n, n_conn, n_valid)
        else:
            out = self._classifier_modules(h, B, n, n_conn, n_valid)
        return out.squeeze(1), node_coords.reshape(B * 4, -1) if self.use_coordinate_graph else None

    # ---- the 4 classifier heads in train mode as ONE stacked network ----------------------------------------
    def _stacked_heads_ok(self) -> bool:
        mods = [hd._modules for hd in self.node_classifiers]
        ref = mods[0]["1"]
        plain_bn = all(m.training and m.affine and m.track_running_stats and m.momentum is not None and
                       m.momentum == ref.momentum and m.eps == ref.eps for md in mods for m in (md["1"], md["5"]))
        drops_on = all(m.training for md in mods for m in (md["3"], md["7"]))
        return (not self._narrow and self.num_output_channels == 4 and self.classifier_hidden_dim == 32 and self.node_embedding_dim == C
                and plain_bn and drops_on and ROUTES.stacked_heads)

    def _classifier_train_cfg(self):
        """(cfg, the 40 head parameters, finish()) for the heads block of a train node (_train.HeadsCfg.cls).  Running statistics: the
        kernels update stacked copies, which finish() writes back to the 8 BatchNorm modules with two multi-tensor copies."""
        heads = list(self.node_classifiers)
        bn1, bn2 = [hd._modules["1"] for hd in heads], [hd._modules["5"] for hd in heads]
        p1, p2 = float(heads[0]._modules["3"].p), float(heads[0]._modules["7"].p)
        seeds = torch.randint(0, 2 ** 62, (2,)).tolist() if (p1 > 0 or p2 > 0) else [0, 0]      # host RNG, like the layers
        if self.dropout_seed_hook is not None:
            self.dropout_seed_hook("heads", self.node_classifiers, tuple(seeds))
        params = [p for hd in heads for p in _seq_params(hd)]
        stat_list = [b.running_mean for b in bn1] + [b.running_var for b in bn1] + [b.running_mean for b in bn2] + [b.running_var for b in bn2]
        banks = self._heads_in_place(params, stat_list, bn1, bn2)
        with torch.no_grad():
            if banks is not None:                          # the modules' running statistics ARE the stacked arrays: nothing to copy, either way
                stats = banks[1]
            else:                                          # stacked copies of the running statistics: one multi-tensor copy
                stats = torch.empty(2 * 128 + 2 * 64, dtype=torch.float32, device=bn1[0].running_mean.device)
            rm1, rv1, rm2, rv2 = stats[:128], stats[128:256], stats[256:320], stats[320:384]
            if banks is None:
                torch._foreach_copy_(list(rm1.split(32)) + list(rv1.split(32)) + list(rm2.split(16)) + list(rv2.split(16)), stat_list)
        cfg = dict(running_mean1=rm1, running_var1=rv1, running_mean2=rm2, running_var2=rv2, eps1=bn1[0].eps, eps2=bn2[0].eps,
                   momentum1=bn1[0].momentum, momentum2=bn2[0].momentum, p1=p1, p2=p2, seed1=seeds[0], seed2=seeds[1])
        if banks is not None:
            cfg["_param_bank"] = banks[0]

        def finish(more_counters=()):
            with torch.no_grad():
                if banks is None:
                    torch._foreach_copy_(stat_list, list(rm1.split(32)) + list(rv1.split(32)) + list(rm2.split(16)) + list(rv2.split(16)))
                torch._foreach_add_([b.num_batches_tracked for b in bn1 + bn2] + list(more_counters), 1)
        return cfg, params, finish

    def _heads_in_place(self, params, stat_list, bn1, bn2):
        """(parameter bank [4 * sum(_HEAD_SIZES)], statistics bank [384]) with the 40 head parameters and the 16 running-statistics
        buffers living INSIDE them, in the stacked layout the kernels take -- or None (ROUTES.heads_state_in_place off, tensors that are
        not CUDA float32, a stream capture under way).  Stacking them per step was three multi-tensor copy launches; here the tensors
        are moved into the banks once (``p.data`` / the buffer re-pointed at its slice: same values, same Parameter objects, so
        optimizers, state_dict() and load_state_dict() see no difference) and every later step only checks addresses.  Whatever
        re-allocates them (``.to()``, a Parameter assigned by hand, copy.deepcopy of the model) is noticed by that check and they
        are moved again."""
        if not ROUTES.heads_state_in_place:
            return None
        offs_p = _head_param_offsets()
        offs_s = [32 * k for k in range(4)] + [128 + 32 * k for k in range(4)] + [256 + 16 * k for k in range(4)] + [320 + 16 * k for k in range(4)]
        banks = self.__dict__.get("_head_banks")
        if banks is not None and _views_of(banks[0], params, offs_p) and _views_of(banks[1], stat_list, offs_s):
            return banks
        dev = params[0].device
        if dev.type != "cuda" or any(t.dtype != torch.float32 or t.device != dev for t in list(params) + list(stat_list)) or \
                torch.cuda.is_current_stream_capturing():
            return None
        pbank = torch.empty(4 * sum(_HEAD_SIZES), dtype=torch.float32, device=dev)
        sbank = torch.empty(384, dtype=torch.float32, device=dev)

        def set_param(i, view):
            params[i].data = view

        def set_stat(i, view):
            kind, k = divmod(i, 4)
            setattr((bn1 if kind < 2 else bn2)[k], "running_mean" if kind % 2 == 0 else "running_var", view)
            stat_list[i] = view
        _move_into(pbank, params, offs_p, set_param)
        _move_into(sbank, stat_list, offs_s, set_stat)
        banks = self.__dict__["_head_banks"] = (pbank, sbank)
        return banks

    def _heads_plan(self, B: int, n: int, row_lo: int, n_valid: int):
        """(HeadsCfg, the 40 head parameters, finish()) of this step."""
        cls, params, finish = self._classifier_train_cfg()
        return HeadsCfg(B, n, row_lo, n_valid, self.output_activation == "sigmoid", cls), params, finish

    def _classifier_train(self, h: torch.Tensor, B: int, n: int, row_lo: int, n_valid: int) -> torch.Tensor:
        """models.py:363-377, :485-490 in train mode on the HIP kernels (the heads block of _train): the node-type filter is a row
        range, the four heads run as one stacked network."""
        heads, params, finish = self._heads_plan(B, n, row_lo, n_valid)
        out = _TrainFn.apply(h, None, Plan(heads=heads), *params)[0]
        finish()
        return out

    def _classifier_modules(self, h: torch.Tensor, B: int, n: int, row_lo: int, n_valid: int) -> torch.Tensor:
        """The same as the torch modules the heads are."""
        hv = h.view(B, n, h.shape[1])[:, row_lo:row_lo + n_valid, :].reshape(B * n_valid, h.shape[1])
        return torch.cat([clf(hv) for clf in self.node_classifiers], dim=1)

    def _layer_cfg_static_ok(self, i: int) -> bool:
        l = self.gnn_layers[i]
        return bool(l.module_1.training and l.module_1.affine and l.module_2.training)

    def _kidsum_buffers(self, graph, gb):
        key = (id(graph), gb)
        hit = self._kidsum.get(key)
        if hit is None or hit[0] is not graph:
            if len(self._kidsum) > 4:
                self._kidsum.clear()                  # (captured HIP graphs keep their own references, see below)
            hit = (graph, ops.new_kidsum(graph, gb), ops.new_kidsum(graph, gb))
            self._kidsum[key] = hit
        return hit[1], hit[2]

    def _jk_buffers(self, graph, gb, like):
        key = ("jk", id(graph), gb, tuple(like.shape))
        hit = self._kidsum.get(key)
        if hit is None or hit[0] is not graph:
            hit = (graph, torch.empty_like(like), torch.empty_like(like))
            self._kidsum[key] = hit
        return hit[1], hit[2]

    def _forward_nodes_graphed(self, node_feats, edge_index, B):
        # keyed on what the captured kernels actually point at: the input buffer's ADDRESS (the entry holds a reference to the
        # tensor it was captured on, so that address cannot be handed to anybody else while the entry lives: another tensor
        # object with the same data_ptr is a view of the same storage), the graph handle the edge_index resolves to (an equal
        # edge_index in a fresh tensor replays too), and the parameter versions -- not on the identity of either input tensor
        graph, gb = self._resolver.resolve(edge_index, node_feats.shape[0])
        banks = self.__dict__.get("_head_banks")          # (the heads' running statistics move when _heads_in_place re-banks them)
        key = (node_feats.data_ptr(), tuple(node_feats.shape), node_feats.device, id(graph), gb, B,
               tuple(_versions(l) for l in self.gnn_layers), tuple(_versions(c) for c in self.node_classifiers),
               None if banks is None else banks[1].data_ptr())
        hit = self._hip_graphs.get(key)
        if hit is not None and hit[4][0] is not graph:
            hit = None
        if hit is None:
            was = self.use_hip_graph
            self.use_hip_graph = False
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                     # warm-up outside capture (allocations, caches)
                    self.forward_nodes(node_feats, edge_index, B)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out, _ = self.forward_nodes(node_feats, edge_index, B)
            finally:
                self.use_hip_graph = was
            self.hip_graph_captures += 1
            if len(self._hip_graphs) > 8:
                self._hip_graphs.clear()
            # everything the captured kernels point at stays alive with the entry: the input buffer, the graph handle,
            # the child-sum side buffers and the folded / packed parameters (their caches may evict independently)
            keep = (graph, self._kidsum.get((id(graph), gb)), self._kidsum.get(("jk", id(graph), gb, tuple(node_feats.shape))),
                    self._fold_cache.get("layers"), self._fold_cache.get("cls"), self._fold_cache.get("fold_last"))
            hit = (g, out, node_feats, None, keep)
            self._hip_graphs[key] = hit
        hit[0].replay()
        return hit[1]

    # ---- avg-pool node features (models.py:498-537): the step in front of the hot path ---------
    def create_node_pixels(self, echo_frames: torch.Tensor, num_samples_per_batch: int, node_coords=None):
        """models.py:498-537: average-pooled pyramid of the frame embedding + the frame itself, node-major."""
        B = int(num_samples_per_batch)
        conn = None
        mode = self._conn_rows_mode("frame")
        if self.use_connection_nodes and not self.use_main_graph_only and not mode:
            conn = echo_frames.mean(dim=(2, 3)).unsqueeze(1).expand(B, self.num_aux_graphs + 1, C)
        sides = [] if self.use_main_graph_only else [2 ** g for g in range(1, self.num_aux_graphs + 1)]
        if sides and echo_frames.shape[1] == C and ops.pyramid_supported(echo_frames, sides) and os.environ.get("EG_POOL_PYRAMID", "1") != "0":
            # the pooled pyramid and the packing as ONE autograd node, two launches each way (eg_avg_pool_pyramid_*, eg_pack_levels):
            # torch's adaptive_avg_pool2d is a launch per level (219 us each at 224 x 224, batch 1) and, backwards, a launch of float
            # atomics per level (254 us each) -- 3.3 ms of a batch-1 training step whose GNN stack takes 1 ms
            n, n_conn = self._row_ranges()[:2]
            x = echo_frames.float()
            feats = ops.pyramid_pack(x, sides, B, n, n_conn, out=self._static_node_feats(B, [x, conn]), **mode)
            return self._finish_node_features(feats, B, node_coords, conn)
        maps = [F.adaptive_avg_pool2d(echo_frames, output_size=(p, p)) for p in sides]
        maps.append(echo_frames)
        return self.pack_node_features(maps, B, node_coords, conn, **mode)

    def _finish_node_features(self, feats, B, node_coords, connection_embed):
        """Connection-node rows and coordinate-node samples on top of the packed levels (models.py:524-533).  connection_embed
        None: the packing call has written the connection rows itself (``conn_rows=``)."""
        n, n_conn, _, main_base, coord_base = self._row_ranges()
        if n_conn and connection_embed is not None:
            feats = feats.clone() if feats.requires_grad else feats
            feats.view(B, n, C)[:, :n_conn, :] = connection_embed
        if self.use_coordinate_graph and not self.use_main_graph_only:
            new = ops.bilinear4(feats, node_coords.reshape(B, 4, 2).contiguous(), B, n, main_base, self.frame_size)
            feats = ops.scatter_coord_rows(feats, new, B, n, coord_base)
        return feats

    def pack_node_features(self, level_maps, num_samples_per_batch: int, node_coords=None, connection_embed=None,
                           conn_rows: Optional[str] = None):
        """The tail every create_node_pixels variant of the reference shares (models.py:511-537, :603-636, :726-756):
        NCHW level maps (coarse to fine, the last one is the frame-sized map) -> [B*N, 128] in the GNN's node order,
        in one packing launch (eg_pack_levels) instead of a per-sample permute / cat loop.  The UNet / CNN variants
        pass their own per-level feature maps and connection-node embeddings [B, naux+1, 128] -- or ``conn_rows`` ("level" /
        "frame", ops.pack_levels) and no embeddings: the packing call then takes the means itself."""
        B = int(num_samples_per_batch)
        n, n_conn = self._row_ranges()[:2]
        maps = [m.float() for m in level_maps]
        feats = ops.pack_levels(maps, B, n, n_conn, out=self._static_node_feats(B, maps + [connection_embed]),
                                **({"conn_rows": conn_rows} if conn_rows else {}))
        return self._finish_node_features(feats, B, node_coords, connection_embed)

    def pack_node_features_linear(self, features, linears, num_samples_per_batch: int, node_coords=None, connection_embed=None,
                                  backward: str = "torch", conn_rows: Optional[str] = None):
        """The UNet variant's whole tail (models.py:707-756): ``F.relu(self.linears[i](features[i]))`` for every level (1x1
        convolutions to 128 channels) AND the node-major packing in one launch (eg_conv1x1_relu_pack_levels); the 128-channel
        NCHW maps are never formed.  ``features``: decoder maps coarse to fine [B, C_l, p_l, p_l] (the last one frame-sized),
        ``linears``: the matching ``nn.Conv2d(C_l, 128, kernel_size=1)`` modules.  Connection-node embeddings
        [B, naux+1, 128] (means of the activated maps) come from the caller, as in ``pack_node_features``.  ``backward``: "torch" or
        "hip" (ops.conv1x1_relu_pack_levels: the fixed-order HIP backward of the tail).  ``conn_rows`` as in ``pack_node_features``."""
        B = int(num_samples_per_batch)
        n, n_conn = self._row_ranges()[:2]
        fl = [f.float() for f in features]
        ws, bs = [m.weight for m in linears], [m.bias for m in linears]
        feats = ops.conv1x1_relu_pack_levels(fl, ws, bs, B, n, n_conn,
                                             out=self._static_node_feats(B, fl + ws + bs + [connection_embed]), backward=backward,
                                             **({"conn_rows": conn_rows} if conn_rows else {}))
        return self._finish_node_features(feats, B, node_coords, connection_embed)

    def forward(self, data_batch=None, x=None, node_coords=None, edge_index=None, node_type=None, batch_idx=None):
        if data_batch is not None:
            x, edge_index, batch_idx, node_type = data_batch.x, data_batch.edge_index, data_batch.batch, \
                data_batch.node_type
            if self.use_coordinate_graph:
                node_coords = data_batch.node_coords
        # the reference reads B = batch_idx[-1] + 1 from the device (models.py:420); the frame
        # count is implied by the static topology, so no host sync is needed here.
        B = x.shape[0]
        nc = node_coords.reshape(B, 4, -1) if self.use_coordinate_graph else None
        node_feats = self.create_node_pixels(x, B, nc)
        return self.forward_nodes(node_feats, edge_index, B, node_coords)
