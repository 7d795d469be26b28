"""The torch_geometric-compatible modules: GCNConv, Sequential, JumpingKnowledge, and the eval-mode parameter folding."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._resolve import _SHARED_RESOLVER
from ._train import LayerCfg, Plan, _GCNConvFn, _TrainFn, _bn_step

C = ops.C


def _fold_bn(bn: nn.BatchNorm1d, lin_bias: Optional[torch.Tensor]):
    """eval-mode BN(z + b) == z * scale + shift (without affine parameters: gamma = 1, beta = 0)."""
    gamma = bn.weight if bn.affine else torch.ones_like(bn.running_var)
    scale = gamma / torch.sqrt(bn.running_var + bn.eps)
    shift = (bn.bias if bn.affine else 0.0) - bn.running_mean * scale
    if lin_bias is not None:
        shift = shift + lin_bias * scale
    return scale.contiguous(), shift.contiguous()


def _versions(module: nn.Module) -> tuple:
    return tuple(t._version for t in list(module.parameters()) + list(module.buffers())) + \
           tuple(t.data_ptr() for t in module.parameters())


class _GlorotLinear(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        a = (6.0 / (in_channels + out_channels)) ** 0.5
        nn.init.uniform_(self.weight, -a, a)


class GCNConv(nn.Module):
    """Counterpart of ``torch_geometric.nn.GCNConv(in_channels, out_channels)`` as the
    reference constructs it (src/core/models.py:330-331: defaults improved=False,
    cached=False, add_self_loops=True, normalize=True, bias=True).
    ``forward(x, edge_index) -> x``.  The kernels are built for 128 -> 128 (default.yml:13-14); narrower layers -- the
    reference's signature defaults are 128 -> 64 -> 64 (models.py:286-301) -- run on the same kernels zero-padded to 128
    channels (a compatibility route: correct, differentiable, and half of its bytes are padding)."""

    def __init__(self, in_channels: int, out_channels: int, **kwargs):
        super().__init__()
        if not (1 <= in_channels <= C and 1 <= out_channels <= C):
            raise NotImplementedError(f"the HIP GCNConv is built for up to {C} channels, got {in_channels}->{out_channels}")
        for k, default in (("improved", False), ("cached", False), ("add_self_loops", True), ("normalize", True),
                           ("bias", True)):
            if kwargs.get(k, default) != default:
                raise NotImplementedError(f"GCNConv({k}={kwargs[k]!r}) is not supported")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = _GlorotLinear(in_channels, out_channels)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        graph, batch = _SHARED_RESOLVER.resolve(edge_index, x.shape[0])
        return self.forward_graph(x, graph, batch)

    def forward_graph(self, x, graph: ops.Graph, batch: int) -> torch.Tensor:
        if self.in_channels == C and self.out_channels == C:
            return _GCNConvFn.apply(x, self.lin.weight, self.bias, graph, batch)
        # narrower than the kernels' 128 channels: zero-padded input columns / weight rows and columns / bias, sliced output
        # (autograd runs through the pads and the slice, so the gradients of the real entries are the kernels' own)
        xp = F.pad(x, (0, C - self.in_channels))
        wp = F.pad(self.lin.weight, (0, C - self.in_channels, 0, C - self.out_channels))
        bp = F.pad(self.bias, (0, C - self.out_channels))
        return _GCNConvFn.apply(xp, wp, bp, graph, batch)[:, :self.out_channels]


class Sequential(nn.Module):
    """Counterpart of ``torch_geometric.nn.Sequential('x, edge_index', [(conv, 'x, edge_index -> x'), m, ...])``
    (src/core/models.py:329-335): children are registered as ``module_{i}``.

    The reference's layer -- ``[GCNConv, BatchNorm1d(128), Dropout, ReLU | Identity]`` -- is recognised and runs as ONE
    kernel launch through this module's own ``forward(x, edge_index)``, so the reference's ``models.py`` loop
    (``self.gnn_layers[i](hidden_embeds[i], edge_index)``, :431) reaches the fused kernels unchanged:
      * eval mode, no gradient wanted: ``eg_gcn_layer_fwd`` with bias + BatchNorm folded into scale / shift and the ReLU in
        the kernel's epilogue (three ``[B*N,128]`` elementwise passes fewer per layer);
      * train mode (BatchNorm on batch statistics, Dropout on): the layer block of ``_train`` as one autograd node
        (``eg_gcn_layer_train_fwd`` / ``eg_gcn_layer_bwd``) without a residual -- that stays the caller's
        ``h + hidden_embeds[i]`` (:434-435);
      * anything else (frozen sub-modules inside a training model, eval with gradients, forward hooks on a child, other
        module lists): module by module, as before.  ``EG_SEQ_FUSED=0`` forces that route."""

    def __init__(self, input_args: str, modules: Sequence):
        super().__init__()
        self._takes_graph: List[bool] = []
        for i, m in enumerate(modules):
            takes = False
            if isinstance(m, (tuple, list)):
                m, desc = m
                takes = "edge_index" in desc.split("->")[0]
            self.add_module(f"module_{i}", m)
            self._takes_graph.append(takes)
        self._fold: Optional[tuple] = None

    def __len__(self):
        return len(self._takes_graph)

    def __getitem__(self, i):
        return getattr(self, f"module_{i}")

    # ---- the reference's layer as one launch ------------------------------------------------------------------------
    def _reference_layer(self):
        """(conv, bn, dropout, relu?) when the children are exactly models.py:329-335's list and none of them is observed
        through a hook (a hook must see the intermediate tensor it was registered for), else None."""
        if self._takes_graph != [True, False, False, False] or os.environ.get("EG_SEQ_FUSED", "1") == "0":
            return None
        conv, bn, drop, act = self.module_0, self.module_1, self.module_2, self.module_3
        if type(conv) is not GCNConv or type(bn) is not nn.BatchNorm1d or bn.num_features != C or type(drop) is not nn.Dropout \
                or type(act) not in (nn.ReLU, nn.Identity):
            return None
        for m in (conv, bn, drop, act):
            if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
                return None
        return conv, bn, drop, type(act) is nn.ReLU

    def _folded(self, conv, bn):
        key = _versions(self)
        if self._fold is None or self._fold[0] != key:
            with torch.no_grad():
                self._fold = (key, conv.lin.weight.detach().contiguous(), *_fold_bn(bn, conv.bias))
        return self._fold[1:]

    def _fused(self, x, graph: ops.Graph, batch: int):
        """The layer as one launch, or None when this call is not one of the two fused cases."""
        ref = self._reference_layer()
        if ref is None or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != C:
            return None
        conv, bn, drop, relu = ref
        wants_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not bn.training and bn.running_mean is not None and not wants_grad and not (drop.training and drop.p > 0):
            w, scale, shift = self._folded(conv, bn)
            return ops.gcn_layer_fwd(graph, batch, x.contiguous(), w, scale, shift, None, relu)
        if bn.training and bn.affine and drop.training and torch.is_grad_enabled():
            p = float(drop.p)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0          # host RNG, like the model's own route
            _, momentum = _bn_step(bn)
            cfg = LayerCfg(graph, batch, relu, p, seed, False, momentum, bn.eps, bn.running_mean, bn.running_var)
            return _TrainFn.apply(x, None, Plan(layer=cfg), conv.lin.weight, conv.bias, bn.weight, bn.bias)[0]
        return None

    def _stepwise(self, x, conv_call):
        """Module by module; conv_call(m, x) runs a child that takes the graph."""
        for i, takes in enumerate(self._takes_graph):
            m = getattr(self, f"module_{i}")
            x = conv_call(m, x) if takes else m(x)
        return x

    def forward(self, x, edge_index):
        if self._reference_layer() is not None:
            graph, batch = _SHARED_RESOLVER.resolve(edge_index, x.shape[0])
            out = self._fused(x, graph, batch)
            if out is not None:
                return out
        return self._stepwise(x, lambda m, x: m(x, edge_index))

    def forward_graph(self, x, graph: ops.Graph, batch: int):
        out = self._fused(x, graph, batch)
        if out is not None:
            return out
        return self._stepwise(x, lambda m, x: m.forward_graph(x, graph, batch))


class JumpingKnowledge(nn.Module):
    def __init__(self, mode: str):
        super().__init__()
        if mode not in ("max",):
            raise NotImplementedError("only gnn_jk_mode in ('last', 'max') is supported "
                                      "('cat' cannot work in the reference either: models.py:365)")
        self.mode = mode

    def forward(self, xs):
        return torch.stack(xs, dim=-1).max(dim=-1)[0]
