"""Train-mode layers and heads: the reductions and BatchNorm pieces, the whole train-mode layer forward and backward
(eg_gcn_layer_train_fwd / _bwd*), and the classifier heads' train forward and backward (eg_classifier_train_fwd* / _bwd*)."""
from __future__ import annotations

import ctypes as ct
import os
from typing import Optional

import torch

from .. import _lib
from ._core import C, _check, _check_rows, _check_vec, _cls_workspace, _scratch, _seed, _workspace, call, raw
from .graph import Graph


def colsum128(x: torch.Tensor) -> torch.Tensor:
    _check_rows(x, "x")
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    call("eg_colsum128", x, x.shape[0], _workspace(x.device), out)
    return out


def dweight128(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """g^T x -> [128(out), 128(in)]"""
    _check_rows(g, "g")
    _check_rows(x, "x", g.shape[0])
    out = torch.empty(C, C, dtype=torch.float32, device=x.device)
    call("eg_dweight128", g, x, x.shape[0], _workspace(x.device), out)
    return out


def bn_stats(x: torch.Tensor):
    """(mean[128], biased var[128]) over all rows."""
    _check_rows(x, "x")
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    var = torch.empty(C, dtype=torch.float32, device=x.device)
    call("eg_bn_stats", x, x.shape[0], _workspace(x.device), mean, var)
    return mean, var


def bn_act_fwd(z, scale, shift, residual=None, relu=False, dropout_p=0.0, seed=0) -> torch.Tensor:
    _check_rows(z, "z")
    _check_vec(scale, "scale", C)
    _check_vec(shift, "shift", C)
    _check_rows(residual, "residual", z.shape[0], optional=True)
    out = torch.empty_like(z)
    call("eg_bn_act_fwd", z, z.shape[0], scale, shift, residual, relu, dropout_p, _seed(seed), out)
    return out


def bn_act_fwd_tiles(graph: Graph, batch: int, z, scale, shift, residual=None, relu=False, dropout_p=0.0, seed=0,
                     kidsum_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bn_act_fwd in the layer kernels' tile order; kidsum_out (optional) receives the child sums of the result."""
    _check_rows(z, "z", graph.num_nodes * batch)
    _check_vec(scale, "scale", C)
    _check_vec(shift, "shift", C)
    _check_rows(residual, "residual", z.shape[0], optional=True)
    _check_rows(kidsum_out, "kidsum_out", graph.kidsum_rows * batch, optional=True)
    out = torch.empty_like(z)
    call("eg_bn_act_fwd_tiles", graph._h, batch, z, scale, shift, residual, relu, dropout_p, _seed(seed), out, kidsum_out)
    return out


def bn_act_bwd(dy, z, mean, invstd, gamma, beta, relu=False, dropout_p=0.0, seed=0):
    """-> (dz, dgamma, dbeta)"""
    _check_rows(dy, "dy")
    _check_rows(z, "z", dy.shape[0])
    for t, n in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (beta, "beta")):
        _check_vec(t, n, C)
    dz = torch.empty_like(z)
    dgamma = torch.empty(C, dtype=torch.float32, device=z.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=z.device)
    call("eg_bn_act_bwd", dy, z, z.shape[0], mean, invstd, gamma, beta, relu, dropout_p, _seed(seed), _workspace(z.device),
         dz, dgamma, dbeta)
    return dz, dgamma, dbeta


# ---------------------------------------------------------------------------
# whole train-mode layers (eg_gcn_layer_train_fwd / _bwd)
# ---------------------------------------------------------------------------
def gcn_layer_train_fwd(graph: Graph, batch: int, x, weight, bias, gamma, beta, running_mean, running_var, momentum,
                        eps: float, relu: bool, dropout_p: float, seed: int, residual: bool, want_agg: bool = True,
                        kidsum_in: Optional[torch.Tensor] = None, kidsum_out: Optional[torch.Tensor] = None,
                        want_out: bool = True):
    """-> (out, z, agg | None, bn [4,128] = mean, invstd, scale, shift).  running_* are updated in place
    (momentum None: no update).  kidsum_in / kidsum_out: child-sum side buffers of a chained train forward (`new_kidsum`)."""
    rows = graph.num_nodes * batch
    _check_rows(x, "x", rows)
    for name, t in (("kidsum_in", kidsum_in), ("kidsum_out", kidsum_out)):
        if t is not None:
            if graph.kidsum_rows == 0:
                raise RuntimeError("this graph handle has no child-sum side buffer (kidsum_rows == 0)")
            _check_rows(t, name, graph.kidsum_rows * batch)
    for t, n in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _check_vec(t, n, C)
    z = torch.empty_like(x)
    out = torch.empty_like(x) if want_out else None           # None: z, agg and the statistics only (no activation pass)
    agg = torch.empty_like(x) if want_agg else None
    bn = torch.empty(4, C, dtype=torch.float32, device=x.device)
    upd = momentum is not None and running_mean is not None
    call("eg_gcn_layer_train_fwd", graph._h, batch, x, weight, bias, gamma, beta, running_mean if upd else None,
         running_var if upd else None, float(momentum) if upd else -1.0, eps, relu, dropout_p, _seed(seed), residual,
         _workspace(x.device), z, agg, bn, out, kidsum_in, kidsum_out)
    return out, z, agg, bn


def lower_sums_supported(graph_bwd: Graph) -> bool:
    """May the dX launch on this handle also take the BatchNorm-backward sums of the layer below (eg_gcn_layer_bwd_lower)?"""
    return bool(graph_bwd.structured) and os.environ.get("EG_TRAIN_PS", "1") != "0"


def _lower_sums(lower, rows: int, row_hi: int = 0, tile_scratch=None, sums_out=None) -> "_lib.LowerSums":
    """eg_lower_sums from lower = (z, bn, relu, dropout_p, seed, ...) of the layer below.  The struct holds addresses only: the
    tensors behind them are the caller's, alive until the launch that reads the struct has been enqueued."""
    lz, lbn, lrelu, lp, lseed = lower[:5]
    _check_rows(lz, "lower z", rows)
    return _lib.LowerSums(lz.data_ptr(), lbn.data_ptr(), int(lrelu), float(lp), _seed(lseed), int(row_hi),
                          None if tile_scratch is None else tile_scratch.data_ptr(),
                          None if sums_out is None else sums_out.data_ptr())


def _given_sums(dy_sums) -> "_lib.GivenSums":
    sums, frames, row_lo, n_valid = dy_sums[:4]
    taps = dy_sums[4] if len(dy_sums) > 4 else None
    _check(sums, "dy_sums", dtype=torch.float64, numel=2 * C)
    if taps is not None:
        _check(taps, "taps", numel=int(frames) * 2 * C)
    gs = _lib.GivenSums(sums.data_ptr(), int(frames), int(row_lo), int(n_valid), None if taps is None else taps.data_ptr())
    gs._keep = (sums, taps)
    return gs


def gcn_layer_bwd(graph_bwd: Graph, batch: int, dy, z, agg, weight, gamma, beta, bn, relu: bool, dropout_p: float, seed: int,
                  residual: bool, need_dx: bool, need_dw: bool, dy_sums=None, lower=None):
    """-> (dx | None, dw | None, db | None (zeros), dgamma, dbeta)   [+ lower_sums when ``lower`` is given].
    dy_sums = (sums [256] float64, frames, row_lo, n_valid[, taps]) from classifier_bwd(..., layer=...) or from the dX launch of
    the layer above (``lower``): the BatchNorm-backward sums over those rows of every frame are given, the layer's own sums pass
    only adds the other rows (eg_gcn_layer_bwd_presummed / _lower); taps [frames, 2, 128]: bilinear4_bwd(..., lower=)'s sums.
    lower = (z, bn, relu, dropout_p, seed, row_hi) of the layer BELOW: the dX launch takes its BatchNorm-backward sums over rows
    [0, row_hi) of every frame from the rows it writes (eg_gcn_layer_bwd_lower) -> 6th result, float64 [256]."""
    rows = graph_bwd.num_nodes * batch
    dev = dy.device
    _check_rows(dy, "dy", rows)
    ls, lsums = None, None
    if lower is not None:
        if not (need_dx and residual and lower_sums_supported(graph_bwd)):
            raise RuntimeError("lower sums go with the producer / consumer kernel's dX launch (ops.lower_sums_supported, need_dx, residual)")
        _check(lower[1], "lower bn", numel=4 * C)           # the [4,128] float32 tensor of gcn_layer_train_fwd
        lsums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        tiles = _scratch("tiles", dev, graph_bwd.num_tiles * batch * 2 * C * 4)       # [tiles, 2, 128] floats: per-tile partials
        ls = _lower_sums(lower, rows, lower[5], tiles, lsums)
    dz = torch.empty_like(dy) if (need_dx or not need_dw) else None       # dW alone comes out of the fused apply pass
    dx = torch.empty_like(dy) if need_dx else None
    dw = torch.empty(C, C, dtype=torch.float32, device=dev) if need_dw else None
    small = torch.empty(3, C, dtype=torch.float32, device=dev)           # db, dgamma, dbeta
    common = (graph_bwd._h, batch, dy, z, agg, weight, gamma, beta, bn, relu, dropout_p, _seed(seed), residual, _workspace(dev),
              dz, dx, dw, small[0], small[1], small[2])
    if ls is not None or (dy_sums is not None and len(dy_sums) > 4 and dy_sums[4] is not None):
        # a lower layer to take sums for, or sums with the bilinear backward's later additions: the struct form
        gs = None if dy_sums is None else _given_sums(dy_sums)
        call("eg_gcn_layer_bwd_lower", *common, None if gs is None else ct.byref(gs), None if ls is None else ct.byref(ls))
    elif dy_sums is not None:
        sums, frames, row_lo, n_valid = dy_sums[:4]
        _check(sums, "dy_sums", dtype=torch.float64, numel=2 * C)
        call("eg_gcn_layer_bwd_presummed", *common, sums, int(frames), int(row_lo), int(n_valid))
    else:
        call("eg_gcn_layer_bwd", *common)
    res = (dx, dw, small[0], small[1], small[2])
    return res if lower is None else res + (lsums,)


# ---------------------------------------------------------------------------
# the classifier heads in train mode (eg_classifier_train_fwd / _fwd_act / _bwd / _bwd_sums)
# ---------------------------------------------------------------------------
CLS_GRADS_FLOATS = 19076
_CLS_TENSORS = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3", "running_mean1", "running_var1",
                "running_mean2", "running_var2")


def _cls_params(P: dict) -> "_lib.ClsTrainParams":
    s = _lib.ClsTrainParams()
    for k in _CLS_TENSORS:
        t = P.get(k)
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"classifier parameter {k} must be a contiguous CUDA float32 tensor")
        setattr(s, k, None if t is None else t.data_ptr())
    for k in ("eps1", "eps2", "p1", "p2"):
        setattr(s, k, float(P[k]))
    s.momentum1 = -1.0 if P.get("momentum1") is None else float(P["momentum1"])
    s.momentum2 = -1.0 if P.get("momentum2") is None else float(P["momentum2"])
    s.seed1, s.seed2 = _seed(P["seed1"]), _seed(P["seed2"])
    return s


def _heads_fwd_outputs(rows: int, dev):
    """(z1, z2, bn [768], logits) of the heads' train forward over `rows` filtered rows."""
    return (torch.empty(rows, C, dtype=torch.float32, device=dev), torch.empty(rows, 64, dtype=torch.float32, device=dev),
            torch.empty(4 * C + 4 * 64, dtype=torch.float32, device=dev), torch.empty(rows, 4, dtype=torch.float32, device=dev))


def classifier_train_fwd(h, batch: int, n_per_frame: int, row_lo: int, n_valid: int, P: dict, sigmoid: bool):
    """-> (logits [batch*n_valid,4], z1, z2, bn [768])"""
    _check_rows(h, "h", batch * n_per_frame)
    z1, z2, bn, logits = _heads_fwd_outputs(batch * n_valid, h.device)
    s = _cls_params(P)
    call("eg_classifier_train_fwd", h, batch, n_per_frame, row_lo, n_valid, ct.byref(s), _cls_workspace(h.device), z1, z2, bn,
         sigmoid, logits)
    return logits, z1, z2, bn


def classifier_recompute_h_supported(batch: int, n_per_frame: int, n_valid: int) -> bool:
    """May the heads' backward rebuild the layer output it needs from z and the residual (classifier_bwd(recompute=), so that
    classifier_train_fwd_act(h_sparse=True) never writes it)?  Where the layer's sums come out of the heads' backward, arrays < 2 GB."""
    lim = (1 << 31) - (1 << 20)
    return (classifier_layer_sums_supported(batch, n_per_frame, n_valid) and batch * n_valid * C * 4 < lim and
            batch * n_per_frame * C * 4 < lim)


def classifier_train_fwd_act(z, layer_bn, residual, relu: bool, dropout_p: float, seed: int, batch: int, n_per_frame: int,
                             row_lo: int, n_valid: int, P: dict, sigmoid: bool, h_sparse: bool = False):
    """The heads' train forward with the last GNN layer's activation pass folded in (eg_classifier_train_fwd_act): z, layer_bn =
    what gcn_layer_train_fwd(..., want_out=False) returned, residual = that layer's input rows or None.
    -> (h [batch*n_per_frame,128], logits [batch*n_valid,4], z1, z2, bn [768]).  h_sparse: only the rows of h OUTSIDE the heads'
    filter are written (the rest of the tensor is uninitialised memory: the backward must take classifier_bwd(recompute=))."""
    _check_rows(z, "z", batch * n_per_frame)
    _check_rows(residual, "residual", batch * n_per_frame, optional=True)
    h = torch.empty_like(z)
    z1, z2, bn, logits = _heads_fwd_outputs(batch * n_valid, z.device)
    s = _cls_params(P)
    call("eg_classifier_train_fwd_act", z, layer_bn, residual, relu, dropout_p, _seed(seed), h, batch, n_per_frame, row_lo,
         n_valid, ct.byref(s), _cls_workspace(z.device), z1, z2, bn, sigmoid, logits, bool(h_sparse))
    return h, logits, z1, z2, bn


def classifier_layer_sums_supported(batch: int, n_per_frame: int, n_valid: int) -> bool:
    """Does eg_classifier_bwd_sums cover this shape (the fused first-layers kernel: n_valid >= 64, < 2^32 elements)?"""
    return n_valid >= 64 and batch * n_per_frame * C < (1 << 32)


def classifier_bwd(dlogits, h, batch: int, n_per_frame: int, row_lo: int, n_valid: int, P: dict, z1, z2, bn, need_dh: bool,
                   layer=None, recompute=False):
    """-> (dh | None [batch*n_per_frame,128], grads [19076] packed as in include/echoglad_hip.h)
    layer = (z, bn, gamma, beta, relu, dropout_p, seed) of the GNN layer whose output h is: also returns that layer's
    BatchNorm-backward sums over the heads' rows, -> (dh, grads, sums [256] float64 | None) (eg_classifier_bwd_sums; None where
    the entry point does not cover the shape -- see classifier_layer_sums_supported -- and the plain backward ran instead).
    recompute = (residual rows | None,): h was written sparsely (classifier_train_fwd_act(h_sparse=True)); the kernel rebuilds the
    rows it needs from the layer's z and residual (needs ``layer``; classifier_recompute_h_supported)."""
    rows = batch * n_valid
    dev = h.device
    _check_rows(dlogits, "dlogits", rows, 4)
    dh1 = torch.empty(rows, C, dtype=torch.float32, device=dev)
    dh = torch.empty_like(h) if need_dh else None
    grads = torch.empty(CLS_GRADS_FLOATS, dtype=torch.float32, device=dev)
    s = _cls_params(P)
    common = (dlogits, h, batch, n_per_frame, row_lo, n_valid, ct.byref(s), z1, z2, bn, _cls_workspace(dev), dh1, dh, grads)
    if layer is None:
        call("eg_classifier_bwd", *common)
        return dh, grads
    lz, lbn, lgamma, lbeta, relu, p, seed = layer
    _check_rows(lz, "layer z", batch * n_per_frame)
    _check_vec(lgamma, "layer gamma", C)
    _check_vec(lbeta, "layer beta", C)
    sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
    rec = recompute is not False and recompute is not None
    res = recompute[0] if rec else None
    _check_rows(res, "layer residual", batch * n_per_frame, optional=True)
    rc = raw("eg_classifier_bwd_sums", *common, lz, lbn, lgamma, lbeta, relu, p, _seed(seed), sums, res, rec)
    if rc == _lib.EG_ERR_UNSUPPORTED and rec:
        raise RuntimeError("classifier_bwd(recompute=): " + _lib.last_error())      # (h does not exist: there is no plain backward to fall back to)
    if rc == _lib.EG_ERR_UNSUPPORTED:           # nothing was launched (include/echoglad_hip.h): the plain backward, no sums
        call("eg_classifier_bwd", *common)
        return dh, grads, None
    _lib.check(rc, "eg_classifier_bwd_sums")
    return dh, grads, sums
