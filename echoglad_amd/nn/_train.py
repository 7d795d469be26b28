"""The train-mode autograd nodes over the C-ABI.

Three blocks, each written once as a pair of plain functions -- the layer (layer_fwd / layer_bwd), the classifier heads
(heads_fwd / heads_bwd) and the coordinate-graph update (_coord_update_fwd / _coord_update_bwd) -- and ONE node, _TrainFn, that
runs the blocks its Plan names in a fixed order.  Every kernel is reached as ``ops.<name>(...)``, looked up at call time."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import ops
from ._heads import _mlp_grads, _mlp_kernel_params, _stack_head_params, _unstack_head_grads, _without_running


class Routes:
    """Switches of the fused routes whose FALLBACK must exist anyway -- module states and shapes the fused kernels do not cover
    (frozen sub-modules, hooks, JumpingKnowledge on irregular handles, ...) take it by themselves -- so that a test can run the
    fallback on the inputs of the fused route and compare.  Python attributes, deliberately NOT environment variables (rounds 3 - 5
    had one EG_* knob per route: ~20 untimed routes a user could land on by accident; the run-time variables that are left are
    listed in include/echoglad_hip.h)."""
    layer_sums_in_heads = True      # the last layer's BatchNorm-backward sums inside the heads' backward
    coord_mlp_kernel = True         # node_coordinate_mlp on eg_coord_mlp_* (off: the torch modules)
    coord_fused = True              # coordinate update folded into the consuming node (off: autograd nodes of its own)
    act_in_heads = True             # the last layer's activation pass inside the heads' first kernel
    train_chain = True              # child sums handed from layer to layer in the train forward
    jk_fused = True                 # JumpingKnowledge('max') as a running maximum inside the layer kernels
    stacked_heads = True            # the four heads as one stacked network in train mode
    heads_recompute_h = True        # the last layer's output is never written in full: the heads' backward rebuilds its tile (off: h is kept)
    heads_state_in_place = True     # the 4 heads' parameters and running statistics LIVE in the stacked arrays the kernels take (off: copied per step)
    chain_layers = True             # eval: child sums handed from layer to layer (default of HierarchicalPatchModel.chain_layers)
    fuse_classifier = True          # eval: the heads inside the last layer's kernel (default of HierarchicalPatchModel.fuse_classifier)
    fold_last = True                # eval: ... from the last layer folded into the heads' first Linear (off: the layer's tile is formed in LDS)


ROUTES = Routes()


def _bn_step(bn: nn.BatchNorm1d, pending: Optional[list] = None):
    """What nn.BatchNorm1d.forward decides before calling F.batch_norm: (use batch statistics?, update factor | None).
    Counts the batch in ``num_batches_tracked``; ``momentum=None`` is the cumulative moving average.  ``pending``: a list that
    collects the counters instead (the caller bumps them all with one multi-tensor add: a launch per BatchNorm otherwise)."""
    use_batch = bn.training or bn.running_mean is None
    factor = None
    if bn.training and bn.track_running_stats and bn.running_mean is not None:
        if pending is not None and bn.momentum is not None:
            pending.append(bn.num_batches_tracked)
        else:
            with torch.no_grad():
                bn.num_batches_tracked += 1
        factor = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
    return use_batch, factor


class _GCNConvFn(torch.autograd.Function):
    """y = A_hat x W^T + b.  Backward: dx = (A_hat^T dy) W, dW = (A_hat^T dy)^T x, db = sum dy
    (graph.bwd is the graph itself whenever A_hat is symmetric, i.e. for every undirected edge_index)."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, batch):
        ctx.graph, ctx.batch = graph, batch
        ctx.save_for_backward(x, weight)
        return ops.gcn_layer_fwd(graph, batch, x.contiguous(), weight.contiguous(), None,
                                 bias.contiguous() if bias is not None else None, None, False)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gcn_layer_fwd(ctx.graph.bwd, ctx.batch, dy, weight.contiguous(), None, None, None, False,
                                   transpose_w=True)
        if ctx.needs_input_grad[1]:
            g = ops.gcn_aggregate(ctx.graph.bwd, ctx.batch, dy)
            dw = ops.dweight128(g, x.contiguous())
        if ctx.needs_input_grad[2]:
            db = ops.colsum128(dy)
        return dx, dw, db, None, None


# ---- BatchNorm-backward sums handed DOWN the stack ------------------------------------------------------------------------------
# dx of layer i + 1 is dy of layer i: the dX launch takes layer i's sums where the rows leave it (ops.gcn_layer_bwd(lower=)), and
# the node of layer i picks them up instead of running its own sums pass over dy and z.  The carrier is layer i's BOX, a two-slot
# list that both nodes of one step share (HierarchicalPatchModel._sums_down_boxes):
#   box[0]  forwards: (z, bn, relu, p, seed) of layer i, written by its forward, taken out by the forward of layer i + 1;
#   box[1]  backwards: (key of dx, sums entry), written by the backward of layer i + 1, taken out by the backward of layer i.
# The entry is used only if the dy that layer i receives still IS that dx -- address, shape, version, never a Python identity that
# autograd may not preserve: autograd accumulating another gradient into dx bumps the version, the sums would be stale, the entry is
# dropped and the layer takes its own.  Either way the backward of layer i leaves its box empty, and a box dies with its step.
def new_box() -> list:
    return [None, None]


def _sums_key(t: torch.Tensor) -> tuple:
    return (t.data_ptr(), tuple(t.shape), t.device, t._version)


def _hand_down(box: list, dx: torch.Tensor, sums, frames: int, row_hi: int, taps=None) -> None:
    box[1] = (_sums_key(dx), (sums, frames, 0, row_hi, taps))


def _handed_down(box: Optional[list], dy: torch.Tensor):
    """The ``dy_sums`` that the layer above left in ``box`` for this very dy, or None; the box is empty afterwards."""
    if box is None or box[1] is None:
        return None
    (key, entry), box[1] = box[1], None
    return entry if key == _sums_key(dy) else None


# ---- the layer block (models.py:328-335, :431-435) ------------------------------------------------------------------------------
class LayerCfg(NamedTuple):
    """One train-mode layer: z = A_hat x W^T + b;  out = relu|id(dropout(BN_batch(z))) [+ x].  kid_in / kid_out: child-sum side
    buffers of a chained train forward (the layer that produces x leaves the child sums of x behind, eg_gcn_layer_train_fwd).
    mine / below: the hand-down boxes of this layer and of the one below (above), row_hi: the rows of a frame the sums cover."""
    graph: ops.Graph
    batch: int
    relu: bool
    p: float
    seed: int
    residual: bool
    momentum: Optional[float]
    eps: float
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]
    kid_in: Optional[torch.Tensor] = None
    kid_out: Optional[torch.Tensor] = None
    mine: Optional[list] = None
    below: Optional[list] = None
    row_hi: int = 0


class _LayerState(NamedTuple):
    """What the backward reads of a LayerCfg (not the running statistics, not the child-sum buffers)."""
    graph: ops.Graph
    batch: int
    relu: bool
    p: float
    seed: int
    residual: bool
    had_agg: bool
    lower: Optional[tuple]          # (relu, p, seed, row_hi) of the layer below when its z and bn are the last two saved tensors
    mine: Optional[list]
    below: Optional[list]


def layer_fwd(x, weight, bias, gamma, beta, cfg: LayerCfg, want_out: bool = True):
    """-> (out | None, tensors to save, state).  Kept for the backward: z, the aggregated input A_hat x (so that dW = dz^T (A_hat x)
    needs no second aggregation) and the batch statistics -- not x; and z and bn of the layer below where this layer's dX launch is
    to take that layer's sums."""
    need_w = weight.requires_grad
    out, z, agg, bn = ops.gcn_layer_train_fwd(cfg.graph, cfg.batch, x, weight.contiguous(), bias.contiguous(), gamma.contiguous(),
                                              beta.contiguous(), cfg.running_mean, cfg.running_var, cfg.momentum, cfg.eps,
                                              cfg.relu, cfg.p, cfg.seed, cfg.residual, want_agg=need_w, kidsum_in=cfg.kid_in,
                                              kidsum_out=cfg.kid_out, want_out=want_out)
    if cfg.mine is not None:
        cfg.mine[0] = (z, bn, cfg.relu, cfg.p, cfg.seed)
    saved = [z, agg if agg is not None else z.new_zeros(0), weight.detach().contiguous(), gamma.detach().contiguous(),
             beta.detach().contiguous(), bn]
    lower = None
    if cfg.below is not None and cfg.below[0] is not None:           # (empty: the layer below ran as its torch modules)
        (lz, lbn, *lower), cfg.below[0] = cfg.below[0], None
        saved += [lz, lbn]
        lower = (*lower, cfg.row_hi)
    return out, saved, _LayerState(cfg.graph, cfg.batch, cfg.relu, cfg.p, cfg.seed, cfg.residual, need_w, lower, cfg.mine,
                                   cfg.below if lower is not None else None)


def layer_bwd(saved, st: _LayerState, dy, need_x: bool, need_w: bool, presum=None, patch=None):
    """-> ((dx, dw, db, dgamma, dbeta), what patch returned | None).  The BatchNorm-backward sums of dy come from ``presum`` (the
    heads' backward), else from the layer above through this layer's box, else from a pass of the layer's own.
    patch(dx, lower) -> (.., .., taps): a coordinate update in front of the layer, whose backward rewrites rows of dx AFTER the dX
    launch has taken the lower layer's sums -- it returns the sums of what it added, and they travel down with the others."""
    z, agg, weight, gamma, beta, bn, *lz = saved
    given = presum if presum is not None else _handed_down(st.mine, dy)
    lower = (lz[0], lz[1]) + st.lower if (st.lower is not None and need_x and st.residual) else None
    res = ops.gcn_layer_bwd(st.graph.bwd, st.batch, dy.contiguous(), z, agg if st.had_agg else None, weight, gamma, beta, bn,
                            st.relu, st.p, st.seed, st.residual, need_x, need_w and st.had_agg, dy_sums=given, lower=lower)
    patched = None if patch is None else patch(res[0], lower)
    if lower is not None:
        _hand_down(st.below, res[0], res[5], st.batch, lower[5], None if patched is None else patched[2])
    return res[:5], patched


# ---- the heads block (models.py:363-377, :485-490) ------------------------------------------------------------------------------
class HeadsCfg(NamedTuple):
    """Node-type filter (rows [row_lo, row_lo + n_valid) of every frame's n) + the four heads as one stacked network (first
    layers one [128 -> 128] product, 4 x BatchNorm1d(32) == BatchNorm1d(128) on the stacked output; second layers block-diagonal
    [128 -> 64]; third a 16-wide dot).  cls: epsilons, momenta, rates, seeds and the stacked running statistics
    (HierarchicalPatchModel._classifier_train_cfg)."""
    batch: int
    n: int
    row_lo: int
    n_valid: int
    sigmoid: bool
    cls: dict


class _HeadsState(NamedTuple):
    """What the backward reads: the row range, the kernels' parameters without the running statistics, was h written sparsely."""
    batch: int
    n: int
    row_lo: int
    n_valid: int
    sigmoid: bool
    P: dict
    h_sparse: bool


def heads_fwd(h, params, cfg: HeadsCfg, act=None):
    """-> (logits, h, tensors to save, state).  params: for each head its 10 parameters in _HEAD_PARAM_IDX order.  h: the rows the
    heads run on, or None in the act form, where the kernel produces them.
    act = (z, bn, residual rows | None, relu, p, seed) of the last layer, run with want_out=False: its activation pass runs inside
    the heads' first kernel (eg_classifier_train_fwd_act: h is written once and never read back for the heads' first product)."""
    B, n, row_lo, n_valid, sigmoid, cls = cfg
    P = _stack_head_params(params, cls)
    sparse = False
    if act is None:
        logits, z1, z2, bn = ops.classifier_train_fwd(h, B, n, row_lo, n_valid, P, sigmoid)
    else:
        # h = act(z) + h_prev feeds the heads' first product (inside this kernel) and, backwards, dW1 = dz1^T h: where the backward takes
        # the layer's sums in the heads' kernel it holds z anyway and rebuilds its h tile from z and h_prev, so h is never written in
        # full (1.18 GB per step at batch 32) -- only the coordinate rows the landmark MLP reads are
        sparse = bool(ROUTES.heads_recompute_h and ROUTES.layer_sums_in_heads and ops.classifier_recompute_h_supported(B, n, n_valid))
        h, logits, z1, z2, bn = ops.classifier_train_fwd_act(*act, B, n, row_lo, n_valid, P, sigmoid, h_sparse=sparse)
    saved = [h, z1, z2, bn, logits if sigmoid else logits.new_zeros(0)]
    return logits, h, saved, _HeadsState(B, n, row_lo, n_valid, sigmoid, _without_running(P), sparse)


def heads_bwd(saved, st: _HeadsState, dy, need_dh: bool, layer=None):
    """-> (dh | None, packed gradients, the layer's ``dy_sums`` | None).
    layer = (z, bn, gamma, beta, relu, p, seed, residual rows | None) of the layer whose output h is (the act form): its
    BatchNorm-backward sums over the heads' rows are taken where dh leaves the heads' backward (no separate sums pass over dh and z
    for the layer afterwards: only the rows the filter drops are added there)."""
    h, z1, z2, bn, y = saved
    B, n, row_lo, n_valid, sigmoid = st[:5]
    if dy is None:
        dy = torch.zeros(B * n_valid, 4, dtype=torch.float32, device=h.device)
    dl = dy.contiguous()
    if sigmoid:
        dl = dl * y * (1.0 - y)
    kw = {}
    if layer is not None and (st.h_sparse or (ops.classifier_layer_sums_supported(B, n, n_valid) and ROUTES.layer_sums_in_heads)):
        kw = dict(layer=layer[:7], recompute=(layer[7],) if st.h_sparse else False)
    dh, g, *sums = ops.classifier_bwd(dl, h, B, n, row_lo, n_valid, st.P, z1, z2, bn, need_dh, **kw)      # (dh: a buffer of this node)
    presum = (sums[0], B, row_lo, n_valid) if sums and sums[0] is not None else None
    return dh, g, presum


# ---- the coordinate-graph update (models.py:438-473) as part of the node that CONSUMES the layer output -------------------------
# The update of layer i reads the layer's output h (its 4 coordinate rows per frame -> node_coordinate_mlp -> new landmark
# positions), samples h's main grid at the new positions and overwrites the coordinate rows with the samples.  Under autograd
# that is a scatter into a [B*N,128] tensor and, backwards, a patch of 4 + up to 16 rows per frame of a [B*N,128] gradient.  Done
# as nodes of their own those patches either cost dense copies / adds per layer (autograd sums two [B*N,128] gradients), or have
# to happen in place on a gradient buffer that autograd may have handed to somebody else as well.  Neither: the update is
# folded into the NEXT node (layer i + 1, or the classifier heads after the last layer), whose backward allocates the gradient
# it returns -- every in-place row patch happens on a buffer that node created itself, and the forward overwrites rows of a
# tensor that is the fresh output of the node before it (nothing else holds it; forward_nodes takes this route only when no
# hook could have seen it).
class CoordCfg(NamedTuple):
    """frames, rows per frame, first main-grid row, frame side, first coordinate row; mlp: epsilons, momenta, rates, seeds, running
    statistics of node_coordinate_mlp[i] (HierarchicalPatchModel._coord_mlp_train_cfg)."""
    frames: int
    n: int
    main_base: int
    frame: int
    coord_base: int
    mlp: dict


def _coord_update_fwd(h, coords_prev, cfg: CoordCfg, mlp_params, sample=True):
    """h [B*N,128] (coordinate rows overwritten IN PLACE) -> (new coords [4B,2], the new coordinates once more in a tensor of their
    own -- `new` is saved for the backward, the other one is what the node hands out --, tensors to save, (dims, kernel parameters)
    for the backward).
    sample=False: the coordinate rows are NOT resampled (after the last layer nobody reads them -- the heads drop the coordinate
    rows, models.py:485 -- and with h written sparsely the main grid the samples would come from does not exist)."""
    B, n, main_base, frame, coord_base, mlp = cfg
    P = _mlp_kernel_params(mlp, mlp_params)
    flat = coords_prev.reshape(B * 4, 2).contiguous()
    # the MLP reads the coordinate rows where they live (and leaves the packed copy the backward needs: the rows change below),
    # the samples are written straight into them: no gather / scatter launches around the two kernels
    (new, new_out), lm, saved = ops.coord_update_fwd(h, flat, B, n, coord_base, main_base, P, True, frame, True, resample=sample)
    return new, new_out, [new, lm, flat, *saved], (cfg[:5], _without_running(P))


def _coord_update_bwd(dx, dcoords_new, h, saved, state, need_dprev, sampled_rows_used=True, lower=None):
    """dx: gradient w.r.t. the tensor AFTER the overwrite, a buffer the caller has just allocated; turned IN PLACE into the
    gradient w.r.t. the tensor BEFORE it.  -> (dcoords_prev [4B,2] | None, packed MLP gradients, taps | None).
    lower: dx is the dy of a layer whose BatchNorm-backward sums were taken before this call (ops.gcn_layer_bwd(lower=)): the sums
    of what the 16 taps per frame add are returned as taps [B,2,128]."""
    (B, n, main_base, frame, coord_base), P = state
    new, lm, flat, *saved = saved
    if sampled_rows_used:
        # the sampled rows' gradient is read where it lies (the coordinate rows of dx), 16 taps per frame go into dx's main-grid rows,
        # d lm is written into the coordinate rows (their old values were overwritten in the forward): one launch up to batch 16
        return ops.coord_update_bwd(dx, None if dcoords_new is None else dcoords_new.contiguous().view(B * 4, 2), h, new, lm, flat, B, n,
                                    coord_base, main_base, P, frame, tuple(saved), need_dprev, lower=lower)
    total = dcoords_new
    if total is None:
        total = torch.zeros(B * 4, 2, dtype=torch.float32, device=dx.device)
    # d lm is ADDED to the coordinate rows: they fed the MLP and nothing else, and their samples were not used
    _, dprev, g = ops.coord_mlp_bwd(total.contiguous().view(B * 4, 2), lm, flat, B, P, frame, tuple(saved), True, need_dprev,
                                    out_rows=(dx, n, coord_base), accumulate=True)
    return dprev, g, None


# ---- the node -------------------------------------------------------------------------------------------------------------------
class Plan(NamedTuple):
    """The blocks of one node, in the order they run:
        front   coordinate update on the node's input x (the update of the layer that produced x)
        layer   a train-mode layer on x
        heads   the classifier heads on the layer's output h -- with the layer's activation pass inside their first kernel -- or,
                without a layer, on x
        behind  coordinate update on h (layer + heads only: the heads drop the coordinate rows, so the rows it samples feed nothing)
    Every combination forward_nodes builds: layer | front + layer | heads | front + heads | [front +] layer + heads [+ behind]."""
    layer: Optional[LayerCfg] = None
    heads: Optional[HeadsCfg] = None
    front: Optional[CoordCfg] = None
    behind: Optional[CoordCfg] = None


class _TrainFn(torch.autograd.Function):
    """(x [B*N,128], coords [B,4,2] | None) -> (h or logits, coords [B,4,2] | None).
    params = [weight, bias, gamma, beta of the layer] + [10 tensors of front's MLP] + [10 of behind's] + [4 x 10 of the heads],
    each group present when its block is.  A coordinate update whose rows a layer of this node reads is differentiated through
    the bilinear samples; one that only the heads follow passes nothing but the MLP's gradient into the coordinate rows."""

    @staticmethod
    def forward(ctx, x, coords, plan, *params):
        layer, heads, front, behind = plan
        a = 0 if layer is None else 4
        b = a + (0 if front is None else 10)
        c = b + (0 if behind is None else 10)
        x = x.contiguous()
        out, coords_out = x, None
        # what the backward reads of each block, None where the node has none (the Plan itself is not kept: its configs hold the
        # running statistics and the child-sum buffers, which no backward needs)
        st_front = st_layer = st_heads = st_behind = None
        # x itself is kept only where a backward reads it: the update in front (its landmark rows), the heads' rebuilt h tile
        saved = [x] if front is not None or (layer is not None and heads is not None) else []
        cuts = [len(saved)]
        if front is not None:
            coords, coords_out, sv, st_front = _coord_update_fwd(x, coords, front, params[a:b])
            saved += sv
        cuts.append(len(saved))
        if layer is not None:
            out, sv, st_layer = layer_fwd(x, *params[:4], layer, want_out=heads is None)
            saved += sv
        cuts.append(len(saved))
        if heads is not None:
            if layer is None:
                out, h, sv, st_heads = heads_fwd(x, params[c:], heads)
            else:               # (the layer ran without its activation pass: z, bn and the residual rows go to the heads' first kernel)
                out, h, sv, st_heads = heads_fwd(None, params[c:], heads, (sv[0], sv[5], x if layer.residual else None, layer.relu,
                                                                          layer.p, layer.seed))
            saved += sv
            cuts.append(len(saved))
            if behind is not None:
                _, coords_out, sv, st_behind = _coord_update_fwd(h, coords, behind, params[b:c], sample=not st_heads.h_sparse)
                saved += sv
        ctx.blocks, ctx.cuts = (st_layer, st_heads, st_front, st_behind), cuts
        ctx.save_for_backward(*saved)
        # (coords_out: a tensor of its own, the update's `new` is saved for the backward)
        return out, None if coords_out is None else coords_out.view(-1, 4, 2)

    @staticmethod
    def backward(ctx, dy, dcoords=None):
        layer, heads, front, behind = ctx.blocks
        need = ctx.needs_input_grad             # (x, coords, plan, weight, bias, ...)
        saved, cuts = ctx.saved_tensors, ctx.cuts
        x = saved[0] if cuts[0] else None
        f_saved, l_saved = saved[cuts[0]:cuts[1]], saved[cuts[1]:cuts[2]]
        dc = None if dcoords is None else dcoords.reshape(-1, 2)
        g_layer = g_front = g_behind = g_heads = ()
        presum = None
        if heads is not None:
            h_saved = saved[cuts[2]:cuts[3]]
            of_layer = None if layer is None else (l_saved[0], l_saved[5], l_saved[3], l_saved[4], layer.relu, layer.p, layer.seed,
                                                   x if layer.residual else None)
            dy, g, presum = heads_bwd(h_saved, heads, dy, layer is not None or front is not None or need[0], of_layer)
            g_heads = _unstack_head_grads(g)
            if behind is not None:
                dc, g, _ = _coord_update_bwd(dy, dc, h_saved[0], saved[cuts[3]:], behind, front is not None or need[1],
                                             sampled_rows_used=False)
                g_behind = _mlp_grads(g)

        def front_bwd(dx, lower=None):
            return _coord_update_bwd(dx, dc, x, f_saved, front, need[1], sampled_rows_used=layer is not None, lower=lower)
        dx, patched = dy, None
        if layer is not None:
            (dx, dw, db, dgamma, dbeta), patched = layer_bwd(l_saved, layer, dy, front is not None or need[0], need[3], presum,
                                                             None if front is None else front_bwd)
            g_layer = (dw, db if need[4] else None, dgamma, dbeta)
        elif front is not None:
            patched = front_bwd(dx)
        if patched is not None:
            dc, g_front = patched[0], _mlp_grads(patched[1])
        if front is None and behind is None:
            dc = None
        return (dx if need[0] else None, None if dc is None else dc.view(-1, 4, 2), None) + g_layer + g_front + g_behind + g_heads


class _CoordMlpFn(torch.autograd.Function):
    """models.py:441-453 in train mode as one autograd node over eg_coord_mlp_fwd / eg_coord_mlp_bwd:
    (landmark rows [4B,128], coords [B,4,2]) -> clamp(coords + node_coordinate_mlp(cat(lm, pairwise offsets)), 0, frame-1).
    dims = (frames, frame side); ``params`` = the MLP's 10 parameters in _HEAD_PARAM_IDX order."""

    @staticmethod
    def forward(ctx, lm, coords, dims, cfg, *params):
        batch, frame = dims
        P = _mlp_kernel_params(cfg, params)
        lm = lm.contiguous()
        flat = coords.reshape(batch * 4, 2).contiguous()
        new, saved = ops.coord_mlp_fwd(lm, flat, batch, P, True, frame, True)
        ctx.P, ctx.dims = _without_running(P), dims
        ctx.save_for_backward(lm, flat, *saved)
        return new.view(batch, 4, 2)

    @staticmethod
    def backward(ctx, dnew):
        lm, flat, *saved = ctx.saved_tensors
        batch, frame = ctx.dims
        dlm, dc, g = ops.coord_mlp_bwd(dnew.contiguous().view(batch * 4, 2), lm, flat, batch, ctx.P, frame, tuple(saved),
                                       ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (dlm, dc.view(batch, 4, 2) if dc is not None else None, None, None) + _mlp_grads(g)
