"""A plain reference of the train-mode layer and of the four stacked classifier heads (train.hip, cls_train.hip, the train form of
gcn_layer*.hip): torch on the CPU, float64 by default, no kernel of the library in it.  The conventions are coord_reference.py's:
every function takes ``dtype`` (float64 is the truth, the same code in float32 the yardstick), kernel inputs are converted to double
exactly, gradients come from torch autograd in that dtype, and every reduction comes with the scale `coord_reference.Report.check`
needs: the same expression evaluated on absolute values, per output.  Purely elementwise quantities take their largest magnitude.

    |kernel - fp64| <= FACTOR * max|ref32 - fp64| + 8 * 2^-23 * scale          (coord_reference.Report, FACTOR = 4, unchanged)

Input condition (on the float64 reference alone): every BatchNorm output in front of a ReLU is at least
max(MARGIN, 2 * FACTOR * e32) away from 0, e32 = max|ref32 - fp64| of those outputs -- a kernel that meets the rule then cannot
sit on the other side of a kink, so no element of any compared array has to be left out of a comparison."""
import functools

import numpy as np
import torch

from coord_reference import FACTOR, MARGIN, hash_mask
from oracle import gnn_oracle as O
from echoglad_amd.topology import HierTopology, TopologySpec

C = 128
H1, H2, HEADS = 128, 64, 4                   # the stacked hidden widths (4 x 32, 4 x 16)
F64 = torch.float64
MOMENTUM, EPS = 0.1, 1e-5
GRAD_SLICES = (("w1", 128 * 128), ("b1", 128), ("gamma1", 128), ("beta1", 128), ("w2", 4 * 16 * 32), ("b2", 64), ("gamma2", 64),
               ("beta2", 64), ("w3", 64), ("b3", 4))            # grads [19076] of include/echoglad_hip.h
GRADS_FLOATS = sum(s for _, s in GRAD_SLICES)


# ---------------------------------------------------------------------------
# A_hat = D^-1/2 (A + I) D^-1/2 from edges: degree = 1 + in-edges (self loops of the list dropped, duplicates counted)
# ---------------------------------------------------------------------------
def edges_of(edge_index, n: int):
    """(n, source, target, weight of every edge, weight of every self loop), float64, of an arbitrary directed edge_index [2, E]
    over n nodes.  The forward aggregates over in-edges (out[target] += w x[source]); autograd through it aggregates over out-edges."""
    e = torch.from_numpy(np.array(edge_index, dtype=np.int64))
    e = e[:, e[0] != e[1]]
    deg = torch.ones(n, dtype=F64)
    deg.index_add_(0, e[1], torch.ones(e.shape[1], dtype=F64))
    dis = deg.pow(-0.5)
    return n, e[0], e[1], dis[e[0]] * dis[e[1]], dis * dis


def graph_types(diag_main=False, diag_aux=False):
    """(main_graph_type, aux_graph_type) of a TopologySpec: 'grid-diagonal' levels have 8 neighbours, 'grid' levels 4."""
    return ("grid-diagonal" if diag_main else "grid"), ("grid-diagonal" if diag_aux else "grid")


@functools.lru_cache(maxsize=None)
def topo_edges(frame, naux, main_only=False, coord=False, conn=False, diag_main=False, diag_aux=False):
    """edges_of one frame of the (frame, naux, main_only, coord, conn, diag_main, diag_aux) topology (eval_reference.topo_edges is
    this function)."""
    topo = HierTopology(TopologySpec(frame, naux, main_only, coord, conn, *graph_types(diag_main, diag_aux)))
    return edges_of(topo.edge_index(), topo.num_nodes)


def ahat(E, x, B: int):
    """A_hat x for every one of the B frames of x [B * n, 128] (x's dtype; stays on the autograd graph): the self term and an
    index_add over the edges.  With x >= 0 this is also the scale of the result (every weight is positive)."""
    n, src, dst, w_edge, w_self = E
    xv = x.view(B, n, C)
    out = xv * w_self.to(x.dtype)[None, :, None]
    out = out.index_add(1, dst, xv[:, src, :] * w_edge.to(x.dtype)[None, :, None])
    return out.reshape(B * n, C)


def ahat_t(E, x, B: int):
    """A_hat^T x: the aggregation over out-edges (what a backward handle computes)."""
    n, src, dst, w_edge, w_self = E
    return ahat((n, dst, src, w_edge, w_self), x, B)


def ahat_dense(E):
    n, src, dst, w_edge, w_self = E
    a = torch.diag(w_self.clone())
    a.index_put_((dst, src), w_edge, accumulate=True)
    return a


# ---------------------------------------------------------------------------
# BatchNorm with batch statistics
# ---------------------------------------------------------------------------
class _KeepMul(torch.autograd.Function):
    """x * keep, with a backward mask of its own.  The two are the same mask everywhere but in the mutation checks of
    test_train_reference.py (a backward that forgets 1 / (1 - p))."""

    @staticmethod
    def forward(ctx, x, keep, keep_bwd):
        ctx.save_for_backward(keep_bwd)
        return x * keep

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def _keep(x, mask, mask_bwd=None):
    if mask is None:
        return x
    m = mask.to(x.dtype)
    return x * m if mask_bwd is None else _KeepMul.apply(x, m, mask_bwd.to(x.dtype))


def _bn(z, gamma, beta, eps):
    """-> (y, mean, biased var, invstd, xhat) of nn.BatchNorm1d in train mode."""
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * invstd
    return xhat * gamma + beta, mean, var, invstd, xhat


def _stats(z, z_abs, mean, var, rmean, rvar, momentum, dtype):
    """The running statistics after nn.BatchNorm1d's update (momentum, unbiased variance) and the scales of mean, var and of both
    updates: mean |z|, mean (|z| + |mean|)^2, (1 - m) |old| + m * that."""
    R = z.shape[0]
    unb = R / (R - 1.0) if R > 1 else 1.0
    res = {}
    with torch.no_grad():
        mean_s = z_abs.to(F64).mean(0)
        var_s = ((z_abs.to(F64) + mean.detach().to(F64).abs()) ** 2).mean(0)
        res.update(mean_scale=mean_s, var_scale=var_s)
        if rmean is not None:
            rm, rv = rmean.detach().to(dtype), rvar.detach().to(dtype)
            res["running_mean"] = (1 - momentum) * rm + momentum * mean.detach()
            res["running_var"] = (1 - momentum) * rv + momentum * unb * var.detach()
            res["running_mean_scale"] = (1 - momentum) * rm.to(F64).abs() + momentum * mean_s
            res["running_var_scale"] = (1 - momentum) * rv.to(F64).abs() + momentum * unb * var_s
    return res


def _d(t):
    return t.detach().to(F64)


# ---------------------------------------------------------------------------
# one train-mode layer (train.hip: "one whole train-mode GNN layer")
# ---------------------------------------------------------------------------
def layer64(E, B, x, weight, bias, gamma, beta, rmean=None, rvar=None, momentum=MOMENTUM, eps=EPS, relu=True, p=0.0, seed=0,
            residual=True, dy=None, mask=None, mask_bwd=None, dtype=F64):
    """agg = A_hat x, z = agg W^T + b, batch statistics of z, running-statistics update, out = relu?(dropout(BN(z))) + (residual ? x : 0)
    -> {"agg", "z", "mean", "var", "invstd", "scale", "shift", "y" (the BatchNorm output), "out", "mask", "running_mean",
    "running_var"}; with an upstream dy also {"dx", "dw", "db", "dgamma", "dbeta", "g" (= dy * mask * gate), "dz"} and for every
    reduction "<name>_scale".  mask: hash_mask(rows, 128, p, seed) unless given."""
    rows = B * E[0]
    want = dy is not None
    xs, W, b, ga, be = (t.detach().to(dtype).clone().requires_grad_(want) for t in (x, weight, bias, gamma, beta))
    if mask is None and p > 0:
        mask = hash_mask(rows, C, p, seed)
    agg = ahat(E, xs, B)
    z = agg @ W.t() + b
    y, mean, var, invstd, xhat = _bn(z, ga, be, eps)
    v = _keep(y, mask, mask_bwd)
    if relu:
        v = torch.relu(v)
    out = v + xs if residual else v
    res = dict(agg=agg.detach(), z=z.detach(), mean=mean.detach(), var=var.detach(), invstd=invstd.detach(), y=y.detach(),
               out=out.detach(), mask=mask, scale=(ga * invstd).detach(), shift=(be - mean * ga * invstd).detach())
    with torch.no_grad():
        agg_s = ahat(E, _d(x).abs(), B)
        z_s = agg_s @ _d(weight).abs().t() + _d(bias).abs()
        res.update(agg_scale=agg_s, z_scale=z_s, shift_scale=_d(beta).abs() + (_d(mean) * _d(ga) * _d(invstd)).abs())
    res.update(_stats(z.detach(), z_s, mean, var, rmean, rvar, momentum, dtype))
    if not want:
        return res
    g_out = dy.detach().to(dtype)
    dx, dw, db, dga, dbe, dyy, dz = torch.autograd.grad(out, (xs, W, b, ga, be, y, z), g_out)
    res.update(dx=dx, dw=dw, db=db, dgamma=dga, dbeta=dbe, g=dyy, dz=dz)
    with torch.no_grad():
        g_a, dz_a = _d(dyy).abs(), _d(dz).abs()
        res.update(dgamma_scale=(g_a * _d(xhat).abs()).sum(0), dbeta_scale=g_a.sum(0), dw_scale=dz_a.t() @ _d(agg).abs(),
                   dx_scale=ahat_t(E, dz_a, B) @ _d(weight).abs() + (_d(dy).abs() if residual else 0.0))
    return res


def layer_bwd64(E, B, dy, z, agg, weight, gamma, beta, mean, invstd, relu, mask, residual, count=None, dtype=F64):
    """The layer's backward written out on the tensors the forward kept (no autograd; what eg_gcn_layer_bwd is given):
    g = dy * mask * gate, dbeta = sum g, dgamma = sum g xhat, dz = gamma invstd (g - dbeta / R - xhat dgamma / R),
    dx = (A_hat^T dz) W + (residual ? dy : 0), dw = dz^T agg -> the keys and scales of layer64's backward.  count: R (the mutation
    checks pass R - 1)."""
    dy, z, agg, W, ga, be, mean, invstd = (t.detach().to(dtype) for t in (dy, z, agg, weight, gamma, beta, mean, invstd))
    R = z.shape[0] if count is None else count
    xhat = (z - mean) * invstd
    g = dy if mask is None else dy * mask.to(dtype)
    if relu:
        g = g * (xhat * ga + be > 0).to(dtype)
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dz = ga * invstd * (g - dbeta / R - xhat * dgamma / R)
    dx = ahat_t(E, dz, B) @ W + (dy if residual else 0.0)
    res = dict(g=g, dz=dz, dbeta=dbeta, dgamma=dgamma, dx=dx, dw=dz.t() @ agg)
    g_a, dz_a = g.to(F64).abs(), dz.to(F64).abs()
    res.update(dgamma_scale=(g_a * xhat.to(F64).abs()).sum(0), dbeta_scale=g_a.sum(0), dw_scale=dz_a.t() @ agg.to(F64).abs(),
               dx_scale=ahat_t(E, dz_a, B) @ W.to(F64).abs() + (dy.to(F64).abs() if residual else 0.0))
    return res


def layer_sums64(dy, z, bn, gamma, beta, relu, mask, rows, dtype=F64, absolute=False):
    """The two per-channel sums [256] the layer's BatchNorm backward takes over the rows `rows` (an index or a boolean mask over the
    rows of z): sum g, sum g xhat with g = dy * mask * gate, xhat = (z - mean) invstd (eg_launch_bn_bwd; `layer_sums` of
    eg_classifier_bwd_sums, `sums_out` of eg_lower_sums).  bn [4, 128] = mean, invstd, scale, shift as the forward left them;
    the gate is (xhat gamma + beta > 0), or with gamma None (z scale + shift > 0), the form the dX launch has.
    absolute: the sums of the summands' magnitudes (the scale), dy then being the magnitude (or the scale) of the upstream gradient."""
    bn = bn.detach().to(dtype).reshape(4, C)
    dy, z = dy.detach().to(dtype)[rows], z.detach().to(dtype)[rows]
    xhat = (z - bn[0]) * bn[1]
    g = dy if mask is None else dy * mask.to(dtype)[rows]
    if relu:
        v = z * bn[2] + bn[3] if gamma is None else xhat * gamma.detach().to(dtype) + beta.detach().to(dtype)
        g = g * (v > 0).to(dtype)
    if absolute:        # (|xhat| <= invstd (|z| + |mean|): the dX launch sums g z per tile in float32 and takes mean sum g off afterwards)
        g, xhat = g.abs(), (z.abs() + bn[0].abs()) * bn[1].abs()
    return torch.cat([g.sum(0), (g * xhat).sum(0)])


def frame_rows(B, n, lo, hi):
    """Boolean mask over B * n rows: rows [lo, hi) of every frame."""
    m = torch.zeros(B, n, dtype=torch.bool)
    m[:, lo:hi] = True
    return m.reshape(-1)


# ---------------------------------------------------------------------------
# the four stacked heads (cls_train.hip)
# ---------------------------------------------------------------------------
def stack_heads(classifiers):
    """The eg_cls_train_params arrays (float32, CPU) of four oracle heads (Linear 128-32, BatchNorm, ReLU, Dropout, Linear 32-16,
    BatchNorm, ReLU, Dropout, Linear 16-1, activation): w1 [128,128] = 4 x [32,128], b1 / gamma1 / beta1 [128], w2 [4,16,32],
    b2 / gamma2 / beta2 [64], w3 [4,16], b3 [4], and the running statistics."""
    cat = lambda f: torch.cat([f(hd).detach().float().reshape(-1) for hd in classifiers])
    P = dict(w1=cat(lambda h: h[0].weight).view(128, 128), b1=cat(lambda h: h[0].bias), gamma1=cat(lambda h: h[1].weight),
             beta1=cat(lambda h: h[1].bias), w2=cat(lambda h: h[4].weight).view(4, 16, 32), b2=cat(lambda h: h[4].bias),
             gamma2=cat(lambda h: h[5].weight), beta2=cat(lambda h: h[5].bias), w3=cat(lambda h: h[8].weight).view(4, 16),
             b3=cat(lambda h: h[8].bias), running_mean1=cat(lambda h: h[1].running_mean), running_var1=cat(lambda h: h[1].running_var),
             running_mean2=cat(lambda h: h[5].running_mean), running_var2=cat(lambda h: h[5].running_var))
    hd = classifiers[0]
    P.update(eps1=hd[1].eps, eps2=hd[5].eps, momentum1=hd[1].momentum, momentum2=hd[5].momentum)
    return {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in P.items()}


def heads64(P, h, B, n, row_lo, n_valid, p=0.0, seed1=0, seed2=0, sigmoid=False, dlogits=None, mask1=None, mask2=None,
            mask_bwd=None, dtype=F64):
    """The heads over rows [row_lo, row_lo + n_valid) of every frame of h [B * n, 128] -> {"logits" [R, 4], "z1" [R, 128], "z2" [R, 64],
    "y1", "y2" (the BatchNorm outputs), "bn" [768] = {mean, invstd, scale, shift} of both layers, "running_*"}; with dlogits [R, 4]
    also "dh" [B * n, 128] (exactly zero outside the filter) and "grads" [19076]; and "<name>_scale" of every reduction
    ("bn_scale", "grads_scale" packed alike).  Masks: hash_mask(R, 128, p, seed1), hash_mask(R, 64, p, seed2)."""
    R = B * n_valid
    want = dlogits is not None
    names = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")
    Q = {k: P[k].detach().cpu().to(dtype).clone().requires_grad_(want) for k in names}
    hs = h.detach().to(dtype).clone().requires_grad_(want)
    if p > 0:
        mask1 = hash_mask(R, H1, p, seed1) if mask1 is None else mask1
        mask2 = hash_mask(R, H2, p, seed2) if mask2 is None else mask2
    mb1, mb2 = mask_bwd if mask_bwd is not None else (None, None)
    hv = hs.view(B, n, C)[:, row_lo:row_lo + n_valid, :].reshape(R, C)
    z1 = hv @ Q["w1"].t() + Q["b1"]
    y1, mean1, var1, invstd1, xhat1 = _bn(z1, Q["gamma1"], Q["beta1"], P["eps1"])
    a1 = _keep(torch.relu(y1), mask1, mb1)
    z2 = (torch.einsum("rhk,hok->rho", a1.view(R, HEADS, 32), Q["w2"]) + Q["b2"].view(HEADS, 16)).reshape(R, H2)
    y2, mean2, var2, invstd2, xhat2 = _bn(z2, Q["gamma2"], Q["beta2"], P["eps2"])
    a2 = _keep(torch.relu(y2), mask2, mb2)
    pre = (a2.view(R, HEADS, 16) * Q["w3"]).sum(-1) + Q["b3"]
    logits = torch.sigmoid(pre) if sigmoid else pre
    sc1, sc2 = Q["gamma1"] * invstd1, Q["gamma2"] * invstd2
    bn = torch.cat([mean1, invstd1, sc1, Q["beta1"] - mean1 * sc1, mean2, invstd2, sc2, Q["beta2"] - mean2 * sc2]).detach()
    res = dict(logits=logits.detach(), z1=z1.detach(), z2=z2.detach(), y1=y1.detach(), y2=y2.detach(), bn=bn, mask1=mask1, mask2=mask2)
    A = {k: _d(v).abs() for k, v in Q.items()}
    with torch.no_grad():
        z1_s = _d(hv).abs() @ A["w1"].t() + A["b1"]
        z2_s = (torch.einsum("rhk,hok->rho", _d(a1).abs().view(R, HEADS, 32), A["w2"]) + A["b2"].view(HEADS, 16)).reshape(R, H2)
        # (the sigmoid's slope is at most 1 / 4: the scale of the sum in front of it bounds its rounding as well)
        res.update(z1_scale=z1_s, z2_scale=z2_s, logits_scale=(_d(a2).abs().view(R, HEADS, 16) * A["w3"]).sum(-1) + A["b3"] + 1.0 * sigmoid)
    st1 = _stats(z1.detach(), z1_s, mean1, var1, P.get("running_mean1"), P.get("running_var1"), P["momentum1"], dtype)
    st2 = _stats(z2.detach(), z2_s, mean2, var2, P.get("running_mean2"), P.get("running_var2"), P["momentum2"], dtype)
    for i, (st, mean, var) in enumerate(((st1, mean1, var1), (st2, mean2, var2)), 1):
        res.update({f"mean{i}": mean.detach(), f"var{i}": var.detach(), f"mean{i}_scale": st["mean_scale"], f"var{i}_scale": st["var_scale"]})
        for k in ("running_mean", "running_var"):
            if k in st:
                res[f"{k}{i}"], res[f"{k}{i}_scale"] = st[k], st[k + "_scale"]
    with torch.no_grad():
        big = lambda t: torch.full_like(_d(t), float(_d(t).abs().max()))
        res["bn_scale"] = torch.cat([st1["mean_scale"], big(invstd1), big(sc1), A["beta1"] + (_d(mean1) * _d(sc1)).abs(),
                                     st2["mean_scale"], big(invstd2), big(sc2), A["beta2"] + (_d(mean2) * _d(sc2)).abs()])
    if not want:
        return res
    g = dlogits.detach().to(dtype).reshape(R, HEADS)
    grads = torch.autograd.grad(logits, [hs] + [Q[k] for k in names] + [z1, y1, z2, y2, pre], g)
    dh, pg = grads[0], grads[1:11]
    dz1, dy1, dz2, dy2, dpre = (_d(t).abs() for t in grads[11:])
    res.update(dh=dh, grads=torch.cat([t.reshape(-1) for t in pg]))
    with torch.no_grad():
        scales = [dz1.t() @ _d(hv).abs(), torch.zeros(H1, dtype=F64), (dy1 * _d(xhat1).abs()).sum(0), dy1.sum(0),
                  torch.einsum("rho,rhk->hok", dz2.view(R, HEADS, 16), _d(a1).abs().view(R, HEADS, 32)), torch.zeros(H2, dtype=F64),
                  (dy2 * _d(xhat2).abs()).sum(0), dy2.sum(0), dpre[:, :, None] .mul(_d(a2).abs().view(R, HEADS, 16)).sum(0), dpre.sum(0)]
        res["grads_scale"] = torch.cat([t.reshape(-1) for t in scales])
        dh_s = torch.zeros(B, n, C, dtype=F64)
        dh_s[:, row_lo:row_lo + n_valid, :] = (dz1 @ A["w1"]).view(B, n_valid, C)
        res["dh_scale"] = dh_s.reshape(B * n, C)
    return res


# ---------------------------------------------------------------------------
# the input condition and the cases of tests/test_gpu_train_fp64.py
# ---------------------------------------------------------------------------
SEED_L, SEED1, SEED2 = 4321, 101, 202       # the dropout seeds of the layer and of the heads' two hidden layers in every test


def condition(outs64, outs32, masks=()):
    """(smallest magnitude of the BatchNorm outputs in front of a ReLU, the margin max(MARGIN, 2 FACTOR e32) they have to keep, the
    ReLU-active share of every one of them, the kept share of every mask) -- outs64 / outs32: those outputs in float64 / float32."""
    e32 = max(float((b.to(F64) - a).abs().max()) for a, b in zip(outs64, outs32))
    return (min(float(a.abs().min()) for a in outs64), max(MARGIN, 2 * FACTOR * e32), [float((a > 0).double().mean()) for a in outs64],
            [float((m > 0).double().mean()) for m in masks if m is not None])


def condition_met(cond):
    smallest, margin, active, kept = cond
    return smallest >= margin and all(0.25 <= a <= 0.75 for a in active) and all(0.45 <= k <= 0.55 for k in kept)


def assert_input_condition(cond):
    assert condition_met(cond), cond
    return cond


# -- the layer: (kind, handle arguments..., B).  "topo": (frame, naux, main_only, coord, conn); "directed": a random directed graph
# (nodes, edges); "batched": the undirected (frame, naux) graph of B frames as ONE edge list (a CSR handle, batch 1)
TOPO_HANDLES = [(8, 1, False, False, False),        # 68 nodes: a 4-row last tile
                (16, 3, False, False, False),
                (17, 3, False, False, False),       # ragged patches
                (16, 2, True, False, False),        # main grid only: no child sums
                (16, 3, False, True, False),        # coordinate nodes
                (16, 3, False, False, True)]        # connection nodes
LAYER_CASES = [("topo",) + h + (B,) for h in TOPO_HANDLES for B in (1, 3)] + [("directed", 300, 1500, 1), ("batched", 16, 3, 2)]
# "diag": (frame, naux, main_only, coord, conn, diag_main, diag_aux) -- handles with 'grid-diagonal' (8-neighbour) levels, whose
# train forward and residual dX run as the {mode 1 / 2 / 3, diag} forms of the producer / consumer kernel (ps_form.h), the
# activation pass with child sums in tile order (bn_act_tiles.hip), the connection-node pre-pass (conn.hip) and, residual off, the
# symmetric kernel on the handle's one-frame CSR
DIAG_TRAIN_HANDLES = [(16, 3, False, False, False, True, True),        # both grids diagonal
                      (17, 3, False, True, False, True, True),         # ragged patches + coordinate nodes
                      (30, 3, False, False, False, False, True),       # aux levels only; sides that do not divide the frame
                      (16, 2, True, False, False, True, False),        # main grid only: no child sums
                      (8, 2, False, False, False, True, True),         # levels below 8 columns: node by node, parents never written
                      (16, 3, False, False, True, True, True),         # connection nodes on diagonal levels
                      (30, 3, False, True, True, True, False)]         # connection + coordinate nodes, diagonal main grid
DIAG_CASES = [("diag",) + h + (B,) for h in DIAG_TRAIN_HANDLES for B in (1, 3)]
LAYER_CASES += DIAG_CASES
# input seeds found on the CPU (search_seed: the first of at most 200 that meets the condition); a case it finds none for gets a smaller B
LAYER_SEED = {("topo", 8, 1, False, False, False, 1): 1000, ("topo", 8, 1, False, False, False, 3): 1000,
              ("topo", 16, 3, False, False, False, 1): 1002, ("topo", 16, 3, False, False, False, 3): 1021,
              ("topo", 17, 3, False, False, False, 1): 1001, ("topo", 17, 3, False, False, False, 3): 1008,
              ("topo", 16, 2, True, False, False, 1): 1005, ("topo", 16, 2, True, False, False, 3): 1020,
              ("topo", 16, 3, False, True, False, 1): 1001, ("topo", 16, 3, False, True, False, 3): 1036,
              ("topo", 16, 3, False, False, True, 1): 1000, ("topo", 16, 3, False, False, True, 3): 1057,
              ("directed", 300, 1500, 1): 1000, ("batched", 16, 3, 2): 1015}
# the "diag" cases: search_seed(layer_condition, case, 1000, tries=4000), the condition, the margin and the headroom as they are.  The
# 200 seeds of the default search hold none for (17, 3, coordinate nodes) at B = 3 (1131 rows: 1371 is the first) and none for the two
# frame-30 handles (984 / 992 nodes) at B = 3 or at B = 2.  Those two run at B = 2 (LAYER_B: about 252 000 BatchNorm outputs, of
# which none may lie within 1.5 x 2.2e-5 of 0), where 1871 / 4377 are the first seeds with the search's headroom of 1.5
LAYER_SEED.update({("diag", 16, 3, False, False, False, True, True, 1): 1004, ("diag", 16, 3, False, False, False, True, True, 3): 1077,
                   ("diag", 17, 3, False, True, False, True, True, 1): 1000, ("diag", 17, 3, False, True, False, True, True, 3): 1371,
                   ("diag", 30, 3, False, False, False, False, True, 1): 1006, ("diag", 30, 3, False, False, False, False, True, 3): 1871,
                   ("diag", 16, 2, True, False, False, True, False, 1): 1001, ("diag", 16, 2, True, False, False, True, False, 3): 1034,
                   ("diag", 8, 2, False, False, False, True, True, 1): 1000, ("diag", 8, 2, False, False, False, True, True, 3): 1000,
                   ("diag", 16, 3, False, False, True, True, True, 1): 1008, ("diag", 16, 3, False, False, True, True, True, 3): 1023,
                   ("diag", 30, 3, False, True, True, True, False, 1): 1020, ("diag", 30, 3, False, True, True, True, False, 3): 4377})
# case -> the B it runs with where that is not the B it names
LAYER_B = {("diag", 30, 3, False, False, False, False, True, 3): 2, ("diag", 30, 3, False, True, True, True, False, 3): 2}

# -- the lower layer's sums out of the dX launch: ((frame, naux, main_only, coord, conn, diag_main, diag_aux), B, row_hi - n of every
# run).  row_hi = n: every row of a frame; n - 4: without the last four (the coordinate rows, where a handle has them)
LOWER_SUMS_CASES = [((16, 3, False, False, False, False, False), 2, (0, -4)),
                    ((224, 7, False, False, False, False, False), 4, (-4,)),        # above TILE_SUMS_SMALL: the two-stage reduction
                    ((16, 3, False, True, False, False, False), 2, (0, -4)),        # coordinate nodes
                    ((16, 3, False, False, True, False, False), 2, (0,)),           # connection nodes
                    ((16, 3, False, False, False, True, True), 2, (0,)),            # diagonal
                    ((16, 3, False, False, True, True, True), 2, (0,)),             # diagonal + connection nodes
                    ((8, 2, False, False, False, True, True), 2, (0,)),             # diagonal levels that run node by node
                    ((30, 3, False, True, True, True, False), 2, (0, -4))]          # coordinate + connection nodes, diagonal main grid


def layer_edges(case):
    """(E, frames the reference and the kernels walk, rows) of a layer case."""
    kind, B = case[0], LAYER_B.get(case, case[-1])
    if kind in ("topo", "diag"):
        E = topo_edges(*case[1:-1])
        return E, B, B * E[0]
    if kind == "directed":
        n, m = case[1], case[2]
        rs = np.random.RandomState(1)
        E = edges_of(np.stack([rs.randint(0, n, m), rs.randint(0, n, m)]).astype(np.int64), n)
        return E, 1, n
    topo = HierTopology(TopologySpec(case[1], case[2]))
    E = edges_of(topo.batched_edge_index(B), B * topo.num_nodes)
    return E, 1, B * topo.num_nodes


def case_edge_index(case):
    """The edge_index [2, E] int64 of a "directed" / "batched" case (what Graph.csr takes)."""
    if case[0] == "directed":
        rs = np.random.RandomState(1)
        return np.stack([rs.randint(0, case[1], case[2]), rs.randint(0, case[1], case[2])]).astype(np.int64)
    return HierTopology(TopologySpec(case[1], case[2])).batched_edge_index(LAYER_B.get(case, case[-1])).astype(np.int64)


def layer_inputs(case, seed=None):
    """float32 inputs of a layer case: x, W, bias, gamma, beta, running mean / var before the step, the upstream dy."""
    rows = layer_edges(case)[2]
    rs = np.random.RandomState(LAYER_SEED.get(case, 1000) if seed is None else seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return dict(x=f(rs.standard_normal((rows, C))), weight=f(rs.uniform(-0.15, 0.15, (C, C))), bias=f(0.1 * rs.standard_normal(C)),
                gamma=f(1 + 0.3 * rs.standard_normal(C)), beta=f(0.1 * rs.standard_normal(C)), rmean=f(0.2 * rs.standard_normal(C)),
                rvar=f(rs.uniform(0.5, 1.5, C)), dy=f(rs.standard_normal((rows, C))))


def layer_condition(case, seed=None):
    E, B, rows = layer_edges(case)
    I = layer_inputs(case, seed)
    args = (E, B, I["x"], I["weight"], I["bias"], I["gamma"], I["beta"])
    a, b = layer64(*args), layer64(*args, dtype=torch.float32)
    return condition([a["y"]], [b["y"]], [hash_mask(rows, C, 0.5, SEED_L)])


# -- the heads: (n, row_lo, n_valid, B, need_dh)
HEADS_CASES = [(68, 0, 68, 3, True),                # tiles span frames
               (72, 4, 64, 2, True),                # filter off the frame start, n_valid exactly one tile: the fused threshold
               (67, 4, 63, 2, True),                # n_valid < 64: the unfused route with dh
               (340, 0, 340, 2, True),
               (68, 0, 68, 3, False)]
# (keyed by (n, row_lo, n_valid, B); at 680 rows no seed of 2000 .. 2199 has the search's headroom of 1.5: 2070 is the one with the
# most, 1.496 times the margin)
HEADS_SEED = {(68, 0, 68, 3): 2003, (72, 4, 64, 2): 2000, (67, 4, 63, 2): 2001, (340, 0, 340, 2): 2070}
HEADS_B = {}


@functools.lru_cache(maxsize=None)
def oracle_heads(weight_seed: int = 5, activation: str = "logit"):
    """node_classifiers of the oracle model gpu_util.model_pair(16, 3, 1, seed=weight_seed) builds (trained-like weights and
    running statistics), without the HIP model next to it."""
    from fixtures_util import fill_state_dict
    ref = O.OracleHierarchicalPatchModel(frame_size=16, gnn_dropout_p=0.5, classifier_dropout_p=0.5, node_embedding_dim=128,
                                         node_hidden_dim=128, num_output_channels=4, num_gnn_layers=1, num_aux_graphs=3,
                                         classifier_hidden_dim=32, use_coordinate_graph=False, output_activation=activation,
                                         use_main_graph_only=False)
    fill_state_dict(ref, weight_seed)
    return ref.node_classifiers


def heads_shape(case):
    n, row_lo, n_valid, B, need_dh = case
    return n, row_lo, n_valid, HEADS_B.get(case, B), need_dh


def heads_inputs(case, seed=None):
    """float32 inputs of a heads case: h [B * n, 128], dlogits [B * n_valid, 4]."""
    n, row_lo, n_valid, B, _ = heads_shape(case)
    rs = np.random.RandomState(HEADS_SEED.get(case[:4], 2000) if seed is None else seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return f(1.5 * rs.standard_normal((B * n, C))), f(rs.standard_normal((B * n_valid, HEADS)))


def heads_condition(case, seed=None):
    n, row_lo, n_valid, B, _ = heads_shape(case)
    P = stack_heads(oracle_heads())
    h, _ = heads_inputs(case, seed)
    a, b = heads64(P, h, B, n, row_lo, n_valid), heads64(P, h, B, n, row_lo, n_valid, dtype=torch.float32)
    R = B * n_valid
    return condition([a["y1"], a["y2"]], [b["y1"], b["y2"]], [hash_mask(R, H1, 0.5, SEED1), hash_mask(R, H2, 0.5, SEED2)])


def search_seed(cond_of, case, first, tries=200, headroom=1.5):
    """The first seed of first, first + 1, ... (at most `tries`) whose inputs meet the condition, or None.  The search asks for
    `headroom` times the margin: e32 is measured again wherever the tests run, and another host's float32 sums round differently."""
    for s in range(first, first + tries):
        cond = cond_of(case, s)
        if condition_met(cond) and cond[0] >= headroom * cond[1]:
            return s
    return None
