"""A plain reference of the eval-mode forward (gcn_layer*.hip in their eval forms, conn.hip, classifier.hip, the fused last layer +
heads, unfolded and folded): torch on the CPU, float64 by default, no kernel of the library in it.  The conventions are
train_reference.py's and coord_reference.py's: every function takes ``dtype`` (float64 is the truth, the same code in float32 the
yardstick), kernel inputs are converted to double exactly, and every quantity comes with the scale `coord_reference.Report.check`
needs: the same expression evaluated on absolute values, per output element.

    |kernel - fp64| <= FACTOR * max|ref32 - fp64| + 8 * 2^-23 * scale          (coord_reference.Report, FACTOR = 4, unchanged)

The eval forward is continuous (ReLU has a kink but no jump), so there is no input condition: no element of any compared array is
left out.  The case tables of tests/test_gpu_eval_fp64.py live here, with fixed seeds, so that tests/test_eval_reference.py can
check them on the CPU."""
import functools

import numpy as np
import torch

from coord_reference import FACTOR, ULP, Report                 # noqa: F401  (the rule: unchanged, re-exported for the tests)
from train_reference import ahat, ahat_t, edges_of              # noqa: F401
from train_reference import graph_types as _graph_types, topo_edges as _topo_edges
from echoglad_amd.topology import HierTopology, TopologySpec

C = 128
HEADS = 4
F64, F32 = torch.float64, torch.float32
HEAD_KEYS = ("w1", "s1", "t1", "w2", "s2", "t2", "w3", "b3")    # the packed inference parameters of the 4 heads, in call order


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def topology(frame, naux, main_only=False, coord=False, conn=False, diag_main=False, diag_aux=False):
    return HierTopology(TopologySpec(frame, naux, main_only, coord, conn, *_graph_types(diag_main, diag_aux)))


def topo_edges(frame, naux, main_only=False, coord=False, conn=False, diag_main=False, diag_aux=False):
    """train_reference.edges_of one frame of the topology, 'grid-diagonal' levels and connection nodes included: the one
    implementation is train_reference.topo_edges."""
    return _topo_edges(frame, naux, main_only, coord, conn, diag_main, diag_aux)


def transposed(E):
    """The edges of A_hat^T (what a `.bwd` handle aggregates over): ahat(transposed(E), x, B) == ahat_t(E, x, B)."""
    n, src, dst, w_edge, w_self = E
    return n, dst, src, w_edge, w_self


def without_edges(E, drop):
    """E without the edges of the boolean mask `drop`, every other weight as it was (the mutation checks: a kernel that skips a
    neighbour still uses the right degrees)."""
    n, src, dst, w_edge, w_self = E
    keep = ~drop
    return n, src[keep], dst[keep], w_edge[keep], w_self


def with_edges(E, src_new, dst_new):
    """E with further edges of weight (deg_s + 1)^-1/2 (deg_t + 1)^-1/2 (the mutation checks: a row that receives a sum it should not)."""
    n, src, dst, w_edge, w_self = E
    s, d = torch.as_tensor(src_new, dtype=torch.long), torch.as_tensor(dst_new, dtype=torch.long)
    return n, torch.cat([src, s]), torch.cat([dst, d]), torch.cat([w_edge, (w_self[s] * w_self[d]).sqrt()]), w_self


# ---------------------------------------------------------------------------
# one eval-mode layer
# ---------------------------------------------------------------------------
def _d(t):
    return t.detach().cpu().to(F64)


def layer_eval(E, B, x, w, scale=None, shift=None, residual=None, relu=False, transpose_w=False, dtype=F64, agg_hook=None):
    """act((A_hat x) W^T * scale + shift) + residual for the B frames of x [B * n, 128] (eg_gcn_layer_fwd and its kin):
    residual None, "x" or a tensor [B * n, 128]; transpose_w: the product is (A_hat x) W (the backward's dX form).
    -> {"agg", "out", "agg_scale", "out_scale"}: agg_scale = A_hat |x|, out_scale = (A_hat |x|) |W|^T |scale| + |shift| + |residual|,
    per output element, float64.  agg_hook: a function applied to agg in front of the product (the mutation checks)."""
    xs, W = x.detach().cpu().to(dtype), w.detach().cpu().to(dtype)
    agg = ahat(E, xs, B)
    a = agg if agg_hook is None else agg_hook(agg)
    h = a @ (W if transpose_w else W.t())
    if scale is not None:
        h = h * scale.detach().cpu().to(dtype)
    if shift is not None:
        h = h + shift.detach().cpu().to(dtype)
    if relu:
        h = torch.relu(h)
    res = None if residual is None else (xs if isinstance(residual, str) else residual.detach().cpu().to(dtype))
    if res is not None:
        h = h + res
    agg_s = ahat(E, _d(x).abs(), B)
    Wa = _d(w).abs()
    out_s = agg_s @ (Wa if transpose_w else Wa.t())
    if scale is not None:
        out_s = out_s * _d(scale).abs()
    if shift is not None:
        out_s = out_s + _d(shift).abs()
    if res is not None:
        out_s = out_s + res.to(F64).abs()
    return dict(agg=agg, out=h, agg_scale=agg_s, out_scale=out_s)


def kidsum(topo, out, B, dtype=F64, out_scale=None):
    """The child sums of finished rows (eg_gcn_layer_fwd_chain's kidsum_out, and what kidsum_in has to hold for x) -> (sums, scale),
    [B * kid_rows, 128] each.

    Layout (topo_tables.hip build_topo_tables, pair_segments; graph.hip eg_graph_kidsum_rows): a frame's slice of the side buffer
    has kid_rows = topo.main.base rows, and row p belongs to NODE p of the frame -- `par0` of a segment is a node id.  Row p =
    sum over the children c of node p of (deg_c + 1)^-1/2 out[c]; the children of a node are its neighbours one grid level down (aux
    level k -> k + 1, the cropped part of the last aux level -> the main grid).  On a handle with connection nodes the node ids, and
    with them the rows, start with the naux + 1 connection nodes: those rows belong to no parent, no launch writes or reads them
    (they keep what ops.new_kidsum put there: zero), and a connection node's edges into its level are NOT child edges although the
    level's ids are larger.  Rows of aux nodes without children (the last aux level outside the crop) are zero as well.
    A 'grid-diagonal' aux level of fewer than 8 columns runs node by node (topo_tables.hip build_segments: `ldiag && cnt != 8`), names
    no parents (pair_segments: pad1 = 0 off the run path) and writes no sums: the rows of ITS parents -- the 2 x 2 level above the
    4 x 4 one; they run node by node too and pull their children through the handle's CSR -- are neither written nor read and stay
    zero here as well.

    scale: the same sums over `out_scale` (the scales of the rows summed; |out| without it): the kernel sums ITS rows, whose own
    error is bounded by a multiple of their scales, not of their magnitudes."""
    E = edges_of(topo.edge_index(), topo.num_nodes)
    n, src, dst, _, w_self = E
    bases = torch.tensor([lv.base for lv in topo.aux_levels] + [topo.main.base, topo.coord_base], dtype=torch.long)
    level = lambda ids: torch.bucketize(ids, bases, right=True)          # connection nodes 0, aux levels 1 .., main, coordinate nodes
    down = (level(src) == level(dst) + 1) & (dst >= topo.n_conn) & (dst < topo.main.base) & (src < topo.coord_base)
    if topo.spec.aux_graph_type == "grid-diagonal":
        for lv in topo.aux_levels:
            if lv.side < 8:
                down &= ~((src >= lv.base) & (src < lv.base + lv.size))
    rows = topo.main.base if topo.aux_levels else 0
    s, d = src[down], dst[down]

    def sums(v, dt):
        kid = torch.zeros(B, rows, C, dtype=dt)
        if rows:
            kid.index_add_(1, d, v.view(B, n, C)[:, s, :] * w_self.to(dt).sqrt()[s][None, :, None])
        return kid.reshape(B * rows, C)
    o = out.detach().cpu()
    return sums(o.to(dtype), dtype), sums(o.to(F64).abs() if out_scale is None else out_scale.to(F64), F64)


# ---------------------------------------------------------------------------
# the four heads, eval mode, on the packed arrays the kernels take
# ---------------------------------------------------------------------------
def pack_heads(classifiers, dtype=F32):
    """The packed eval arrays of four oracle heads (Linear 128-32, BatchNorm, ReLU, Dropout, Linear 32-16, BatchNorm, ReLU, Dropout,
    Linear 16-1): w1 [128,128], s1 / t1 [128] (the BatchNorm's scale, and its shift with the Linear's bias folded in), w2 [4,16,32],
    s2 / t2 [64], w3 [4,16], b3 [4].  Folded in float64, then cast to `dtype` (float32: rounded once, what a kernel is given)."""
    def bn(m, bias):
        s = m.weight.detach().to(F64) / torch.sqrt(m.running_var.detach().to(F64) + m.eps)
        return s, m.bias.detach().to(F64) - m.running_mean.detach().to(F64) * s + bias.detach().to(F64) * s
    st1 = [bn(c[1], c[0].bias) for c in classifiers]
    st2 = [bn(c[5], c[4].bias) for c in classifiers]
    P = dict(w1=torch.cat([c[0].weight.detach().to(F64) for c in classifiers]), s1=torch.cat([s for s, _ in st1]),
             t1=torch.cat([t for _, t in st1]), w2=torch.stack([c[4].weight.detach().to(F64) for c in classifiers]),
             s2=torch.cat([s for s, _ in st2]), t2=torch.cat([t for _, t in st2]),
             w3=torch.cat([c[8].weight.detach().to(F64) for c in classifiers]), b3=torch.cat([c[8].bias.detach().to(F64) for c in classifiers]))
    return {k: v.to(dtype).contiguous() for k, v in P.items()}


def uniform_heads(seed):
    """The made-up parameters of the existing tests: uniform(-0.3, 0.3), s1 / s2 shifted by 1.  float32, CPU."""
    rs = np.random.RandomState(seed)
    f = lambda *shape: torch.from_numpy(rs.uniform(-0.3, 0.3, shape).astype(np.float32))
    return {"w1": f(128, 128), "s1": f(128) + 1.0, "t1": f(128), "w2": f(4, 16, 32), "s2": f(64) + 1.0, "t2": f(64), "w3": f(4, 16), "b3": f(4)}


def heads_eval(packed, h, B, n, row_lo, n_valid, sigmoid=False, dtype=F64, h_scale=None):
    """The node-type filter (rows [row_lo, row_lo + n_valid) of every frame of h [B * n, 128]) and the four heads
    (eg_classifier_fwd): u = relu(s1 (h w1^T) + t1), z = relu(s2 (u_h w2_h^T) + t2) per head, y = z_h . w3_h + b3
    -> (logits or sigmoid(logits) [B * n_valid, 4], scale [B * n_valid, 4]).
    scale: the network evaluated on absolute values of inputs, weights and shifts (ReLU changes no magnitude); h_scale [B * n, 128]:
    the scales of the rows of h where h is itself a sum (the fused last layer), |h| without it.  With the sigmoid the scale is the
    logit's + 1, as train_reference.heads64 has it: the sigmoid's slope is at most 1 / 4, so the scale of the sum in front of it
    bounds what it hands through, and the 1 covers the rounding of a result that is at most 1."""
    P = {k: packed[k].detach().cpu().to(dtype) for k in HEAD_KEYS}
    A = {k: _d(packed[k]).abs() for k in HEAD_KEYS}
    rows = lambda t: t.view(B, n, C)[:, row_lo:row_lo + n_valid, :].reshape(B * n_valid, C)

    def net(hv, Q):
        u = torch.relu(Q["s1"] * (hv @ Q["w1"].t()) + Q["t1"]).view(-1, HEADS, 32)
        z = torch.einsum("nhk,hok->nho", u, Q["w2"])
        z = torch.relu(Q["s2"].view(HEADS, 16) * z + Q["t2"].view(HEADS, 16))
        return (z * Q["w3"]).sum(-1) + Q["b3"]
    y = net(rows(h.detach().cpu().to(dtype)), P)
    y_s = net(rows(_d(h).abs() if h_scale is None else h_scale.to(F64)), A)
    return (torch.sigmoid(y), y_s + 1.0) if sigmoid else (y, y_s)


def last_layer_heads(E, B, x, w, scale, shift, residual, packed, n_conn, sigmoid=False, dtype=F64, layer=None):
    """eg_gcn_layer_cls_fwd / eg_gcn_layer_cls_fold_fwd: layer_eval without ReLU (residual: add x) followed by heads_eval on rows
    [n_conn, n) of every frame, the layer's scale handed on as the heads' h_scale.  Always the UNFOLDED formula, started from x alone
    -> (logits [B * (n - n_conn), 4], scale).  layer: what layer_eval returned for the same arguments and dtype (several heads on one layer)."""
    L = layer_eval(E, B, x, w, scale, shift, "x" if residual else None, relu=False, dtype=dtype) if layer is None else layer
    n = E[0]
    return heads_eval(packed, L["out"], B, n, n_conn, n - n_conn, sigmoid, dtype, h_scale=L["out_scale"])


# ---------------------------------------------------------------------------
# inputs (fixed seeds)
# ---------------------------------------------------------------------------
def rand_rows(rows, seed, scale=1.0):
    """gpu_util.rand_rows (written out: this module stays importable without the library)."""
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((rows, C)) * scale).astype(np.float32))


def glorot(seed):
    rs = np.random.RandomState(seed)
    b = float(np.sqrt(6.0 / 256.0))
    return torch.from_numpy(rs.uniform(-b, b, (C, C)).astype(np.float32))


def layer_params(seed):
    """(Glorot weight, scale in [0.5, 1.5] with mixed sign, shift ~ 0.1 randn), float32, CPU."""
    rs = np.random.RandomState(seed)
    sc = rs.uniform(0.5, 1.5, C) * np.where(rs.uniform(size=C) < 0.5, -1.0, 1.0)
    return glorot(seed + 1), torch.from_numpy(sc.astype(np.float32)), torch.from_numpy((0.1 * rs.standard_normal(C)).astype(np.float32))


MAGNITUDES = (1e-3, 1.0, 30.0, 1e4)
MIXED_B = len(MAGNITUDES) + 1


def mixed_rows(n, seed):
    """The second input set: MIXED_B = 5 frames of n rows scaled 1e-3, 1, 30 and 1e4, the fifth mixing the four per element
    (test 3 of tests/test_gpu_layer_split.py) -> [5 n, 128]."""
    x = rand_rows(MIXED_B * n, seed).view(MIXED_B, n, C)
    mags = torch.tensor(MAGNITUDES, dtype=torch.float32)
    for b in range(len(MAGNITUDES)):
        x[b] *= mags[b]
    x[len(MAGNITUDES)] *= mags[torch.from_numpy(np.random.RandomState(seed + 1).randint(0, len(MAGNITUDES), (n, C)))]
    return x.reshape(MIXED_B * n, C).contiguous()


# ---------------------------------------------------------------------------
# the cases of tests/test_gpu_eval_fp64.py
# ---------------------------------------------------------------------------
# a. handles float64 has not seen: (frame, naux, main_only, coord, conn, diag_main, diag_aux)
DIAG_HANDLES = [(16, 3, False, False, False, True, True),
                (17, 3, False, True, False, True, True),         # ragged patches + coordinate nodes
                (30, 3, False, False, False, False, True),       # aux levels only
                (16, 2, True, False, False, True, False),        # main grid only
                (8, 2, False, False, False, True, True),         # levels of fewer than 8 columns: node by node
                (64, 5, False, False, False, True, True)]
CONN_HANDLES = [(8, 2, False, False, True, False, False),
                (16, 3, False, False, True, False, False),
                (30, 3, False, True, True, True, False),         # + coordinate nodes + diagonal main grid
                (64, 5, False, False, True, False, False),       # the last wired level (16 x 16) is exactly one 256-row chunk of the pre-pass
                (64, 5, False, False, True, True, True),
                (64, 6, False, False, True, False, False)]       # a wired level of 1024 rows: four chunks
FORMS = ("pulled", "handed in", "handed out", "handed in and out")
IDENTITY_HANDLES = [(17, 3, False, False, False, True, True), (64, 5, False, False, True, False, False)]
PER_TERM_HANDLES = [(30, 3, False, False, False, False, True), (16, 3, False, False, True, False, False)]
PER_TERM_BOUND = 1e-6                                           # test 3 of tests/test_gpu_layer_split.py, the same constant
ALONE_HANDLES = [(17, 3, False, True, False, True, True), (16, 3, False, False, True, False, False)]

# b. graphs of the symmetric kernel
CSR_GRAPHS = ("directed", "multigraph", "tiny", "isolated", "star", "cycle")


def csr_graph(kind):
    """(edge_index [2, E] int64 numpy, nodes)."""
    rs = np.random.RandomState(17)
    if kind == "directed":
        n = 300
        e = np.stack([rs.randint(0, n, 1500), rs.randint(0, n, 1500)])
    elif kind == "multigraph":                                   # duplicate edges and explicit self loops
        n = 200
        s, d = rs.randint(0, n, 900), rs.randint(0, n, 900)
        loops = np.arange(0, n, 7)
        e = np.stack([np.concatenate([s, d, s[:150], loops]), np.concatenate([d, s, d[:150], loops])])
    elif kind == "tiny":
        n = 37
        e = np.stack([rs.randint(0, n, 90), rs.randint(0, n, 90)])
    elif kind == "isolated":                                     # only the first 100 nodes have edges
        n = 1000
        e = np.stack([rs.randint(0, 100, 600), rs.randint(0, 100, 600)])
    elif kind == "star":                                         # node 0 <-> every other: one row of degree n - 1
        n = 1000
        leaves = np.arange(1, n)
        e = np.stack([np.concatenate([np.zeros(n - 1, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(n - 1, dtype=np.int64)])])
    elif kind == "cycle":
        n = 130
        i = np.arange(n)
        e = np.stack([np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i])])
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(e.astype(np.int64)), n


def batched(edge_index, n, B):
    """B copies of a graph as one edge list over B * n nodes."""
    return np.ascontiguousarray(np.concatenate([edge_index + b * n for b in range(B)], axis=1))


# topology handles on which eg_launch_layer_ps declines a plain call (no child-sum buffer, more than one level, no diagonal level,
# no connection nodes): the symmetric kernel's stencil form.  (8, 2): levels smaller than a tile; (20, 2): ragged patches
STENCIL_HANDLES = [(8, 2, False, False), (20, 2, False, False)]
LINEAR_ROWS = (1, 31, 32, 33, 64, 65)
AGGREGATE_HANDLES = [(17, 3, False, False, False, False, False), (17, 3, False, False, False, True, True), (16, 3, False, False, True, False, False)]

# c. the stand-alone heads: (n_per_frame, row_lo, n_valid, B).  Tiles are cut per frame: last tiles of 1, 31, 32, 33 (both sides
# of the kernel's `rows_here <= 32`), 63, 64 rows, of 1, 4 and 20 rows after full ones, filters off the frame start
HEADS_SHAPES = [(1, 0, 1, 1), (100, 3, 1, 1), (35, 4, 31, 2), (40, 4, 32, 2), (37, 4, 33, 3), (63, 0, 63, 2), (64, 0, 64, 2), (70, 5, 65, 3),
                (68, 0, 68, 3), (340, 0, 340, 2)]

# d. last layer + heads: (frame, naux, main_only, conn, diag_main, diag_aux)
CLS_HANDLES = [(16, 3, False, False, False, False),
               (16, 2, True, False, False, False),
               (100, 5, False, False, False, False),
               (64, 6, False, False, False, True),
               (16, 3, False, False, True, True),
               (16, 3, False, True, False, False),
               (64, 5, False, True, False, False),
               (64, 5, False, True, True, True)]
CLS_DECLINED = [(8, 2, False, False, False, False)]             # no child-sum buffer, more than one level
CONN_ROWS_FACTOR = 1e4


def cls_args(handle):
    """CLS_HANDLES entry -> the arguments of topology() / topo_edges()."""
    frame, naux, main_only, conn, dm, da = handle
    return frame, naux, main_only, False, conn, dm, da


def bf16_hi_mid(t):
    """t rounded to the sum of its two leading bf16 pieces (float32 in, float32 out): what a split product sees that drops the
    third piece of its left operand."""
    t = t.to(F32)
    hi = t.to(torch.bfloat16).to(F32)
    mid = (t - hi).to(torch.bfloat16).to(F32)
    return hi + mid
