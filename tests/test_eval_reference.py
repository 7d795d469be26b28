"""The fp64 reference of the eval-mode forward (tests/eval_reference.py), checked on the CPU: against the oracle's sparse
convolution + eval BatchNorm1d + ReLU + residual and its four heads in float64, every scale against the magnitude it bounds, the
child-sum layout against the children written out by hand -- and the tolerance rule itself against planted errors of the kind the
fixed bounds of tests/test_gpu_diag.py, test_gpu_layer.py and test_gpu_layer_split.py let through."""
import copy

import numpy as np
import pytest
import torch

import eval_reference as E
import train_reference as T
from oracle import gnn_oracle as O

C = 128
F64, F32 = torch.float64, torch.float32


def _close(a, b, rel=1e-12):
    err = float((a.to(F64) - b.to(F64)).abs().max())
    return err <= rel * max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------
# the reference against the oracle's own modules, float64, eval mode
# ---------------------------------------------------------------------------
def _oracle_layer(x, ei, w, bias, bn, relu):
    with torch.no_grad():
        y = bn(O.gcn_conv_sparse(x.double(), ei, w.double(), bias.double()))
        return (torch.relu(y) if relu else y) + x.double()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("kind", ["diagonal", "connection nodes", "directed"])
def test_layer_eval_equals_the_oracle_layer_in_float64(kind, relu):
    if kind == "directed":
        ei_np, n = E.csr_graph("directed")
        B, Eg, ei = 1, E.edges_of(ei_np, n), torch.from_numpy(ei_np)
    else:
        handle = (17, 3, False, True, False, True, True) if kind == "diagonal" else (16, 3, False, False, True, False, False)
        B, Eg, topo = 2, E.topo_edges(*handle), E.topology(*handle)
        n, ei = topo.num_nodes, torch.from_numpy(topo.batched_edge_index(2).astype(np.int64))
    x = E.rand_rows(B * n, seed=3)
    w, _, _ = E.layer_params(5)
    bias = 0.1 * E.rand_rows(1, seed=6).reshape(C)
    bn = torch.nn.BatchNorm1d(C).double().eval()
    O.randomize_bn_stats(bn, seed=7)
    want = _oracle_layer(x, ei, w, bias, bn, relu)
    with torch.no_grad():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale + bias.double() * scale
    got = E.layer_eval(Eg, B, x, w, scale, shift, "x", relu)
    assert _close(got["out"], want)
    assert _close(got["agg"], O.gcn_conv_dense64(x, ei, torch.eye(C, dtype=F64), None))
    # the transposed-weight form and a residual tensor of its own; A_hat^T through transposed()
    res = E.rand_rows(B * n, seed=8)
    got = E.layer_eval(Eg, B, x, w, None, None, res, False, transpose_w=True)
    assert _close(got["out"], O.gcn_conv_dense64(x, ei, w.t().contiguous(), None) + res.double())
    assert _close(E.ahat(E.transposed(Eg), x.double(), B), E.ahat_t(Eg, x.double(), B))


@pytest.mark.parametrize("n,row_lo,n_valid,B", [(37, 4, 33, 3), (70, 5, 65, 3), (100, 3, 1, 1)])
@pytest.mark.parametrize("act", ["logit", "sigmoid"])
def test_heads_eval_equals_the_oracle_heads_in_float64(n, row_lo, n_valid, B, act):
    heads = copy.deepcopy(T.oracle_heads(5, act)).double().eval()
    packed = E.pack_heads(heads, F64)
    h = E.rand_rows(B * n, seed=3, scale=1.5)
    hv = h.double().view(B, n, C)[:, row_lo:row_lo + n_valid].reshape(-1, C)
    with torch.no_grad():
        want = torch.cat([clf(hv) for clf in heads], dim=1)
    got, scale = E.heads_eval(packed, h, B, n, row_lo, n_valid, sigmoid=act == "sigmoid")
    assert got.shape == want.shape == scale.shape and _close(got, want)
    # rounded once, the packed arrays are what the HIP model packs (nn/model.py _packed_classifier folds in float32)
    p32 = E.pack_heads(heads)
    assert all(p32[k].dtype == F32 and _close(p32[k], packed[k], 1e-6) for k in E.HEAD_KEYS)


def test_last_layer_heads_is_the_unfolded_formula_on_the_rows_behind_the_connection_nodes():
    handle = (16, 3, False, False, True, False, False)
    topo, Eg = E.topology(*handle), E.topo_edges(*handle)
    n, B = topo.num_nodes, 2
    x = E.rand_rows(B * n, seed=4)
    w, sc, sh = E.layer_params(9)
    packed = E.uniform_heads(3)
    got, scale = E.last_layer_heads(Eg, B, x, w, sc, sh, True, packed, topo.n_conn)
    L = E.layer_eval(Eg, B, x, w, sc, sh, "x")
    want, _ = E.heads_eval(packed, L["out"], B, n, topo.n_conn, n - topo.n_conn)
    assert got.shape == (B * (n - topo.n_conn), 4) and torch.equal(got, want)
    # the folded formula (nn/_heads.py fold_last_into_heads) is the same function of x
    d = lambda t: t.double()
    m1 = (d(packed["s1"])[:, None] * d(packed["w1"])) @ (d(sc)[:, None] * d(w))
    c1 = d(packed["s1"]) * (d(packed["w1"]) @ d(sh)) + d(packed["t1"])
    u = L["agg"] @ m1.t() + d(x) @ (d(packed["s1"])[:, None] * d(packed["w1"])).t() + c1
    folded = dict(packed, w1=torch.eye(C), s1=torch.ones(C), t1=torch.zeros(C))
    alt, _ = E.heads_eval(folded, u, B, n, topo.n_conn, n - topo.n_conn)
    assert _close(alt, want, 1e-11)


def test_child_sums_are_the_four_children_written_out():
    """kidsum against the parent / child rule of echoglad_amd/topology.py spelled out node by node, on a handle with connection
    nodes and a crop: rows of the connection nodes and of childless aux nodes are zero."""
    handle = (30, 3, False, True, True, True, False)
    topo = E.topology(*handle)
    n, B = topo.num_nodes, 2
    out = E.rand_rows(B * n, seed=2).double()
    dis = torch.from_numpy(1.0 / np.sqrt(topo.degree() + 1.0))
    want = torch.zeros(B, topo.main.base, C, dtype=F64)
    levels = topo.aux_levels + [topo.main]
    for k, par in enumerate(topo.aux_levels):
        kid = levels[k + 1]
        last = k + 1 == len(topo.aux_levels)
        for r in range(par.side):
            for c in range(par.side):
                if last and (r not in topo.crop_rows or c not in topo.crop_rows):
                    continue
                rr, cc = (r - topo.crop_rows[0], c - topo.crop_rows[0]) if last else (r, c)
                for dr in (0, 1):
                    for dc in (0, 1):
                        ch = kid.base + (2 * rr + dr) * kid.side + 2 * cc + dc
                        want[:, par.base + r * par.side + c] += dis[ch] * out.view(B, n, C)[:, ch]
    got, scale = E.kidsum(topo, out, B)
    assert got.shape == (B * topo.main.base, C) and _close(got, want.reshape(-1, C))
    assert float(got.view(B, -1, C)[:, :topo.n_conn].abs().max()) == 0.0 and topo.n_conn == 4
    assert bool((scale * (1 + 1e-12) >= got.abs()).all())
    # a 'grid-diagonal' 4 x 4 level hands no sums up: the rows of the 2 x 2 level stay zero, every other row is as without diagonals
    plain, diag = E.topology(16, 3), E.topology(16, 3, False, False, False, True, True)
    o = E.rand_rows(plain.num_nodes, seed=5).double()
    # (the sums weigh a child with ITS degree, which the diagonals change: compare which rows are written, and one row by hand)
    kp, kd = E.kidsum(plain, o, 1)[0], E.kidsum(diag, o, 1)[0]
    assert float(kd[:4].abs().max()) == 0.0 and float(kp[:4].abs().min()) > 0.0 and bool((kd[4:].abs().sum(1) > 0).all())
    dis = torch.from_numpy(1.0 / np.sqrt(diag.degree() + 1.0))
    lv3 = diag.aux_levels[2]
    kids = [lv3.base + r * lv3.side + c for r in (0, 1) for c in (0, 1)]
    assert _close(kd[diag.aux_levels[1].base], sum(dis[c] * o[c] for c in kids))
    # a main-only handle has no side buffer
    assert E.kidsum(E.topology(16, 2, True), E.rand_rows(256, seed=1), 1)[0].shape == (0, C)


# ---------------------------------------------------------------------------
# every scale is at least the magnitude of its quantity
# ---------------------------------------------------------------------------
def _bounded(value, scale):
    return bool((scale * (1 + 1e-12) >= value.to(F64).abs()).all())


@pytest.mark.parametrize("handle", [E.DIAG_HANDLES[1], E.CONN_HANDLES[2]], ids=str)
def test_scales_bound_their_quantities(handle):
    topo, Eg = E.topology(*handle), E.topo_edges(*handle)
    n = topo.num_nodes
    w, sc, sh = E.layer_params(11)
    packed = E.uniform_heads(5)
    for x, B in ((E.rand_rows(2 * n, seed=1), 2), (E.mixed_rows(n, seed=13), E.MIXED_B)):
        for relu, residual, affine in ((True, "x", True), (False, None, False), (True, E.rand_rows(B * n, seed=2), True)):
            L = E.layer_eval(Eg, B, x, w, sc if affine else None, sh if affine else None, residual, relu, transpose_w=residual is None)
            assert _bounded(L["agg"], L["agg_scale"]) and _bounded(L["out"], L["out_scale"])
            kid, kid_s = E.kidsum(topo, L["out"], B, out_scale=L["out_scale"])
            assert _bounded(kid, kid_s)
        for sigmoid in (False, True):
            y, y_s = E.last_layer_heads(Eg, B, x, w, sc, sh, True, packed, topo.n_conn, sigmoid)
            assert _bounded(y, y_s)
            y, y_s = E.heads_eval(packed, x, B, n, 3, n - 5, sigmoid)
            assert _bounded(y, y_s)


# ---------------------------------------------------------------------------
# the rule itself: a float32 evaluation with a planted error must fail Report.check on the quantity the error reaches
# ---------------------------------------------------------------------------
def _verdict(what, got, r64, r32, scale, old_bound):
    """(fails the rule?, would have failed the old fixed bound?) of a float32 evaluation with a planted error; printed."""
    rep = E.Report()
    ok = rep.check(what, got, r64, r32, scale)
    err = float((got.to(F64) - r64).abs().max())
    old = err >= old_bound
    print(f"\n  {what:66s} rule ratio {rep.rows[what][0]:9.3e}  max|err| {err:.3e}  old bound {old_bound:.3e}: "
          f"{'failed too' if old else 'PASSED the old bound'}")
    return not ok, old


def _level_border(topo, lv):
    ids = lv.base + torch.arange(lv.size).view(lv.side, lv.side)
    border = torch.zeros(lv.side, lv.side, dtype=torch.bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    return ids[border]


def test_the_rule_passes_float32_and_fails_planted_errors_in_the_layer():
    w, sc, sh = E.layer_params(21)
    seen = {}
    # -- a diagonal handle: old bound 3e-5 max(1, max|want|) (tests/test_gpu_diag.py)
    handle = (16, 3, False, False, False, True, True)
    topo, Eg = E.topology(*handle), E.topo_edges(*handle)
    n, B = topo.num_nodes, 2
    x = E.rand_rows(B * n, seed=9)
    args = (B, x, w, sc, sh, "x", True)
    r64, r32 = E.layer_eval(Eg, *args), E.layer_eval(Eg, *args, dtype=F32)
    old = 3e-5 * max(1.0, float(r64["out"].abs().max()))
    assert not _verdict("float32, nothing planted", r32["out"], r64["out"], r32["out"], r64["out_scale"], old)[0]
    _, src, dst, _, _ = Eg
    main = topo.main
    r_s, c_s = (src - main.base) // main.side, (src - main.base) % main.side
    r_d, c_d = (dst - main.base) // main.side, (dst - main.base) % main.side
    on_border = torch.isin(dst, _level_border(topo, main))
    drop = (src >= main.base) & (dst >= main.base) & on_border & (r_s == r_d + 1) & (c_s == c_d + 1)      # the lower-right neighbour
    assert 0 < int(drop.sum()) < 4 * main.side
    m = E.layer_eval(E.without_edges(Eg, drop), *args, dtype=F32)
    seen["diag"] = _verdict("one diagonal neighbour dropped on the main grid's border", m["out"], r64["out"], r32["out"], r64["out_scale"], old)
    # -- the product's left operand without its third bf16 piece: old bound 2e-5 max(1, max|want|) (tests/test_gpu_layer_split.py).
    # The piece is 2^-17 of its element at most and of either sign: over 128 terms of one size it stays inside 8 ulp of their sum of
    # magnitudes (ratio 0.35 on the rows above).  Inputs that show it: one channel carries every row, the rest are 1e-4 of it
    # (and no edges, A_hat = I: the float32 yardstick's own error is then the product's alone)
    # the carrying channel holds the 1000 of 128000 random numbers whose third piece is the largest share of them
    cand = E.rand_rows(1000, seed=12).reshape(-1)
    share = ((cand - E.bf16_hi_mid(cand)) / cand).abs()
    xs = E.rand_rows(1000, seed=13) * 1e-4
    xs[:, 0] = cand[share.argsort(descending=True)[:1000]]
    args3 = (1, xs, w, None, None, None, False)
    Eg = E.edges_of(np.zeros((2, 0), dtype=np.int64), 1000)
    p64, p32 = E.layer_eval(Eg, *args3), E.layer_eval(Eg, *args3, dtype=F32)
    old3 = 2e-5 * max(1.0, float(p64["out"].abs().max()))
    assert not _verdict("float32, nothing planted (one channel carries)", p32["out"], p64["out"], p32["out"], p64["out_scale"], old3)[0]
    m = E.layer_eval(Eg, *args3, dtype=F32, agg_hook=E.bf16_hi_mid)
    seen["pieces"] = _verdict("left operand rounded to its bf16 hi + mid pieces", m["out"], p64["out"], p32["out"], p64["out_scale"], old3)
    # -- a connection-node handle: old bound 5e-5 max(1, max|want|) (tests/test_gpu_diag.py)
    handle = E.CONN_HANDLES[-1]                                      # (64, 6): the last wired level has 1024 rows
    topo, Eg = E.topology(*handle), E.topo_edges(*handle)
    n, B = topo.num_nodes, 2
    x = E.rand_rows(B * n, seed=10)
    args = (B, x, w, sc, sh, "x", True)
    r64, r32 = E.layer_eval(Eg, *args), E.layer_eval(Eg, *args, dtype=F32)
    old = 5e-5 * max(1.0, float(r64["out"].abs().max()))
    assert not _verdict("float32, nothing planted (connection nodes)", r32["out"], r64["out"], r32["out"], r64["out_scale"], old)[0]
    _, src, dst, _, _ = Eg
    wired = topo.aux_levels[topo.spec.num_aux_graphs - 2]           # the last level that hangs on a connection node: 32 x 32
    hub = topo.spec.num_aux_graphs - 2
    assert wired.size == 1024
    m = E.layer_eval(E.without_edges(Eg, (dst == hub) & (src == wired.base + wired.size - 1)), *args, dtype=F32)
    seen["last row"] = _verdict("a connection node's level sum misses the level's last row", m["out"], r64["out"], r32["out"], r64["out_scale"], old)
    m = E.layer_eval(E.without_edges(Eg, (src == hub) & (dst >= wired.base) & (dst < wired.base + wired.size)), *args, dtype=F32)
    seen["scaled"] = _verdict("scaled[h] not added to the nodes of the last wired level", m["out"], r64["out"], r32["out"], r64["out_scale"], old)
    lv = topo.aux_levels[0]
    extra_src = torch.arange(lv.base, lv.base + lv.size).repeat(2)
    extra_dst = torch.tensor([topo.n_conn - 2, topo.n_conn - 1]).repeat_interleave(lv.size)
    m = E.layer_eval(E.with_edges(Eg, extra_src, extra_dst), *args, dtype=F32)
    seen["unwired"] = _verdict("the last two connection nodes receive a level sum", m["out"], r64["out"], r32["out"], r64["out_scale"], old)
    assert all(v[0] for v in seen.values()), seen
    assert not seen["pieces"][1], seen                               # ... which the fixed bound lets through


def test_the_rule_passes_float32_and_fails_planted_errors_in_the_heads():
    packed = E.pack_heads(T.oracle_heads())
    seen = {}
    old = 2e-5                                                       # tests/test_gpu_layer.py::test_classifier_heads
    n, row_lo, n_valid, B = 37, 4, 33, 3
    h = E.rand_rows(B * n, seed=3, scale=1.5)
    args = (h, B, n, row_lo, n_valid)
    r64, s64 = E.heads_eval(packed, *args)
    r32, _ = E.heads_eval(packed, *args, dtype=F32)
    assert not _verdict("float32, nothing planted (heads)", r32, r64, r32, s64, old)[0]
    swapped = dict(packed, w2=packed["w2"][[1, 0, 3, 2]])
    seen["w2"] = _verdict("a head reads w2 of head h ^ 1", E.heads_eval(swapped, *args, dtype=F32)[0], r64, r32, s64, old)
    hm = h.clone().view(B, n, C)
    hm[:, row_lo + n_valid - 1] = hm[:, row_lo + n_valid - 2]
    seen["last row"] = _verdict("the last valid row of a frame replaced by its neighbour", E.heads_eval(packed, hm.view(-1, C), *args[1:], dtype=F32)[0],
                                r64, r32, s64, old)
    # tiles are cut per frame (classifier.hip: tiles_per_frame): n_valid = 33 is one tile of exactly 33 rows, its rows 32 .. read as zero
    hz = h.clone().view(B, n, C)
    hz[:, row_lo + 32:row_lo + n_valid] = 0.0
    assert n_valid == 33
    seen["33 rows"] = _verdict("the second 32 rows of a 33-row tile taken as zero", E.heads_eval(packed, hz.view(-1, C), *args[1:], dtype=F32)[0],
                               r64, r32, s64, old)
    g64, u64 = E.heads_eval(packed, *args, sigmoid=True)
    g32, _ = E.heads_eval(packed, *args, sigmoid=True, dtype=F32)
    seen["sigmoid"] = _verdict("the sigmoid dropped", r32, g64, g32, u64, old)
    assert all(v[0] for v in seen.values()), seen


def test_case_tables_are_what_the_gpu_file_expects():
    """Sizes the GPU tests rely on: the wired level of 1024 rows, the last tiles of the heads' shapes, no child-sum-free handle
    among the fused-heads ones but the declined one."""
    assert E.topology(*E.CONN_HANDLES[-1]).aux_levels[4].size == 1024 and E.topology(*E.CONN_HANDLES[3]).aux_levels[3].size == 256
    assert {nv % 64 for _, _, nv, _ in E.HEADS_SHAPES} >= {1, 31, 32, 33, 63, 0, 4, 20}        # the last tile of a frame (tiles are per frame)
    for kind in E.CSR_GRAPHS:
        ei, n = E.csr_graph(kind)
        assert ei.shape[0] == 2 and int(ei.max()) < n
    deg = np.bincount(E.csr_graph("star")[0][1], minlength=1000)
    assert deg[0] == 999 and int(deg[1:].max()) == 1
