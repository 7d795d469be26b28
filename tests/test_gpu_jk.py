"""-m gpu: the two k_gcn_layer_ps instantiations that carry the running JumpingKnowledge('max') maximum -- the plain layer
(eg_gcn_layer_fwd_jk: jk_out = max(jk_in, out)) and the last layer with the heads fused in (eg_gcn_layer_cls_fwd with jk_in: the heads
run on max(jk_in, tile)) -- against a float64 evaluation on the CPU that contains no HIP kernel, on ragged patches, the coordinate
tile and single-level grids, with a jk_in that wins about half of the elements; the refusals; and the model's route through them
at other depths, without the residual, over stale buffers and under HIP-graph replay."""
import functools
import itertools

import numpy as np
import pytest
import torch

from fixtures_util import initial_coords, synthetic_node_feats
from gpu_util import DEV, graph_tensors, model_pair, rand_rows
from oracle import gnn_oracle as O
from echoglad_amd import nn as egnn
from echoglad_amd import ops
from echoglad_amd.topology import HierTopology, TopologySpec

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the model tests' bound on logits against the oracle (test_gpu_model.py)

# (frame, naux, main_only, coordinate nodes): every handle the running maximum covers in one of its forms
HANDLES = [(16, 3, False, False),          # levels smaller than a tile
           (17, 3, False, False),          # ragged patches: absent segments, short segments
           (30, 3, False, False),
           (100, 5, False, False),
           (64, 6, False, False),
           (16, 2, True, False),           # a single level ('flat'): no child sums
           (20, 0, True, False),           # ... with ragged patches
           (16, 3, False, True),           # the 4-row coordinate tile
           (32, 4, False, True)]
CLS_HANDLES = [h for h in HANDLES if not h[3]]          # (the fused heads take no coordinate nodes)


def _params(seed, w_scale=0.08):
    """The distributions of test_gpu_fold_heads.py's _params."""
    rs = np.random.RandomState(seed)
    f = lambda *shape: torch.from_numpy(rs.uniform(-0.3, 0.3, shape).astype(np.float32)).to(DEV)
    w = rand_rows(128, seed=21).to(DEV) * w_scale
    sc = rand_rows(1, seed=30).to(DEV).reshape(128) * 0.1 + 1.0
    sh = rand_rows(1, seed=31).to(DEV).reshape(128) * 0.1
    packed = {"w1": f(128, 128), "s1": f(128) + 1.0, "t1": f(128), "w2": f(4, 16, 32), "s2": f(64) + 1.0, "t2": f(64),
              "w3": f(4, 16), "b3": f(4)}
    return w, sc, sh, packed


# ---- the float64 reference: CPU only, no kernel of the library in it -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edges(frame, naux, main_only, coord):
    """(nodes per frame, source, target, weight of every edge, weight of every self loop) of one frame, float64: the degree is
    1 + the in-edge count, A_hat = D^-1/2 (A + I) D^-1/2."""
    topo = HierTopology(TopologySpec(frame, naux, main_only, coord))
    e = torch.from_numpy(np.ascontiguousarray(topo.edge_index())).long()
    n = topo.num_nodes
    deg = torch.ones(n, dtype=torch.float64)
    deg.index_add_(0, e[1], torch.ones(e.shape[1], dtype=torch.float64))
    dis = deg.pow(-0.5)
    return n, e[0], e[1], dis[e[0]] * dis[e[1]], dis * dis


def _ahat64(handle, x, B):
    """A_hat x per frame: the self term and an index_add_ over the edges."""
    n, src, dst, w_edge, w_self = _edges(*handle)
    xv = x.detach().cpu().double().view(B, n, 128)
    out = xv * w_self[None, :, None]
    out.index_add_(1, dst, xv[:, src, :] * w_edge[None, :, None])
    return out.reshape(B * n, 128)


def _layer64(xw, x, sc, sh, residual, relu):
    """((A_hat x) W^T) * scale + shift, ReLU, + x from xw = (A_hat x) W^T (float64; shared by the combinations of a case)."""
    h = xw
    if sc is not None:
        h = h * sc.cpu().double()
    if sh is not None:
        h = h + sh.cpu().double()
    if relu:
        h = torch.relu(h)
    if residual:
        h = h + x.cpu().double()
    return h


def _heads64(h, packed, sigmoid):
    """The heads' formula of test_gpu_fold_heads.py's _logits64 on finished rows h (no connection nodes in these handles)."""
    d = lambda t: t.cpu().double()
    u = torch.relu(d(packed["s1"]) * (h @ d(packed["w1"]).T) + d(packed["t1"])).view(-1, 4, 32)
    z = torch.einsum("nhk,hok->nho", u, d(packed["w2"]))
    z = torch.relu(d(packed["s2"]).view(4, 16) * z + d(packed["t2"]).view(4, 16))
    y = (z * d(packed["w3"])).sum(-1) + d(packed["b3"])
    return torch.sigmoid(y) if sigmoid else y


def _share(jk64, out64):
    """The share of elements in which jk_in wins.  A condition on the inputs, taken on the float64 reference alone: within
    [0.25, 0.75] a kernel that ignored jk_in, or read it from another row, cannot pass."""
    share = float((jk64 > out64).double().mean())
    assert 0.25 <= share <= 0.75, share
    return share


def _one_launch(g, fn):
    before = g.ps_launches
    got = fn()
    assert g.ps_launches == before + 1                      # the producer / consumer kernel, once
    return got


def _inputs(handle, g, B, chained, w, sc, sh):
    """(x, kidsum_in): fresh rows -- or, chained, the output of a layer together with the child sums that launch left behind."""
    x, ka = rand_rows(B * g.num_nodes, seed=9).to(DEV), None
    if chained:
        ka = ops.new_kidsum(g, B)
        x = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, relu=True, kidsum_out=ka))
    return x, ka


def _frame1(t, B):
    return None if t is None else t.view(B, -1, 128)[1].contiguous()


# ---- 1. the plain layer with the running maximum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frame,naux,main_only,coord", HANDLES)
def test_plain_layer_with_running_maximum_vs_float64(frame, naux, main_only, coord, B):
    handle = (frame, naux, main_only, coord)
    g = ops.Graph.topo(*handle)
    n = g.num_nodes
    assert n == _edges(*handle)[0] and (g.kidsum_rows > 0) != main_only
    w, sc, sh, _ = _params(frame + naux)
    jk_in = rand_rows(B * n, seed=10).to(DEV)
    jk64, jk_keep = jk_in.cpu().double(), jk_in.clone()
    for chained in (False, True) if g.kidsum_rows > 0 else (False,):
        x, ka = _inputs(handle, g, B, chained, w, sc, sh)
        x_keep = x.clone()
        xw = _ahat64(handle, x, B) @ w.cpu().double().T
        kb, kb_plain = (ops.new_kidsum(g, B), ops.new_kidsum(g, B)) if chained else (None, None)
        worst, shares = (0.0, 1.0), []
        for relu, residual, affine in itertools.product((True, False), repeat=3):
            scale, shift = (sc, sh) if affine else (None, None)
            args = (g, B, x, w, scale, shift, x if residual else None, relu)
            want = _layer64(xw, x, scale, shift, residual, relu)
            shares.append(_share(jk64, want))
            bound = 2e-5 * max(1.0, float(want.abs().max()))
            jk_out = torch.full_like(x, float("nan"))
            out = _one_launch(g, lambda: ops.gcn_layer_fwd(*args, kidsum_in=ka, kidsum_out=kb, jk_in=jk_in, jk_out=jk_out))
            plain = _one_launch(g, lambda: ops.gcn_layer_fwd(*args, kidsum_in=ka, kidsum_out=kb_plain))
            err_64, err_p = float((out.cpu().double() - want).abs().max()), float((out - plain).abs().max())
            if err_64 / bound > worst[0] / worst[1]:
                worst = (err_64, bound)
            what = (chained, relu, residual, affine)
            assert err_64 < bound and err_p < bound, (what, err_64, err_p, bound)
            # fmaxf is exact: a row or a channel mapped wrongly on a ragged patch is a mismatch, not an error to bound
            assert torch.equal(jk_out, torch.maximum(jk_in, out)), what
            assert torch.equal(jk_in, jk_keep) and torch.equal(x, x_keep), what
            if chained:
                assert float((kb - kb_plain).abs().max()) < 1e-5, what
            jk_again, kb_again = torch.full_like(x, float("nan")), ops.new_kidsum(g, B) if chained else None
            again = _one_launch(g, lambda: ops.gcn_layer_fwd(*args, kidsum_in=ka, kidsum_out=kb_again, jk_in=jk_in, jk_out=jk_again))
            assert torch.equal(again, out) and torch.equal(jk_again, jk_out), what
            if chained:
                assert torch.equal(kb_again, kb), what
            if B == 3:                                      # frame 1 does not depend on its neighbours
                x1, jk1, jk1_out = _frame1(x, B), _frame1(jk_in, B), torch.full((n, 128), float("nan"), device=DEV)
                k1_out = ops.new_kidsum(g, 1) if chained else None
                alone = _one_launch(g, lambda: ops.gcn_layer_fwd(g, 1, x1, w, scale, shift, x1 if residual else None, relu,
                                                                 kidsum_in=_frame1(ka, B), kidsum_out=k1_out, jk_in=jk1, jk_out=jk1_out))
                assert torch.equal(out.view(B, n, 128)[1], alone) and torch.equal(jk_out.view(B, n, 128)[1], jk1_out), what
                if chained:
                    assert torch.equal(kb.view(B, -1, 128)[1], k1_out), what
        print(f"{frame}/{naux}{' main-only' if main_only else ''}{' coord' if coord else ''} B={B} child sums {'handed in' if chained else 'pulled'}: "
              f"max|hip - float64| {worst[0]:.2e}, bound {worst[1]:.2e}; jk_in wins {min(shares):.2f} .. {max(shares):.2f} of the elements")


# ---- 2. the last layer with the heads fused in, on max(jk_in, tile) ---------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frame,naux,main_only,coord", CLS_HANDLES)
def test_last_layer_with_fused_heads_and_running_maximum_vs_float64(frame, naux, main_only, coord, B):
    handle = (frame, naux, main_only, coord)
    g = ops.Graph.topo(*handle)
    n = g.num_nodes
    assert g.fused_classifier_ok and g.num_conn == 0
    w, sc, sh, packed = _params(frame + naux)
    jk_in = rand_rows(B * n, seed=10).to(DEV)
    jk64, jk_keep = jk_in.cpu().double(), jk_in.clone()
    for chained in (False, True) if g.kidsum_rows > 0 else (False,):
        x, ka = _inputs(handle, g, B, chained, w, sc, sh)
        x_keep = x.clone()
        xw = _ahat64(handle, x, B) @ w.cpu().double().T
        worst, shares = (0.0, 1.0), []
        for sigmoid, residual in itertools.product((False, True), (True, False)):
            res = x if residual else None
            h64 = _layer64(xw, x, sc, sh, residual, False)
            shares.append(_share(jk64, h64))
            want = _heads64(torch.maximum(jk64, h64), packed, sigmoid)
            bound = 2e-5 * max(1.0, float(want.abs().max()))
            got = _one_launch(g, lambda: ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, res, False, packed, sigmoid, kidsum_in=ka, jk_in=jk_in))
            # the same from separately checked launches: the layer without the maximum, torch's maximum, the heads' own kernel
            h = _one_launch(g, lambda: ops.gcn_layer_fwd(g, B, x, w, sc, sh, res, False, kidsum_in=ka))
            apart = ops.classifier_fwd(torch.maximum(jk_in, h), B, n, 0, n, packed, sigmoid)
            assert got.shape == apart.shape == want.shape == (B * n, 4)
            err_64, err_a = float((got.cpu().double() - want).abs().max()), float((got - apart).abs().max())
            if err_64 / bound > worst[0] / worst[1]:
                worst = (err_64, bound)
            what = (chained, sigmoid, residual)
            assert err_64 < bound and err_a < bound, (what, err_64, err_a, bound)
            assert torch.equal(jk_in, jk_keep) and torch.equal(x, x_keep), what
            again = _one_launch(g, lambda: ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, res, False, packed, sigmoid, kidsum_in=ka, jk_in=jk_in))
            assert torch.equal(again, got), what
            if B == 3:
                x1 = _frame1(x, B)
                alone = _one_launch(g, lambda: ops.gcn_layer_cls_fwd(g, 1, x1, w, sc, sh, x1 if residual else None, False, packed, sigmoid,
                                                                     kidsum_in=_frame1(ka, B), jk_in=_frame1(jk_in, B)))
                assert torch.equal(got.view(B, n, 4)[1], alone), what
        print(f"{frame}/{naux}{' main-only' if main_only else ''} B={B} heads on max(jk_in, tile), child sums {'handed in' if chained else 'pulled'}: "
              f"max|hip - float64| {worst[0]:.2e}, bound {worst[1]:.2e}; jk_in wins {min(shares):.2f} .. {max(shares):.2f} of the elements")


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(g, tensors, launch, match=None):
    """launch() raises before any kernel runs on the handle, and leaves every tensor as it was."""
    keep, before = [t.clone() for t in tensors], g.layer_launches
    with pytest.raises(RuntimeError, match=match):
        launch()
    torch.cuda.synchronize()
    assert g.layer_launches == before
    assert all(torch.equal(t, k) for t, k in zip(tensors, keep))


@pytest.mark.parametrize("frame,naux,kw", [(8, 2, {}), (64, 2, {}),                        # no child sums, not a single level
                                           (16, 3, {"diag_aux": True}),                     # 'grid-diagonal' levels
                                           (16, 3, {"use_connection_nodes": True})])        # connection nodes
def test_running_maximum_is_refused_where_the_kernel_does_not_cover_the_handle(frame, naux, kw):
    B = 2
    g = ops.Graph.topo(frame, naux, **kw)
    assert g.hybrid == bool(kw) and (g.kidsum_rows == 0) != bool(kw)
    w, sc, sh, _ = _params(frame + naux)
    x, jk_in = rand_rows(B * g.num_nodes, seed=9).to(DEV), rand_rows(B * g.num_nodes, seed=10).to(DEV)
    out, jk_out = torch.zeros_like(x), torch.zeros_like(x)
    for res, relu in ((x, True), (None, False)):
        _refused(g, (x, jk_in, out, jk_out), lambda: ops.gcn_layer_fwd(g, B, x, w, sc, sh, res, relu, out=out, jk_in=jk_in, jk_out=jk_out),
                 match="unsupported")
    plain = ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, True)              # (the handle itself is fine: the caller takes the maximum outside)
    assert bool(torch.isfinite(plain).all())


@pytest.mark.parametrize("frame,naux", [(16, 3), (32, 4)])
def test_fused_heads_with_running_maximum_are_refused_on_coordinate_nodes(frame, naux):
    B = 2
    g = ops.Graph.topo(frame, naux, False, True)
    assert not g.fused_classifier_ok
    w, sc, sh, packed = _params(frame + naux)
    x, jk_in = rand_rows(B * g.num_nodes, seed=9).to(DEV), rand_rows(B * g.num_nodes, seed=10).to(DEV)
    _refused(g, (x, jk_in), lambda: ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, x, False, packed, jk_in=jk_in), match="unsupported")


def test_running_maximum_argument_checks_come_before_the_launch():
    B = 2
    g = ops.Graph.topo(17, 3)
    w, sc, sh, _ = _params(20)
    rows = B * g.num_nodes
    x, jk_in = rand_rows(rows, seed=9).to(DEV), rand_rows(rows, seed=10).to(DEV)
    jk_out, ka, kb = torch.zeros_like(x), ops.new_kidsum(g, B), ops.new_kidsum(g, B)
    every = (x, jk_in, jk_out, ka, kb)
    layer = lambda **kw: ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, True, **kw)
    _refused(g, every, lambda: layer(jk_in=jk_in))                                          # one without the other
    _refused(g, every, lambda: layer(jk_out=jk_out))
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=jk_in))                            # the maximum written over an input
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=x))
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=jk_out, out=jk_out))               # ... or over the layer's output
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=jk_out, kidsum_in=ka, kidsum_out=jk_in))     # child sums over the maximum
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=jk_out, kidsum_in=ka, kidsum_out=ka))
    _refused(g, every, lambda: layer(jk_in=jk_in, jk_out=jk_out, transpose_w=True))
    _refused(g, every, lambda: ops.gcn_layer_fwd(g, B, x, w, sc, sh, jk_in, True, jk_in=jk_in, jk_out=jk_out),       # a residual of its own
             match="unsupported")
    out = _one_launch(g, lambda: layer(jk_in=jk_in, jk_out=jk_out, kidsum_in=None, kidsum_out=kb))       # (and the same call, well formed)
    assert torch.equal(jk_out, torch.maximum(jk_in, out))


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------
def _count_jk_calls(monkeypatch):
    """Calls of ops.gcn_layer_fwd that carry the running maximum (the model looks the function up on the module at every call)."""
    calls, real = [], ops.gcn_layer_fwd

    def counted(*a, **k):
        if k.get("jk_in") is not None:
            assert k.get("jk_out") is not None
            calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "gcn_layer_fwd", counted)
    return calls


def _both(hip, ref, feats, ei, nt, B, coords=None, **kw):
    with torch.no_grad():
        want = ref.forward_nodes(feats, ei, nt, B, None if coords is None else coords.clone(), **kw)
        got = hip.forward_nodes(feats.to(DEV), ei.to(DEV), B, None if coords is None else coords.clone().to(DEV))
    return got[0].cpu().clone(), want


def _assert_logits(got, want, B, frame):
    err = float((got - want).abs().max())
    assert err < TOL, err
    assert torch.equal(O.landmark_argmax(got, B, frame), O.landmark_argmax(want, B, frame))
    return err


@pytest.mark.parametrize("fuse_heads", [True, False])
@pytest.mark.parametrize("frame,naux,main_only,L", [(16, 3, False, 1), (16, 3, False, 2), (16, 3, False, 4), (17, 3, False, 3),
                                                    (20, 0, True, 3)])
def test_model_at_other_depths_and_on_ragged_patches(frame, naux, main_only, L, fuse_heads, monkeypatch):
    """The ping-pong of the two maximum buffers at every parity of L, the first layer's jk_in = x, and both tails: the heads inside
    the last layer's launch (L - 1 launches write a maximum, the last one only reads it) and the heads' own kernel on the last
    maximum buffer (L launches write one)."""
    B = 2
    hip, ref = model_pair(frame, naux, L, main_only=main_only, seed=frame + L, gnn_jk_mode="max")
    hip.fuse_classifier = fuse_heads
    topo, ei, nt, bi = graph_tensors(frame, naux, B, main_only=main_only)
    feats = synthetic_node_feats(B * topo.num_nodes, 128, seed=200)
    calls = _count_jk_calls(monkeypatch)
    graph, _ = hip._resolver.resolve(ei.to(DEV), feats.shape[0])
    before = graph.ps_launches
    got, (want, _) = _both(hip, ref, feats, ei, nt, B)
    assert len(calls) == (L - 1 if fuse_heads else L)
    assert graph.ps_launches - before == L                  # one launch of the producer / consumer kernel per layer, either way
    err = _assert_logits(got, want, B, frame)
    print(f"{frame}/{naux} L={L} heads {'fused' if fuse_heads else 'apart'}: max|err| vs oracle {err:.2e}")


@pytest.mark.parametrize("fuse_heads", [True, False])
def test_model_without_the_residual_where_earlier_layers_win(fuse_heads, monkeypatch):
    """With the residual, h1 = relu(..) + x >= x and so on: the last layer but one always holds the maximum of what came before
    and a kernel that dropped jk_in on the way would pass.  Without it the earlier embeddings win inside the stack."""
    frame, naux, L, B = 17, 3, 3, 2
    hip, ref = model_pair(frame, naux, L, seed=23, gnn_jk_mode="max", residual=False)
    assert hip.residual is False and ref.residual is False
    hip.fuse_classifier = fuse_heads
    topo, ei, nt, bi = graph_tensors(frame, naux, B)
    feats = synthetic_node_feats(B * topo.num_nodes, 128, seed=200)
    calls = _count_jk_calls(monkeypatch)
    got, (want, _, hidden) = _both(hip, ref, feats, ei, nt, B, return_hidden=True)
    assert len(hidden) == L + 1 and len(calls) == (L - 1 if fuse_heads else L)
    earlier = torch.stack(hidden[:-1]).max(dim=0).values
    inside = torch.stack(hidden[1:-1]).max(dim=0).values                      # h_1 .. h_(L-1): kept by the buffers alone
    share, share_inside = float((earlier > hidden[-1]).double().mean()), float((inside > torch.maximum(hidden[0], hidden[-1])).double().mean())
    print(f"no residual: the final maximum comes from before the last layer in {share:.2f} of the elements, "
          f"from a hidden layer alone in {share_inside:.2f}")
    assert share >= 0.25 and share_inside >= 0.25
    _assert_logits(got, want, B, frame)


@pytest.mark.parametrize("kind", ["coordinate", "connection", "grid-diagonal"])
def test_model_takes_the_maximum_outside_the_kernels_on_handles_they_do_not_cover(kind, monkeypatch):
    frame, naux, L, B = 16, 3, 3, 2
    coord, conn = kind == "coordinate", kind == "connection"
    hip, ref = model_pair(frame, naux, L, coord=coord, seed=31, gnn_jk_mode="max", use_connection_nodes=conn)
    topo, ei, nt, bi = graph_tensors(frame, naux, B, coord=coord, conn=conn, aux_type="grid-diagonal" if kind == "grid-diagonal" else "grid")
    feats = synthetic_node_feats(B * topo.num_nodes, 128, seed=200)
    graph, _ = hip._resolver.resolve(ei.to(DEV), feats.shape[0])
    assert graph.structured and graph.hybrid == (not coord)
    calls = _count_jk_calls(monkeypatch)
    got, want = _both(hip, ref, feats, ei, nt, B, initial_coords(B, frame) if coord else None)
    assert calls == []
    _assert_logits(got, want[0], B, frame)


# (64, 6), batch 2, three layers: the shape of the other model-level tests
FRAME, NAUX, BATCH = 64, 6, 2


def _jk_model(frame=FRAME, naux=NAUX, seed=21):
    return model_pair(frame, naux, 3, seed=seed, gnn_jk_mode="max")[0]


def _fresh_copy(model, frame=FRAME, naux=NAUX):
    twin = _jk_model(frame, naux, seed=99)
    twin.load_state_dict(model.state_dict(), strict=True)
    return twin.eval()


def _forward(model, feats, ei, B=BATCH):
    with torch.no_grad():
        return model.forward_nodes(feats, ei, B)[0].clone()


def test_model_reads_no_stale_maximum():
    """The two maximum buffers are cached per handle.  A maximum is monotone: a buffer of the previous forward read as jk_in gives
    larger, plausible values -- so the second input lies below everything the first one left behind."""
    hip = _jk_model()
    topo, ei, nt, bi = graph_tensors(FRAME, NAUX, BATCH)
    feats, ei = synthetic_node_feats(BATCH * topo.num_nodes, 128, seed=200).to(DEV), ei.to(DEV)
    low = -feats.abs() - 1
    first = _forward(hip, feats, ei)
    second = _forward(hip, low, ei)
    assert not torch.equal(first, second)
    assert torch.equal(second, _forward(_fresh_copy(hip), low, ei))
    assert torch.equal(_forward(hip, feats, ei), first)


@pytest.mark.parametrize("frame,naux", [(17, 3), (FRAME, NAUX)])
def test_model_graph_replay_returns_the_eager_bits_for_every_input(frame, naux):
    hip = _jk_model(frame, naux)
    topo, ei, nt, bi = graph_tensors(frame, naux, BATCH)
    ei = ei.to(DEV)
    feats = synthetic_node_feats(BATCH * topo.num_nodes, 128, seed=200).to(DEV)
    inputs = [feats, -feats.abs() - 1, synthetic_node_feats(BATCH * topo.num_nodes, 128, seed=201).to(DEV)]
    eager = [_forward(hip, t, ei) for t in inputs]
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[0], eager[2])
    hip.enable_hip_graph(True)
    buf = torch.empty_like(feats)                           # (a captured graph is keyed on the address of its input)
    for k in (0, 1, 2, 1, 0):
        buf.copy_(inputs[k])
        assert torch.equal(_forward(hip, buf, ei), eager[k]), k
    assert hip.hip_graph_captures == 1


def test_model_fused_and_unfused_maximum_agree_on_ragged_patches(monkeypatch):
    frame, naux = 17, 3
    hip = _jk_model(frame, naux)
    topo, ei, nt, bi = graph_tensors(frame, naux, BATCH)
    feats, ei = synthetic_node_feats(BATCH * topo.num_nodes, 128, seed=200).to(DEV), ei.to(DEV)
    calls = _count_jk_calls(monkeypatch)
    fused = _forward(hip, feats, ei)
    assert len(calls) == 2
    egnn.ROUTES.jk_fused = False
    try:
        unfused = _forward(hip, feats, ei)
    finally:
        egnn.ROUTES.jk_fused = True
    assert len(calls) == 2                                  # (torch took the maximum)
    assert float((fused - unfused).abs().max()) < 2e-5
