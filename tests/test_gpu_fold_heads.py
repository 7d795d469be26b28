"""-m gpu: the last GCN layer folded into the heads' first Linear (eg_gcn_layer_cls_fold_fwd, k_gcn_layer_ps FOLD) against the
unfolded launch (eg_gcn_layer_cls_fwd) and a float64 evaluation of the unfolded formula; the consumers' write-after-read on the
A tile at full grid; the model's route, its cache and its captured graphs."""
import numpy as np
import pytest
import torch

from fixtures_util import synthetic_node_feats
from gpu_util import DEV, graph_tensors, model_pair, rand_rows
from oracle import gnn_oracle as O
from echoglad_amd import nn as egnn
from echoglad_amd import ops
from echoglad_amd.nn._heads import fold_last_into_heads

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the model tests' bound on logits against the oracle (test_gpu_model.py)

# (frame, naux, main_only, connection nodes, diag_main, diag_aux, child sums from a preceding launch)
TOPOS = [(8, 2, False, False, False, False, False),          # levels smaller than a tile
         (16, 3, False, False, False, False, False),
         (16, 2, True, False, False, False, False),         # a single level: no child sums
         (100, 5, False, False, False, False, False),       # ragged patches
         (64, 6, False, False, False, False, True),         # kidsum_in from the launch that wrote the input
         (64, 6, False, False, False, True, True),          # 'grid-diagonal' aux levels
         (64, 5, False, True, False, False, True)]          # connection nodes (no logits row)


def _params(seed, w_scale=0.08):
    """The distributions of test_gpu_layer.py's fused-classifier test."""
    rs = np.random.RandomState(seed)
    f = lambda *shape: torch.from_numpy(rs.uniform(-0.3, 0.3, shape).astype(np.float32)).to(DEV)
    w = rand_rows(128, seed=21).to(DEV) * w_scale
    sc = rand_rows(1, seed=30).to(DEV).reshape(128) * 0.1 + 1.0
    sh = rand_rows(1, seed=31).to(DEV).reshape(128) * 0.1
    packed = {"w1": f(128, 128), "s1": f(128) + 1.0, "t1": f(128), "w2": f(4, 16, 32), "s2": f(64) + 1.0, "t2": f(64),
              "w3": f(4, 16), "b3": f(4)}
    return w, sc, sh, packed


def _fold(w, sc, sh, packed, residual):
    return fold_last_into_heads(w, sc, sh, packed["w1"], packed["s1"], packed["t1"], residual)


def _logits64(agg, x, B, n, n_conn, w, sc, sh, residual, packed, sigmoid):
    """The UNFOLDED formula in float64 on the aggregated rows: layer (scale, shift, residual, no ReLU), node-type filter, 4 heads."""
    d = lambda t: t.double()
    h3 = d(agg) @ d(w).T
    if sc is not None:
        h3 = h3 * d(sc)
    if sh is not None:
        h3 = h3 + d(sh)
    if residual:
        h3 = h3 + d(x)
    h3 = h3.view(B, n, 128)[:, n_conn:, :].reshape(-1, 128)
    u = torch.relu(d(packed["s1"]) * (h3 @ d(packed["w1"]).T) + d(packed["t1"])).view(-1, 4, 32)
    z = torch.einsum("nhk,hok->nho", u, d(packed["w2"]))
    z = torch.relu(d(packed["s2"]).view(4, 16) * z + d(packed["t2"]).view(4, 16))
    y = (z * d(packed["w3"])).sum(-1) + d(packed["b3"])
    return torch.sigmoid(y) if sigmoid else y


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("frame,naux,main_only,conn,dm,da,chained", TOPOS)
def test_folded_launch_vs_unfolded_launch_and_float64(frame, naux, main_only, conn, dm, da, chained, B):
    g = ops.Graph.topo(frame, naux, main_only, False, use_connection_nodes=conn, diag_main=dm, diag_aux=da)
    assert g.num_conn == (naux + 1 if conn else 0)
    n, rows = g.num_nodes, B * g.num_nodes
    w, sc, sh, packed = _params(frame + naux)
    x, kid = rand_rows(rows, seed=9).to(DEV), None
    if not g.fused_classifier_ok:
        # a pyramid whose small levels do not pair up into child-sum segments ((8, 2) is one): the fused classifier does not cover
        # the handle, and the folded entry point refuses it the way the unfolded one does
        assert (frame, naux) == (8, 2)
        for launch in (lambda: ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, x, False, packed),
                       lambda: ops.gcn_layer_cls_fold_fwd(g, B, x, _fold(w, sc, sh, packed, True), True, packed)):
            with pytest.raises(RuntimeError, match="unsupported"):
                launch()
        return
    if chained:                                             # the input is a layer's output, with the child sums that layer left
        kid = ops.new_kidsum(g, B)
        x = ops.gcn_layer_fwd(g, B, x, w, sc, sh, x, relu=True, kidsum_out=kid)
    agg = ops.gcn_aggregate(g, B, x)
    before = g.ps_launches
    for sigmoid in (False, True):
        for residual in (True, False):
            for scale, shift in ((sc, sh), (None, None)):
                res = x if residual else None
                got = ops.gcn_layer_cls_fold_fwd(g, B, x, _fold(w, scale, shift, packed, residual), residual, packed, sigmoid, kidsum_in=kid)
                unfolded = ops.gcn_layer_cls_fwd(g, B, x, w, scale, shift, res, False, packed, sigmoid, kidsum_in=kid)
                want = _logits64(agg, x, B, n, g.num_conn, w, scale, shift, residual, packed, sigmoid)
                assert got.shape == unfolded.shape == want.shape == ((n - g.num_conn) * B, 4)
                bound = 2e-5 * max(1.0, float(want.abs().max()))
                err_u, err_64 = float((got - unfolded).abs().max()), float((got.double() - want).abs().max())
                print(f"{frame}/{naux} B={B} sigmoid={sigmoid} residual={residual} scale={scale is not None}: vs unfolded {err_u:.2e}, "
                      f"vs float64 {err_64:.2e} (unfolded vs float64 {float((unfolded.double() - want).abs().max()):.2e}), bound {bound:.2e}")
                assert err_u < bound and err_64 < bound, (sigmoid, residual, scale is not None, err_u, err_64, bound)
    assert g.ps_launches == before + 16                     # every call was one launch of the producer / consumer kernel


def test_folded_launch_is_deterministic_and_frame_independent():
    frame, naux, B = 64, 6, 3
    g = ops.Graph.topo(frame, naux)
    n = g.num_nodes
    w, sc, sh, packed = _params(3)
    kid = ops.new_kidsum(g, B)
    x = ops.gcn_layer_fwd(g, B, rand_rows(B * n, seed=4).to(DEV), w, sc, sh, None, relu=True, kidsum_out=kid)
    folded = _fold(w, sc, sh, packed, True)
    a = ops.gcn_layer_cls_fold_fwd(g, B, x, folded, True, packed, kidsum_in=kid)
    b = ops.gcn_layer_cls_fold_fwd(g, B, x, folded, True, packed, kidsum_in=kid)
    assert torch.equal(a, b)
    x1 = x[n:2 * n].contiguous()
    k1 = kid.view(B, g.kidsum_rows, 128)[1].contiguous()
    alone = ops.gcn_layer_cls_fold_fwd(g, 1, x1, folded, True, packed, kidsum_in=k1)
    assert torch.equal(a.view(B, n, 4)[1], alone)


def test_hidden_tile_write_after_read_at_full_grid():
    """hidden_group writes a wave's column slice of the A tile while the other consumer waves may still be reading it: the signal
    after a wave's last A fragment and the wait in front of its first write keep them apart.  A miss shows as a different logit
    in some launch, and only when every CU is busy and the four consumer waves drift apart: (224, 7), batch 8, 200 launches back
    to back, each compared with the first on the device."""
    frame, naux, B = 224, 7, 8
    g = ops.Graph.topo(frame, naux)
    w, sc, sh, packed = _params(11)
    x = torch.randn(B * g.num_nodes, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(6))     # (274 MB: drawn on the device)
    folded = _fold(w, sc, sh, packed, True)
    first = ops.gcn_layer_cls_fold_fwd(g, B, x, folded, True, packed)
    differ = torch.zeros((), dtype=torch.int64, device=DEV)
    for _ in range(199):
        differ += (ops.gcn_layer_cls_fold_fwd(g, B, x, folded, True, packed) != first).sum()
    assert int(differ) == 0
    want = ops.gcn_layer_cls_fwd(g, B, x, w, sc, sh, x, False, packed)
    assert float((first - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


# ---- model level: (64, 6), batch 2, eval ------------------------------------------------------------------------------------
FRAME, NAUX, BATCH = 64, 6, 2


@pytest.fixture(scope="module")
def stack():
    hip, ref = model_pair(FRAME, NAUX, 3, seed=13)
    topo, ei, nt, bi = graph_tensors(FRAME, NAUX, BATCH)
    feats = synthetic_node_feats(BATCH * topo.num_nodes, 128, seed=200)
    with torch.no_grad():
        want, _ = ref.forward_nodes(feats, ei, nt, BATCH)
    return hip, ref, feats.to(DEV), ei.to(DEV), want


@pytest.fixture
def route():
    yield egnn.ROUTES
    egnn.ROUTES.fold_last = True


def _forward(model, feats, ei):
    with torch.no_grad():
        return model.forward_nodes(feats, ei, BATCH)[0].clone()


def _count_folded_calls(monkeypatch):
    calls, real = [], ops.gcn_layer_cls_fold_fwd
    monkeypatch.setattr(ops, "gcn_layer_cls_fold_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _fresh_copy(model):
    twin, _ = model_pair(FRAME, NAUX, 3, seed=99)
    twin.load_state_dict(model.state_dict(), strict=True)
    return twin.eval()


def test_model_route_on_and_off_against_the_oracle(stack, route, monkeypatch):
    hip, _, feats, ei, want = stack
    calls = _count_folded_calls(monkeypatch)
    for on in (True, False):
        route.fold_last = on
        n0 = len(calls)
        got = _forward(hip, feats, ei).cpu()
        assert len(calls) == n0 + (1 if on else 0)
        err = float((got - want).abs().max())
        print(f"fold_last={on}: max|err| vs oracle {err:.2e}")
        assert err < TOL
        assert torch.equal(O.landmark_argmax(got, BATCH, FRAME), O.landmark_argmax(want, BATCH, FRAME))


def test_model_refolds_after_a_weight_change_and_a_mode_round_trip(stack, route):
    hip, _, feats, ei, _ = stack
    hip = _fresh_copy(hip)
    before = _forward(hip, feats, ei)
    with torch.no_grad():
        hip.gnn_layers[-1].module_0.lin.weight.mul_(1.25)
    after = _forward(hip, feats, ei)
    assert not torch.equal(after, before)
    assert torch.equal(after, _forward(_fresh_copy(hip), feats, ei))
    with torch.no_grad():
        hip.node_classifiers[2][0].weight.add_(0.01)                          # ... and of a head's first Linear
    assert torch.equal(_forward(hip, feats, ei), _forward(_fresh_copy(hip), feats, ei))
    hip.train()
    with torch.no_grad():
        hip.gnn_layers[-1].module_1.running_mean.add_(0.05)                   # (what a training step would have moved)
    hip.eval()
    assert torch.equal(_forward(hip, feats, ei), _forward(_fresh_copy(hip), feats, ei))


def test_model_graph_replay_equals_eager_and_recaptures_on_a_weight_change(stack, route):
    hip, _, feats, ei, _ = stack
    hip = _fresh_copy(hip)
    eager = _forward(hip, feats, ei)
    hip.enable_hip_graph(True)
    assert torch.equal(_forward(hip, feats, ei), eager) and hip.hip_graph_captures == 1
    assert torch.equal(_forward(hip, feats, ei), eager) and hip.hip_graph_captures == 1
    with torch.no_grad():
        hip.gnn_layers[-1].module_0.lin.weight.mul_(0.8)
    replayed = _forward(hip, feats, ei)
    assert hip.hip_graph_captures == 2
    hip.enable_hip_graph(False)
    assert torch.equal(replayed, _forward(hip, feats, ei)) and not torch.equal(replayed, eager)


def test_jumping_knowledge_max_stays_off_the_folded_route(stack, route, monkeypatch):
    """The heads of gnn_jk_mode='max' run on max(jk_in, layer output): not linear in the layer's operands.  The switch changes
    nothing for such a model (off is the code path from before the fold existed), and the folded entry point is never called."""
    _, _, feats, ei, _ = stack
    hip, _ = model_pair(FRAME, NAUX, 3, seed=21, gnn_jk_mode="max")
    calls = _count_folded_calls(monkeypatch)
    on = _forward(hip, feats, ei)
    route.fold_last = False
    off = _forward(hip, feats, ei)
    assert calls == [] and torch.equal(on, off)
