"""The CPU oracle against the golden vectors produced by the reference's own models.py
(tests/golden/make_golden.py) and against its independent dense fp64 restatement."""
import os

import numpy as np
import pytest
import torch

from fixtures_util import fill_state_dict, initial_coords, synthetic_frames
from oracle import gnn_oracle as O
from echoglad_amd.topology import HierTopology, TopologySpec


def _oracle_model(frame, naux, layers, coord=False, main_only=False, seed=0):
    m = O.OracleHierarchicalPatchModel(frame_size=frame, gnn_dropout_p=0.5, classifier_dropout_p=0.5,
                                       node_embedding_dim=128, node_hidden_dim=128, num_output_channels=4,
                                       num_gnn_layers=layers, num_aux_graphs=naux, classifier_hidden_dim=32,
                                       use_coordinate_graph=coord, output_activation="logit",
                                       use_main_graph_only=main_only)
    fill_state_dict(m, seed)
    return m.eval()


def _graph(frame, naux, batch, coord=False, main_only=False):
    topo = HierTopology(TopologySpec(frame, naux, main_only, coord))
    ei = torch.from_numpy(topo.batched_edge_index(batch))
    nt = torch.from_numpy(np.tile(topo.node_type(), batch))
    bi = torch.arange(batch).repeat_interleave(topo.num_nodes)
    return topo, ei, nt, bi


def test_kat_layers_and_logits(golden_dir):
    g = np.load(os.path.join(golden_dir, "kat_f16_a3.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, seed=int(g["weight_seed"]))
    topo, ei, nt, bi = _graph(frame, naux, B)
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    with torch.no_grad():
        feats = m.create_node_pixels(frames, B)
        assert torch.allclose(feats, torch.from_numpy(g["node_feats"]), atol=1e-6)
        logits, _, hidden = m.forward_nodes(feats, ei, nt, B, return_hidden=True)
        # the reference's own edge order (from_networkx) vs the closed form's sorted order: fp noise only
        logits_ref_order, _ = m.forward_nodes(feats, torch.from_numpy(g["edge_index"]), nt, B)
    assert np.abs(logits.numpy() - g["logits"]).max() < 2e-5
    assert np.abs(logits_ref_order.numpy() - g["logits"]).max() < 1e-6
    for i in range(L):
        pre_res = hidden[i + 1] - hidden[i]
        assert np.abs(pre_res.numpy() - g[f"layer{i}"]).max() < 5e-5


def test_gcn_sparse_vs_dense64(golden_dir):
    g = np.load(os.path.join(golden_dir, "kat_f16_a3.npz"))
    x = torch.from_numpy(g["node_feats"])
    ei = torch.from_numpy(g["edge_index"])
    rs = np.random.RandomState(3)
    w = torch.from_numpy(rs.uniform(-0.15, 0.15, (128, 128)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(128).astype(np.float32))
    s = O.gcn_conv_sparse(x, ei, w, b)
    d = O.gcn_conv_dense64(x, ei, w, b)
    assert (s.double() - d).abs().max() < 1e-5
    m = _oracle_model(16, 3, 3, seed=int(g["weight_seed"]))
    conv = m.gnn_layers[0].module_0
    d0 = O.gcn_conv_dense64(x, ei, conv.lin.weight.detach(), conv.bias.detach())
    assert np.abs(d0.numpy() - g["gcn0_dense64"]).max() < 1e-12


def test_gcn_norm_known_answer():
    # path graph 0-1-2: deg+1 = [2,3,2]
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    ei2, w = O.gcn_norm(ei, 3)
    assert ei2.shape[1] == 7
    dis = torch.tensor([2.0, 3.0, 2.0]).pow(-0.5)
    assert torch.allclose(w, dis[ei2[0]] * dis[ei2[1]])
    # existing self loops are replaced, not doubled
    ei3, w3 = O.gcn_norm(torch.tensor([[0, 0, 1], [0, 1, 0]]), 2)
    assert ei3.shape[1] == 4 and torch.allclose(w3, torch.full((4,), 0.5))


def test_gcn_conv_literal_known_answer():
    """Both restatements against hand-computed numbers: an existing self loop, an isolated node, a one-directional edge
    and a duplicate edge (which PyG's scatter_add counts twice)."""
    from fixtures_util import gcn_known_answer
    ei, x, w, b, want, dis = gcn_known_answer()
    s = O.gcn_conv_sparse(x, ei, w, b)
    d = O.gcn_conv_dense64(x, ei, w, b)
    assert (s.double() - want).abs().max() < 1e-6
    assert (d - want).abs().max() < 1e-7
    ei2, wts = O.gcn_norm(ei, 6)
    assert ei2.shape[1] == 6 + 6                       # 7 edges - 1 self loop + 6 self loops
    deg = torch.zeros(6, dtype=torch.float64).index_add_(0, ei2[1], torch.ones(12, dtype=torch.float64))
    assert deg.tolist() == [2, 4, 2, 1, 2, 1]
    assert (deg.pow(-0.5) - dis).abs().max() < 1e-7


@pytest.mark.parametrize("n", [3, 7, 64, 130])
def test_gcn_conv_closed_form_families(n):
    """Complete graph, cycle, star: A_hat has a closed form (fixtures_util.gcn_closed_form_families) -- both restatements of
    GCNConv must reproduce it, with a random weight and bias applied on top (out = A_hat (x W^T) + b)."""
    from fixtures_util import gcn_closed_form_families
    rs = np.random.RandomState(n)
    x = torch.from_numpy(rs.standard_normal((n, 128)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(-0.2, 0.2, (128, 128)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(128).astype(np.float32))
    for name, ei, a_hat in gcn_closed_form_families(n, seed=n):
        want = a_hat(x.double() @ w.double().t()) + b.double()
        assert (O.gcn_conv_dense64(x, ei, w, b) - want).abs().max() < 1e-12, name
        assert (O.gcn_conv_sparse(x, ei, w, b).double() - want).abs().max() < 2e-5, name


def test_dense_and_sparse_agree_on_multigraphs():
    rs = np.random.RandomState(0)
    n, e = 40, 300                                     # dense enough that many (src, dst) pairs repeat
    ei = torch.from_numpy(np.stack([rs.randint(0, n, e), rs.randint(0, n, e)]).astype(np.int64))
    assert len({(int(a), int(b)) for a, b in ei.t()}) < e
    x = torch.from_numpy(rs.standard_normal((n, 128)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(-0.1, 0.1, (128, 128)).astype(np.float32))
    s = O.gcn_conv_sparse(x, ei, w, None)
    d = O.gcn_conv_dense64(x, ei, w, None)
    assert (s.double() - d).abs().max() < 1e-5


def test_cfg1_plumbing(golden_dir):
    """BASELINE config 1: single 64x64 frame, 2 aux levels, 2 GNN layers, batch 1."""
    g = np.load(os.path.join(golden_dir, "cfg1_f64_a2.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, seed=int(g["weight_seed"]))
    topo, ei, nt, bi = _graph(frame, naux, B)
    assert topo.num_nodes == int(g["num_nodes"]) == 4116
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    with torch.no_grad():
        logits, _ = m(x=frames, edge_index=ei, node_type=nt, batch_idx=bi)
    rows = g["sample_rows"]
    assert np.abs(logits.numpy()[rows] - g["logits_rows"]).max() < 2e-5
    assert abs(logits.double().sum().item() - float(g["logits_sum"])) < 1e-2
    assert np.array_equal(O.landmark_argmax(logits, B, frame).numpy(), g["argmax"])


def test_coordinate_graph_path(golden_dir):
    g = np.load(os.path.join(golden_dir, "coord_f32_a4.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, coord=True, seed=int(g["weight_seed"]))
    topo, ei, nt, bi = _graph(frame, naux, B, coord=True)
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    coords0 = initial_coords(B, frame)
    assert np.allclose(coords0.numpy(), g["coords0"])
    with torch.no_grad():
        logits, coords = m(x=frames, node_coords=coords0.clone(), edge_index=ei, node_type=nt, batch_idx=bi)
    assert np.abs(coords.numpy() - g["out_coords"]).max() < 1e-4
    assert np.abs(logits.numpy() - g["logits"]).max() < 5e-5
    assert torch.equal(coords0, initial_coords(B, frame)), "the oracle must not mutate the caller's coords"


def test_coordinate_graph_train_gradients(golden_dir):
    g = np.load(os.path.join(golden_dir, "coord_f32_a4.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, coord=True, seed=int(g["weight_seed"]))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.train()
    topo, ei, nt, bi = _graph(frame, naux, B, coord=True)
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    logits, coords = m(x=frames, node_coords=initial_coords(B, frame), edge_index=ei, node_type=nt, batch_idx=bi)
    assert np.abs(logits.detach().numpy() - g["train_logits"]).max() < 2e-4
    loss = (logits ** 2).mean() + (coords ** 2).mean() * 1e-3
    assert abs(loss.item() - float(g["train_loss"])) < 1e-4 * max(1.0, abs(float(g["train_loss"])))
    loss.backward()
    gn = {k: float(p.grad.double().norm()) for k, p in m.named_parameters() if p.grad is not None}
    for k, ref in zip(g["grad_keys"], g["grad_norms"]):
        assert abs(gn[str(k)] - ref) <= 2e-3 * max(ref, 1e-6) + 1e-7, (k, gn[str(k)], ref)


def test_main_graph_only(golden_dir):
    g = np.load(os.path.join(golden_dir, "mainonly_f16.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, main_only=True, seed=int(g["weight_seed"]))
    topo, ei, nt, bi = _graph(frame, naux, B, main_only=True)
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    with torch.no_grad():
        logits, _ = m(x=frames, edge_index=ei, node_type=nt, batch_idx=bi)
    assert np.abs(logits.numpy() - g["logits"]).max() < 2e-5


def test_dense_bilinear_equals_four_taps():
    """models.py:539-553 is a 4-tap bilinear sample incl. the clamped edges 0 and F-1."""
    rs = np.random.RandomState(0)
    S = 12
    frame = torch.from_numpy(rs.standard_normal((5, S, S)).astype(np.float32))
    coords = torch.tensor([[0.0, 0.0], [S - 1.0, S - 1.0], [3.25, 7.75], [10.999, 0.001], [5.0, 11.0]])
    dense = O.bilinear_interpolation_dense(coords, frame)
    for p, (h, w) in enumerate(coords.tolist()):
        h0, w0 = int(np.floor(h)), int(np.floor(w))
        acc = torch.zeros(5)
        for hh, wh in ((h0, 1 - (h - h0)), (h0 + 1, h - h0)):
            for ww, wwt in ((w0, 1 - (w - w0)), (w0 + 1, w - w0)):
                if hh < S and ww < S:
                    acc += wh * wwt * frame[:, hh, ww]
        assert torch.allclose(dense[p], acc, atol=1e-5)


def test_argmax_fixture_with_near_ties():
    B, F = 2, 8
    rs = np.random.RandomState(1)
    logits = torch.from_numpy(rs.standard_normal((B * (4 + 16 + F * F), 4)).astype(np.float32))
    per = logits.view(B, -1, 4)
    per[0, -1, 0] = 50.0
    per[0, -2, 0] = 50.0 - 1e-5          # near tie: the larger one must win
    per[1, 20 + 7, 3] = 60.0
    idx = O.landmark_argmax(logits, B, F)
    assert idx[0, 0].item() == F * F - 1 and idx[1, 3].item() == 7
    e = O.landmark_expected_coords(logits, B, F)
    assert e.shape == (B, 4, 2) and (e >= 0).all() and (e <= F - 1).all()


# ---------------------------------------------------------------- losses / landmark decode
from oracle import loss_oracle as LO   # noqa: E402

DECODE_FIXTURES = ["decode_f16_a3.npz", "decode_f30_a3.npz"]


@pytest.mark.parametrize("name", DECODE_FIXTURES)
def test_loss_oracle_matches_reference_losses_and_gradients(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    B, F, naux = int(d["batch"]), int(d["frame"]), int(d["naux"])
    lg = torch.from_numpy(d["logits"]).requires_grad_(True)
    y, v = torch.from_numpy(d["labels"]), torch.from_numpy(d["valid"])
    n = lg.shape[0] // B
    bce = LO.weighted_bce_with_logits(lg.view(B, n, 4), y.view(B, n, 4), v, ones_weight=9000, loss_weight=1)
    g, = torch.autograd.grad(bce, lg)
    assert abs(float(bce.detach()) - float(d["bce"])) <= 1e-5 * abs(float(d["bce"]))
    assert np.allclose(g.numpy(), d["grad_bce"], rtol=1e-5, atol=1e-9)
    elm = LO.expected_landmark_mse(lg, y, v, B, F, naux, loss_weight=10)
    g, = torch.autograd.grad(elm, lg)
    assert abs(float(elm.detach()) - float(d["elm"])) <= 1e-5 * abs(float(d["elm"]))
    assert np.allclose(g.numpy(), d["grad_elm"], rtol=1e-4, atol=1e-8)
    # old value-only fixture of the KAT logits
    assert LO.level_grids(16, 3) == [(0, 2), (4, 4), (20, 8), (84, 16)]


@pytest.mark.parametrize("name", DECODE_FIXTURES)
def test_loss_oracle_matches_reference_evaluator(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    B, F = int(d["batch"]), int(d["frame"])
    got = LO.evaluate_landmarks(torch.from_numpy(d["logits"]), torch.from_numpy(d["labels"]),
                                torch.from_numpy(d["pix2mm_x"]), torch.from_numpy(d["pix2mm_y"]),
                                torch.from_numpy(d["valid"]), B, F)
    for k, want in zip(d["last_keys"], d["last_vals"]):
        assert abs(got[str(k)] - float(want)) <= 1e-5 * max(1.0, abs(float(want))), k
    assert np.array_equal(got["gt_coords"].numpy(), d["gt_coords"])
    assert np.allclose(got["pred_coords"].numpy(), d["pred_coords"], rtol=1e-6, atol=1e-5)
    for k, want in zip(d["width_keys"], d["width_vals"]):
        assert np.allclose(got["widths"][str(k)].numpy(), want, rtol=1e-5, atol=1e-5), k
    # hard argmax over the main grid: the first of two equal maxima wins (frame 0, channel 1)
    am = O.landmark_argmax(torch.from_numpy(d["logits"]), B, F).numpy()
    assert np.array_equal(am, d["argmax_main"])
    assert am[0, 1] == 3 * F + 5


def test_cfg4_fixture_eval(golden_dir):
    """BASELINE configs[3] shape (224x224, 7 aux levels, coordinate graph on) at B = 2: the oracle against what the
    reference's own forward produced (sampled rows, coordinates after every layer, arg-max indices)."""
    g = np.load(os.path.join(golden_dir, "cfg4_f224_a7_coord.npz"))
    frame, naux, L, B = int(g["frame"]), int(g["naux"]), int(g["layers"]), int(g["batch"])
    m = _oracle_model(frame, naux, L, coord=True, seed=int(g["weight_seed"]))
    topo, ei, nt, bi = _graph(frame, naux, B, coord=True)
    assert topo.num_nodes == int(g["num_nodes"])
    frames = synthetic_frames(B, 128, frame, int(g["frame_seed"]))
    coords0 = torch.from_numpy(g["coords0"])
    with torch.no_grad():
        feats = m.create_node_pixels(frames, B, coords0.view(B, 4, 2))
        assert np.abs(feats.numpy()[g["hidden_rows"]] - g["node_feats_rows"]).max() < 1e-5
        logits, coords, hidden = m.forward_nodes(feats, ei, nt, B, coords0.clone(), return_hidden=True)
    assert np.abs(coords.numpy() - g["out_coords"]).max() < 1e-4
    assert np.abs(logits.numpy()[g["sample_rows"]] - g["logits_rows"]).max() < 5e-5
    assert abs(float(logits.double().sum()) - float(g["logits_sum"])) < 1e-6 * float(g["logits_abs_sum"])
    assert np.array_equal(O.landmark_argmax(logits, B, frame).numpy(), g["argmax"])


# ---- oracle/adam_oracle.py: the fp64 form against torch's own Adam in double, and how hard the GPU tests' tolerance bites ----------
def _adam_case(seed=11, n=1500, steps=6, t0=0):
    """Parameters, per-step gradients (scaled differently per step, a few elements close to 0), and non-zero moments when the run
    starts at a loaded step count t0 > 0."""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    scales = [1.0, 0.3, 2.0, 0.7, 3.0, 1.5]
    grads = [(rs.standard_normal(n) * scales[k % 6]).astype(np.float32) for k in range(steps)]
    for g in grads:
        g[::97] *= 1e-3
    m = (rs.standard_normal(n) * 0.3).astype(np.float32) if t0 else np.zeros(n, np.float32)
    v = (rs.standard_normal(n) ** 2 * 0.2).astype(np.float32) if t0 else np.zeros(n, np.float32)
    return p, grads, m, v


def _run_adam(step_fn, p, grads, m, v, t0, dtype, **hyper):
    p, m, v = (a.astype(dtype) for a in (p, m, v))
    for k, g in enumerate(grads):
        p, m, v = step_fn(p, g, m, v, t0 + k + 1, dtype=dtype, **hyper)
    return p, m, v


@pytest.mark.parametrize("hyper", [dict(), dict(weight_decay=0.01), dict(maximize=True), dict(lr=3e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.1)])
def test_adam_oracle_fp64_is_torch_adam_in_double(hyper):
    """The oracle was written from the documented formulas; torch's single-tensor CPU implementation in float64 is an independent
    evaluation of them.  One tensor sits a step out (its count stays behind)."""
    from oracle import adam_oracle as AO
    p0, grads, _, _ = _adam_case()
    q0 = p0[:40] * 2
    tp = [torch.nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in (p0, q0)]
    opt = torch.optim.Adam(tp, foreach=False, **hyper)
    o = AO.AdamOracle([p0, q0])
    for k, g in enumerate(grads):
        gs = [g, None if k == 2 else g[:40] * 0.5]
        for t, gk in zip(tp, gs):
            t.grad = None if gk is None else torch.from_numpy(gk.astype(np.float64))
        opt.step()
        o.step(gs, **hyper)
    assert o.t == [6, 5] and [int(opt.state[t]["step"]) for t in tp] == [6, 5]
    for k, t in enumerate(tp):
        for got, want in ((o.p[k], t), (o.m[k], opt.state[t]["exp_avg"]), (o.v[k], opt.state[t]["exp_avg_sq"])):
            want = want.detach().numpy()
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def _eps_inside_step(p, g, m, v, t, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, dtype=np.float32):
    """adam_step with ONE mistake: eps added before the division by sqrt(1 - b2^t)."""
    f = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a).astype(dtype) for a in (p, g, m, v))
    b1, b2, lr, eps, wd = f(betas[0]), f(betas[1]), f(lr), f(eps), f(weight_decay)
    g = -g if maximize else g
    g = g + wd * p
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    step_size = f(np.float64(lr) / (1.0 - np.float64(b1) ** np.float64(t)))
    bc2_sqrt = f(np.sqrt(1.0 - np.float64(b2) ** np.float64(t)))
    return p - step_size * m / ((np.sqrt(v) + eps) / bc2_sqrt), m, v


def _worst_ratio(got, want32, want64):
    """max over p, exp_avg, exp_avg_sq of max|got - fp64 oracle| / bound: > 1 fails the GPU tests' comparison."""
    from oracle import adam_oracle as AO
    ratios = [np.abs(g.astype(np.float64) - w64).max() / AO.bound(w32, w64) for g, w32, w64 in zip(got, want32, want64)]
    return max(ratios), ratios


def test_adam_oracle_tolerance_bites():
    """The bound of the GPU comparisons -- 4 * max(|fp32 oracle - fp64 oracle|, one fp32 ulp of the largest value) -- against what a
    subtly wrong kernel would compute: each mistake, evaluated in fp32, is at least 100 bounds away; the fp32 oracle itself is inside."""
    from oracle import adam_oracle as AO
    f32 = AO.as_float32
    for name, hyper, t0, wrong in [
            ("step count behind by one", dict(lr=f32(1e-3)), 3, lambda h: _run_adam(AO.adam_step, *case, 2, np.float32, **h)),
            ("eps inside the bias correction", dict(lr=f32(1e-3), eps=f32(1e-3)), 0, lambda h: _run_adam(_eps_inside_step, *case, 0, np.float32, **h)),
            ("weight decay dropped", dict(lr=f32(1e-3), weight_decay=f32(0.01)), 0,
             lambda h: _run_adam(AO.adam_step, *case, 0, np.float32, **dict(h, weight_decay=0.0)))]:
        hyper = dict(hyper, betas=(f32(0.9), f32(0.999)))
        case = _adam_case(t0=t0)
        o64 = _run_adam(AO.adam_step, *case, t0, np.float64, **hyper)
        o32 = _run_adam(AO.adam_step, *case, t0, np.float32, **hyper)
        inside, _ = _worst_ratio(o32, o32, o64)
        worst, ratios = _worst_ratio(wrong(hyper), o32, o64)
        print(f"{name}: p, exp_avg, exp_avg_sq are {ratios[0]:.0f}, {ratios[1]:.0f}, {ratios[2]:.0f} bounds away; the fp32 oracle {inside:.2f}")
        assert inside <= 0.25 + 1e-12, name               # (e32 / (4 max(e32, ulp)) by construction)
        assert ratios[0] >= 100.0, (name, ratios)        # every one of them shows in the parameters
        assert worst >= 100.0, (name, ratios)


def test_adam_hyper_parameters_as_c_floats():
    """eg_adam_step takes the hyper-parameters as C floats.  1 - float32(0.999) is 1.3e-5 (relative) off 1 - 0.999, and exp_avg_sq with
    it; the bias correction uses the same rounded beta, so the parameters are a few fp32 ulps off the update with the exact
    hyper-parameters, no more.  The GPU tests hand the fp64 oracle the rounded values: this is the size of what that leaves out."""
    from oracle import adam_oracle as AO
    case = _adam_case()
    exact = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    rounded = dict(lr=AO.as_float32(1e-3), betas=(AO.as_float32(0.9), AO.as_float32(0.999)), eps=AO.as_float32(1e-8))
    pe, me, ve = _run_adam(AO.adam_step, *case, 0, np.float64, **exact)
    pr, mr, vr = _run_adam(AO.adam_step, *case, 0, np.float64, **rounded)
    rel_v = np.abs(vr / ve - 1).max()
    assert 1.2e-5 < rel_v < 1.4e-5
    assert np.abs(mr - me).max() < 5e-7 * np.abs(me).max()
    assert np.abs(pr - pe).max() <= 4 * AO.ulp32(np.abs(pe).max())
