"""-m gpu: WeightedBCE on probabilities (eg_bce_probs_*) and the one-node criteria with the BCE on probabilities and / or the coordinate
MAE (eg_criteria_ex_*), against the fixtures produced by the reference's own criterion classes (make_criteria_golden.py), against the
criteria computed one by one, and through the engine: losses.build's criteria fuse, capture into a graph and train a sigmoid model."""
import copy
import ctypes as ct
import os

import numpy as np
import pytest
import torch

import make_criteria_golden as G
from gpu_util import DEV, graph_tensors, model_pair
from oracle import loss_oracle as LO
from echoglad_amd import _lib, data, engine, losses, ops
from echoglad_amd.synthetic import synthetic_frames

pytestmark = pytest.mark.gpu

BCE_CASES = sorted(G.BCE_CASES)


def _bce_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"crit_bce_{name}.npz"))
    frame, naux, batch, seed, ow = G.BCE_CASES[name]
    p, y, v = G.bce_inputs(frame, naux, batch, seed)
    assert G.input_digest(p, y, v) == str(z["digest"])
    return z, frame, naux, batch, ow, p, y, v


def _mae_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "crit_mae.npz"))
    names = [str(s) for s in z["names"]]
    k = names.index(name)
    rows, seed, w = G.MAE_CASES[name]
    off = sum(G.MAE_CASES[m][0] * 2 for m in names[:k])
    pred, y = G.mae_inputs(rows, seed)
    assert G.input_digest(pred, y) == str(z["digests"][k])
    return float(z["values"][k]), z["grads"][off:off + rows * 2].reshape(rows, 2), w, pred, y


def _sampled(g, z):
    g = g.reshape(-1)
    return g[z["idx"]] if "idx" in z else g


def _close(got, want, rtol):
    return abs(float(got) - float(want)) <= rtol * abs(float(want))


@pytest.mark.parametrize("name", BCE_CASES)
def test_weighted_bce_matches_the_reference_and_is_reproducible(golden_dir, name):
    z, frame, naux, B, ow, p, y, v = _bce_case(golden_dir, name)
    n = p.shape[0] // B
    crit = losses.WeightedBCE(reduction="none", ones_weight=ow, loss_weight=1)
    runs = []
    for _ in range(2):
        pt = torch.from_numpy(p).to(DEV).requires_grad_(True)
        loss = crit.compute(pt.view(B, n, 4), torch.from_numpy(y).to(DEV).view(B, n, 4), torch.from_numpy(v).to(DEV))
        g, = torch.autograd.grad(loss, pt)
        runs.append((loss.detach().cpu(), g.cpu()))
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1) and torch.equal(g0, g1)                   # same bits on every run
    # fp64 sums of fp32 element values vs the reference's fp32 sums; gradient entries one fp32 formula each, in another order
    assert _close(l0, z["bce"], 1e-5), (float(l0), float(z["bce"]))
    got = _sampled(g0.numpy(), z)
    assert np.allclose(got, z["grad_bce"], rtol=1e-5, atol=0.0)
    # the exact 0 / 1 probabilities: torch's clamps, e.g. d/dp at p = 0, y = 1 is -1e12 * w / sum(valid)
    zero_pos = (p == 0.0) & (y == 1.0) & (v > 0)
    if zero_pos.any():
        assert np.allclose(g0.numpy()[zero_pos], -1e12 * (ow if ow > 1 else 1.0) / v.astype(np.float64).sum(), rtol=1e-5)


def test_weighted_bce_out_of_range_probability_gives_nan():
    """torch raises for p outside [0, 1]; the kernels cannot: the loss is NaN -- also when that element is not valid -- and so is that
    element's gradient; in-range elements keep finite gradients."""
    rs = np.random.RandomState(3)
    p = torch.from_numpy(rs.uniform(0, 1, (512, 4)).astype(np.float32))
    y = torch.from_numpy((rs.uniform(0, 1, (512, 4)) < 0.1).astype(np.float32))
    v = torch.ones(512, 4)
    v[7] = 0.0
    for bad in (-1e-6, 1.0 + 1e-6, float("nan"), float("inf")):
        q = p.clone()
        q[7, 2] = bad                                                     # an invalid row
        qt = q.to(DEV).requires_grad_(True)
        loss = losses.WeightedBCE("none", 9000, 1).compute(qt.view(1, 512, 4), y.to(DEV).view(1, 512, 4), v.to(DEV))
        g, = torch.autograd.grad(loss, qt)
        assert torch.isnan(loss).item(), bad
        g = g.cpu()
        assert torch.isnan(g[7, 2]).item()
        mask = torch.ones_like(g, dtype=torch.bool)
        mask[7, 2] = False
        assert torch.isfinite(g[mask]).all()
        out = ops.bce_probs_fwd(q.to(DEV), y.to(DEV), None, 1.0)
        assert torch.isnan(out[0]).item() and torch.isnan(out[2]).item() and float(out[1]) == q.numel()
    # the fused node follows the same rule
    B, frame, naux = 1, 16, 3
    pp, yy, vv = (torch.from_numpy(a).to(DEV) for a in G.bce_inputs(frame, naux, B, 101)[:3])
    pp = pp.clone()
    pp[5, 1] = 1.5
    crit = {"bce": losses.WeightedBCE("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, frame, naux)}
    ls = engine.compute_loss(crit, pp, yy, None, None, vv, B)
    assert isinstance(ls, losses.LossDict) and torch.isnan(ls["bce"]).item() and torch.isfinite(ls["elm"]).item()


def _one_by_one(crit, preds, y, valid, cp, cy, B, monkeypatch):
    with monkeypatch.context() as m:
        m.setenv("EG_FUSED_CRITERIA", "0")
        out = engine.compute_loss(crit, preds, y, cp, cy, valid, B)
    assert not isinstance(out, losses.LossDict)
    return out


@pytest.mark.parametrize("name", ["f16_b1_w9000", "f16_b2_w9000", "f224_b1_w9000", "f224_b2_w1"])
@pytest.mark.parametrize("coord", [None, "mse", "mae"])
@pytest.mark.parametrize("form", ["probs", "logits"])
def test_fused_node_matches_one_by_one_and_the_fixture(golden_dir, monkeypatch, name, coord, form):
    z, frame, naux, B, ow, p, y, v = _bce_case(golden_dir, name)
    mae_val, mae_grad, w, cpred, cy = _mae_case(golden_dir, "b1" if B == 1 else "b2")
    if form == "logits":                                                  # same labels and valid, logits instead of probabilities
        p = (np.random.RandomState(B * frame).standard_normal(p.shape) * 2).astype(np.float32)
    bce = (losses.WeightedBCE if form == "probs" else losses.WeightedBCEWithLogitsLoss)("none", ow, 1)
    crit = {"bce": bce, "elm": losses.ExpectedLandmarkMSE(G.ELM_WEIGHT, B, frame, naux)}
    if coord:
        crit["coordinate"] = engine.MAE(w) if coord == "mae" else engine.MSE(w)
    yt, vt = torch.from_numpy(y).to(DEV), torch.from_numpy(v).to(DEV)
    res = []
    for fused in (True, False):
        pt = torch.from_numpy(p).to(DEV).requires_grad_(True)
        ct_ = torch.from_numpy(cpred).to(DEV).requires_grad_(True)
        cyt = torch.from_numpy(cy).to(DEV)
        if fused:
            ls = engine.compute_loss(crit, pt, yt, ct_, cyt, vt, B)
            assert isinstance(ls, losses.LossDict) and list(ls) == list(crit)
            total = engine.total_loss(ls)
        else:
            ls = _one_by_one(crit, pt, yt, vt, ct_, cyt, B, monkeypatch)
            total = sum(ls.values())
        gp, gc = torch.autograd.grad(total, [pt, ct_], allow_unused=True)
        res.append(({k: float(t.detach()) for k, t in ls.items()}, float(total.detach()), gp.cpu().numpy(),
                     None if gc is None else gc.cpu().numpy()))
    (lf, tf, gpf, gcf), (lo, to, gpo, gco) = res
    for k in crit:
        assert _close(lf[k], lo[k], 2e-6), (k, lf[k], lo[k])
    assert _close(tf, to, 2e-6)
    # (entrywise: with probabilities the exact 0 / 1 entries are ~1e15 and would hide everything else)
    atol = 1e-5 * float(np.quantile(np.abs(gpo), 0.99))
    assert np.allclose(gpf, gpo, rtol=1e-5, atol=atol), float(np.abs(gpf - gpo).max())
    if coord:
        assert np.allclose(gcf, gco, rtol=1e-6, atol=0)
    else:
        assert gcf is None
    if coord == "mae":                                                   # against the reference's L1Loss
        assert _close(lf["coordinate"], mae_val, 1e-6)
        assert np.array_equal(gcf, mae_grad)
    if form == "probs":                                                  # against the reference's WeightedBCE + ExpectedLandmarkMSE
        assert _close(lf["bce"], z["bce"], 1e-5) and _close(lf["elm"], z["elm"], 1e-5)
        gb, ge = z["grad_bce"].astype(np.float64), z["grad_elm"].astype(np.float64)
        got = _sampled(gpf, z)
        assert np.all(np.abs(got - (gb + ge)) <= 2e-5 * np.abs(gb) + 2e-4 * np.abs(ge) + 1e-6 * np.abs(ge).max())


def _raw_criteria(ex, x, y, v, B, levels, inv_side, ow, cp, cy, wc, flags=(0, 0)):
    """eg_criteria_fwd / _bwd, or eg_criteria_ex_fwd / _bwd with ``flags``: every output, forward and backward."""
    lib = _lib.load()
    start, side, n = ops._level_arrays(levels)
    ws = torch.zeros(int(lib.eg_criteria_workspace_bytes(B, side, n)), dtype=torch.uint8, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    o = {k: torch.full((B, n, 4, 2), float("nan"), **f32) for k in ("expect", "stats", "d_expect")}
    o.update({k: torch.full((), float("nan"), **f32) for k in ("total", "bce", "elm", "coord")})
    o["bce_scale"] = torch.full((1,), float("nan"), **f32)
    o["d_coord"] = torch.full_like(cp, float("nan"))
    P = ops._ptr
    args = [P(x), P(y), P(v), B, x.shape[0] // B, start, side, n, P(inv_side), ct.c_float(ow), ct.c_float(1.0), ct.c_float(10.0), P(cp),
            P(cy), cp.numel(), ct.c_float(wc), P(ws), P(o["expect"]), P(o["stats"]), P(o["d_expect"]), P(o["d_coord"]), P(o["bce_scale"]),
            P(o["total"]), P(o["bce"]), P(o["elm"]), P(o["coord"])]
    fn = lib.eg_criteria_ex_fwd if ex else lib.eg_criteria_fwd
    _lib.check(fn(*(args + (list(flags) if ex else []) + [ops._stream()])), "criteria fwd")
    one = torch.ones(1, **f32)
    o["d_logits"] = torch.full_like(x, float("nan"))
    o["d_coord_out"] = torch.full_like(cp, float("nan"))
    args = [P(x), P(y), P(v), B, x.shape[0] // B, start, side, n, ct.c_float(ow), P(o["expect"]), P(o["stats"]), P(o["d_expect"]),
            P(o["bce_scale"]), P(o["d_coord"]), cp.numel(), P(one), None, None, None, P(o["d_logits"]), P(o["d_coord_out"])]
    fn = lib.eg_criteria_ex_bwd if ex else lib.eg_criteria_bwd
    _lib.check(fn(*(args + (list(flags) if ex else []) + [ops._stream()])), "criteria bwd")
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in o.items()}


@pytest.mark.parametrize("B,extra_rows", [(1, 0), (2, 0), (8, 0), (2, 8)])
def test_criteria_ex_00_gives_the_bits_of_criteria(B, extra_rows):
    """eg_criteria_ex_*(0, 0) is eg_criteria_*: every output bit for bit -- through the one-launch ticket path (batch <= 2), the
    two-launch final step (batch 8) and the separate BCE pass (rows outside every level)."""
    frame, naux = 16, 3
    levels = losses.level_grids(frame, naux)
    n = levels[-1][0] + frame * frame + extra_rows
    rs = np.random.RandomState(B + extra_rows)
    x = torch.from_numpy((rs.standard_normal((B * n, 4)) * 3).astype(np.float32)).to(DEV)
    y = torch.from_numpy((rs.uniform(0, 1, (B * n, 4)) < 0.05).astype(np.float32)).to(DEV)
    v = torch.from_numpy((rs.uniform(0, 1, (B * n, 4)) < 0.8).astype(np.float32)).to(DEV)
    cp = torch.from_numpy(rs.uniform(0, 16, (4 * B, 2)).astype(np.float32)).to(DEV)
    cy = torch.from_numpy(rs.randint(0, 16, (4 * B, 2)).astype(np.float32)).to(DEV)
    inv_side = (1.0 / torch.tensor([s for _, s in levels], dtype=torch.float32, device=DEV)).contiguous()
    a = _raw_criteria(False, x, y, v, B, levels, inv_side, 9000.0, cp, cy, 0.5)
    b = _raw_criteria(True, x, y, v, B, levels, inv_side, 9000.0, cp, cy, 0.5, (0, 0))
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.isfinite(a["d_logits"]).all() and torch.isfinite(a["total"])
    # the other forms on the same arrays run through the same launches (probabilities: the logits squashed into [0, 1])
    xp = torch.sigmoid(x).contiguous()
    c = _raw_criteria(True, xp, y, v, B, levels, inv_side, 9000.0, cp, cy, 0.5, (1, 1))
    d = _raw_criteria(True, xp, y, v, B, levels, inv_side, 9000.0, cp, cy, 0.5, (1, 0))
    assert torch.equal(c["bce"], d["bce"]) and torch.equal(c["elm"], d["elm"]) and torch.equal(c["d_logits"], d["d_logits"])
    want_l1 = 0.5 * (cp - cy).abs().mean().cpu()
    assert _close(c["coord"], want_l1, 1e-6) and _close(d["coord"], 0.5 * ((cp - cy) ** 2).mean().cpu(), 1e-6)
    assert torch.equal(c["d_coord_out"], torch.sign(cp - cy).cpu() * (0.5 / cp.numel()))          # torch's l1_loss backward
    with pytest.raises(RuntimeError, match="0 or 1"):
        _raw_criteria(True, x, y, v, B, levels, inv_side, 9000.0, cp, cy, 0.5, (2, 0))


def _builder_config(B, frame, naux, coord, block=None):
    cfg = {k: dict(v) for k, v in (block or G.DEFAULT_BLOCK).items()}
    cfg.update({"batch_size": B, "frame_size": frame, "num_aux_graphs": naux, "use_coordinate_graph": coord,
                "use_main_graph_only": False, "num_output_channels": 4})
    return cfg


@pytest.mark.parametrize("block", ["default", "bce"])
def test_compute_loss_fuses_the_builders_coordinate_graph_criteria(golden_dir, monkeypatch, block):
    """The reference's criteria for a coordinate-graph config (WeightedBceWithLogits or bce, ExpectedLandmarkMse, coordinate MAE) run
    as ONE node -- engine.compute_loss returns a losses.LossDict -- with the values of the one-by-one route."""
    B, frame, naux = 2, 16, 3
    crit = losses.build(_builder_config(B, frame, naux, True, G.DEFAULT_BLOCK if block == "default" else G.BCE_BLOCK))
    assert type(crit["coordinate"]) is engine.MAE
    p, y, v = (torch.from_numpy(a).to(DEV) for a in G.bce_inputs(frame, naux, B, 102))
    if block == "default":
        p = torch.logit(p.clamp(1e-4, 1 - 1e-4)).contiguous()
    _, _, _, cpred, cy = _mae_case(golden_dir, "b2")
    cp, cyt = torch.from_numpy(cpred).to(DEV), torch.from_numpy(cy).to(DEV)
    ls = engine.compute_loss(crit, p, y, cp, cyt, v, B)
    assert isinstance(ls, losses.LossDict), type(ls)
    assert list(ls) == list(crit)
    lo = _one_by_one(crit, p, y, v, cp, cyt, B, monkeypatch)
    for k in crit:
        assert _close(ls[k], lo[k], 2e-6), (k, float(ls[k]), float(lo[k]))


def _setup_coord_model(frame, naux, seed, B):
    hip, _ = model_pair(frame, naux, 2, coord=True, seed=seed)
    torch.manual_seed(seed)
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
    np.random.seed(seed)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=True)
    batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
    return hip, emb, batch


def test_graphed_train_step_with_the_builders_criteria_replays_equal_eager_steps():
    """engine.GraphedTrainStep at batch 1 (the reference's batch size) on a coordinate-graph model with losses.build's criteria
    (WeightedBceWithLogits + ExpectedLandmarkMse + coordinate MAE, one node): replay k is the eager step under dropout epoch k, bit
    for bit, as the existing graphed-step tests check for the MSE form."""
    B, frame, naux, p, warm, replays = 1, 32, 4, 0.5, 2, 3

    def build():
        hip, emb, batch = _setup_coord_model(frame, naux, 11, B)
        for m in hip.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = p
        hip.train()
        crit = losses.build(_builder_config(B, frame, naux, True))
        for q in emb.parameters():
            q.requires_grad_(False)
        params = list(hip.parameters())
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        model = {"embedder": emb, "landmark": hip}
        coords0 = batch.node_coords.clone()

        def loss_fn():
            batch.node_coords = coords0.clone()
            preds, coord_preds = engine.forward_batch(model, batch, True)
            ls = engine.compute_loss(crit, preds, batch.y, coord_preds, batch.node_coord_y, batch.valid_labels, B)
            assert isinstance(ls, losses.LossDict)
            return engine.total_loss(ls), preds, ls["coordinate"]
        return hip, opt, loss_fn, params

    ops.dropout_epoch_set(0)
    torch.manual_seed(123)
    hip_g, opt_g, loss_g, params_g = build()
    torch.manual_seed(77)
    step = engine.GraphedTrainStep(loss_g, opt_g, warmup=warm)
    e0 = ops.dropout_epoch()
    got = []
    for _ in range(replays):
        out = step()
        got.append((float(out[0]), out[1].clone(), float(out[2])))
    assert ops.dropout_epoch() == e0 + replays
    ops.dropout_epoch_set(e0)
    torch.manual_seed(123)
    hip_e, opt_e, loss_e, params_e = build()
    torch.manual_seed(77)

    def eager():
        out = loss_e()
        opt_e.zero_grad(set_to_none=True)
        out[0].backward()
        opt_e.step()
        return out
    for _ in range(warm):
        eager()
    rng = torch.get_rng_state()
    for k in range(replays):
        torch.set_rng_state(rng)
        ops.dropout_epoch_set(e0 + k + 1)
        out = eager()
        assert float(out[0].detach()) == got[k][0], (k, float(out[0].detach()), got[k][0])
        assert torch.equal(out[1].detach(), got[k][1]), k
        assert float(out[2].detach()) == got[k][2] and got[k][2] > 0, k
    for a, b in zip(params_g, params_e):
        assert torch.equal(a.detach(), b.detach())
    assert len({g[0] for g in got}) == replays                           # fresh dropout masks at every replay
    ops.dropout_epoch_set(0)


def test_sigmoid_model_trains_with_bce_and_expected_landmark_mse_against_fp64(capsys):
    """A model built with output_activation='sigmoid', trained with the builder's 'bce' + 'ExpectedLandmarkMse' (the fused node on
    probabilities): one train step's loss and every parameter gradient against the same step restated in fp64 on the CPU (the oracle
    model in double, torch's binary_cross_entropy and the oracle's ExpectedLandmarkMSE).  Tolerance DERIVED per quantity: FACTOR x
    |the same restatement in fp32 - fp64| + 8 ulp of the quantity's scale (the test_gpu_train parity rule)."""
    FACTOR = 4.0
    B, frame, naux, L = 2, 16, 3, 2
    hip, ref = model_pair(frame, naux, L, seed=5, output_activation="sigmoid")
    for m in list(hip.modules()) + list(ref.modules()):
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    hip.train(); ref.train()
    ref64 = copy.deepcopy(ref).double().train()
    topo, ei, nt, bi = graph_tensors(frame, naux, B)
    frames = synthetic_frames(B, 128, frame, 13)
    _, y, v = G.bce_inputs(frame, naux, B, 102)
    yt, vt = torch.from_numpy(y), torch.from_numpy(v)
    crit = losses.build(_builder_config(B, frame, naux, False, G.BCE_BLOCK))
    got, _ = hip(x=frames.to(DEV), node_coords=None, edge_index=ei.to(DEV), node_type=nt.to(DEV), batch_idx=bi.to(DEV))
    ls = engine.compute_loss(crit, got, yt.to(DEV), None, None, vt.to(DEV), B)
    assert isinstance(ls, losses.LossDict) and list(ls) == ["ExpectedLandmarkMse", "bce"]
    loss = engine.total_loss(ls)
    loss.backward()

    def restated(model, dtype):
        out, _ = model(x=frames.to(dtype), node_coords=None, edge_index=ei, node_type=nt, batch_idx=bi)
        yy, vv = yt.to(dtype), vt.to(dtype)
        el = torch.nn.functional.binary_cross_entropy(out, yy, reduction="none")
        w = torch.where(yy == 1, torch.tensor(9000.0, dtype=dtype), torch.tensor(1.0, dtype=dtype))
        total = (el * w * vv).sum() / vv.sum() + LO.expected_landmark_mse(out, yy, vv, B, frame, naux, loss_weight=10)
        total.backward()
        return float(total.detach()), {k: q.grad.detach().double().reshape(-1) for k, q in model.named_parameters()}
    l32, g32 = restated(ref, torch.float32)
    l64, g64 = restated(ref64, torch.float64)
    ulp = 2.0 ** -23
    report, bad = [], []
    for name, q in hip.named_parameters():
        assert q.grad is not None, name
        hv = q.grad.detach().double().reshape(-1).cpu()
        scale = float(g64[name].abs().max())
        if scale < 1e-9 * max(float(t.abs().max()) for t in g64.values()):
            continue                                                      # analytically zero (a bias in front of a train-mode BatchNorm)
        err = float((hv - g64[name]).abs().max())
        ref_err = float((g32[name] - g64[name]).abs().max())
        tol = FACTOR * ref_err + 8 * ulp * scale
        report.append((name, err, ref_err, tol))
        if err > tol:
            bad.append((name, err, tol))
    err = abs(float(loss.detach()) - l64)
    tol = FACTOR * abs(l32 - l64) + 8 * ulp * abs(l64)
    with capsys.disabled():
        print(f"\n  sigmoid model, bce + ExpectedLandmarkMse: loss {float(loss.detach()):.6f} (fp64 {l64:.6f}, err {err:.2e}, tol {tol:.2e})")
        for name, e, r, t in sorted(report, key=lambda r: -r[1] / r[3])[:6]:
            print(f"    {name:42s} |hip-fp64| {e:.3e}   |fp32-fp64| {r:.3e}   tol {t:.3e}")
    assert err <= tol, (float(loss.detach()), l64, l32)
    assert not bad, bad
    assert len(report) > 10
