"""-m gpu: examples.UNetNoGNN, the reference's no-GNN baseline -- its eval forward (ONE launch behind the decoder) bit for bit against
the composed route and against tests/nognn_reference.py in float64; one training step against the float64 restatement; the
reproducible step; and engine.GraphedEvalStep on it."""
import copy

import numpy as np
import pytest
import torch

import eval_reference as E
import nognn_reference as N
import train_reference as T
from coord_reference import Report
from echoglad_amd import data, engine, evaluators as EV, losses, ops
from echoglad_amd.examples import UNetNoGNN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
B = 2
# (frame, encoder dims, flags)
SHAPES = [(16, [8, 16, 32], {}), (32, [8, 16, 32, 64], {}), (32, [8, 16, 32, 64], {"use_coordinate_graph": True}),
          (32, [8, 16, 32, 64], {"use_connection_nodes": True}), (16, [8, 16, 32], {"use_main_graph_only": True})]


def _model(frame, dims, flags=None, seed=31, **kw):
    torch.manual_seed(seed)
    naux = len(dims)
    args = dict(encoder_embedding_widths=[2 ** g for g in range(naux, 0, -1)], encoder_embedding_dims=dims, frame_size=frame, num_aux_graphs=naux,
                node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit",
                gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    args.update(flags or {})
    args.update(kw)
    m = UNetNoGNN(**args)
    rs = np.random.RandomState(seed)
    with torch.no_grad():                                   # running statistics and affine parameters as after some training
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                n = mod.num_features
                mod.running_mean.copy_(torch.from_numpy(0.2 * rs.standard_normal(n)))
                mod.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, n)))
                mod.weight.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, n)))
                mod.bias.copy_(torch.from_numpy(0.1 * rs.standard_normal(n)))
    return m


def _frames(frame, seed=12):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, frame, frame, generator=g).to(DEV), (torch.rand(B * 4, 2, generator=g) * (frame - 1)).to(DEV)


def _count(monkeypatch, names=("conv1x1_relu_heads", "conv1x1_relu_pack_levels", "classifier_fwd")):
    """A counter on the ops wrappers (these launches go through no graph handle: there is no launch counter to read)."""
    calls = {n: 0 for n in names}
    for n in names:
        inner = getattr(ops, n)

        def counted(*a, _n=n, _inner=inner, **k):
            calls[_n] += 1
            return _inner(*a, **k)
        monkeypatch.setattr(ops, n, counted)
    return calls


def _check_against_fp64(model, x, got, sigmoid, title, capsys):
    """The kernels' inputs -- the decoder's maps, the 1 x 1 weights, the packed heads -- through tests/nognn_reference.py."""
    with torch.no_grad():
        feats = [f.float().cpu() for f in model.decoder_maps(x)]
    lin = list(model.linears)
    if model.use_main_graph_only:
        feats, lin = feats[-1:], lin[-1:]
    ws, bs = [m.weight.detach().cpu() for m in lin], [m.bias.detach().cpu() for m in lin]
    packed = {k: v.detach().cpu() for k, v in model._packed_classifier().items()}
    fold64 = E.pack_heads(copy.deepcopy(model.node_classifiers).cpu())
    for k in packed:                                        # (the folding itself: float32 against the float64 folding, rounded once)
        assert torch.allclose(packed[k], fold64[k], rtol=1e-5, atol=1e-6), k
    (r64, s64), (r32, _) = (N.tail_heads(feats, ws, bs, B, packed, sigmoid, dtype=dt) for dt in (F64, F32))
    rep = Report()
    rep.check("sigmoid" if sigmoid else "logits", got, r64, r32, s64)
    with capsys.disabled():
        print(rep.table(title))
    assert not rep.failed(), rep.failed()


@pytest.mark.parametrize("frame,dims,flags", SHAPES, ids=lambda v: str(v))
def test_eval_forward_is_one_launch_and_equals_the_composed_route(frame, dims, flags, monkeypatch, capsys):
    model = _model(frame, dims, flags).to(DEV).eval()
    x, coords = _frames(frame)
    nc = coords if flags.get("use_coordinate_graph") else None
    n_valid = model._row_ranges()[2]
    calls = _count(monkeypatch)
    with torch.no_grad():
        got, none = model(x=x, node_coords=nc, edge_index=None)
        assert calls == {"conv1x1_relu_heads": 1, "conv1x1_relu_pack_levels": 0, "classifier_fwd": 0}
        assert none is None and got.shape == (B * n_valid, 4)
        want = model.forward_heads(model.create_node_pixels(x, B, None if nc is None else nc.reshape(B, 4, 2)), B)
        assert calls == {"conv1x1_relu_heads": 1, "conv1x1_relu_pack_levels": 1, "classifier_fwd": 1}
        assert torch.equal(got, want)
        model.fuse_tail = False
        unfused, _ = model(x=x, node_coords=nc, edge_index=None)
        assert calls == {"conv1x1_relu_heads": 1, "conv1x1_relu_pack_levels": 2, "classifier_fwd": 2}
        assert torch.equal(unfused, got)
    _check_against_fp64(model, x, got, False, f"UNetNoGNN eval {frame} {flags}", capsys)


def test_eval_forward_with_the_sigmoid(monkeypatch, capsys):
    model = _model(16, [8, 16, 32], output_activation="sigmoid").to(DEV).eval()
    x, _ = _frames(16)
    calls = _count(monkeypatch)
    with torch.no_grad():
        got, _ = model(x=x)
        want = model.forward_heads(model.create_node_pixels(x, B), B)
    assert calls["conv1x1_relu_heads"] == 1 and torch.equal(got, want)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    _check_against_fp64(model, x, got, True, "UNetNoGNN eval 16, sigmoid", capsys)


# ---- training ------------------------------------------------------------------------------------------------------------------
TRAIN_SEED = 2589        # found on the CPU: the smallest |ReLU input| of the float64 restatement is 3.9e-5 against a margin of 2.2e-5
TRAIN_SIDES, TRAIN_CHANS = (2, 4, 8, 16), (32, 16, 8, 4)


def _train_inputs():
    maps = N.level_inputs(TRAIN_SIDES, TRAIN_CHANS, B, TRAIN_SEED)[0]
    dlogits = torch.randn(B * 340, 4, generator=torch.Generator().manual_seed(TRAIN_SEED))
    return maps, dlogits


@pytest.fixture(scope="module")
def train_refs():
    model = _model(16, [8, 16, 32]).train()
    maps, dlogits = _train_inputs()
    r64, r32 = (N.train_restatement(model, None, B, dlogits, dt, maps=maps) for dt in (F64, F32))
    return model, r64, r32


def test_train_inputs_keep_every_relu_decision_a_margin_from_its_kink(train_refs):
    """train_reference.py's input condition on the float64 restatement: every tensor a ReLU is applied to (the tail's 1 x 1
    convolutions, the heads' BatchNorm outputs) is at least max(MARGIN, 2 FACTOR e32) away from 0 -- nothing is left out below."""
    _, r64, r32 = train_refs
    smallest, margin, active, _ = T.condition(r64["pre"], r32["pre"])
    assert len(r64["pre"]) == 4 + 8 and sum(a.numel() for a in r64["pre"]) == B * 340 * (128 + 4 * 48)
    assert smallest >= margin, (smallest, margin)
    assert all(0.25 <= a <= 0.75 for a in active), active


@pytest.mark.parametrize("hip", [False, True], ids=["torch tail backward", "hip tail backward"])
def test_training_step_behind_the_decoder_against_float64(train_refs, hip, monkeypatch, capsys):
    """One training step of the model's own forward() on given decoder maps (the same numbers on every host; the decoder in front
    of them has its own float64 tests): logits and the gradients of linears.* and node_classifiers.* under Report's rule, scale =
    the last reduction of each on absolute values (nognn_reference.train_restatement); gnn_layers get no gradient.

    Why behind the decoder: started from the frames, the float32 restatement is 1.3e-5 .. 2.3e-5 off at the heads' BatchNorm outputs
    (twelve train-mode BatchNorms in front of them), train_reference.py's margin 2 FACTOR e32 becomes 1e-4 .. 4.6e-4, and of the
    239,104 ReLU inputs about a dozen lie that close to 0 for any seed (300 seeds tried: smallest input 1.5e-5 .. 2.9e-5 at best).
    From given maps e32 is 2e-6 .. 3e-6 and a seed that meets the condition with room exists; everything compared here lies
    behind the maps.  test_training_step_from_frames runs the step with the decoder in it."""
    cpu_model, r64, r32 = train_refs
    model = copy.deepcopy(cpu_model).to(DEV).train()
    if hip:
        model.enable_hip_frontend(True, train=True, tail=True)
    maps, dlogits = _train_inputs()
    maps_dev = [f.to(DEV) for f in maps]
    monkeypatch.setattr(model, "decoder_maps", lambda frames: maps_dev)
    calls = _count(monkeypatch, ("conv1x1_relu_heads",))
    logits, none = model(x=torch.zeros(B, 4, 16, 16, device=DEV), edge_index=None)
    assert none is None and calls["conv1x1_relu_heads"] == 0 and logits.shape == (B * 340, 4)
    (logits * dlogits.to(DEV)).sum().backward()
    rep = Report()
    rep.check("logits", logits, r64["logits"], r32["logits"], r64["logits_scale"])
    named = dict(model.named_parameters())
    assert sorted(r64["grads"]) == sorted(n for n in named if n.startswith(("linears.", "node_classifiers.")))
    for name in r64["grads"]:
        assert named[name].grad is not None, name
        rep.check(name, named[name].grad, r64["grads"][name], r32["grads"][name], r64["scales"][name])
    with capsys.disabled():
        print(rep.table(f"UNetNoGNN training step behind the decoder, hip={hip}"))
    assert not rep.failed(), rep.failed()
    gnn = [n for n in named if n.startswith("gnn_layers.")]
    assert gnn and all(named[n].grad is None for n in gnn)
    assert [n for n in r64["unused"] if n.startswith("gnn_layers.")] == sorted(gnn)


def test_training_step_from_frames():
    """The whole step with the decoder in it: every parameter but gnn_layers.* receives a finite gradient."""
    model = _model(16, [8, 16, 32]).to(DEV).train()
    x, _ = _frames(16, seed=14)
    logits, none = model(x=x, edge_index=None)
    assert none is None and logits.shape == (B * 340, 4) and logits.requires_grad
    (logits ** 2).mean().backward()
    for name, q in model.named_parameters():
        if name.startswith("gnn_layers."):
            assert q.grad is None, name
        else:
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name


def test_reproducible_training_step():
    """enable_hip_frontend(True, train=True, tail=True), dropout 0.5: two runs of the same step agree bit for bit in the logits and
    in every gradient."""
    x, _ = _frames(16, seed=15)
    epoch0 = ops.dropout_epoch()
    try:
        runs = []
        for _ in range(2):
            ops.dropout_epoch_set(5)
            model = _model(16, [8, 16, 32], classifier_dropout_p=0.5, gnn_dropout_p=0.5).to(DEV).train().enable_hip_frontend(True, train=True, tail=True)
            torch.manual_seed(77)
            logits, _ = model(x=x, edge_index=None)
            (logits ** 2).mean().backward()
            named = [(n, q.grad) for n, q in model.named_parameters() if q.grad is not None]
            assert len(named) == sum(1 for n, _ in model.named_parameters() if not n.startswith("gnn_layers."))
            runs.append([("logits", logits.detach())] + named)
        for (na, a), (nb, b) in zip(*runs):
            assert na == nb and torch.equal(a, b), na
    finally:
        ops.dropout_epoch_set(epoch0)


# ---- engine.GraphedEvalStep ---------------------------------------------------------------------------------------------------
def test_graphed_eval_step_equals_eager_eval_steps(monkeypatch):
    frame, naux, n_batches = 16, 3, 3
    landmark = _model(frame, [8, 16, 32]).to(DEV).eval()
    torch.manual_seed(5)
    model = {"embedder": torch.nn.Conv2d(1, 4, kernel_size=1).to(DEV).eval(), "landmark": landmark}
    np.random.seed(5)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame)
    host = [data.collate([ds[B * i + j] for j in range(B)], ds.topology) for i in range(n_batches)]
    crit = losses.build({"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
                         "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": frame, "num_aux_graphs": naux, "batch_size": B,
                         "use_coordinate_graph": False, "use_main_graph_only": False, "num_output_channels": 4})
    evs = lambda: EV.build({"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": B, "frame_size": frame,
                            "use_coordinate_graph": False}, max_updates=n_batches)
    calls = _count(monkeypatch, ("conv1x1_relu_heads",))
    with torch.no_grad():
        evs_e, preds_e, totals = evs(), [], []
        for hb in host:
            p, _, ls = engine.eval_step(model, data.to_device(copy.copy(hb), DEV), crit, B, False, evs_e)
            preds_e.append(p.clone())
            totals.append(float(engine.total_loss(ls)))
        assert calls["conv1x1_relu_heads"] == n_batches
        static = data.to_device(copy.copy(host[0]), DEV)
        evs_g = evs()
        step = engine.GraphedEvalStep(model, static, crit, B, evaluators=evs_g, warmup=1)
        launched = calls["conv1x1_relu_heads"]
        for k, hb in enumerate(host):
            data.copy_batch_(static, hb)
            p, _, _ = step()
            assert torch.equal(p, preds_e[k]), k
    assert step.captures == 1 and calls["conv1x1_relu_heads"] == launched == n_batches + 2       # warm-up and capture; replays run no host code
    assert np.array_equal(evs_g["balancedaccuracy"].counts(), evs_e["balancedaccuracy"].counts())
    lm_g, lm_e = evs_g["landmarkcoorderror"], evs_e["landmarkcoorderror"]
    assert lm_g._count() == lm_e._count() == n_batches
    assert torch.equal(lm_g._state[1][:n_batches], lm_e._state[1][:n_batches]) and torch.equal(lm_g._state[2][:n_batches], lm_e._state[2][:n_batches])
    want = float(np.mean(np.asarray(totals, np.float64)))
    assert abs(step.loss_avg() - want) <= 1e-6 * abs(want), (step.loss_avg(), want)
