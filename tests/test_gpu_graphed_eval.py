"""-m gpu: the device-history mode of the landmark evaluator (csrc/heatmap.hip eg_landmark_record_*) against the reference
fixtures and the host mode, its capture into a HIP graph, and engine.GraphedEvalStep -- the whole evaluation step as one graph --
against eager eval_step on the same batches."""
import copy
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV, model_pair
from echoglad_amd import data, engine, evaluators as EV, losses

pytestmark = pytest.mark.gpu

FIXTURES = ["decode_f16_a3.npz", "decode_f30_a3.npz"]
NAMES = ["lvid_top", "lvid_bot", "lvpw", "ivs"]


def _close(a, b, rel=1e-6):
    """Equal within rel (relative, absolute below 1), NaN and inf in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]), (a, b)
    assert np.all(np.abs(a[fin] - b[fin]) <= rel * np.maximum(1.0, np.abs(b[fin]))), (a, b)


def _same_records(dev_ev, host_ev):
    """Every recorded number and the detail block of a device-mode evaluator against a host-mode one."""
    for table in ("coordinate_errors", "width_MAE", "width_MPE"):
        got, want = getattr(dev_ev, table), getattr(host_ev, table)
        assert list(got) == list(want), table
        for k in want:
            _close(got[k], want[k])
    assert dev_ev.valid_errors == host_ev.valid_errors
    gp, hp = dev_ev.get_predictions(), host_ev.get_predictions()
    for part in ("coordinates", "widths"):
        assert list(gp[part]) == list(hp[part]), part
        for k in hp[part]:
            _close(gp[part][k].numpy(), hp[part][k].numpy())


def _heatmaps(frame, naux, B, seed, no_valid=(), zero_width=False):
    """logits / labels / valid [B * n, 4] on the device with one labelled main-grid pixel per (frame, landmark)."""
    rs = np.random.RandomState(seed)
    levels = losses.level_grids(frame, naux)
    n = levels[-1][0] + frame * frame
    main = levels[-1][0]
    logits = (rs.standard_normal((B, n, 4)) * 2).astype(np.float32)
    y = np.zeros((B, n, 4), np.float32)
    for b in range(B):
        hw = rs.randint(0, frame, (4, 2))
        if zero_width:
            hw[0] = hw[3]                                   # ivs: landmarks 3 and 0 on one pixel -> gt width 0
        for c in range(4):
            y[b, main + hw[c, 0] * frame + hw[c, 1], c] = 1.0
            logits[b, main + hw[c, 0] * frame + min(frame - 1, hw[c, 1] + 1), c] += 8.0
    valid = np.ones_like(y)
    for c in no_valid:
        valid[:, :, c] = 0.0
    if B > 1:
        valid[0, :, 1] = 0.0                                # a frame without a label for one landmark
    px = (0.3 + rs.rand(B)).astype(np.float32)
    py = (0.3 + rs.rand(B)).astype(np.float32)
    t = lambda a: torch.from_numpy(a.reshape(B * n, 4)).to(DEV)
    return t(logits), t(y), t(valid), torch.from_numpy(px), torch.from_numpy(py)


@pytest.mark.parametrize("name", FIXTURES)
def test_device_mode_matches_reference_fixture(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    B, F = int(d["batch"]), int(d["frame"])
    ev = EV.LandmarkExpectedCoordiantesEvaluator(None, B, F, use_coord_graph=False, max_updates=4)
    for _ in range(2):
        ev.update(torch.from_numpy(d["logits"]).to(DEV), torch.from_numpy(d["labels"]).to(DEV),
                  torch.from_numpy(d["pix2mm_x"]), torch.from_numpy(d["pix2mm_y"]), torch.from_numpy(d["valid"]).to(DEV))
    last = ev.get_last()
    for k, want in zip(d["last_keys"], d["last_vals"]):
        assert abs(float(last[str(k)]) - float(want)) <= 2e-5 * max(1.0, abs(float(want))), k
    co = ev.get_predictions()["coordinates"]
    assert np.array_equal(torch.stack([co["gt_" + k] for k in NAMES], 1).numpy().astype(np.int64), d["gt_coords"])
    assert np.allclose(torch.stack([co["pred_" + k] for k in NAMES], 1).numpy(), d["pred_coords"], rtol=1e-6, atol=2e-5)
    for k, want in zip(d["width_keys"], d["width_vals"]):
        assert np.allclose(ev.get_predictions()["widths"][str(k)].numpy(), want, rtol=2e-5, atol=2e-5), k
    mean = ev.compute()
    for k in last:
        assert abs(float(mean[k]) - float(last[k])) <= 1e-6 * max(1.0, abs(float(last[k])))


@pytest.mark.parametrize("B,no_valid,zero_width", [(1, (), False), (3, (), False), (8, (), False), (3, (2,), False), (2, (), True)])
def test_device_mode_matches_host_mode(B, no_valid, zero_width):
    """224/7 heat maps: every recorded number and the detail block within 1e-6 relative; a landmark without a valid row (flag false,
    divisor 1) and a zero gt width (inf / NaN in the same places) included.  Three updates, compute() and the sums as well."""
    host = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, False)
    dev = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, False, max_updates=8)
    for it in range(3):
        args = _heatmaps(224, 7, B, 100 * B + it, no_valid, zero_width)
        host.update(*args[:2], args[3], args[4], args[2])
        dev.update(*args[:2], args[3], args[4], args[2])
    _same_records(dev, host)
    if no_valid:
        assert dev.valid_errors[NAMES[no_valid[0]]] == [False] * 3
    if zero_width:
        assert not np.isfinite(dev.width_MPE["ivs"]).any()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, v in host.compute().items():
            _close(dev.compute()[k], v)
        _close(dev.get_sum_of_width_MAE(), host.get_sum_of_width_MAE())
        _close(dev.get_sum_of_width_MPE(), host.get_sum_of_width_MPE())


@pytest.mark.parametrize("B", [1, 4])
def test_coordinate_branch_matches_host_mode(B):
    rs = np.random.RandomState(B)
    host = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, True)
    dev = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, True, max_updates=3)
    for _ in range(2):
        cp = torch.from_numpy((rs.rand(B * 4, 2) * 223).astype(np.float32)).to(DEV)
        cy = torch.from_numpy(rs.randint(0, 224, (B * 4, 2)).astype(np.float32)).to(DEV)
        px, py = (torch.from_numpy((0.3 + rs.rand(B)).astype(np.float32)) for _ in range(2))
        host.update(cp, cy, px, py, None)
        dev.update(cp, cy, px.to(DEV), py.to(DEV), None)
    _same_records(dev, host)


def test_device_updates_do_not_synchronise():
    B = 2
    ev = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, False, max_updates=8)
    evc = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 224, True, max_updates=8)
    lg, y, v, px, py = _heatmaps(224, 7, B, 5)
    px, py = px.to(DEV), py.to(DEV)
    cp = torch.rand(B * 4, 2, device=DEV) * 200
    ev.update(lg, y, px, py, v)                       # (first launch on the stream: the completion ticket is allocated here)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(5):
            ev.update(lg, y, px, py, v)
            evc.update(cp, cp, px, py, None)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ev.width_MAE["ivs"]) == 6 and len(evc.width_MAE["ivs"]) == 5


@pytest.mark.parametrize("coord", [False, True])
def test_captured_update_equals_eager_updates(coord):
    """An update captured with torch.cuda.graph and replayed over K input sets copied into static tensors leaves K records (and detail
    blocks) bit-equal to K eager device-mode updates."""
    B, K = 3, 4
    sets = []
    for k in range(K):
        lg, y, v, px, py = _heatmaps(64, 6, B, 40 + k)
        if coord:
            lg, y = torch.rand(B * 4, 2, device=DEV) * 63, torch.randint(0, 64, (B * 4, 2), device=DEV).float()
        sets.append((lg, y, px.to(DEV), py.to(DEV), v))
    eager = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 64, coord, max_updates=K)
    for s in sets:
        eager.update(*s)
    graphed = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 64, coord, max_updates=K)
    static = [t.clone() for t in sets[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graphed.update(*static)                        # warm-up on the capture stream (ticket word)
    torch.cuda.synchronize()
    graphed.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        graphed.update(*static)
    assert graphed._count() == 0                        # (the capture executes nothing)
    for s in sets:
        for dst, src in zip(static, s):
            dst.copy_(src)
        g.replay()
    torch.cuda.synchronize()
    assert graphed._count() == K
    assert torch.equal(graphed._state[1], eager._state[1]) and torch.equal(graphed._state[2], eager._state[2])


def test_overflow_reset_and_argument_checks():
    B = 2
    ev = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 64, False, max_updates=2)
    lg, y, v, px, py = _heatmaps(64, 6, B, 9)
    for _ in range(3):
        ev.update(lg, y, px, py, v)
    for read in (ev.compute, ev.get_last, ev.get_predictions, ev.get_sum_of_width_MAE, lambda: ev.width_MAE):
        with pytest.raises(RuntimeError, match="max_updates"):
            read()
    ev.reset()
    assert ev.get_predictions() == {} and ev.width_MAE == {"lvid": [], "ivs": [], "lvpw": []}
    ev.update(lg, y, px, py, v)
    assert len(ev.coordinate_errors["ivs"]) == 1
    with pytest.raises(ValueError, match="batch size"):
        ev.update(lg, y, px[:1], py[:1], v)                                   # one pix2mm value for two frames
    ev3 = EV.LandmarkExpectedCoordiantesEvaluator(None, 3, 64, False, max_updates=2)
    with pytest.raises(ValueError, match="batch size"):
        ev3.update(lg, y, torch.ones(3), torch.ones(3), v)                  # two frames of logits for a batch of three
    evc = EV.LandmarkExpectedCoordiantesEvaluator(None, B, 64, True, max_updates=2)
    with pytest.raises(ValueError, match="batch size"):
        evc.update(torch.zeros(3 * 4, 2, device=DEV), torch.zeros(3 * 4, 2, device=DEV), px, py, None)
    # CPU pix2mm under a capture: refused before anything is launched
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ev.update(lg, y, px.to(DEV), py.to(DEV), v)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="device tensors"):
        with torch.cuda.graph(g, stream=stream):
            ev.update(lg, y, px, py, v)
    assert len(ev.coordinate_errors["ivs"]) == 2


# ---- engine.GraphedEvalStep ---------------------------------------------------------------------------------------------------
def _eval_setup(frame, naux, layers, coord, B, n_batches, seed):
    hip, _ = model_pair(frame, naux, layers, coord=coord, seed=seed)
    torch.manual_seed(seed)
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV).eval()
    np.random.seed(seed)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=coord)
    host = [data.collate([ds[B * i + j] for j in range(B)], ds.topology) for i in range(n_batches)]
    cfg = {"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
           "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": frame, "num_aux_graphs": naux, "batch_size": B,
           "use_coordinate_graph": coord, "use_main_graph_only": False, "num_output_channels": 4}
    crit = losses.build(cfg)
    return {"embedder": emb, "landmark": hip}, host, crit


def _evaluators(frame, B, coord, n):
    return EV.build({"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": B, "frame_size": frame,
                     "use_coordinate_graph": coord}, max_updates=n)


def _eager_eval(model, host, crit, B, coord, frame):
    evs = _evaluators(frame, B, coord, len(host))
    preds, totals = [], []
    for hb in host:
        b = data.to_device(copy.copy(hb), DEV)
        p, _, ls = engine.eval_step(model, b, crit, B, coord, evs)
        preds.append(p.clone())
        totals.append(float(engine.total_loss(ls)))
    return preds, totals, evs


def _graphed_eval(step, static, host):
    preds = []
    for hb in host:
        data.copy_batch_(static, hb)
        p, _, _ = step()
        preds.append(p.clone())
    return preds


def _assert_same_evaluation(pg, evs_g, loss_avg, pe, totals, evs_e):
    for a, b in zip(pg, pe):
        assert torch.equal(a, b)
    ba_g, ba_e = evs_g["balancedaccuracy"], evs_e["balancedaccuracy"]
    assert np.array_equal(ba_g.counts(), ba_e.counts())
    lm_g, lm_e = evs_g["landmarkcoorderror"], evs_e["landmarkcoorderror"]
    n = lm_e._count()
    assert lm_g._count() == n == len(pe)
    assert torch.equal(lm_g._state[1][:n], lm_e._state[1][:n]) and torch.equal(lm_g._state[2][:n], lm_e._state[2][:n])
    want = float(np.mean(np.asarray(totals, np.float64)))
    assert abs(loss_avg - want) <= 1e-6 * abs(want), (loss_avg, want)


@pytest.mark.parametrize("B,coord", [(1, False), (8, False), (1, True)])
def test_graphed_eval_step_equals_eager_eval_step(B, coord):
    """configs[1] shape (224/7, 3 layers), the default config's criteria and both evaluation standards: N calls over N different
    batches give the eager step's logits bit for bit, the same confusion counts and landmark records, and the mean loss -- from
    ONE capture.  The caller's node_coords are not written."""
    frame, naux, N = 224, 7, 3
    model, host, crit = _eval_setup(frame, naux, 3, coord, B, N, seed=21)
    pe, totals, evs_e = _eager_eval(model, host, crit, B, coord, frame)
    static = data.to_device(copy.copy(host[0]), DEV)
    coords0 = static.node_coords.clone() if coord else None
    evs_g = _evaluators(frame, B, coord, N)
    step = engine.GraphedEvalStep(model, static, crit, B, use_coordinate_graph=coord, evaluators=evs_g, warmup=2)
    assert step.loss_avg() == 0.0 and evs_g["landmarkcoorderror"]._count() == 0 and evs_g["balancedaccuracy"].counts() is None
    pg = _graphed_eval(step, static, host)
    assert step.captures == 1
    _assert_same_evaluation(pg, evs_g, step.loss_avg(), pe, totals, evs_e)
    if coord:
        assert torch.equal(static.node_coords, host[-1].node_coords.to(DEV))        # what copy_batch_ wrote, nothing else
        data.copy_batch_(static, host[0])
        step()
        assert torch.equal(static.node_coords, coords0)


def test_graphed_eval_step_follows_parameter_changes():
    """Evaluate; train eagerly; evaluate; load other weights (in place, eval mode); evaluate; train with a GraphedTrainStep;
    evaluate.  Every evaluation equals eager eval_step under the parameters of that moment."""
    frame, naux, B, N = 32, 4, 2, 2
    model, host, crit = _eval_setup(frame, naux, 2, False, B, N, seed=5)
    lm, emb = model["landmark"], model["embedder"]
    for q in emb.parameters():
        q.requires_grad_(False)
    static = data.to_device(copy.copy(host[0]), DEV)
    evs_g = _evaluators(frame, B, False, 4 * N)
    step = engine.GraphedEvalStep(model, static, crit, B, evaluators=evs_g)

    def evaluate():
        step.reset_meter()
        for ev in evs_g.values():
            ev.reset()
        pg = _graphed_eval(step, static, host)
        pe, totals, evs_e = _eager_eval(model, host, crit, B, False, frame)
        _assert_same_evaluation(pg, evs_g, step.loss_avg(), pe, totals, evs_e)
        return pg[0]

    first = evaluate()
    opt = torch.optim.Adam(lm.parameters(), lr=1e-2)
    lm.train()
    train_batch = data.to_device(copy.copy(host[1]), DEV)
    for _ in range(3):
        engine.train_step(model, train_batch, crit, opt, B)
    lm.eval()
    second = evaluate()
    assert not torch.equal(first, second) and step.captures == 2
    other, _ = model_pair(frame, naux, 2, seed=99)
    lm.load_state_dict(other.state_dict())
    third = evaluate()
    assert not torch.equal(second, third) and step.captures == 3
    # a captured training step: its replays update the parameters without running host code
    lm.train()
    gopt = torch.optim.Adam(lm.parameters(), lr=1e-2, capturable=True)

    def loss_fn():
        p, cp = engine.forward_batch(model, train_batch, False)
        return engine.total_loss(engine.compute_loss(crit, p, train_batch.y, cp, None, train_batch.valid_labels, B))
    from echoglad_amd import ops
    e0 = ops.dropout_epoch()
    try:
        tstep = engine.GraphedTrainStep(loss_fn, gopt, warmup=1)
        for _ in range(3):
            tstep()
    finally:
        ops.dropout_epoch_set(e0)                # (every replay bumps the dropout epoch: later tests expect it where it was)
    lm.eval()
    fourth = evaluate()
    assert not torch.equal(third, fourth) and step.captures == 4
    assert torch.equal(evaluate(), fourth) and step.captures == 4       # nothing moved: no capture


def test_graphed_eval_step_refuses_what_it_cannot_capture():
    frame, naux, B = 32, 4, 1
    model, host, crit = _eval_setup(frame, naux, 2, False, B, 1, seed=2)
    static = data.to_device(copy.copy(host[0]), DEV)
    host_lm = {"landmarkcoorderror": EV.LandmarkExpectedCoordiantesEvaluator(None, B, frame, False)}
    with pytest.raises(ValueError, match="max_updates"):
        engine.GraphedEvalStep(model, static, crit, B, evaluators=host_lm)
    model["landmark"].train()
    with pytest.raises(ValueError, match="training mode"):
        engine.GraphedEvalStep(model, static, crit, B, evaluators=_evaluators(frame, B, False, 2))
    model["landmark"].eval()
    step = engine.GraphedEvalStep(model, static, crit, B, evaluators=_evaluators(frame, B, False, 2))
    model["landmark"].train()
    with pytest.raises(ValueError, match="training mode"):
        step()
