"""-m gpu: frame preparation on the device (csrc/frame_prep.hip, eg_frame_prep; ops.frame_prep, data.device_frames_) against the fp64
restatement of its rule (tests/frame_prep_reference.py), alone, captured into a graph, and as the first node of
engine.GraphedTrainStep / GraphedEvalStep against the same steps fed with batches prepared beforehand.

Tolerance of the pixel comparisons: per case d = max |torch CPU float32 composition - fp64| on the same inputs (the code under test is
not involved); the bound is 4 d + 2^-20 max |source value| -- two independent float32 routes, each carrying the rounding of its own
source coordinate, which dominates; the constant covers cases where d is 0.  Every output is pre-filled with NaN, so an element the
kernel skipped shows."""
import copy
import functools

import numpy as np
import pytest
import torch

import frame_prep_reference as R
import make_frame_prep_golden as G
from gpu_util import DEV, model_pair
from echoglad_amd import data, engine, evaluators as EV, losses, ops

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _matrices(crop, W, params=G.PARAMS):
    pairs = [data.affine_matrix(tx=tx, ty=ty, sx=crop / W, sy=crop / W, rotation_theta=rot, shear_theta=sh) for tx, ty, rot, sh in params]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _prep(src, F, inv=None, W=0, flip=None, gray=False):
    """ops.frame_prep into a NaN-filled tensor -> out on the host."""
    B, C = src.shape[:2]
    out = torch.full((B, 1 if gray else C, F, F), NAN, device=DEV)
    got = ops.frame_prep(_dev(src), out, matrix_inv=_dev(inv), warp_size=W, flip=_dev(flip, torch.uint8), gray=gray)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu()


def _bound(src, F, inv, W, flip, gray, want):
    """4 d + 2^-20 max |source value|, d from torch's CPU float32 composition against the fp64 restatement `want`."""
    d = float((R.torch_composition(src, F, inv, W, flip, gray, dtype=torch.float32).double() - torch.from_numpy(want)).abs().max())
    vmax = float(np.abs(R.source_values(src)).max())
    return d, 4.0 * d + 2.0 ** -20 * vmax


def _compare(tag, src, F, inv=None, W=0, flip=None, gray=False):
    want = R.frame_prep_fp64(src, F, inv, W, flip, gray)
    d, bound = _bound(src, F, inv, W, flip, gray, want)
    got = _prep(src, F, inv, W, flip, gray)
    assert tuple(got.shape) == want.shape and not bool(got.isnan().any())
    err = float((got.double() - torch.from_numpy(want)).abs().max())
    print(f"{tag}: d = {d:.3g}, bound = {bound:.3g}, achieved = {err:.3g}")
    assert err <= bound, (tag, err, bound)
    return got


@functools.lru_cache(maxsize=None)
def _case(name, channels, dtype):
    sh, sw, W, F, crop, _ = G.CASES[name]
    src, _ = G.case_inputs(name, channels, dtype)
    _, inv = _matrices(crop, W)
    return src, inv, W, F


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("mode", ["c1", "c3", "c3gray"])
@pytest.mark.parametrize("name", list(G.CASES))
def test_warp_and_resize(name, mode, dtype):
    """B = 3 with three different matrices and flip = [0, 1, 0]."""
    src, inv, W, F = _case(name, 1 if mode == "c1" else 3, dtype)
    _compare(f"{name} {mode} {dtype}", src, F, inv, W, G.FLIP, mode == "c3gray")


def test_full_size_warp_and_resize():
    """640 -> 608 -> 224, C = 3, B = 2: the reference's own sizes."""
    rng = np.random.default_rng(311)
    src = rng.integers(0, 256, size=(2, 3, 640, 640)).astype(np.uint8)
    _, inv = _matrices(640, 608, [(0.02, -0.03, 0.15, 0.05), (0.0, 0.0, 0.0, 0.0)])
    _compare("640 -> 608 -> 224 c3 uint8", src, 224, inv, 608, [1, 0], False)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("S,F", [(28, 16), (12, 16)])
def test_resize_only(S, F, channels, dtype):
    rng = np.random.default_rng(320 + S)
    src = rng.integers(0, 256, size=(3, channels, S, S)).astype(np.uint8)
    if dtype == "float32":
        src = (rng.standard_normal(src.shape) + src / 255.0).astype(np.float32)
    _compare(f"{S} -> {F} c{channels} {dtype}", src, F, flip=G.FLIP)
    if channels == 3:
        _compare(f"{S} -> {F} gray {dtype}", src, F, flip=G.FLIP, gray=True)


def test_identity_resize_is_the_division():
    rng = np.random.default_rng(330)
    src = rng.integers(0, 256, size=(2, 3, 16, 16)).astype(np.uint8)
    src[0, 0].reshape(-1)[:256] = np.arange(256)                       # every byte value
    assert torch.equal(_prep(src, 16), torch.from_numpy(src).float() / 255)
    f = rng.standard_normal((2, 1, 16, 16)).astype(np.float32)
    assert torch.equal(_prep(f, 16), torch.from_numpy(f))
    # a rectangular source, no warp stage: each axis has its own scale
    r = rng.integers(0, 256, size=(2, 1, 24, 40)).astype(np.uint8)
    _compare("24x40 -> 30 c1 uint8", r, 30)


def test_flip_mirrors_and_runs_are_bit_equal():
    src, inv, W, F = _case("s40_w38_f16", 3, "uint8")
    for gray in (False, True):
        plain = _prep(src, F, inv, W, None, gray)
        assert torch.equal(_prep(src, F, inv, W, [0, 0, 0], gray), plain)
        flipped = _prep(src, F, inv, W, [1, 1, 1], gray)
        assert torch.equal(flipped, plain.flip(-1))
        mixed = _prep(src, F, inv, W, [0, 1, 0], gray)
        assert torch.equal(mixed[1], plain[1].flip(-1)) and torch.equal(mixed[0], plain[0]) and torch.equal(mixed[2], plain[2])
        assert torch.equal(_prep(src, F, inv, W, None, gray), plain)
    r = np.random.default_rng(331).integers(0, 256, size=(2, 1, 28, 28)).astype(np.uint8)
    assert torch.equal(_prep(r, 16, flip=[1, 0])[0], _prep(r, 16)[0].flip(-1))


def _landmark_batch(rng, B, crop, W):
    params = np.stack([rng.uniform(-0.1, 0.1, B), rng.uniform(-0.1, 0.1, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-0.2, 0.2, B)], 1)
    fwd, inv = _matrices(crop, W, [tuple(p) for p in params])
    coords = rng.uniform(0.0, crop, size=(B, 4, 2)).astype(np.float32)
    flip = (rng.random(B) < 0.5).astype(np.uint8)
    return coords, fwd, inv, flip


@pytest.mark.parametrize("S,W,F,B,launches", [(40, 38, 16, 512, 1), (640, 608, 224, 64, 4)])
def test_landmark_sweep(S, W, F, B, launches):
    """Random landmarks through random matrices, flipped rows among them, must equal data.prep_coords exactly wherever fp64 q is at
    least 2^-10 from an integer on both axes (closer, two correct evaluations may truncate differently)."""
    rng = np.random.default_rng(340 + S)
    src = torch.zeros(B, 1, S, S, dtype=torch.uint8, device=DEV)
    out = torch.empty(B, 1, F, F, device=DEV)
    drawn = kept = 0
    for _ in range(launches):
        coords, fwd, inv, flip = _landmark_batch(rng, B, S, W)
        lc = torch.full((B, 4, 2), -12345, dtype=torch.int32, device=DEV)
        cy = torch.full((4 * B, 2), NAN, device=DEV)
        ops.frame_prep(src, out, matrix_inv=_dev(inv), warp_size=W, flip=_dev(flip), coords=_dev(coords), matrix=_dev(fwd),
                       crop_size=S, out_label_coords=lc, out_coord_y=cy)
        torch.cuda.synchronize()
        q = R.landmark_q_fp64(coords, F, fwd, S, W)
        keep = (np.abs(q - np.round(q)) >= 2.0 ** -10).all(axis=-1)
        drawn += keep.size
        kept += int(keep.sum())
        want = data.prep_coords(coords, F, fwd, S, W, flip)
        got = lc.cpu().numpy()
        assert np.array_equal(got[keep], want[keep])
        assert torch.equal(cy.cpu(), lc.cpu().float().view(-1, 2))
        assert flip.any() and not flip.all()
    print(f"{S} -> {W} -> {F}: {drawn} landmarks drawn, {drawn - kept} discarded")
    assert drawn - kept <= drawn // 100


def test_landmarks_without_a_warp_stage():
    F = 16
    coords = np.array([[[-1, -1], [F - 1, 0], [3, F - 1], [0, 7]], [[-1, -1], [F - 1, 0], [3, F - 1], [0, 7]]], dtype=np.float32)
    flip = np.array([0, 1], dtype=np.uint8)
    src = torch.zeros(2, 1, 28, 28, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 1, F, F), NAN, device=DEV)
    lc = torch.full((2, 4, 2), -12345, dtype=torch.int32, device=DEV)
    cy = torch.full((8, 2), NAN, device=DEV)
    ops.frame_prep(src, out, flip=_dev(flip), coords=_dev(coords), out_label_coords=lc, out_coord_y=cy)
    torch.cuda.synchronize()
    assert lc.cpu().tolist() == [[[-1, -1], [15, 0], [3, 15], [0, 7]], [[-1, 16], [15, 15], [3, 0], [0, 8]]]
    assert np.array_equal(lc.cpu().numpy(), data.prep_coords(coords, F, flip=flip))
    assert torch.equal(cy.cpu(), lc.cpu().float().view(-1, 2)) and float(out.abs().max()) == 0.0
    only = torch.full((2, 4, 2), -12345, dtype=torch.int32, device=DEV)             # coord_y is optional
    ops.frame_prep(src, out, flip=_dev(flip), coords=_dev(coords), out_label_coords=only)
    assert torch.equal(only, lc)
    with pytest.raises(RuntimeError, match="needs out_label_coords"):
        ops.frame_prep(src, out, coords=_dev(coords))
    with pytest.raises(RuntimeError, match="1 or 3 channels"):
        ops.frame_prep(torch.zeros(2, 2, 28, 28, dtype=torch.uint8, device=DEV), out)
    with pytest.raises(RuntimeError, match="gray needs"):
        ops.frame_prep(src, out, gray=True)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_prep(torch.zeros(2, 1, 28, 56, dtype=torch.uint8, device=DEV)[..., ::2], out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frame_prep(src, torch.empty(2, 1, F, F + 1, device=DEV))


def test_a_captured_launch_replays_on_new_batches():
    sh, sw, W, F, crop, _ = G.CASES["s40_w38_f16"]
    rng = np.random.default_rng(350)
    batches = []
    for k in range(4):
        coords, fwd, inv, flip = _landmark_batch(rng, 3, crop, W)
        batches.append((rng.integers(0, 256, size=(3, 3, sh, sw)).astype(np.uint8), coords, fwd, inv, flip))
    static = [_dev(a) for a in batches[0]]
    out = torch.full((3, 1, F, F), NAN, device=DEV)
    lc = torch.zeros(3, 4, 2, dtype=torch.int32, device=DEV)
    cy = torch.zeros(12, 2, device=DEV)

    def launch(t, o, l, c):
        ops.frame_prep(t[0], o, matrix_inv=t[3], warp_size=W, flip=t[4], gray=True, coords=t[1], matrix=t[2], crop_size=crop,
                       out_label_coords=l, out_coord_y=c)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        launch(static, out, lc, cy)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch(static, out, lc, cy)
    for k in (1, 2, 3):
        fresh = [_dev(a) for a in batches[k]]
        eo, el, ec = torch.full_like(out, NAN), torch.zeros_like(lc), torch.zeros_like(cy)
        launch(fresh, eo, el, ec)
        for s, f in zip(static, fresh):
            s.copy_(f)
        out.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eo) and torch.equal(lc, el) and torch.equal(cy, ec), k
        assert not bool(out.isnan().any())


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: raw batches into captured steps against batches prepared beforehand
# ---------------------------------------------------------------------------------------------------------------------------------
RAW = dict(frames="raw", crop_size=40, warp_size=38, flip_p=0.5, make_gray=True,
           augment={"rotation": (-0.2, 0.2), "shear": (-0.1, 0.1), "translation": (-0.05, 0.05)})
_RAW_ATTRS = ("raw_frame", "raw_coords", "prep_matrix", "prep_matrix_inv", "prep_flip", "prep_crop_size", "prep_warp_size",
              "prep_frame_size", "prep_gray")


def _raw_batches(frame, naux, B, n, seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=True, labels="coords", **RAW)
    return [data.collate([ds[B * i + j] for j in range(B)], ds.topology) for i in range(n)]


def _prepared(hb):
    """The host batch `hb` with x / label_coords / node_coord_y produced by an eager ops.frame_prep, and no raw attributes."""
    d = data.to_device(copy.copy(hb), DEV)
    B, F = int(d.raw_frame.shape[0]), int(d.prep_frame_size)
    x = torch.full((B, 1, F, F), NAN, device=DEV)
    lc = torch.zeros(B, 4, 2, dtype=torch.int32, device=DEV)
    cy = torch.full((4 * B, 2), NAN, device=DEV)
    ops.frame_prep(d.raw_frame, x, matrix_inv=d.prep_matrix_inv, warp_size=d.prep_warp_size, flip=d.prep_flip, gray=d.prep_gray,
                   coords=d.raw_coords, matrix=d.prep_matrix, crop_size=d.prep_crop_size, out_label_coords=lc, out_coord_y=cy)
    torch.cuda.synchronize()
    p = copy.copy(hb)
    for k in _RAW_ATTRS:
        delattr(p, k)
    p.x, p.label_coords, p.node_coord_y = x.cpu(), lc.cpu(), cy.cpu()
    return p


def _criteria(frame, naux, B):
    return losses.build({"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
                         "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": frame, "num_aux_graphs": naux, "batch_size": B,
                         "use_coordinate_graph": True, "use_main_graph_only": False, "num_output_channels": 4})


def _graphed_training(host, frame, naux, B, steps):
    hip, _ = model_pair(frame, naux, 2, coord=True, seed=13, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    hip.train()
    torch.manual_seed(13)
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
    for q in emb.parameters():
        q.requires_grad_(False)
    model = {"embedder": emb, "landmark": hip}
    crit = _criteria(frame, naux, B)
    params = list(hip.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    static = data.to_device(copy.copy(host[0]), DEV)
    coords0 = static.node_coords.clone()

    def loss_fn():
        data.device_frames_(static)                        # raw frames: the step's first node; prepared: nothing
        data.device_labels_(static)                        # ... and the dense labels from what it wrote, the second
        static.node_coords = coords0.clone()
        preds, cp = engine.forward_batch(model, static, True)
        return engine.total_loss(engine.compute_loss(crit, preds, static.y, cp, static.node_coord_y, static.valid_labels, B))

    step = engine.GraphedTrainStep(loss_fn, opt, warmup=1)
    got = []
    for k in range(1, steps + 1):
        data.copy_batch_(static, host[k])
        got.append(float(step()[0]))
    torch.cuda.synchronize()
    assert step.replays == steps
    return got, [p.detach().clone() for p in params], static


def test_graphed_train_step_from_raw_frames_equals_the_prepared_run():
    frame, naux, B, steps = 16, 3, 2, 3
    raw = _raw_batches(frame, naux, B, steps + 1, 61)
    prepared = [_prepared(hb) for hb in raw]
    assert not hasattr(raw[0], "x") and not hasattr(raw[0], "label_coords") and tuple(raw[0].raw_frame.shape) == (B, 3, 40, 40)
    e0 = ops.dropout_epoch()
    try:
        loss_p, params_p, static_p = _graphed_training(prepared, frame, naux, B, steps)
        loss_r, params_r, static_r = _graphed_training(raw, frame, naux, B, steps)
    finally:
        ops.dropout_epoch_set(e0)
    assert torch.equal(static_r.x, static_p.x) and torch.equal(static_r.x.cpu(), prepared[-1].x)
    assert torch.equal(static_r.label_coords, static_p.label_coords) and torch.equal(static_r.node_coord_y, static_p.node_coord_y)
    assert torch.equal(static_r.y, static_p.y)
    assert loss_r == loss_p and len(set(loss_p)) == steps, (loss_r, loss_p)
    for a, b in zip(params_r, params_p):
        assert torch.equal(a, b)


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                                      b.contiguous().view(torch.int32))


def _graphed_evaluation(host, model, frame, naux, B):
    n = len(host)
    crit = _criteria(frame, naux, B)
    evs = EV.build({"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": B, "frame_size": frame,
                    "use_coordinate_graph": True}, max_updates=n)
    static = data.to_device(copy.copy(host[0]), DEV)
    step = engine.GraphedEvalStep(model, static, crit, B, use_coordinate_graph=True, evaluators=evs, warmup=1)
    preds, totals = [], []
    for hb in host:
        data.copy_batch_(static, hb)
        p, _, ls = step()
        preds.append(p.clone())
        totals.append(float(engine.total_loss(ls)))
    assert step.captures == 1
    return preds, totals, evs, step.loss_avg()


def test_graphed_eval_step_from_raw_frames_equals_the_prepared_run():
    frame, naux, B, n = 16, 3, 2, 3
    hip, _ = model_pair(frame, naux, 2, coord=True, seed=17, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    torch.manual_seed(17)
    model = {"embedder": torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV).eval(), "landmark": hip}
    raw = _raw_batches(frame, naux, B, n, 67)
    prepared = [_prepared(hb) for hb in raw]
    pp, tp, ep, avg_p = _graphed_evaluation(prepared, model, frame, naux, B)
    pr, tr, er, avg_r = _graphed_evaluation(raw, model, frame, naux, B)
    for a, b in zip(pr, pp):
        assert torch.equal(a, b)
    assert tr == tp and avg_r == avg_p and len(set(tp)) == n
    assert np.array_equal(er["balancedaccuracy"].counts(), ep["balancedaccuracy"].counts())
    lr, lp = er["landmarkcoorderror"], ep["landmarkcoorderror"]
    assert lr._count() == lp._count() == n
    for k in (1, 2):                                       # history and per-frame detail, bit for bit
        assert _same_bits(lr._state[k][:n], lp._state[k][:n]), k
    # ... and the eager steps prepare raw frames as well; inside a capture the outputs must exist already
    b = data.to_device(copy.copy(raw[0]), DEV)
    p, _, ls = engine.eval_step(model, b, _criteria(frame, naux, B), B, True)
    assert torch.equal(p, pp[0]) and float(engine.total_loss(ls)) == tp[0]
    assert tuple(b.x.shape) == (B, 1, frame, frame) and b.label_coords.dtype == torch.int32
    fresh = data.to_device(copy.copy(raw[1]), DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with pytest.raises(RuntimeError, match="stream capture must not allocate"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
            data.device_frames_(fresh)
