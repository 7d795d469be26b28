"""-m gpu: dense node labels built on the device from landmark coordinates (csrc/labels.hip, eg_node_labels) against the host's
data.node_labels, alone, captured into a graph, and as the first node of engine.GraphedTrainStep / GraphedEvalStep against the same
steps fed with dense host labels.  The outputs are exactly 0.0 and 1.0: every comparison is torch.equal."""
import copy
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV, model_pair
from echoglad_amd import data, engine, evaluators as EV, losses, ops

pytestmark = pytest.mark.gpu

CONFIGS = [(16, 3, False), (30, 3, False), (16, 4, False), (16, 2, True)]      # 30/3: sides that do not divide F; 16/4: an aux level of side F


def _host_dense(coords, frame, naux, main_only, extra=0):
    """[B, 4, 2] -> the stacked data.node_labels of every frame, [B * (N_grid + extra), 4] with `extra` zero rows per frame."""
    frames = []
    for hw in np.asarray(coords):
        y = np.stack([data.node_labels(c, frame, naux, main_only) for c in hw], axis=1)
        frames.append(np.concatenate([y, np.zeros((extra, 4), np.float32)]))
    return torch.from_numpy(np.concatenate(frames))


def _device_dense(coords, valid4, frame, naux, main_only, extra=0):
    """ops.node_labels into NaN-filled tensors (a row the kernel skipped would show) -> (y, valid_labels) on the host."""
    levels = losses.level_grids(frame, naux, main_only)
    B = len(coords)
    rows = B * (levels[-1][0] + frame * frame + extra)
    y = torch.full((rows, 4), float("nan"), device=DEV)
    v = torch.full((rows, 4), float("nan"), device=DEV)
    c = torch.from_numpy(np.asarray(coords).astype(np.int32)).to(DEV)
    v4 = None if valid4 is None else torch.from_numpy(np.asarray(valid4, np.float32)).to(DEV)
    out = ops.node_labels(c, v4, B, levels, frame, y, v)
    assert out is y
    torch.cuda.synchronize()
    return y.cpu(), v.cpu()


def _sweep(frame):
    """B = 2F frames: every v in [-F, F) once as h (landmark 0) and once as w (landmark 1) of some landmark; 2 and 3 mix them."""
    v = np.arange(-frame, frame)
    k = np.arange(2 * frame)
    wrap = lambda a: (a % (2 * frame)) - frame
    coords = np.stack([np.stack([v, wrap(7 * k + 3)], 1), np.stack([wrap(5 * k + 1), v], 1), np.stack([v, v], 1),
                       np.stack([wrap(3 * k + 1), wrap(11 * k + 2)], 1)], axis=1)
    valid4 = ((k[:, None] + np.arange(4)[None, :]) % 3 != 0).astype(np.float32)        # differs per frame and channel
    return coords, valid4


@pytest.mark.parametrize("frame,naux,main_only", CONFIGS)
def test_every_coordinate_of_a_small_grid(frame, naux, main_only):
    coords, valid4 = _sweep(frame)
    B = len(coords)
    for extra in (0, 4):                                   # 4: the coordinate nodes' rows of a coordinate-graph batch -> zeros
        want = _host_dense(coords, frame, naux, main_only, extra)
        y, v = _device_dense(coords, valid4, frame, naux, main_only, extra)
        assert torch.equal(y, want), extra
        n = want.shape[0] // B
        assert torch.equal(v, torch.from_numpy(valid4).repeat_interleave(n, dim=0)), extra
    y, v = _device_dense(coords, None, frame, naux, main_only)          # no flags: valid = 1; out_valid is optional
    assert torch.equal(y, _host_dense(coords, frame, naux, main_only)) and torch.equal(v, torch.ones_like(v))
    levels = losses.level_grids(frame, naux, main_only)
    only = torch.full_like(y, float("nan")).to(DEV)
    ops.node_labels(torch.from_numpy(coords.astype(np.int32)).to(DEV), None, B, levels, frame, only)
    assert torch.equal(only.cpu(), y)


def test_targets_on_the_edges_of_a_workgroups_rows():
    """64/2: 4116 rows = 5 workgroups of 1024 rows, the last one short; the main grid starts at row 20.  Landmarks whose 1 sits on the
    last row of a workgroup, the first of the next, the first and the last row of the frame's main grid."""
    frame, naux = 64, 2
    rows = [1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 4115, 20, 1025, 3000]
    hw = [divmod(r - 20, frame) for r in rows]
    coords = np.asarray(hw).reshape(3, 4, 2)
    assert np.array_equal(data.label_rows(coords.reshape(-1, 2), frame, naux)[-1], rows)
    valid4 = np.asarray([[1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1]], np.float32)
    for extra in (0, 4):
        y, v = _device_dense(coords, valid4, frame, naux, False, extra)
        assert torch.equal(y, _host_dense(coords, frame, naux, False, extra))
        assert torch.equal(v, torch.from_numpy(valid4).repeat_interleave(4116 + extra, dim=0))


def test_full_size_frames_equal_the_host_labels(golden_dir):
    d = np.load(os.path.join(golden_dir, "labels.npz"))
    c8 = d["F224_A7_mo0_coords"]
    coords = np.stack([c8[[(4 * b + c) % 8 for c in range(4)]] for b in range(3)])      # B = 3, includes 223 and -1
    valid4 = np.asarray([[1, 1, 0, 1], [0, 1, 1, 1], [1, 0, 1, 0]], np.float32)
    y, v = _device_dense(coords, valid4, 224, 7, False)
    assert tuple(y.shape) == (3 * 72020, 4)
    assert torch.equal(y, _host_dense(coords, 224, 7, False))
    assert torch.equal(v, torch.from_numpy(valid4).repeat_interleave(72020, dim=0))
    assert np.array_equal(np.nonzero(y[:72020, 0].numpy())[0], d["F224_A7_mo0_ones"][0])


def test_a_landmark_outside_the_frame_gets_no_label():
    """h or w outside [-F, F) -- IndexError on the host -- leaves that channel 0 on every level; the other channels are not affected."""
    frame, naux = 16, 3
    big = 2 ** 31 - 1
    outside = [(frame, 3), (3, frame), (-frame - 1, 0), (0, -frame - 1), (1000, 1000), (-1000, 5), (big, -big - 1), (-big - 1, 2)]
    coords, _ = _sweep(frame)
    coords = coords[: len(outside)].astype(np.int64)
    inside = coords.copy()
    for b, hw in enumerate(outside):
        with pytest.raises(IndexError):
            data.label_rows([hw], frame, naux)
        coords[b, 2] = hw
    y, _ = _device_dense(coords, None, frame, naux, False)
    want = _host_dense(inside, frame, naux, False)
    assert float(y[:, 2].abs().sum()) == 0.0
    for c in (0, 1, 3):
        assert torch.equal(y[:, c], want[:, c]), c


def _host_batches(frame, naux, coord, B, n, labels, seed):
    """n collated batches of B samples; the same seed gives the same frames and landmarks in both label modes."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=coord, labels=labels)
    return [data.collate([ds[B * i + j] for j in range(B)], ds.topology) for i in range(n)]


def test_device_labels_captured_into_a_graph():
    frame, naux, B = 16, 3, 2
    dense = _host_batches(frame, naux, True, B, 4, "dense", 31)
    sparse = _host_batches(frame, naux, True, B, 4, "coords", 31)
    for k, hb in enumerate(sparse):
        hb.label_valid = torch.tensor([[1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, float(k % 2)]])
    static = data.to_device(copy.copy(sparse[0]), DEV)
    assert not hasattr(static, "y") and static.label_coords.is_cuda and static.label_coords.dtype == torch.int32
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture must not allocate"):
        with torch.cuda.graph(graph, stream=stream):
            data.device_labels_(static)                    # y / valid_labels do not exist yet: refused, nothing launched
    with torch.cuda.stream(stream):
        assert data.device_labels_(static) is static       # the eager call allocates
    torch.cuda.synchronize()
    y, v = static.y, static.valid_labels
    assert tuple(y.shape) == (B * 340, 4) and torch.equal(y.cpu(), dense[0].y)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        data.device_labels_(static)
    for k in (1, 2, 3):
        data.copy_batch_(static, sparse[k])
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert static.y is y and static.valid_labels is v
        assert torch.equal(y.cpu(), dense[k].y), k
        assert torch.equal(v.cpu(), sparse[k].label_valid.repeat_interleave(340, dim=0)), k


def _criteria(frame, naux, B, coord):
    return losses.build({"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
                         "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": frame, "num_aux_graphs": naux, "batch_size": B,
                         "use_coordinate_graph": coord, "use_main_graph_only": False, "num_output_channels": 4})


def _graphed_training(labels, frame, naux, B, steps):
    host = _host_batches(frame, naux, True, B, steps + 1, labels, 47)
    hip, _ = model_pair(frame, naux, 2, coord=True, seed=13, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    hip.train()
    torch.manual_seed(13)
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
    for q in emb.parameters():
        q.requires_grad_(False)
    model = {"embedder": emb, "landmark": hip}
    crit = _criteria(frame, naux, B, True)
    assert list(crit) == ["WeightedBceWithLogits", "ExpectedLandmarkMse", "coordinate"]
    params = list(hip.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
    static = data.to_device(copy.copy(host[0]), DEV)
    coords0 = static.node_coords.clone()

    def loss_fn():
        data.device_labels_(static)                        # coordinate labels: the step's first node; dense: nothing
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
    return got, [p.detach().clone() for p in params], static, host


def test_graphed_train_step_from_coordinate_labels_equals_the_dense_run():
    frame, naux, B, steps = 16, 3, 2, 3
    e0 = ops.dropout_epoch()
    try:
        loss_d, params_d, static_d, host_d = _graphed_training("dense", frame, naux, B, steps)
        loss_c, params_c, static_c, host_c = _graphed_training("coords", frame, naux, B, steps)
    finally:
        ops.dropout_epoch_set(e0)
    assert not hasattr(host_c[0], "y") and tuple(host_c[0].label_coords.shape) == (B, 4, 2)
    assert torch.equal(static_c.y, static_d.y) and torch.equal(static_c.valid_labels, static_d.valid_labels)
    assert torch.equal(static_c.y.cpu(), host_d[-1].y)
    assert loss_c == loss_d and len(set(loss_d)) == steps, (loss_c, loss_d)
    for a, b in zip(params_c, params_d):
        assert torch.equal(a, b)


def _graphed_evaluation(labels, model, frame, naux, B, coord, n):
    host = _host_batches(frame, naux, coord, B, n, labels, 53)
    crit = _criteria(frame, naux, B, coord)
    evs = EV.build({"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": B, "frame_size": frame,
                    "use_coordinate_graph": coord}, max_updates=n)
    static = data.to_device(copy.copy(host[0]), DEV)
    step = engine.GraphedEvalStep(model, static, crit, B, use_coordinate_graph=coord, evaluators=evs, warmup=1)
    preds, totals = [], []
    for hb in host:
        data.copy_batch_(static, hb)
        p, _, ls = step()
        preds.append(p.clone())
        totals.append(float(engine.total_loss(ls)))
    assert step.captures == 1
    return preds, totals, evs, step.loss_avg()


def _same_bits(a, b):
    """Bit equality of two fp32 tensors.  A landmark record holds the reference's IEEE results: a ground-truth width of zero (two
    landmarks on one pixel, common at F = 16) makes the width MPE inf or NaN, and torch.equal calls NaN different from itself."""
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                                      b.contiguous().view(torch.int32))


@pytest.mark.parametrize("coord", [False, True])
def test_graphed_eval_step_from_coordinate_labels_equals_the_dense_run(coord):
    frame, naux, B, n = 16, 3, 2, 3
    hip, _ = model_pair(frame, naux, 2, coord=coord, seed=17, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    torch.manual_seed(17)
    model = {"embedder": torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV).eval(), "landmark": hip}
    pd, td, ed, avg_d = _graphed_evaluation("dense", model, frame, naux, B, coord, n)
    pc, tc, ec, avg_c = _graphed_evaluation("coords", model, frame, naux, B, coord, n)
    for a, b in zip(pc, pd):
        assert torch.equal(a, b)
    assert tc == td and avg_c == avg_d and len(set(td)) == n
    assert np.array_equal(ec["balancedaccuracy"].counts(), ed["balancedaccuracy"].counts())
    lc, ld = ec["landmarkcoorderror"], ed["landmarkcoorderror"]
    assert lc._count() == ld._count() == n
    for k in (1, 2):                                       # history and per-frame detail, bit for bit
        print(("history", "detail")[k - 1], "NaNs:", int(ld._state[k][:n].isnan().sum()), int(lc._state[k][:n].isnan().sum()))
        assert _same_bits(lc._state[k][:n], ld._state[k][:n]), k
    # ... and the eager steps expand the coordinates as well
    hb = _host_batches(frame, naux, coord, B, 1, "coords", 53)[0]
    b = data.to_device(copy.copy(hb), DEV)
    p, _, ls = engine.eval_step(model, b, _criteria(frame, naux, B, coord), B, coord)
    assert torch.equal(p, pd[0]) and float(engine.total_loss(ls)) == td[0]
