"""-m gpu: the device-side balanced-accuracy evaluator (csrc/metrics.hip) -- counts and scores against the reference's recorded
numbers, inside engine.eval_step next to the landmark evaluator, captured into a HIP graph, past its capacity, and its argument
checks.  Every input here fits one sweep of the capped grid (at most 106 workgroups); the shapes past the cap, every channel
count and the merge's strides are in tests/test_gpu_counts_sweeps.py."""
import os

import numpy as np
import pytest
import torch

import make_eval_golden as G
from gpu_util import DEV, model_pair
from echoglad_amd import data, engine, evaluators, ops

pytestmark = pytest.mark.gpu

BBA = evaluators.BalancedBinaryAccuracyEvaluator


def _dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _recount(pred, y, valid):
    """torch recount on the device tensors -> [C, 4] int64 numpy {TP, FN, FP, TN}."""
    v, pos, pp = valid > 0, y != 0, pred > 0.5
    return torch.stack([(v & pos & pp).sum(0), (v & pos & ~pp).sum(0), (v & ~pos & pp).sum(0), (v & ~pos & ~pp).sum(0)],
                       dim=-1).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_counts_and_scores_equal_the_reference(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"balacc_{name}.npz"))
    ev = BBA(None)
    assert ev.score_per_class is None
    for k, (kind, seed, (rows, ch)) in enumerate(zip(z["kinds"], z["seeds"], z["args"])):
        inputs = G.case_inputs(str(kind), int(seed), int(rows), int(ch))
        assert G.input_digest(*inputs) == str(z["digests"][k]), (name, k)
        ev.update(*_dev(*inputs))
    assert np.array_equal(ev.counts(), z["counts"])
    spc = ev.score_per_class
    assert spc.dtype == np.float64 and np.array_equal(spc, z["score_per_class"])
    assert ev.compute() == z["compute"]
    assert np.array_equal(ev.get_per_class_score(), z["per_class"])
    assert ev.get_last() == z["last"]


def test_eval_step_feeds_both_evaluators():
    B, frame, naux = 2, 16, 3
    hip, _ = model_pair(frame, naux, 2, seed=3)
    torch.manual_seed(3)
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
    np.random.seed(3)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame)
    batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
    n = ds.topology.num_nodes
    batch.valid_labels[n:, 1] = 0.0                                       # landmark 1 unlabelled in frame 1
    model = {"embedder": emb, "landmark": hip}
    evs = {"balancedaccuracy": BBA(None), "landmark": evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, frame, False)}
    preds, _, _ = engine.eval_step(model, batch, None, B, evaluators=evs)
    want = _recount(preds, batch.y, batch.valid_labels)
    assert np.array_equal(evs["balancedaccuracy"].counts(), want[None])
    assert np.array_equal(evs["balancedaccuracy"].score_per_class, evaluators.balanced_accuracy_from_counts(want[None]))
    alone = {"landmark": evaluators.LandmarkExpectedCoordiantesEvaluator(None, B, frame, False)}
    engine.eval_step(model, batch, None, B, evaluators=alone)
    got, ref = evs["landmark"].get_last(), alone["landmark"].get_last()
    assert got.keys() == ref.keys()
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), k


def _random_inputs(count, rows, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(count):
        pred = torch.randn(rows, 4, device=DEV, generator=g) * 1.5
        y = (torch.rand(rows, 4, device=DEV, generator=g) < 0.01).float()
        valid = (torch.rand(1, 4, device=DEV, generator=g) < 0.7).float().expand(rows, 4).contiguous()
        out.append((pred, y, valid))
    return out


def test_a_captured_update_appends_one_record_per_replay():
    rows = 72020
    inputs = _random_inputs(5, rows, 11)
    ev = BBA(None, max_updates=16)
    static = [torch.empty(rows, 4, device=DEV) for _ in range(3)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for s, t in zip(static, inputs[0]):
            s.copy_(t)
        ev.update(*static)                                                # warm-up: the stream's ticket word is allocated here
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                          # a synchronising update would fail the capture
        ev.update(*static)
    for inp in inputs:
        for s, t in zip(static, inp):
            s.copy_(t)
        graph.replay()
    torch.cuda.synchronize()
    eager = BBA(None)
    for inp in inputs:
        eager.update(*inp)
    got = ev.counts()
    assert got.shape == (5, 4, 4)
    assert np.array_equal(got, eager.counts())
    assert np.array_equal(got, np.stack([_recount(*inp) for inp in inputs]))
    assert np.array_equal(ev.score_per_class, eager.score_per_class)


def test_an_update_neither_allocates_nor_synchronises_after_the_first():
    inputs = _random_inputs(2, 9000, 5)
    ev = BBA(None)
    ev.update(*inputs[0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(*inputs[1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    assert ev.counts().shape == (2, 4, 4)


def test_overflow_raises_and_reset_recovers():
    inputs = _random_inputs(3, 3000, 7)
    ev = BBA(None, max_updates=2)
    for inp in inputs:
        ev.update(*inp)
    with pytest.raises(RuntimeError, match="max_updates"):
        ev.compute()
    ev.reset()
    assert ev.score_per_class is None
    ev.update(*inputs[2])
    ev.update(*inputs[0])
    assert np.array_equal(ev.counts(), np.stack([_recount(*inputs[2]), _recount(*inputs[0])]))
    assert ev.compute() == evaluators.balanced_accuracy_from_counts(ev.counts()).mean(axis=0).mean()


def test_records_are_bit_reproducible_and_independent_of_alignment():
    inputs = _random_inputs(3, 200003, 9)
    a, b, c = BBA(None), BBA(None), BBA(None)
    for inp in inputs:
        a.update(*inp)
        b.update(*inp)
        # the same rows at a 4-byte offset: the scalar-load instance of the kernel
        moved = []
        for t in inp:
            buf = torch.empty(t.numel() + 1, device=DEV)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            moved.append(v)
        c.update(*moved)
    assert np.array_equal(a.counts(), b.counts()) and np.array_equal(a.counts(), c.counts())
    assert np.array_equal(a.score_per_class, b.score_per_class)


def test_bad_arguments_raise_before_a_launch():
    rows = 100
    pred, y, valid = _random_inputs(1, rows, 3)[0]
    history = torch.zeros(4, 4, 4, dtype=torch.int64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(ops.CONFUSION_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    bad = [
        (pred.cpu(), y, valid, history, counter, ws),                     # a CPU tensor
        (pred, y[:50], valid, history, counter, ws),                      # a shape mismatch
        (pred, y.double(), valid, history, counter, ws),                  # a wrong dtype
        (pred, y, valid, history[:, :3], counter, ws),                    # history for another channel count
        (pred, y, valid, history.int(), counter, ws),
        (pred, y, valid, history, counter, ws[:100]),                     # a workspace too small
        (pred.t(), y, valid, history, counter, ws),                       # not contiguous
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ops.confusion_counts(*args)
    wide = torch.zeros(rows, 9, device=DEV)
    with pytest.raises(RuntimeError):
        ops.confusion_counts(wide, wide, wide, torch.zeros(4, 9, 4, dtype=torch.int64, device=DEV), counter, ws)
    with pytest.raises(RuntimeError, match="CUDA"):
        BBA(None).update(pred.cpu(), y.cpu(), valid.cpu())
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and int(history.abs().sum().item()) == 0
    ops.confusion_counts(pred, y, valid, history, counter, ws)
    assert int(counter.item()) == 1 and np.array_equal(history[0].cpu().numpy(), _recount(pred, y, valid))
