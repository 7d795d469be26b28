"""CPU: the host side of the balanced-accuracy evaluator -- scores from confusion counts against the reference's recorded
numbers (tests/golden/balacc_*.npz, made by make_eval_golden.py) and against sklearn, the evaluator builder, and the engine's
per-class dispatch of evaluator calls."""
import os

import numpy as np
import pytest
import torch

import make_eval_golden as G
from echoglad_amd import engine, evaluators

CASES = sorted(G.CASES)


def _fixture(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"balacc_{name}.npz"))


@pytest.mark.parametrize("name", CASES)
def test_scores_from_counts_equal_the_reference(golden_dir, name):
    z = _fixture(golden_dir, name)
    spc = evaluators.balanced_accuracy_from_counts(z["counts"])
    assert spc.dtype == np.float64 and spc.shape == z["score_per_class"].shape
    assert np.array_equal(spc, z["score_per_class"])                      # bit for bit
    # the reference's own expressions on the array (evaluators.py:119-143)
    assert spc.mean(axis=0).mean() == z["compute"]
    assert np.array_equal(spc.mean(axis=0), z["per_class"])
    assert spc[-1, :].mean() == z["last"]


@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_regenerate_and_count(golden_dir, name):
    """The seeds still give the inputs the reference saw (digest), and the numpy counts of them are the recorded ones."""
    z = _fixture(golden_dir, name)
    for k, (kind, seed, (rows, ch)) in enumerate(zip(z["kinds"], z["seeds"], z["args"])):
        pred, y, valid = G.case_inputs(str(kind), int(seed), int(rows), int(ch))
        assert G.input_digest(pred, y, valid) == str(z["digests"][k]), (name, k)
        assert np.array_equal(G.numpy_counts(pred, y, valid), z["counts"][k])


def test_edge_fixture_covers_the_edges(golden_dir):
    z = _fixture(golden_dir, "edge")
    spc, kinds = z["score_per_class"], list(z["kinds"])
    assert spc[kinds.index("novalid"), 1] == 0.0                          # a channel without a valid row
    c = z["counts"][kinds.index("negonly")]
    assert np.all(c[:, 0] + c[:, 1] == 0) and spc[kinds.index("negonly"), 3] == 1.0
    assert np.all(spc[kinds.index("negonly"), :3] == c[:3, 3] / (c[:3, 3] + c[:3, 2]))      # TNR
    c = z["counts"][kinds.index("allpos")]
    assert np.all(spc[kinds.index("allpos")] == c[:, 0] / (c[:, 0] + c[:, 1]))                # TPR
    assert tuple(z["shapes"][kinds.index("one")]) == (1, 4)


def test_scores_from_counts_match_sklearn_on_random_tables():
    sk = pytest.importorskip("sklearn.metrics")
    import warnings
    rng = np.random.default_rng(7)
    tables = rng.integers(0, 6, size=(400, 4))
    tables[:40, 0:2] = 0                                                  # no positive label
    tables[40:80, 2:4] = 0                                                # no negative label
    tables[80:100, [0, 2]] = 0                                            # no positive prediction
    tables[100:110] = 0                                                   # no valid row
    got = evaluators.balanced_accuracy_from_counts(tables.reshape(400, 1, 4))[:, 0]
    for (tp, fn, fp, tn), g in zip(tables, got):
        if tp + fn + fp + tn == 0:
            assert g == 0.0
            continue
        y_true = np.array([1] * (tp + fn) + [0] * (fp + tn))
        y_pred = np.array([1] * tp + [0] * fn + [1] * fp + [0] * tn)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = sk.balanced_accuracy_score(y_true, y_pred)
        assert g == want, ((tp, fn, fp, tn), g, want)


def test_scores_from_counts_documented_cases():
    f = evaluators.balanced_accuracy_from_counts
    assert f([[0, 0, 3, 7]])[0] == 0.7                                    # all-negative labels, mixed predictions: TNR
    assert f([[3, 1, 0, 0]])[0] == 0.75                                   # all-positive labels: TPR
    assert f([[0, 0, 0, 9]])[0] == 1.0                                    # all-negative labels and predictions
    assert f([[0, 0, 0, 0]])[0] == 0.0                                    # no valid row
    with pytest.raises(ValueError):
        f(np.zeros((2, 3)))


_CFG = {"batch_size": 2, "frame_size": 16, "use_coordinate_graph": False}


def test_builder_builds_the_reachable_standards():
    evs = evaluators.build({**_CFG, "standards": ["balancedaccuracy", "landmarkcoorderror"]})
    assert list(evs) == ["balancedaccuracy", "landmarkcoorderror"]
    assert isinstance(evs["balancedaccuracy"], evaluators.BalancedBinaryAccuracyEvaluator)
    lm = evs["landmarkcoorderror"]
    assert isinstance(lm, evaluators.LandmarkExpectedCoordiantesEvaluator)
    assert (lm.batch_size, lm.frame_size, lm.use_coord_graph) == (2, 16, False)
    assert evs["balancedaccuracy"].max_updates == 65536


@pytest.mark.parametrize("standard", ["accuracy", "mse", "landmarkerror"])
def test_builder_refuses_what_the_reference_engine_cannot_call(standard):
    with pytest.raises(NotImplementedError, match="reference"):
        evaluators.build({**_CFG, "standards": ["balancedaccuracy", standard]})


class _FakeBalanced(evaluators.BalancedBinaryAccuracyEvaluator):
    def __init__(self):
        self.calls = []

    def update(self, *args):
        self.calls.append(args)


class _FakeLandmark:
    def __init__(self):
        self.calls = []

    def update(self, *args):
        self.calls.append(args)


@pytest.mark.parametrize("coord", [False, True])
def test_update_evaluators_gives_every_evaluator_its_own_call(coord):
    preds, y, cp, cy, px, py, valid = (torch.full((1,), float(i)) for i in range(7))
    evs = {"landmark": _FakeLandmark(), "balancedaccuracy": _FakeBalanced(), "other": _FakeBalanced()}
    engine.update_evaluators(evs, preds, y, cp, cy, px, py, valid, coord)
    lm = evs["landmark"].calls
    assert len(lm) == 1 and len(lm[0]) == 5
    want = (cp, cy, px, py, valid) if coord else (preds, y, px, py, valid)
    assert all(a is b for a, b in zip(lm[0], want))                      # the five-argument call is unchanged
    for key in ("balancedaccuracy", "other"):                            # dispatch on the type, not the key
        calls = evs[key].calls
        assert len(calls) == 1 and len(calls[0]) == 3
        assert all(a is b for a, b in zip(calls[0], (preds, y, valid)))  # the landmark logits, also with the coordinate graph
