"""CPU: losses.build -- the criterion builder -- against what the reference's own criterion_builder.build made of the same configs
(tests/golden/crit_builder.json, made by make_criteria_golden.py), its refusals, and the criterion fixtures' inputs.  Nothing here
touches a device: the HIP library is made unloadable while the builder runs."""
import copy
import json
import os

import numpy as np
import pytest

import make_criteria_golden as G
from echoglad_amd import _lib, engine, losses


class _Logger:
    def __init__(self):
        self.messages = []

    def infov(self, msg):
        self.messages.append(msg)


def _record(golden_dir):
    with open(os.path.join(golden_dir, "crit_builder.json")) as f:
        return json.load(f)


@pytest.fixture
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the criterion builder must not load the HIP library")
    monkeypatch.setattr(_lib, "load", refuse)


def test_fixture_configs_regenerate(golden_dir):
    rec = _record(golden_dir)
    assert sorted(rec) == sorted(n for n, _ in G.builder_configs())
    for name, cfg in G.builder_configs():
        assert rec[name]["config"] == cfg, name


@pytest.mark.parametrize("name", [n for n, _ in G.builder_configs()])
def test_builder_matches_the_reference_builder(golden_dir, no_device, name):
    want = _record(golden_dir)[name]
    cfg = want["config"]
    before = copy.deepcopy(cfg)
    log = _Logger()
    crit = losses.build(cfg, logger=log)
    assert cfg == before                                              # the caller's config is not consumed
    assert list(crit) == want["names"]
    assert log.messages == want["messages"]
    for (key, c), d in zip(crit.items(), want["criteria"]):
        assert type(c).__name__ == d["class"], key
        assert float(c.loss_weight) == d["loss_weight"], key
        for attr in ("ones_weight", "batch_size", "frame_size", "num_aux_graphs", "num_output_channels", "use_main_graph_only"):
            if attr in d:
                assert getattr(c, attr) == d[attr], (key, attr)
        if "grid_sizes" in d:
            assert list(c.grid_sizes) == d["grid_sizes"] and list(c.end_indices) == d["end_indices"], key
            assert c._side == {}                                      # no device tensor made yet
    if cfg["use_coordinate_graph"]:
        assert list(crit)[-1] == "coordinate" and isinstance(crit["coordinate"], engine.MAE)
        assert crit["coordinate"].loss_weight == 1
    else:
        assert "coordinate" not in crit


def test_builder_classes_are_the_fusable_ones(golden_dir, no_device):
    """The classes fused_criteria dispatches on: WeightedBCE for 'bce', its subclass for the logits form, engine.MAE for 'coordinate'."""
    crit = losses.build(_record(golden_dir)["bce_coord_main_only"]["config"])
    assert type(crit["bce"]) is losses.WeightedBCE
    assert isinstance(crit["ExpectedLandmarkMse"], losses.ExpectedLandmarkMSE)
    crit = losses.build(_record(golden_dir)["default_coord"]["config"])
    assert isinstance(crit["WeightedBceWithLogits"], losses.WeightedBCEWithLogitsLoss)
    assert isinstance(crit["WeightedBceWithLogits"], losses.WeightedBCE)          # as in criterion.py:29
    assert type(crit["coordinate"]) is engine.MAE


@pytest.mark.parametrize("name", ["mse", "mae", "HeatmapMse"])
def test_builder_refuses_what_the_reference_engine_cannot_call(golden_dir, no_device, name):
    cfg = dict(_record(golden_dir)["default"]["config"])
    cfg[name] = {"loss_weight": 1} if name != "HeatmapMse" else {"reduction": "none", "ones_weight": 1, "loss_weight": 1}
    with pytest.raises(NotImplementedError, match="three"):
        losses.build(cfg)


def test_builder_unknown_name_and_missing_keys(golden_dir, no_device):
    cfg = dict(_record(golden_dir)["default"]["config"])
    cfg["Focal"] = {}
    with pytest.raises(KeyError, match="Focal"):
        losses.build(cfg)
    cfg = dict(_record(golden_dir)["default"]["config"])
    del cfg["num_output_channels"]
    with pytest.raises(KeyError):
        losses.build(cfg)
    cfg = dict(_record(golden_dir)["default"]["config"])
    cfg["WeightedBceWithLogits"] = dict(cfg["WeightedBceWithLogits"], reduction="mean")
    with pytest.raises(NotImplementedError):                          # reduction='none' only, as WeightedBCEWithLogitsLoss has it
        losses.build(cfg)


def test_builder_without_logger(golden_dir, no_device):
    rec = _record(golden_dir)["default_coord"]
    assert list(losses.build(rec["config"])) == rec["names"]


@pytest.mark.parametrize("name", sorted(G.BCE_CASES))
def test_bce_fixture_inputs_regenerate_and_restate_in_fp64(golden_dir, name):
    """The seeds still give the inputs the reference saw (digest), and the reference's values restate in fp64 numpy -- the
    fixture holds nn.BCELoss on probabilities with its -100 clamp, ones_weight on y == 1 and the valid-weighted mean."""
    z = np.load(os.path.join(golden_dir, f"crit_bce_{name}.npz"))
    frame, naux, batch, seed, ow = G.BCE_CASES[name]
    assert (int(z["frame"]), int(z["naux"]), int(z["batch"]), int(z["seed"]), float(z["ones_weight"])) == (frame, naux, batch, seed, ow)
    p, y, v = G.bce_inputs(frame, naux, batch, seed)
    assert G.input_digest(p, y, v) == str(z["digest"])
    assert np.any(p == 0.0) and np.any(p == 1.0) and np.any((p == 0.0) & (y == 1.0)) and 0 < v.mean() < 1
    p64, y64, v64 = (a.astype(np.float64) for a in (p, y, v))
    with np.errstate(divide="ignore"):
        el = (y64 - 1) * np.maximum(np.log1p(-p64), -100) - y64 * np.maximum(np.log(p64), -100)
        g = (p64 - y64) / np.maximum((1 - p64) * p64, 1e-12)
    w = np.where((y64 == 1) & (ow > 1), ow, 1.0)
    want = (el * w * v64).sum() / v64.sum()
    assert abs(float(z["bce"]) - want) <= 1e-5 * abs(want)
    grad = (g * w * v64 / v64.sum()).reshape(-1)
    if "idx" in z:
        grad = grad[z["idx"]]
    assert z["grad_bce"].shape == grad.shape
    assert np.allclose(z["grad_bce"], grad, rtol=1e-5, atol=1e-30)


def test_mae_fixture_inputs_regenerate_and_restate_in_fp64(golden_dir):
    z = np.load(os.path.join(golden_dir, "crit_mae.npz"))
    off = 0
    for k, name in enumerate(z["names"]):
        rows, seed, w = G.MAE_CASES[str(name)]
        pred, y = G.mae_inputs(rows, seed)
        assert G.input_digest(pred, y) == str(z["digests"][k])
        d = pred.astype(np.float64) - y
        assert np.any(d == 0)
        assert abs(float(z["values"][k]) - w * np.abs(d).mean()) <= 1e-6 * w * np.abs(d).mean()
        g = z["grads"][off:off + d.size]
        off += d.size
        assert np.array_equal(g, (np.sign(d) * np.float32(w / d.size)).astype(np.float32).reshape(-1))
    assert off == z["grads"].size
