"""CPU: the device-history mode's public surface that needs no device -- evaluators.build(..., max_updates=), the constructor's
checks, the read-only tables, and engine.GraphedEvalStep's refusals (all raised before anything touches a device)."""
import types

import pytest
import torch

from echoglad_amd import engine, evaluators as EV


def _cfg(coord=False):
    return {"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": 2, "frame_size": 16, "use_coordinate_graph": coord}


def test_build_passes_max_updates_to_the_landmark_evaluator():
    evs = EV.build(_cfg(), max_updates=7)
    assert evs["landmarkcoorderror"].max_updates == 7
    assert EV.build(_cfg())["landmarkcoorderror"].max_updates is None            # the default stays the host mode
    assert EV.build(_cfg(True), max_updates=3)["landmarkcoorderror"].use_coord_graph


def test_host_mode_keeps_its_lists():
    ev = EV.LandmarkExpectedCoordiantesEvaluator(None, 2, 16, False)
    ev.coordinate_errors["ivs"].append(1.5)
    assert ev.coordinate_errors == {"ivs": [1.5], "lvid_top": [], "lvid_bot": [], "lvpw": []}
    ev.reset()
    assert ev.coordinate_errors["ivs"] == [] and ev.get_predictions() == {}


def test_device_mode_checks_and_read_only_tables():
    with pytest.raises(ValueError, match="max_updates"):
        EV.LandmarkExpectedCoordiantesEvaluator(None, 2, 16, False, max_updates=0)
    ev = EV.LandmarkExpectedCoordiantesEvaluator(None, 2, 16, False, max_updates=4)
    with pytest.raises(AttributeError):
        ev.width_MAE = {}
    if not torch.cuda.is_available():
        assert ev.width_MAE == {"lvid": [], "ivs": [], "lvpw": []} and ev.get_predictions() == {}
        with pytest.raises(RuntimeError, match="CUDA"):
            ev.update(torch.zeros(2 * 340, 4), torch.zeros(2 * 340, 4), torch.ones(2), torch.ones(2), torch.ones(2 * 340, 4))


class _Module(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("a refused step must not run the model")


def _model(training):
    m = {"embedder": _Module(), "landmark": _Module()}
    for v in m.values():
        v.train(training)
    return m


def test_graphed_eval_step_refusals():
    batch = types.SimpleNamespace(x=torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="warm-up"):
        engine.GraphedEvalStep(_model(False), batch, None, 1, warmup=0)
    with pytest.raises(ValueError, match="training mode"):
        engine.GraphedEvalStep(_model(True), batch, None, 1)
    host_lm = {"landmarkcoorderror": EV.LandmarkExpectedCoordiantesEvaluator(None, 1, 16, False)}
    with pytest.raises(ValueError, match="max_updates"):
        engine.GraphedEvalStep(_model(False), batch, None, 1, evaluators=host_lm)
    with pytest.raises(ValueError, match="cannot be captured"):
        engine.GraphedEvalStep(_model(False), batch, None, 1, evaluators={"x": object()})
