#!/usr/bin/env python3
"""Generate the balanced-accuracy fixtures tests/golden/balacc_*.npz by RUNNING THE REFERENCE'S OWN
``BalancedBinaryAccuracyEvaluator`` (src/core/evaluators.py:85-143, sklearn underneath) in this container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py

The reference tree is imported read-only with its missing third-party modules stubbed (the recipe of make_golden.py:
torchvision is not installed; sklearn and matplotlib are).  Only OUTPUT DATA is written.  The inputs themselves are not
stored: ``case_inputs`` regenerates them from the recorded seeds with numpy.random.default_rng (the tests import it from
here, on machines without the reference tree), and every fixture records a digest of them so that a drifting regeneration
fails the test instead of comparing against other data.

Every fixture holds, for a sequence of updates of one evaluator: the seeds, the shapes [rows, C], the input digests, the
confusion counts {TP, FN, FP, TN} computed with numpy, and the reference's per-update ``score_per_class`` rows, ``compute()``,
``get_per_class_score()`` and ``get_last()``.  (One exception: at R = 1 the reference's update raises, see main(); that row is
the sklearn call the reference makes, on a numpy mask.)
"""
import hashlib
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

import numpy as np

# name -> [(kind, seed, rows, channels)], one entry per update of ONE evaluator
CASES = {
    # 224/7 frames (72,020 node rows each), the labels of data.py, valid per (frame, channel)
    "f224_b1": [("frames", 11, 1, 4), ("frames", 12, 1, 4), ("frames", 13, 1, 4)],
    "f224_b3": [("frames", 21, 3, 4), ("frames", 22, 3, 4)],
    # small R: one edge per update
    "edge": [("novalid", 31, 300, 4), ("negonly", 32, 300, 4), ("allpos", 33, 300, 4), ("threshold", 34, 256, 4),
             ("nan", 35, 300, 4), ("halfvalid", 36, 300, 4), ("ragged", 37, 6145, 4), ("one", 38, 1, 4)],
    "c1": [("random", 41, 3000, 1), ("random", 42, 777, 1), ("random", 43, 2049, 1)],
    "c3": [("random", 51, 3000, 3), ("random", 52, 5001, 3)],
}


def _frames(rng, batch, frame=224, naux=7):
    """Logits ~ N(0, 1.5) over the node rows of `batch` frames, data.py's node labels at random landmarks, valid per
    (frame, channel) with some zeros."""
    sys.path.insert(0, REPO)
    from echoglad_amd.data import node_labels
    from echoglad_amd.topology import HierTopology, TopologySpec
    n = HierTopology(TopologySpec(frame, naux)).num_nodes
    pred = (rng.standard_normal((batch, n, 4)) * 1.5).astype(np.float32)
    grid = []
    for _ in range(batch):
        coords = rng.integers(0, frame, size=(4, 2))
        lab = np.stack([node_labels(c, frame, naux) for c in coords], axis=1)        # [grid rows, 4]
        y = np.zeros((n, 4), dtype=np.float32)
        y[:lab.shape[0]] = lab
        grid.append(y)
    y = np.stack(grid)
    valid = np.broadcast_to((rng.random((batch, 1, 4)) < 0.7).astype(np.float32), (batch, n, 4)).copy()
    valid[0, :, 0] = 1.0                                                                  # at least one labelled channel
    return pred.reshape(-1, 4), y.reshape(-1, 4), valid.reshape(-1, 4)


def case_inputs(kind, seed, rows, channels):
    """(pred, y, valid) float32 [rows, channels] of one update (for "frames": rows = the number of frames)."""
    rng = np.random.default_rng(seed)
    if kind == "frames":
        return _frames(rng, rows)
    r, c = rows, channels
    pred = (rng.standard_normal((r, c)) * 1.5).astype(np.float32)
    y = (rng.random((r, c)) < 0.3).astype(np.float32)
    valid = (rng.random((r, c)) < 0.8).astype(np.float32)
    if kind == "novalid":
        valid[:, 1] = 0.0                                      # no valid row: the channel scores 0
    elif kind == "negonly":
        y[:] = 0.0                                             # no positive label: TNR (channels 0-2) ...
        pred[:, 3] = -np.abs(pred[:, 3])                       # ... and 1.0 where no prediction is positive either
    elif kind == "allpos":
        y[:] = 1.0                                             # TPR only
    elif kind == "threshold":
        vals = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0)), -0.5],
                        dtype=np.float32)
        pred = vals[rng.integers(0, 4, size=(r, c))]
    elif kind == "nan":
        pred[rng.random((r, c)) < 0.2] = np.nan
        pred[0, :] = np.inf
        pred[1, :] = -np.inf
    elif kind == "halfvalid":
        valid *= np.float32(0.5)                               # 0.5 counts as valid
    elif kind == "one":
        valid[:] = 1.0
    elif kind not in ("random", "ragged"):
        raise KeyError(kind)
    return np.ascontiguousarray(pred), np.ascontiguousarray(y), np.ascontiguousarray(valid)


def input_digest(pred, y, valid) -> str:
    h = hashlib.sha256()
    for a in (pred, y, valid):
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def numpy_counts(pred, y, valid) -> np.ndarray:
    """[C, 4] int64 {TP, FN, FP, TN} over the rows with valid > 0 (prediction: pred > 0.5; label: y != 0)."""
    v, pos = valid > 0, y != 0
    with np.errstate(invalid="ignore"):
        pp = pred > 0.5
    return np.stack([(v & pos & pp).sum(0), (v & pos & ~pp).sum(0), (v & ~pos & pp).sum(0), (v & ~pos & ~pp).sum(0)],
                    axis=-1).astype(np.int64)


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    tv = mod("torchvision")
    tv.models = mod("torchvision.models")
    try:
        import matplotlib  # noqa: F401
    except Exception:
        mp = mod("matplotlib")
        mp.pyplot = mod("matplotlib.pyplot", new_figure_manager=None)


def main():
    import warnings
    import torch
    _install_stubs()
    sys.path.insert(0, REF)
    from src.core import evaluators as RE     # reference code, executed not copied
    from sklearn.metrics import balanced_accuracy_score
    for name, updates in CASES.items():
        ev = RE.BalancedBinaryAccuracyEvaluator(logger=None)
        ev.reset()
        digests, counts, shapes = [], [], []
        for kind, seed, rows, ch in updates:
            pred, y, valid = case_inputs(kind, seed, rows, ch)
            digests.append(input_digest(pred, y, valid))
            counts.append(numpy_counts(pred, y, valid))
            shapes.append(pred.shape)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                # sklearn: "y_pred contains classes not in y_true"
                if pred.shape[0] > 1:
                    ev.update(torch.from_numpy(pred), torch.from_numpy(y), torch.from_numpy(valid))
                else:
                    # R = 1: the reference's update raises -- numpy takes the one-element torch bool mask valid[:, idx] > 0 as
                    # the integer index 1.  The row it means: the same sklearn call on the numpy mask, appended the same way.
                    row = np.asarray([balanced_accuracy_score(y_true=y[:, i][valid[:, i] > 0], y_pred=pred[:, i][valid[:, i] > 0] > 0.5)
                                      if np.count_nonzero(valid[:, i]) > 0 else 0 for i in range(ch)]).reshape((1, -1))
                    ev.score_per_class = row if ev.score_per_class is None else np.append(ev.score_per_class, row, axis=0)
        spc = np.asarray(ev.score_per_class, dtype=np.float64)
        np.savez_compressed(
            os.path.join(HERE, f"balacc_{name}.npz"),
            kinds=np.array([u[0] for u in updates]), seeds=np.array([u[1] for u in updates], dtype=np.int64),
            args=np.array([[u[2], u[3]] for u in updates], dtype=np.int64), shapes=np.array(shapes, dtype=np.int64),
            digests=np.array(digests), counts=np.stack(counts), score_per_class=spc,
            score_dtype=np.array(str(ev.score_per_class.dtype)),
            compute=np.float64(ev.compute()), per_class=np.asarray(ev.get_per_class_score(), dtype=np.float64),
            last=np.float64(ev.get_last()))
        print(name, spc.shape, float(ev.compute()), np.round(spc, 4).tolist()[:3])


if __name__ == "__main__":
    main()
