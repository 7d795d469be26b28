"""The evaluators of the reference's engine (src/core/evaluators.py, src/builders/evaluator_builder.py) over HIP kernels.

``LandmarkExpectedCoordiantesEvaluator`` -- landmark decode and width errors, host-side mirror of evaluators.py:237-617 (the
class name keeps the reference's spelling so a builder can swap it in) over the HIP decode kernel in csrc/heatmap.hip (SURVEY §8
row f-3).  The reference moves the full logits to the host every step (engine.py:466-492) and evaluates the softmax heat map
there.  Here the logits stay on the device: one kernel pass yields, per frame and landmark, the softmax-expected (h, w) over the
last F*F rows, the label's (h, w) and the mean of ``valid``; only those [B,4,*] numbers are read back.

``BalancedBinaryAccuracyEvaluator`` -- the default config's ``eval.standard`` (evaluators.py:85-143).  The reference runs four
sklearn calls on host copies of the logits, labels and valid every update; here one launch (csrc/metrics.hip) appends the
per-channel confusion counts to a device-side history, and the scores are formed from the counts on the host when read.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

NAMES = ("lvid_top", "lvid_bot", "lvpw", "ivs")


def decode_landmarks(logits: torch.Tensor, batch_size: int, frame_size: int, labels=None, valid=None):
    """Device-side decode of the main-grid heat maps (the last F*F rows of every frame).

    Returns dict: expect [B,4,2] softmax-expected (h, w); argmax [B,4] hard arg max row index (h * F + w);
    gt [B,4,2] / vmean [B,4] when labels / valid are given."""
    lg = logits.reshape(-1, logits.shape[-1]).to(torch.float32).contiguous()
    n_rows = lg.shape[0] // batch_size
    level = [(n_rows - frame_size * frame_size, frame_size)]
    prep = (lambda t: None if t is None else t.reshape(-1, t.shape[-1]).to(torch.float32).contiguous())
    r = ops.heatmap_expect_fwd(lg, batch_size, level, prep(labels), prep(valid), want_argmax=True)
    return {"expect": r["expect"][:, 0], "argmax": r["argmax"][:, 0],
            "gt": None if r["gt"] is None else r["gt"][:, 0], "vmean": None if r["vmean"] is None else r["vmean"][:, 0]}


def pixel_length(x0, y0, x1, y1, pix2mm_x, pix2mm_y):
    """evaluators.py:619-620."""
    return torch.sqrt(((x0 - x1) * pix2mm_x) ** 2 + ((y0 - y1) * pix2mm_y) ** 2)


class LandmarkExpectedCoordiantesEvaluator(object):
    """Same constructor, methods and recorded numbers as the reference class (evaluators.py:237-617)."""

    def __init__(self, logger, batch_size, frame_size, use_coord_graph):
        self.batch_size = batch_size
        self.frame_size = frame_size
        self.use_coord_graph = use_coord_graph
        self.detailed_performance = {}
        self.reset()

    def reset(self):
        self.coordinate_errors = {k: [] for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")}
        self.valid_errors = {k: [] for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")}
        self.width_MAE = {k: [] for k in ("lvid", "ivs", "lvpw")}
        self.width_MPE = {k: [] for k in ("lvid", "ivs", "lvpw")}
        self.detailed_performance.clear()

    def update(self, y_pred, y_true, pix2mm_x, pix2mm_y, valid):
        """evaluators.py:291-391.  y_pred / y_true / valid: [B * nodes, 4] (device tensors are decoded on the device)."""
        self.detailed_performance.clear()
        B, F = self.batch_size, self.frame_size
        if self.use_coord_graph:
            preds = y_pred.detach().reshape(-1, 4, 2).float().cpu()
            gt = y_true.detach().reshape(-1, 4, 2).float().cpu()
            # the reference uses valid_subset / num_valid_samples of the heat-map branch here and fails when they are
            # undefined (evaluators.py:352-354); every landmark of every frame counts as labelled in this branch
            vs = torch.ones(preds.shape[0], 4)
        else:
            d = decode_landmarks(y_pred.detach(), B, F, y_true.detach(), valid)
            preds, gt, vs = d["expect"].cpu(), d["gt"].cpu(), d["vmean"].cpu()
        pix2mm_x, pix2mm_y = pix2mm_x.detach().cpu().float(), pix2mm_y.detach().cpu().float()
        nv = vs.sum(dim=0, keepdim=True)
        for i, name in enumerate(NAMES):
            self.valid_errors[name].append(bool(nv[0, i] > 0))
        nv = torch.where(nv == 0, torch.ones_like(nv), nv)
        gt_h, gt_w, pr_h, pr_w = gt[:, :, 0], gt[:, :, 1], preds[:, :, 0], preds[:, :, 1]
        err = pixel_length(gt_w, gt_h, pr_w, pr_h, pix2mm_x.unsqueeze(1), pix2mm_y.unsqueeze(1)).numpy()
        err = np.squeeze(np.sum(err * vs.numpy(), axis=0) / nv.numpy())
        for i, name in enumerate(NAMES):
            self.coordinate_errors[name].append(err[i])
        widths = self.calculate_widths(preds, gt, pix2mm_x, pix2mm_y)
        w_lvid = vs[:, 0] * vs[:, 1] / torch.min(nv[0, 0], nv[0, 1])
        w_ivs = vs[:, 3] / nv[0, 3]
        w_lvpw = vs[:, 2] / nv[0, 2]
        ivs_e, lvid_e, lvpw_e = self.calculate_width_MAE(widths)
        self.width_MAE["ivs"].append((ivs_e * w_ivs).sum().item())
        self.width_MAE["lvid"].append((lvid_e * w_lvid).sum().item())
        self.width_MAE["lvpw"].append((lvpw_e * w_lvpw).sum().item())
        ivs_e, lvid_e, lvpw_e = self.calculate_width_MPE(widths)
        self.width_MPE["ivs"].append((ivs_e * w_ivs).sum().item())
        self.width_MPE["lvid"].append((lvid_e * w_lvid).sum().item())
        self.width_MPE["lvpw"].append((lvpw_e * w_lvpw).sum().item())
        coordinates = {"pred_ivs": preds[:, 3], "pred_lvid_top": preds[:, 0], "pred_lvid_bot": preds[:, 1],
                       "pred_lvpw": preds[:, 2], "gt_ivs": gt[:, 3], "gt_lvid_top": gt[:, 0], "gt_lvid_bot": gt[:, 1],
                       "gt_lvpw": gt[:, 2]}
        self.detailed_performance = {"widths": widths, "coordinates": coordinates}

    def calculate_widths(self, preds, gt, pix2mm_x, pix2mm_y):
        """evaluators.py:393-407: [N,4,2] (h, w) -> landmark-pair distances in mm."""
        def w3(c, tag):
            return {tag + "_ivs_mm": pixel_length(c[:, 3, 1], c[:, 3, 0], c[:, 0, 1], c[:, 0, 0], pix2mm_x, pix2mm_y),
                    tag + "_lvid_mm": pixel_length(c[:, 0, 1], c[:, 0, 0], c[:, 1, 1], c[:, 1, 0], pix2mm_x, pix2mm_y),
                    tag + "_lvpw_mm": pixel_length(c[:, 1, 1], c[:, 1, 0], c[:, 2, 1], c[:, 2, 0], pix2mm_x, pix2mm_y)}
        return {**w3(preds, "pred"), **w3(gt, "gt")}

    def calculate_width_MAE(self, widths):
        return (torch.abs(widths["pred_ivs_mm"] - widths["gt_ivs_mm"]), torch.abs(widths["pred_lvid_mm"] - widths["gt_lvid_mm"]),
                torch.abs(widths["pred_lvpw_mm"] - widths["gt_lvpw_mm"]))

    def calculate_width_MPE(self, widths):
        return tuple(100 * torch.abs(widths["pred_" + k] - widths["gt_" + k]) / widths["gt_" + k]
                     for k in ("ivs_mm", "lvid_mm", "lvpw_mm"))

    def compute(self):
        """evaluators.py:428-447: means over the recorded iterations, counting only iterations with a labelled landmark."""
        def cnt(*keys):
            m = np.asarray(self.valid_errors[keys[0]])
            for k in keys[1:]:
                m = np.logical_and(m, np.asarray(self.valid_errors[k]))
            return np.count_nonzero(m)
        t = {k: np.asarray(self.coordinate_errors[k]).sum() / cnt(k) for k in NAMES}
        t["ivs_w"] = np.asarray(self.width_MAE["ivs"]).sum() / cnt("ivs")
        t["lvid_w"] = np.asarray(self.width_MAE["lvid"]).sum() / cnt("lvid_top", "lvid_bot")
        t["lvpw_w"] = np.asarray(self.width_MAE["lvpw"]).sum() / cnt("lvpw")
        t["ivs_mpe"] = np.asarray(self.width_MPE["ivs"]).sum() / cnt("ivs")
        t["lvid_mpe"] = np.asarray(self.width_MPE["lvid"]).sum() / cnt("lvid_top", "lvid_bot")
        t["lvpw_mpe"] = np.asarray(self.width_MPE["lvpw"]).sum() / cnt("lvpw")
        return t

    def get_sum_of_width_MAE(self):
        t = self.compute()
        return sum(v for k, v in t.items() if k in ("ivs_w", "lvid_w", "lvpw_w"))

    def get_sum_of_width_MPE(self):
        t = self.compute()
        return sum(v for k, v in t.items() if k in ("ivs_mpe", "lvid_mpe", "lvpw_mpe"))

    def get_last(self):
        t = {k: self.coordinate_errors[k][-1] for k in NAMES}
        for k in ("ivs", "lvid", "lvpw"):
            t[k + "_w"] = self.width_MAE[k][-1]
            t[k + "_mpe"] = self.width_MPE[k][-1]
        return t

    def get_predictions(self):
        return self.detailed_performance


LandmarkExpectedCoordinatesEvaluator = LandmarkExpectedCoordiantesEvaluator


def balanced_accuracy_from_counts(counts) -> np.ndarray:
    """[..., C, 4] confusion counts {TP, FN, FP, TN} -> [..., C] float64 balanced accuracies with sklearn's arithmetic
    (sklearn.metrics.balanced_accuracy_score, adjusted=False): recall = diag / row sum of every class that has support among
    the valid rows (a class present only in the predictions is 0/0 and dropped), the score is the mean of those recalls; a
    channel without a valid row scores 0 (evaluators.py:137-141)."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim < 2 or c.shape[-1] != 4:
        raise ValueError(f"counts must be [..., C, 4], got {c.shape}")
    tp, fn, fp, tn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    neg, pos = tn + fp, tp + fn                              # row sums of the confusion matrix: support of class 0, class 1
    with np.errstate(divide="ignore", invalid="ignore"):
        r0 = tn / neg                                        # recall of class 0 (sorted first, as sklearn's labels are)
        r1 = tp / pos
    # np.mean of [r0, r1] is (0 + r0 + r1) / 2, of [r] is r / 1: the same bits as the expressions below
    both = (r0 + r1) / 2
    return np.where((neg > 0) & (pos > 0), both, np.where(neg > 0, r0, np.where(pos > 0, r1, 0.0))).astype(np.float64)


class BalancedBinaryAccuracyEvaluator(object):
    """Same constructor, methods and numbers as the reference class (evaluators.py:85-143), over device-side counting.

    ``update(y_pred, y_true, valid)`` takes CUDA tensors [rows, C] (float32, contiguous; 1 <= C <= 8) and appends one record of
    confusion counts per call with ONE kernel launch: it neither synchronises nor allocates, so it can be captured into a HIP
    graph (every replay appends a record).  The history holds ``max_updates`` records, sized once (at construction on the current
    CUDA device for ``channels`` channels; an update on another device or with another channel count re-sizes it only while
    nothing has been recorded).  Past ``max_updates`` the records are dropped and reading the scores raises.
    ``score_per_class`` (None before the first update, else [N, C] float64) is read back from the device when accessed."""

    def __init__(self, logger, max_updates: int = 65536, channels: int = 4):
        if max_updates < 1:
            raise ValueError("max_updates must be >= 1")
        self.max_updates = int(max_updates)
        self._state = None               # (device, channels, history [max_updates, C, 4] i64, counter [1] i64, workspace u8)
        self._launched = 0               # update() calls since the state was allocated or reset (host side)
        if torch.cuda.is_available():
            self._allocate(torch.device("cuda", torch.cuda.current_device()), channels)

    def _allocate(self, device, channels):
        history = torch.zeros(self.max_updates, channels, 4, dtype=torch.int64, device=device)
        counter = torch.zeros(1, dtype=torch.int64, device=device)
        workspace = torch.empty(ops.CONFUSION_WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        self._state = (device, channels, history, counter, workspace)
        self._launched = 0

    def reset(self):
        if self._state is not None:
            self._state[3].zero_()
        self._launched = 0

    def update(self, y_pred, y_true, valid):
        """evaluators.py:100-117.  y_pred: the model's output [rows, C] (threshold: > 0.5 on it as it is); y_true: {0, 1} labels."""
        ch = y_pred.shape[-1]
        pred, y, v = (t.detach().reshape(-1, ch) for t in (y_pred, y_true, valid))
        st = self._state
        if st is None or st[0] != pred.device or st[1] != ch:
            if not pred.is_cuda:
                raise RuntimeError("y_pred must be a CUDA (ROCm) tensor: the HIP path has no CPU fallback")
            if st is not None and self._launched:
                raise RuntimeError(f"this evaluator records {st[1]} channels on {st[0]}: got {ch} on {pred.device} (reset() first)")
            self._allocate(pred.device, ch)
            st = self._state
        ops.confusion_counts(pred, y, v, st[2], st[3], st[4])
        self._launched += 1

    def counts(self):
        """[N, C, 4] int64 numpy array of the recorded {TP, FN, FP, TN} (host read-back; None before the first update)."""
        if self._state is None:
            return None
        history, counter = self._state[2], self._state[3]
        n = int(counter.item())
        if n > self.max_updates:
            raise RuntimeError(f"{n} updates since the last reset() but the history holds max_updates = {self.max_updates}: "
                               "construct the evaluator with a larger max_updates")
        if n == 0:
            return None
        return history[:n].cpu().numpy()

    @property
    def score_per_class(self):
        c = self.counts()
        return None if c is None else balanced_accuracy_from_counts(c)

    def compute(self):
        """evaluators.py:119-124."""
        return self.score_per_class.mean(axis=0).mean()

    def get_per_class_score(self):
        return self.score_per_class.mean(axis=0)

    def get_last(self):
        return self.score_per_class[-1, :].mean()


_UNREACHABLE = ("accuracy", "mse", "landmarkerror")


def build(eval_config, logger=None):
    """src/builders/evaluator_builder.py: {standard: evaluator} for ``eval_config['standards']``.  The keys ``batch_size``,
    ``frame_size`` and ``use_coordinate_graph`` configure the landmark evaluator."""
    standards = list(eval_config["standards"])
    batch_size, frame_size = eval_config["batch_size"], eval_config["frame_size"]
    use_coord_graph = eval_config["use_coordinate_graph"]
    evaluators = {}
    for standard in standards:
        if standard == "balancedaccuracy":
            evaluators[standard] = BalancedBinaryAccuracyEvaluator(logger=logger)
        elif standard == "landmarkcoorderror":
            evaluators[standard] = LandmarkExpectedCoordiantesEvaluator(logger=logger, batch_size=batch_size,
                                                                        frame_size=frame_size, use_coord_graph=use_coord_graph)
        elif standard in _UNREACHABLE:
            raise NotImplementedError(f"evaluator {standard!r} is not implemented: its update(y_pred, y_true) takes two arguments and "
                                      "the reference's engine calls every evaluator with three or five (src/engine.py:492), so the "
                                      "reference cannot run it either")
        else:
            raise KeyError(f"unknown evaluation standard {standard!r}")
        if logger is not None and hasattr(logger, "infov"):
            logger.infov("{} evaluator is built.".format(standard.upper()))
    return evaluators
