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


def _host_or_device_table(name):
    """A list-of-values table of the landmark evaluator: the host's own dictionary (host mode), or read back from the device history
    when accessed (device mode, read-only)."""
    def get(self):
        if self.max_updates is None:
            return self.__dict__["_" + name]
        return self._tables()[name]

    def set(self, value):
        if self.max_updates is not None:
            raise AttributeError(f"{name} is read back from the device history in device mode (max_updates = {self.max_updates})")
        self.__dict__["_" + name] = value
    return property(get, set)


class LandmarkExpectedCoordiantesEvaluator(object):
    """Same constructor, methods and recorded numbers as the reference class (evaluators.py:237-617).

    ``max_updates=None`` (host mode): the records are host lists, appended by ``update`` after three small read-backs.
    ``max_updates=N`` (device mode): ``update`` appends one record -- coordinate errors, valid flags, width MAE / MPE and the per-frame
    detail ``get_predictions`` returns -- to a device-side history of N records with two launches (heat-map models: the main grid's
    decode and the record, csrc/heatmap.hip) or one (coordinate-graph models): no host synchronisation, no allocation, so an update
    can be captured into a HIP graph (every replay appends a record).  The history is sized at construction on the current CUDA
    device (an update on another device re-sizes it only while nothing has been recorded).  ``coordinate_errors``,
    ``valid_errors``, ``width_MAE`` and ``width_MPE`` are read back when accessed, with the host mode's shape; ``compute``,
    ``get_last``, ``get_sum_of_width_MAE / MPE`` and ``get_predictions`` read back once per call.  Past N the records are dropped
    and reading raises.  ``pix2mm_x / pix2mm_y`` may be CPU tensors eagerly (copied into a device buffer); under a stream capture
    they must be device tensors."""

    coordinate_errors = _host_or_device_table("coordinate_errors")
    valid_errors = _host_or_device_table("valid_errors")
    width_MAE = _host_or_device_table("width_MAE")
    width_MPE = _host_or_device_table("width_MPE")

    def __init__(self, logger, batch_size, frame_size, use_coord_graph, max_updates=None):
        if max_updates is not None and int(max_updates) < 1:
            raise ValueError("max_updates must be >= 1 (or None: host mode)")
        self.batch_size = batch_size
        self.frame_size = frame_size
        self.use_coord_graph = use_coord_graph
        self.max_updates = None if max_updates is None else int(max_updates)
        self._state = None               # device mode: (device, history [N,16] f32, detail [N,B,24] f32, counter [1] i64, workspace, pix [2,B])
        self._snapshot = None            # device mode: the tables of one read-back, while a method that reads them several times runs
        self.detailed_performance = {}
        if self.max_updates is not None and torch.cuda.is_available():
            self._allocate(torch.device("cuda", torch.cuda.current_device()))
        self.reset()

    def reset(self):
        if self.max_updates is not None:
            if self._state is not None:
                self._state[3].zero_()
            return
        self.coordinate_errors = {k: [] for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")}
        self.valid_errors = {k: [] for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")}
        self.width_MAE = {k: [] for k in ("lvid", "ivs", "lvpw")}
        self.width_MPE = {k: [] for k in ("lvid", "ivs", "lvpw")}
        self.detailed_performance.clear()

    def update(self, y_pred, y_true, pix2mm_x, pix2mm_y, valid):
        """evaluators.py:291-391.  y_pred / y_true / valid: [B * nodes, 4] (device tensors are decoded on the device)."""
        if self.max_updates is not None:
            return self._update_device(y_pred, y_true, pix2mm_x, pix2mm_y, valid)
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
        with self._one_read_back():
            return self._compute()

    def _compute(self):
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
        with self._one_read_back():
            t = {k: self.coordinate_errors[k][-1] for k in NAMES}
            for k in ("ivs", "lvid", "lvpw"):
                t[k + "_w"] = self.width_MAE[k][-1]
                t[k + "_mpe"] = self.width_MPE[k][-1]
            return t

    def get_predictions(self):
        if self.max_updates is None:
            return self.detailed_performance
        n = self._count()
        if n == 0:
            return {}
        d = self._state[2][n - 1].cpu()                              # [B, 24]
        preds, gt = d[:, 0:8].reshape(-1, 4, 2), d[:, 8:16].reshape(-1, 4, 2)
        widths = {}
        for tag, base in (("pred", 16), ("gt", 19)):
            for j, k in enumerate(("ivs", "lvid", "lvpw")):
                widths[f"{tag}_{k}_mm"] = d[:, base + j].clone()
        coordinates = {"pred_ivs": preds[:, 3], "pred_lvid_top": preds[:, 0], "pred_lvid_bot": preds[:, 1], "pred_lvpw": preds[:, 2],
                       "gt_ivs": gt[:, 3], "gt_lvid_top": gt[:, 0], "gt_lvid_bot": gt[:, 1], "gt_lvpw": gt[:, 2]}
        return {"widths": widths, "coordinates": coordinates}

    # ---- the heat-map figure (evaluators.py:485-616), both modes: rendered on the device by ops.heatmap_render -----------------------
    def _logit_rows(self, t, name, frames=None):
        """`t` as device float32 [frames * rows, 4] holding an F x F main grid per frame -> (rows, frames, the main grid's level)."""
        F = self.frame_size
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA (ROCm) tensor: the heat maps are rendered on the device, there is no CPU fallback")
        if t.shape[-1] != 4:
            raise ValueError(f"{name} must end in the 4 landmark channels, got {tuple(t.shape)}")
        if frames is None:
            frames = t.shape[0] if t.dim() == 3 else self.batch_size
        rows = t.detach().reshape(-1, 4).to(torch.float32).contiguous()
        if rows.shape[0] % frames or rows.shape[0] // frames < F * F:
            raise ValueError(f"{rows.shape[0]} rows of {name} are not {frames} frames holding a {F} x {F} main grid each")
        return rows, frames, (rows.shape[0] // frames - F * F, F)

    def get_softmaxed_heatmap(self, y_pred):
        """evaluators.py:485-495 on the device: y_pred [N, rows, 4] or [N * rows, 4] (then N is the evaluator's batch size), a CUDA
        tensor -> the softmax over the main grid's rows as a CUDA float32 [N, F, F, 4] (eg_heatmap_render: exp(x - M) / S with the
        decode kernel's (M, S); a channel without a finite logit is 0 everywhere).  Nothing is read back."""
        rows, n, level = self._logit_rows(y_pred, "y_pred")
        return ops.heatmap_render(rows, n, level, 0, n, want=("heat",))["heat"]

    def get_overlays(self, x, landmark_preds, landmark_y, first=0, count=1):
        """The overlay images of frames first .. first + count - 1 as CUDA uint8 [count, F, F, 3] (HWC, what ToPILImage yields):
        {"pred_img": the frame under the per-channel normalised softmax heat maps, "gt_img": under the label heat maps, "coord_img":
        the frame alone -- what the reference's overlay of an all-zero heat map is (evaluators.py:545)}.  x: CUDA [B, C, F, F], channel
        0 is drawn (0.8 x grey); landmark_preds / landmark_y: the heat-map logits and labels [B * rows, 4] -- also with
        use_coord_graph, where the coordinate predictions enter the figure only as markers.  One decode pass for (max, sum exp) and one
        render launch (ops.heatmap_render), no host read-back and no matplotlib.
        The reference's ``create_overlay_image(x, hms)`` on host tensors is not provided: it would be a torch fallback of this."""
        B, F = self.batch_size, self.frame_size
        lg, _, level = self._logit_rows(landmark_preds, "landmark_preds", B)
        lb, _, _ = self._logit_rows(landmark_y, "landmark_y", B)
        if lb.shape != lg.shape:
            raise ValueError(f"landmark_y holds {lb.shape[0]} rows, landmark_preds {lg.shape[0]}")
        if not x.is_cuda or x.dim() != 4 or x.shape[0] != B or tuple(x.shape[-2:]) != (F, F):
            raise ValueError(f"x must be a CUDA tensor [{B}, C, {F}, {F}], got {tuple(x.shape)}")
        r = ops.heatmap_render(lg, B, level, first, count, labels=lb, image=x.detach().to(torch.float32).contiguous(),
                               want=("pred", "gt", "base"))
        return {"pred_img": r["pred"], "gt_img": r["gt"], "coord_img": r["base"]}

    def get_heatmaps(self, x, landmark_preds, landmark_y, coord_preds, pix2mm_x, pix2mm_y):
        """evaluators.py:497-593: the figure of frame 0 of the batch of the last ``update`` -- one panel per group ("pred", "gt"; with
        coord_preds "pred", "coord", "gt"): the overlay image, a white x per landmark, the IVS and LVPW segments in blue and the LVID
        segment in red, the widths in mm as the panel's title, the width MAE / MPE of the frame as the figure's.  The images come from
        ``get_overlays(count=1)`` (three 3 F^2-byte read-backs), the numbers from ``get_predictions()``; matplotlib draws on the host."""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("LandmarkExpectedCoordiantesEvaluator.get_heatmaps draws its figure with matplotlib, which is not "
                              "installed (get_overlays returns the images without it)") from e
        record = self.get_predictions()
        if not record:
            raise RuntimeError("get_heatmaps shows the predictions of the last update(): there is none since the last reset()")
        images = {k: v[0].cpu().numpy() for k, v in self.get_overlays(x, landmark_preds, landmark_y, 0, 1).items()}
        widths = {k: v[0] for k, v in record["widths"].items()}
        mae = self.calculate_width_MAE(widths)
        mpe = self.calculate_width_MPE(widths)
        points = {k: v[0].tolist() for k, v in record["coordinates"].items()}
        groups = ("pred", "gt")
        if coord_preds is not None:
            c = coord_preds.detach().reshape(self.batch_size, -1, 2)[0].to(torch.float32).cpu()
            px, py = pix2mm_x.detach().reshape(-1)[0].cpu(), pix2mm_y.detach().reshape(-1)[0].cpu()
            for k, name in enumerate(NAMES):
                points["coord_" + name] = c[k].tolist()
            # (the reference passes (h, w) here where calculate_widths passes (w, h): pix2mm_x scales the h difference -- kept)
            for name, (i, j) in (("ivs", (3, 0)), ("lvid", (0, 1)), ("lvpw", (1, 2))):
                widths[f"coord_{name}_mm"] = pixel_length(c[i, 0], c[i, 1], c[j, 0], c[j, 1], px, py)
            groups = ("pred", "coord", "gt")
        fig, axs = plt.subplots(1, len(groups), figsize=(4 * len(groups), 5))
        for ax, g in zip(axs, groups):
            ax.imshow(images[g + "_img"])
            for name in NAMES:
                ax.plot(points[f"{g}_{name}"][1], points[f"{g}_{name}"][0], marker="x", color="white", markersize=4)
            for a, b, colour in (("ivs", "lvid_top", "dodgerblue"), ("lvid_bot", "lvpw", "dodgerblue"), ("lvid_top", "lvid_bot", "red")):
                pa, pb = points[f"{g}_{a}"], points[f"{g}_{b}"]
                ax.plot([pa[1], pb[1]], [pa[0], pb[0]], color=colour, linewidth=1.5)
            ax.set_title(self.heatmap_panel_title(g, widths))
        plt.setp(axs[1].get_yticklabels(), visible=False)
        fig.tight_layout()
        fig.suptitle("MAE [mm] | IVS: {:.1f} | LVID: {:.1f} | LVPW: {:.1f}\nMPE [%] | IVS: {:.1f} | LVID: {:.1f} | LVPW: {:.1f}"
                     .format(*(float(v) for v in mae + mpe)))
        return fig

    @staticmethod
    def heatmap_panel_title(group, widths):
        """The title of one panel of get_heatmaps: the group's three widths in mm (evaluators.py:578-580)."""
        return "{}: [{:.1f}, {:.1f}, {:.1f}]".format(group, *(float(widths[f"{group}_{k}_mm"]) for k in ("ivs", "lvid", "lvpw")))

    # ---- device mode --------------------------------------------------------------------------------------------------------------
    def _allocate(self, device):
        B, N = self.batch_size, self.max_updates
        history = torch.zeros(N, ops.LANDMARK_RECORD_FLOATS, dtype=torch.float32, device=device)
        detail = torch.zeros(N, B, ops.LANDMARK_DETAIL_FLOATS, dtype=torch.float32, device=device)
        counter = torch.zeros(1, dtype=torch.int64, device=device)
        workspace = None
        if not self.use_coord_graph:
            workspace = torch.empty(ops.landmark_record_workspace_bytes(B, self.frame_size), dtype=torch.uint8, device=device)
        pix = torch.zeros(2, B, dtype=torch.float32, device=device)
        self._state = (device, history, detail, counter, workspace, pix)

    def _device_pix(self, t, k, device, capturing):
        """pix2mm_x (k = 0) / pix2mm_y (k = 1) as a device float32 [B] tensor."""
        B = self.batch_size
        if t.numel() != B:
            raise ValueError(f"pix2mm_{'xy'[k]} has {t.numel()} values but the evaluator's batch size is {B}")
        if t.is_cuda:
            if t.device != device:
                raise ValueError(f"pix2mm_{'xy'[k]} is on {t.device}, the predictions on {device}")
            return t.detach().reshape(B).to(torch.float32).contiguous()
        if capturing:
            raise ValueError(f"pix2mm_{'xy'[k]} is a CPU tensor: under a stream capture pix2mm_x / pix2mm_y must already be device "
                             "tensors (a host-to-device copy cannot be part of the captured graph)")
        buf = self._state[5][k]
        buf.copy_(t.detach().reshape(B), non_blocking=True)
        return buf

    def _update_device(self, y_pred, y_true, pix2mm_x, pix2mm_y, valid):
        B, F = self.batch_size, self.frame_size
        if not y_pred.is_cuda:
            raise RuntimeError("y_pred must be a CUDA (ROCm) tensor: the device-history mode has no CPU fallback")
        capturing = torch.cuda.is_current_stream_capturing()
        st = self._state
        if st is None or st[0] != y_pred.device:
            if capturing:
                raise RuntimeError("the evaluator's device history is not allocated on the capturing device: update it once eagerly "
                                   "in front of the capture")
            if st is not None and int(st[3].item()):
                raise RuntimeError(f"this evaluator records on {st[0]}: got predictions on {y_pred.device} (reset() first)")
            self._allocate(y_pred.device)
            st = self._state
        dev, history, detail, counter, workspace, _ = st
        px = self._device_pix(pix2mm_x, 0, dev, capturing)
        py = self._device_pix(pix2mm_y, 1, dev, capturing)
        if self.use_coord_graph:
            cp = y_pred.detach().reshape(-1).to(torch.float32).contiguous()
            cy = y_true.detach().reshape(-1).to(torch.float32).contiguous()
            if cp.numel() != B * 8 or cy.numel() != B * 8:
                raise ValueError(f"coordinate predictions / targets hold {cp.numel() // 8} / {cy.numel() // 8} frames of 4 (h, w) pairs "
                                 f"but the evaluator's batch size is {B}")
            ops.landmark_record_coord(cp, cy, B, px, py, history, detail, counter)
            return
        lg = y_pred.detach().reshape(-1, 4).to(torch.float32).contiguous()
        if lg.shape[0] % B or lg.shape[0] // B < F * F:
            raise ValueError(f"{lg.shape[0]} logit rows are not {B} frames holding a {F} x {F} main grid each "
                             f"(the evaluator's batch size is {B})")
        yy = y_true.detach().reshape(-1, 4).to(torch.float32).contiguous()
        vv = valid.detach().reshape(-1, 4).to(torch.float32).contiguous()
        ops.landmark_record_hm(lg, yy, vv, B, F, px, py, history, detail, counter, workspace)

    def _count(self) -> int:
        """Records appended since the last reset() (host read-back); raises past max_updates."""
        if self._state is None:
            return 0
        n = int(self._state[3].item())
        if n > self.max_updates:
            raise RuntimeError(f"{n} updates since the last reset() but the history holds max_updates = {self.max_updates}: "
                               "construct the evaluator with a larger max_updates")
        return n

    def _tables(self):
        if self._snapshot is not None:
            return self._snapshot
        n = self._count()
        h = self._state[1][:n].cpu().numpy() if n else np.zeros((0, ops.LANDMARK_RECORD_FLOATS), np.float32)
        return {"coordinate_errors": {k: list(h[:, NAMES.index(k)]) for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")},
                "valid_errors": {k: [bool(v) for v in h[:, 4 + NAMES.index(k)] > 0] for k in ("ivs", "lvid_top", "lvid_bot", "lvpw")},
                "width_MAE": {k: [float(v) for v in h[:, 8 + ("ivs", "lvid", "lvpw").index(k)]] for k in ("lvid", "ivs", "lvpw")},
                "width_MPE": {k: [float(v) for v in h[:, 11 + ("ivs", "lvid", "lvpw").index(k)]] for k in ("lvid", "ivs", "lvpw")}}

    def _one_read_back(self):
        """Context: device mode reads the history back once for the whole block (host mode: nothing)."""
        import contextlib
        if self.max_updates is None or self._snapshot is not None:
            return contextlib.nullcontext()

        @contextlib.contextmanager
        def snap():
            self._snapshot = self._tables()
            try:
                yield
            finally:
                self._snapshot = None
        return snap()


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


def build(eval_config, logger=None, max_updates=None):
    """src/builders/evaluator_builder.py: {standard: evaluator} for ``eval_config['standards']``.  The keys ``batch_size``,
    ``frame_size`` and ``use_coordinate_graph`` configure the landmark evaluator; ``max_updates`` (None: host mode) selects its
    device-history mode with that many records (``GraphedEvalStep`` captures only that mode)."""
    standards = list(eval_config["standards"])
    batch_size, frame_size = eval_config["batch_size"], eval_config["frame_size"]
    use_coord_graph = eval_config["use_coordinate_graph"]
    evaluators = {}
    for standard in standards:
        if standard == "balancedaccuracy":
            evaluators[standard] = BalancedBinaryAccuracyEvaluator(logger=logger)
        elif standard == "landmarkcoorderror":
            evaluators[standard] = LandmarkExpectedCoordiantesEvaluator(logger=logger, batch_size=batch_size,
                                                                        frame_size=frame_size, use_coord_graph=use_coord_graph,
                                                                        max_updates=max_updates)
        elif standard in _UNREACHABLE:
            raise NotImplementedError(f"evaluator {standard!r} is not implemented: its update(y_pred, y_true) takes two arguments and "
                                      "the reference's engine calls every evaluator with three or five (src/engine.py:492), so the "
                                      "reference cannot run it either")
        else:
            raise KeyError(f"unknown evaluation standard {standard!r}")
        if logger is not None and hasattr(logger, "infov"):
            logger.infov("{} evaluator is built.".format(standard.upper()))
    return evaluators
