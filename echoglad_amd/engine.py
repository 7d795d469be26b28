"""One training / evaluation step over the HIP path — host-side counterpart of the inner loops of the reference's
``Engine`` (src/engine.py:239-273 train step, :394-398 eval forward, :582-600 ``compute_loss``): embed the frames,
run the landmark model, sum the criteria, backward, (data-parallel gradient all-reduce,) optimizer step, update the
evaluators.  Logging, checkpointing and wandb of the reference are out of scope.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import torch

from .parallel import GradientAllReducer


class MSE:
    """criterion.py:36-48 (the 'coordinate' criterion of the coordinate-graph configs)."""

    def __init__(self, loss_weight=1):
        self.loss_weight = loss_weight

    def compute(self, pred_y, y):
        return self.loss_weight * torch.nn.functional.mse_loss(pred_y, y)


class MAE:
    """criterion.py:51-63."""

    def __init__(self, loss_weight=1):
        self.loss_weight = loss_weight

    def compute(self, pred_y, y):
        return self.loss_weight * torch.nn.functional.l1_loss(pred_y, y)


def compute_loss(criterion: Dict[str, object], node_landmark_preds, node_landmark_y, node_coord_preds, node_coord_y,
                 valid_labels, batch_size: int, num_output_channels: int = 4) -> Dict[str, torch.Tensor]:
    """engine.py:582-600: the 'coordinate' criterion sees the coordinate predictions, every other one the logits
    reshaped to [B, nodes, channels]."""
    if num_output_channels == 4:
        from .losses import fused_criteria
        fused = fused_criteria(criterion, node_landmark_preds, node_landmark_y, valid_labels, node_coord_preds, node_coord_y, batch_size)
        if fused is not None:                # one autograd node, 5 launches; ``.total`` is the sum out of the same node
            return fused
    losses = {}
    preds = node_landmark_preds.view(batch_size, -1, num_output_channels)
    y = node_landmark_y.view(batch_size, -1, num_output_channels)
    for name, crit in criterion.items():
        if name == "coordinate":
            losses[name] = crit.compute(node_coord_preds, node_coord_y)
        else:
            losses[name] = crit.compute(preds, y, valid_labels)
    return losses


def total_loss(losses) -> torch.Tensor:
    """engine.py:271: the sum of the criteria -- straight out of the fused node when compute_loss used it."""
    total = getattr(losses, "total", None)
    return total if total is not None else sum(losses.values())


def _device_labels(batch):
    """A batch of coordinate labels (``label_coords``, data.collate of ``labels="coords"`` samples): its dense ``y`` / ``valid_labels``
    are written on the device first -- one launch, a node of the graph when the step is being captured.  A batch of raw frames
    (``raw_frame``, ``frames="raw"`` samples) is prepared in front of that (``data.device_frames_``: x, and the label coordinates the
    expansion reads), so preparation -> labels are the first two nodes of a captured step."""
    if getattr(batch, "raw_frame", None) is not None:
        from .data import device_frames_
        device_frames_(batch)
    if getattr(batch, "label_coords", None) is not None:
        from .data import device_labels_
        device_labels_(batch)


def forward_batch(model: Dict[str, torch.nn.Module], batch, use_coordinate_graph: bool):
    """engine.py:239-255: frame embeddings, then the landmark model on the collated batch."""
    x = model["embedder"](batch.x)
    node_coords = batch.node_coords if use_coordinate_graph else None
    return model["landmark"](x=x, node_coords=node_coords, edge_index=batch.edge_index, batch_idx=batch.batch,
                             node_type=batch.node_type)


def train_step(model: Dict[str, torch.nn.Module], batch, criterion: Dict[str, object], optimizer, batch_size: int,
               use_coordinate_graph: bool = False, reducer: Optional[GradientAllReducer] = None, evaluators=None):
    """engine.py:239-291 for one batch.  ``reducer`` (parallel.GradientAllReducer) averages the gradients over the
    data-parallel ranks between backward and the optimizer step; it replaces torch_geometric's DataParallel
    (engine.py:105-110).  Returns (loss, losses dict, logits, coordinate predictions)."""
    _device_labels(batch)
    preds, coord_preds = forward_batch(model, batch, use_coordinate_graph)
    coord_y = batch.node_coord_y if use_coordinate_graph else None
    losses = compute_loss(criterion, preds, batch.y, coord_preds, coord_y, batch.valid_labels, batch_size)
    loss = total_loss(losses)
    optimizer.zero_grad()
    loss.backward()                 # with reducer.attach_hooks(): the buckets' all-reduces are issued from inside backward
    if reducer is not None:
        reducer.finish()
    optimizer.step()
    if evaluators:
        with torch.no_grad():
            update_evaluators(evaluators, preds, batch.y, coord_preds, coord_y, batch.pix2mm_x, batch.pix2mm_y,
                              batch.valid_labels, use_coordinate_graph)
    return loss.detach(), {k: v.detach() for k, v in losses.items()}, preds.detach(), coord_preds


class GraphedTrainStep:
    """One WHOLE training step -- forward, criteria, backward, optimizer update (engine.py:239-273 of the reference) -- captured
    once into a HIP graph and replayed: ~130 kernel launches per step leave the host as one.  At the reference's own batch size
    (configs/default.yml:27, ``batch_size: 1``) an eager step is bound by the host's launch rate (2.4 - 3.4 ms for 1.0 ms of GPU
    work); at batch 32 the GPU is the bound and a replay changes nothing.

    ``loss_fn()`` -> loss, or (loss, *tensors to keep): it must read its inputs from tensors that stay where they are (write a new
    batch INTO them before calling the step) and must not synchronise with the host; with coordinate labels it starts with
    ``data.device_labels_(static)``, which becomes a node of the graph.  Dropout: the seeds a train-mode forward
    draws on the host are frozen into the graph's kernel arguments, so the graph's first node bumps the device's dropout EPOCH
    (include/echoglad_hip.h: the kernels hash with seed + epoch) -- every replay draws fresh masks, its forward and backward see
    the same ones.  BatchNorm running statistics, ``num_batches_tracked`` and the optimizer's step count live on the device and
    advance with every replay.

    Single rank (``reducer`` None): the optimizer update is part of the graph, so ``optimizer`` has to be capturable
    (``torch.optim.Adam(..., capturable=True)``; ``fused=True`` as well for one launch).
    Data parallel (``reducer`` = a ``parallel.GradientAllReducer`` WITHOUT attached hooks): the graph holds forward + backward
    only; every call replays it, averages the gradients over the ranks with the reducer's hook-less ``allreduce()`` (a handful of
    RCCL collectives on ~280 KB: they are not captured) and runs ``optimizer.step()`` eagerly -- any optimizer will do.  The
    overlap of the collectives with backward that ``train_step`` + ``attach_hooks()`` gives is traded for the launch-free step:
    the trade pays where the step is host-bound (small per-rank batches), not at batch 32.

    ``warmup`` eager steps run first (on the capture stream, as torch.cuda.graph asks): they allocate every workspace, topology
    handle and the epoch word outside the capture -- and they ARE training steps."""

    def __init__(self, loss_fn, optimizer, warmup: int = 3, reducer: Optional[GradientAllReducer] = None):
        from . import ops
        if warmup < 1:
            raise ValueError("at least one eager warm-up step is needed (workspaces and handles are created by it)")
        if reducer is None:
            for group in optimizer.param_groups:
                if not group.get("capturable", False):
                    raise ValueError("GraphedTrainStep needs a capturable optimizer (e.g. torch.optim.Adam(params, capturable=True))")
        elif getattr(reducer, "_hooks", None):
            raise ValueError("GraphedTrainStep drives the reducer itself: pass a GradientAllReducer without attach_hooks() "
                             "(collectives fired from inside backward cannot be part of the captured graph)")
        self.loss_fn, self.optimizer, self.reducer = loss_fn, optimizer, reducer
        self.replays = 0
        self._written = [p for g in optimizer.param_groups for p in g["params"]]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                self.optimizer.zero_grad(set_to_none=True)
                self._forward_backward(ops, bump=False)
                self._update()
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        # with a reducer the process group's watchdog thread may still poll the event of the last warm-up all-reduce: under the
        # default "global" mode an event query from ANY thread during the capture is an error that terminates the process
        # (hipErrorStreamCaptureUnsupported raised inside the watchdog), so only this thread's calls are policed then
        mode = "global" if reducer is None else "thread_local"
        with torch.cuda.graph(self.graph, stream=stream, capture_error_mode=mode):
            self.outputs = self._forward_backward(ops, bump=True)
            if reducer is None:
                self.optimizer.step()

    def _forward_backward(self, ops, bump: bool):
        if bump:
            ops.dropout_epoch_add(1)
        out = self.loss_fn()
        loss = out[0] if isinstance(out, (tuple, list)) else out
        # (d loss = 1 from a tensor that exists already: autograd's own ones_like is a fill kernel -- one more node of every replay)
        one = getattr(self, "_one", None)
        if one is None or one.device != loss.device or one.dtype != loss.dtype or one.shape != loss.shape:
            one = self._one = torch.ones_like(loss)
        loss.backward(gradient=one)
        if isinstance(out, (tuple, list)):
            return tuple(t.detach() for t in out)
        return (loss.detach(),)

    def _update(self):
        if self.reducer is not None:
            self.reducer.allreduce()
        self.optimizer.step()

    def __call__(self):
        """Replay the step; returns the graph's static output tensors (loss first), valid until the next replay."""
        self.graph.replay()
        if self.reducer is not None:
            self._update()
        else:
            # a replay runs no host code: the in-place version counters of what the captured update wrote stand still -- and whatever
            # is cached on them (the model's folded inference parameters, its inference graphs) would not notice the step
            torch.autograd.graph.increment_version(self._written)
        self.replays += 1
        return self.outputs


def _state_key(module: torch.nn.Module) -> tuple:
    """What a captured graph over ``module`` depends on: every parameter's and buffer's in-place version and address."""
    return tuple((t._version, t.data_ptr()) for t in list(module.parameters()) + list(module.buffers()))


def _record_counter(ev):
    """The device record counter of a capturable evaluator (None before its history exists)."""
    st = ev._state
    return None if st is None else st[3]


class GraphedEvalStep:
    """One WHOLE evaluation step -- embedder, landmark model, criteria, every evaluator's update and the epoch's loss meter
    (engine.py:340-460 of the reference for one batch) -- captured once into a HIP graph and replayed.  The evaluation counterpart
    of ``GraphedTrainStep``; it covers coordinate-graph models, which the model-level ``enable_hip_graph`` replay does not.

    ``static_batch``: a collated batch on the device (``data.to_device``); write every new batch INTO it (``data.copy_batch_``) before
    calling the step; a static batch of coordinate labels (``label_coords``) has its dense labels rebuilt by the graph's first node
    (``data.device_labels_``), a static batch of raw frames (``raw_frame``) is prepared by the node in front of it
    (``data.device_frames_``).  ``pix2mm_x / pix2mm_y`` must be device tensors.  The graph reads ``static_batch.node_coords`` into a private
    buffer first: the caller's tensor is never written.  ``step()`` -> (preds, coord_preds, losses), the graph's static outputs, valid
    until the next call.  ``loss_avg()`` is the reference's ``loss_meter.avg`` (meters.AverageEpochMeter: an fp64 sum of
    ``total_loss * batch_size`` over an fp64 count, kept on the device and read back only there); ``reset_meter()`` zeroes it.

    Evaluators: ``BalancedBinaryAccuracyEvaluator`` and ``LandmarkExpectedCoordiantesEvaluator`` in device-history mode
    (``max_updates`` set): every replay appends one record to each.  Anything else is refused with ValueError, as are a model or
    embedder in training mode and ``warmup < 1``.

    ``warmup`` eager steps run first on the capture stream (they allocate the workspaces and the completion tickets there); their
    records and their meter updates are rolled back on the device, so afterwards no evaluator holds a warm-up record and the meter
    is where it was.  Parameter changes are honoured by RECAPTURE: the graph's kernels point at the model's folded BatchNorm
    parameters and packed heads, which the model caches on in-place version counters; every call compares the version and address
    of every parameter and buffer of both modules (and the model's cache entries) with the captured ones and captures again when
    anything moved -- an optimizer step, ``load_state_dict``, a ``GraphedTrainStep`` replay, a train() / eval() round trip.
    ``captures`` counts the captures."""

    def __init__(self, model: Dict[str, torch.nn.Module], static_batch, criterion: Optional[Dict[str, object]], batch_size: int,
                 use_coordinate_graph: bool = False, evaluators=None, warmup: int = 1):
        from .evaluators import BalancedBinaryAccuracyEvaluator, LandmarkExpectedCoordiantesEvaluator
        if warmup < 1:
            raise ValueError("at least one eager warm-up step is needed (workspaces and completion tickets are created by it)")
        for name in ("embedder", "landmark"):
            if model[name].training:
                raise ValueError(f"model[{name!r}] is in training mode: GraphedEvalStep captures an evaluation step (call .eval() first)")
        evaluators = dict(evaluators or {})
        for name, ev in evaluators.items():
            if isinstance(ev, LandmarkExpectedCoordiantesEvaluator) and ev.max_updates is None:
                raise ValueError(f"evaluator {name!r} is a host-mode LandmarkExpectedCoordiantesEvaluator, which reads its inputs back to "
                                 "the host and cannot be captured: construct it with max_updates (evaluators.build(..., max_updates=N))")
            if not isinstance(ev, (BalancedBinaryAccuracyEvaluator, LandmarkExpectedCoordiantesEvaluator)):
                raise ValueError(f"evaluator {name!r} ({type(ev).__name__}) cannot be captured into a HIP graph")
        if use_coordinate_graph and getattr(static_batch, "node_coords", None) is None:
            raise ValueError("a coordinate-graph step needs static_batch.node_coords")
        self.model, self.criterion, self.batch_size = model, criterion, int(batch_size)
        self.use_coordinate_graph, self.evaluators, self.warmup = bool(use_coordinate_graph), evaluators, int(warmup)
        self.static_batch = static_batch
        device = (static_batch.raw_frame if getattr(static_batch, "x", None) is None else static_batch.x).device
        # the graph's own view of the batch: the caller's tensors, but node_coords through a private buffer the graph refills
        self._batch = copy.copy(static_batch)
        self._coords = None
        if self.use_coordinate_graph:
            self._coords = torch.empty_like(static_batch.node_coords)
            self._batch.node_coords = self._coords
        self._meter = torch.zeros(2, dtype=torch.float64, device=device)        # (sum of loss * batch size, count)
        self._stream = torch.cuda.Stream(device=device)
        self.captures = 0
        self.graph = None
        self.outputs = None
        self._key = None
        self._capture()

    def _key_now(self):
        lm = self.model["landmark"]
        fold = lm.__dict__.get("_fold_cache", {})
        return (_state_key(self.model["embedder"]), _state_key(lm), self.model["embedder"].training, lm.training,
                tuple((k, id(v)) for k, v in fold.items()))

    def _step(self):
        # (coordinate labels: eval_step expands them into self._batch.y / .valid_labels first -- allocated by the eager warm-up,
        # a node of the graph afterwards; self._batch shares label_coords with the caller's static batch)
        if self._coords is not None:
            self._coords.copy_(self.static_batch.node_coords)
        preds, coord_preds, losses = eval_step(self.model, self._batch, self.criterion, self.batch_size, self.use_coordinate_graph,
                                               self.evaluators)
        if losses:
            with torch.no_grad():
                self._meter[0:1].add_(total_loss(losses).detach().reshape(1).to(torch.float64), alpha=self.batch_size)
                self._meter[1:2].add_(self.batch_size)
        return preds, coord_preds, losses

    def _capture(self):
        lm = self.model["landmark"]
        graphed = getattr(lm, "use_hip_graph", False)
        if graphed:
            lm.use_hip_graph = False              # (the model's own replay would stand in for the kernels this graph has to hold)
        try:
            self.graph = None
            self.outputs = None
            meter = self._meter.clone()
            stream = self._stream
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for _ in range(self.warmup):
                    self._step()
                # roll the warm-up back on the device: no evaluator keeps a warm-up record, the meter is where it was
                self._meter.copy_(meter)
                for ev in self.evaluators.values():
                    counter = _record_counter(ev)
                    if counter is not None:
                        counter.sub_(self.warmup)
                    if hasattr(ev, "_launched"):
                        ev._launched = max(0, ev._launched - self.warmup)
            torch.cuda.current_stream().wait_stream(stream)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                outputs = self._step()
        finally:
            if graphed:
                lm.use_hip_graph = True
        self.graph, self.outputs = graph, outputs
        self.captures += 1
        self._key = self._key_now()
        # everything the captured kernels point at that the model caches (and may evict) stays alive with the graph
        self._keep = (dict(lm.__dict__.get("_fold_cache", {})), dict(lm.__dict__.get("_kidsum", {})),
                      list(getattr(getattr(lm, "_resolver", None), "_by_digest", {}).values()))

    def __call__(self):
        """Replay the step (recapturing first if the model's parameters or buffers moved); returns the static outputs."""
        for name in ("embedder", "landmark"):
            if self.model[name].training:
                raise ValueError(f"model[{name!r}] is in training mode: call .eval() before evaluating")
        if self._key_now() != self._key:
            self._capture()
        self.graph.replay()
        return self.outputs

    def loss_avg(self) -> float:
        """The mean of the criteria's total over the evaluated frames since construction or reset_meter() (host read-back)."""
        s, n = self._meter.tolist()
        return s / n if n else 0.0

    def reset_meter(self):
        self._meter.zero_()


@torch.no_grad()
def eval_step(model: Dict[str, torch.nn.Module], batch, criterion: Optional[Dict[str, object]], batch_size: int,
              use_coordinate_graph: bool = False, evaluators=None):
    """engine.py:340-460 for one batch (models in eval mode are the caller's business, like in the reference)."""
    _device_labels(batch)
    preds, coord_preds = forward_batch(model, batch, use_coordinate_graph)
    coord_y = batch.node_coord_y if use_coordinate_graph else None
    losses = {}
    if criterion:
        losses = compute_loss(criterion, preds, batch.y, coord_preds, coord_y, batch.valid_labels, batch_size)
    if evaluators:
        update_evaluators(evaluators, preds, batch.y, coord_preds, coord_y, batch.pix2mm_x, batch.pix2mm_y,
                          batch.valid_labels, use_coordinate_graph)
    return preds, coord_preds, losses


def update_evaluators(evaluators, preds, y, coord_preds, coord_y, pix2mm_x, pix2mm_y, valid, use_coordinate_graph):
    """engine.py:466-492 without the `.detach().cpu()` of every tensor: the evaluators decode / count on the device.  The
    balanced accuracy takes (logits, labels, valid) -- the landmark logits also for coordinate-graph models, as engine.py:492
    passes them; every other evaluator the landmark evaluator's five arguments."""
    from .evaluators import BalancedBinaryAccuracyEvaluator
    for ev in evaluators.values():
        if isinstance(ev, BalancedBinaryAccuracyEvaluator):
            ev.update(preds, y, valid)
        elif use_coordinate_graph:
            ev.update(coord_preds, coord_y, pix2mm_x, pix2mm_y, valid)
        else:
            ev.update(preds, y, pix2mm_x, pix2mm_y, valid)


def prediction_table(evaluators, pix2mm_x, pix2mm_y):
    """engine.py:602-639 (``create_prediction_df``) without pandas: a plain dict of lists, one entry per frame of the last update, in
    the reference's column order -- ``pix2mm_x``, ``pix2mm_y``, the eight coordinate columns (``pred_ivs`` ... ``gt_lvpw``, an (h, w) pair
    per frame) and the six width columns in mm -- from the landmark evaluator's ``get_predictions()`` (``pandas.DataFrame(table)``
    gives the reference's frame).  pix2mm_x / pix2mm_y: tensors or sequences with one value per frame."""
    def as_list(v):
        return v.detach().reshape(-1).tolist() if isinstance(v, torch.Tensor) else [float(a) for a in v]
    record = evaluators["landmarkcoorderror"].get_predictions()
    if not record:
        raise RuntimeError("prediction_table lists the predictions of the landmark evaluator's last update(): there is none")
    table = {"pix2mm_x": as_list(pix2mm_x), "pix2mm_y": as_list(pix2mm_y)}
    for group in ("coordinates", "widths"):
        for key, value in record[group].items():
            table[key] = value.tolist()
    return table
