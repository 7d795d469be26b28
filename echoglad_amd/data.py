"""Synthetic dataset, label construction and batch collation for the hierarchical graph —
host-side counterpart of the reference's ``DummyDataset`` (src/core/datasets.py:1339-1612) and of the PyG
``DataLoader`` collate it is used with (src/builders/dataloader_builder.py:5-33).

The reference builds a networkx graph with O(n^2) list concatenation (7.5 s at the default config) and converts it
with ``from_networkx`` for EVERY sample; here the topology is the closed form of ``echoglad_amd.topology`` (built
once, shared by all samples and all batches) and a batch is a plain namespace with the attribute names the model's
``forward(data_batch)`` reads (models.py:408-413): x, edge_index, batch, node_type, node_coords, plus y,
valid_labels, node_coord_y, pix2mm_x, pix2mm_y for the losses / evaluators.
"""
from __future__ import annotations

import types
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch

from .topology import HierTopology, TopologySpec, get_topology

AVERAGE_COORDS = [[99.99, 112.57], [142.71, 90.67], [151.18, 86.25], [91.81, 117.91]]     # datasets.py:1361


def _wrap(i: int, n: int) -> int:
    """numpy index semantics of ``y[i] = 1`` (datasets.py:1599,1607): negative indices count from the end, anything
    outside [-n, n) is an IndexError there and here."""
    if not -n <= i < n:
        raise IndexError(f"label index {i} is out of bounds for a grid of side {n}")
    return i % n


def node_labels(coordinate: Sequence[int], frame_size: int, num_aux_graphs: int,
                use_main_graph_only: bool = False) -> np.ndarray:
    """One (h, w) landmark -> float32 one-hot over the grid nodes of a frame, one ``1`` per level
    (datasets.py:1586-1612: ``np.digitize`` against ``linspace(0, F, p + 1)`` on the aux levels, the pixel itself
    on the main grid)."""
    h, w = int(coordinate[0]), int(coordinate[1])
    parts: List[np.ndarray] = []
    if not use_main_graph_only:
        for g in range(1, num_aux_graphs + 1):
            p = 2 ** g
            bins = np.linspace(start=0, stop=frame_size, num=p + 1)
            bh, bw = (int(v) for v in (np.digitize([h, w], bins=bins) - 1))
            y = np.zeros(p * p, dtype=np.float32)
            y[_wrap(bh, p) * p + _wrap(bw, p)] = 1.0
            parts.append(y)
    y = np.zeros(frame_size * frame_size, dtype=np.float32)
    y[_wrap(h, frame_size) * frame_size + _wrap(w, frame_size)] = 1.0
    parts.append(y)
    return np.concatenate(parts)


def _level_table(frame_size: int, num_aux_graphs: int, use_main_graph_only: bool = False):
    from .losses import level_grids                 # (losses imports ops: only where a label table is asked for)
    return level_grids(frame_size, num_aux_graphs, use_main_graph_only)


def _check_label_coords(coords: np.ndarray, frame_size: int) -> None:
    """IndexError where ``node_labels`` raises one: a coordinate outside [-F, F) (the main grid's ``y[i] = 1`` of any landmark)."""
    bad = (coords < -frame_size) | (coords >= frame_size)
    if bad.any():
        v = int(coords[bad].ravel()[0])
        raise IndexError(f"label index {v} is out of bounds for a grid of side {frame_size}")


def label_rows(coords, frame_size: int, num_aux_graphs: int, use_main_graph_only: bool = False) -> np.ndarray:
    """(h, w) of the landmarks, [K, 2] integers -> int64 [n_levels, K]: the frame-local row of every landmark's ``1`` on every
    level, i.e. ``np.nonzero(node_labels(c, ...))`` per landmark, in integers (what eg_node_labels computes on the device):
        aux levels, side p:   bin(v) = v * p // F  for 0 <= v < F,   p - 1  for -F <= v < 0
        the main grid (last): bin(v) = v           for 0 <= v < F,   v + F  for -F <= v < 0
    p is a power of two, so linspace(0, F, p + 1) is exact in fp64 and ``digitize(v) - 1 == v * p // F``.  IndexError exactly where
    ``node_labels`` raises one."""
    c = np.asarray(coords).astype(np.int64).reshape(-1, 2)
    F = int(frame_size)
    _check_label_coords(c, F)
    levels = _level_table(F, num_aux_graphs, use_main_graph_only)
    out = np.empty((len(levels), c.shape[0]), dtype=np.int64)
    for l, (start, p) in enumerate(levels):
        if l == len(levels) - 1:
            b = np.where(c < 0, c + F, c)
        else:
            b = np.where(c < 0, p - 1, (c * p) // F)
        out[l] = start + b[:, 0] * p + b[:, 1]
    return out


def draw_coords(frame_size: int, orig_frame_size: int = 224, rng=np.random) -> np.ndarray:
    """datasets.py:1421-1438: three draws of 4 integers (LVIDd, IVS, LVPW) scaled by F/224, assembled in (h, w)
    order as [lvid_top, lvid_bot, lvpw, ivs], each minus one (so -1 occurs and wraps in the labels)."""
    def draw():
        return np.round(rng.randint(low=0, high=frame_size, size=4) * frame_size / orig_frame_size).astype(int)
    lvid, ivs, lvpw = draw(), draw(), draw()
    return np.array([[lvid[1] - 1, lvid[0] - 1], [lvid[3] - 1, lvid[2] - 1], [lvpw[3] - 1, lvpw[2] - 1],
                     [ivs[1] - 1, ivs[0] - 1]])


class SyntheticEchoDataset(torch.utils.data.Dataset):
    """Counterpart of ``DummyDataset``: 100 samples of N(0,1) frames with random landmark labels on the static
    hierarchical graph.  ``transform`` maps the [1, 224, 224] frame to [1, F, F] (default: bilinear resize).

    ``labels="coords"``: a sample carries ``label_coords`` (int32 [4, 2], the landmarks' (h, w)) and ``label_valid`` (float32 [4])
    instead of the dense ``y`` / ``valid_labels`` -- same random draws, same landmarks; ``device_labels_`` expands them on the
    device."""

    def __init__(self, num_aux_graphs: int, frame_size: int = 128, transform=None, average_coords=None,
                 main_graph_type: str = "grid", aux_graph_type: str = "grid", use_coordinate_graph: bool = False,
                 use_connection_nodes: bool = False, use_main_graph_only: bool = False, length: int = 100,
                 labels: str = "dense"):
        if labels not in ("dense", "coords"):
            raise ValueError(f"labels must be 'dense' or 'coords', got {labels!r}")
        self.labels = labels
        self.spec = TopologySpec(frame_size, num_aux_graphs, use_main_graph_only, use_coordinate_graph,
                                 use_connection_nodes, main_graph_type, aux_graph_type)
        self.topology: HierTopology = get_topology(self.spec)
        self.frame_size = frame_size
        self.num_aux_graphs = num_aux_graphs
        self.use_coordinate_graph = use_coordinate_graph
        self.use_main_graph_only = use_main_graph_only
        self.average_coords = AVERAGE_COORDS if average_coords is None else average_coords
        self.transform = transform or (lambda t: torch.nn.functional.interpolate(
            t.unsqueeze(0), size=(frame_size, frame_size), mode="bilinear", align_corners=False).squeeze(0))
        self.length = length
        self.edge_index = torch.from_numpy(self.topology.edge_index())            # shared by every sample
        self.node_type = torch.from_numpy(self.topology.node_type())              # float64 like the reference
        self._label_levels = tuple(_level_table(frame_size, num_aux_graphs, use_main_graph_only)) if labels == "coords" else None

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        frame = self.transform(torch.randn((1, 224, 224))).unsqueeze(0)           # [1,1,F,F]
        coords = draw_coords(self.frame_size)
        g = types.SimpleNamespace()
        g.x = frame
        if self.labels == "coords":
            _check_label_coords(coords, self.frame_size)
            g.label_coords = torch.from_numpy(coords.astype(np.int32))            # [4, 2]
            g.label_valid = torch.ones(4, dtype=torch.float32)
            g.label_levels = self._label_levels
            g.label_frame_size = self.frame_size
        else:
            g.y = torch.from_numpy(np.stack([node_labels(c, self.frame_size, self.num_aux_graphs, self.use_main_graph_only)
                                             for c in coords], axis=1))         # [N_grid, 4]
            g.valid_labels = torch.ones_like(g.y)
        g.edge_index = self.edge_index
        g.node_type = self.node_type
        g.num_nodes = self.topology.num_nodes
        if self.use_coordinate_graph and not self.use_main_graph_only:
            g.node_coords = torch.tensor(self.average_coords, dtype=torch.float32)
            g.node_coord_y = torch.tensor(coords, dtype=torch.float32)
        g.pix2mm_x = torch.tensor(0.1 * 10, dtype=torch.float32)
        g.pix2mm_y = torch.tensor(0.1 * 10, dtype=torch.float32)
        return g


def collate(samples: Sequence, topology: Optional[HierTopology] = None):
    """PyG ``Batch.from_data_list`` semantics for these samples: node-level tensors concatenated on dim 0,
    ``edge_index`` shifted by the per-sample node offset, 0-d tensors stacked, ``batch`` = sample id per node.
    With ``topology`` given the batched ``edge_index`` comes from the closed form instead of B shifted copies."""
    B = len(samples)
    n = samples[0].num_nodes
    out = types.SimpleNamespace()
    out.num_graphs = B
    out.x = torch.cat([s.x for s in samples], dim=0)
    if hasattr(samples[0], "label_coords"):
        # coordinate labels: 32 + 16 bytes per frame; device_labels_() expands them into y / valid_labels on the device
        out.label_coords = torch.stack([s.label_coords for s in samples])          # [B, 4, 2] int32
        out.label_valid = torch.stack([s.label_valid for s in samples])            # [B, 4]
        out.label_levels = tuple(samples[0].label_levels)
        out.label_frame_size = int(samples[0].label_frame_size)
    else:
        out.y = torch.cat([s.y for s in samples], dim=0)
        out.valid_labels = torch.cat([s.valid_labels for s in samples], dim=0)
    if topology is not None:
        # what depends on (topology, B) only is built once and handed out again AS THE SAME TENSORS: the model resolves an
        # edge_index it has seen before by identity (no digest pass), and to_device() below moves such a tensor once per device
        const = topology.__dict__.setdefault("_collate_const", {})
        hit = const.get(B)
        if hit is None or hit[3] is not samples[0].node_type:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                       # (a read-only numpy array behind a tensor nobody writes to)
                ei = torch.from_numpy(topology.batched_edge_index(B))
            hit = (ei, torch.arange(B).repeat_interleave(n), torch.cat([s.node_type for s in samples], dim=0), samples[0].node_type)
            while len(const) >= 4:
                const.pop(next(iter(const)))
            const[B] = hit
            for t in hit[:3]:
                _COLLATE_CONSTS[id(t)] = weakref.ref(t)
        out.edge_index, out.batch, out.node_type = hit[0], hit[1], hit[2]
    else:
        out.node_type = torch.cat([s.node_type for s in samples], dim=0)
        out.edge_index = torch.cat([s.edge_index + i * n for i, s in enumerate(samples)], dim=1)
        out.batch = torch.arange(B).repeat_interleave(n)
    if hasattr(samples[0], "node_coords"):
        out.node_coords = torch.cat([s.node_coords for s in samples], dim=0)
        out.node_coord_y = torch.cat([s.node_coord_y for s in samples], dim=0)
    out.pix2mm_x = torch.stack([s.pix2mm_x for s in samples])
    out.pix2mm_y = torch.stack([s.pix2mm_y for s in samples])
    return out


_COLLATE_CONSTS = {}        # id -> weak reference of every tensor collate(samples, topology) hands out again for later batches
_CONST_ON_DEVICE = {}       # (id of a collate() constant, device) -> (the CPU tensor, its device copy): one host-to-device copy per device
_GRAPH_CONST_ATTRS = ("edge_index", "batch", "node_type")


def _is_collate_const(t) -> bool:
    ref = _COLLATE_CONSTS.get(id(t))
    if ref is None:
        return False
    if ref() is t:
        return True
    if ref() is None:
        del _COLLATE_CONSTS[id(t)]
    return False


def to_device(batch, device):
    """Moves every tensor attribute of a collated batch.  The tensors collate() hands out again for every batch of a (topology,
    batch size) -- edge_index (55 MB at 224/7, batch 8), batch, node_type -- are moved ONCE per device and the same device tensors
    come back afterwards: nothing to copy, and the model recognises the edge_index by identity."""
    device = torch.device(device)
    for k, v in vars(batch).items():
        if not torch.is_tensor(v):
            continue
        if k in _GRAPH_CONST_ATTRS and v.device != device and _is_collate_const(v):
            # (only tensors collate() registered: a fresh edge_index per batch -- collate without a topology, batches unpickled
            # from DataLoader workers -- could never hit again and would only pin copies here)
            hit = _CONST_ON_DEVICE.get((id(v), str(device)))
            if hit is None or hit[0] is not v:
                while len(_CONST_ON_DEVICE) >= 16:
                    _CONST_ON_DEVICE.pop(next(iter(_CONST_ON_DEVICE)))
                hit = _CONST_ON_DEVICE[(id(v), str(device))] = (v, v.to(device))
            setattr(batch, k, hit[1])
        else:
            setattr(batch, k, v.to(device, non_blocking=True))
    return batch


def copy_batch_(dst, src):
    """Writes every tensor attribute of the collated batch ``src`` INTO the tensors of ``dst`` (same shapes; ``dst`` typically on
    the device, ``src`` fresh from ``collate``): what a captured training step (``engine.GraphedTrainStep``) needs -- its graph
    reads the tensors it was captured with, so a new batch has to arrive in place.  Returns ``dst``.

    The graph tensors (``edge_index``, ``batch``, ``node_type``) are NOT copied: a captured step runs on the topology handle it
    was captured with, whatever is written into the edge_index later (and a pageable 7 - 55 MB host-to-device copy per step
    would synchronise a step whose point is ~1 ms of GPU work behind one launch).  When ``src`` carries the collate() constant
    that ``dst``'s tensor was moved from (or ``dst``'s tensor itself) there is nothing to do; any other tensor is compared with
    the static one ONCE per static batch and attribute (equal: later batches are taken on trust by shape; different: ValueError
    -- a captured step takes batches of ONE topology).

    A coordinate-label source (``label_coords`` / ``label_valid``, 48 bytes per frame) leaves ``dst.y`` / ``dst.valid_labels``
    alone: ``device_labels_(dst)`` rewrites them on the device.  The device cannot raise for a coordinate outside the frame, so a
    CPU ``label_coords`` is checked here with ``label_rows``' rule (IndexError) before anything is copied."""
    lc = getattr(src, "label_coords", None)
    if torch.is_tensor(lc) and lc.device.type == "cpu":
        frame_size = getattr(src, "label_frame_size", None) or getattr(dst, "label_frame_size", None)
        if frame_size is None:
            raise ValueError("a batch with label_coords needs label_frame_size (collate() records it)")
        _check_label_coords(lc.numpy(), int(frame_size))
    verified = dst.__dict__.setdefault("_graph_consts_verified", set())
    for k, v in vars(src).items():
        if not torch.is_tensor(v):
            continue
        d = getattr(dst, k, None)
        if not torch.is_tensor(d) or d.shape != v.shape:
            raise ValueError(f"batch attribute {k!r}: {None if d is None else tuple(d.shape)} in the static batch, {tuple(v.shape)} in the new one "
                             "(a captured step takes batches of ONE shape)")
        if k in _GRAPH_CONST_ATTRS:
            if v is d:
                continue
            hit = _CONST_ON_DEVICE.get((id(v), str(d.device)))
            if hit is not None and hit[0] is v and hit[1] is d:
                continue
            if k not in verified:
                if not torch.equal(d, v.to(d.device)):
                    raise ValueError(f"batch attribute {k!r} differs from the static batch's: a captured step takes batches of ONE "
                                     "topology (capture a new step for another graph)")
                verified.add(k)
            continue
        d.copy_(v, non_blocking=True)
    return dst


def device_labels_(batch):
    """Expands ``batch.label_coords`` [B, 4, 2] / ``batch.label_valid`` [B, 4] (a batch of ``labels="coords"`` samples, on the
    device) into the dense ``batch.y`` / ``batch.valid_labels`` [B * N_grid, 4] the criteria and evaluators read: one launch
    (ops.node_labels), no host synchronisation, so it can be the first node of a captured step.  The two dense tensors are
    allocated at the first (eager) call and rewritten in place afterwards; inside a stream capture they must exist already.
    A landmark outside [-F, F) gets no ``1`` (the host path raises IndexError: ``copy_batch_`` checks a CPU source).  A batch
    without ``label_coords`` is returned as it is."""
    coords = getattr(batch, "label_coords", None)
    if coords is None:
        return batch
    from . import ops
    levels = batch.label_levels
    B = int(coords.shape[0])
    y, valid = getattr(batch, "y", None), getattr(batch, "valid_labels", None)
    if y is None or valid is None:
        if coords.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("device_labels_: batch.y / batch.valid_labels do not exist yet and a stream capture must not allocate: "
                               "call device_labels_(batch) once eagerly (a warm-up step does) before capturing")
        n_rows = levels[-1][0] + levels[-1][1] ** 2
        if y is None:
            y = batch.y = torch.empty(B * n_rows, 4, dtype=torch.float32, device=coords.device)
        if valid is None:
            valid = batch.valid_labels = torch.empty(B * n_rows, 4, dtype=torch.float32, device=coords.device)
    ops.node_labels(coords, getattr(batch, "label_valid", None), B, levels, batch.label_frame_size, y, valid)
    return batch
