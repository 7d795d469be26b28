"""Dense node labels from landmark coordinates (labels.hip): what ``data.node_labels`` builds on the host, in one launch."""
from __future__ import annotations

from typing import Optional

import torch

from ._core import _check, _check_rows, _level_arrays, _on_current_device, call


def node_labels(coords: torch.Tensor, valid4: Optional[torch.Tensor], batch: int, levels, frame_size: int,
                out_labels: torch.Tensor, out_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """coords int32 [batch, 4, 2] (h, w) and valid4 float32 [batch, 4] (None: ones) -> out_labels / out_valid float32
    [batch * n_rows, 4], written in place by eg_node_labels (include/echoglad_hip.h has the rule; a landmark outside [-F, F) gets
    no 1).  levels: [(first row inside a frame's rows, side)], the main grid of side `frame_size` last; n_rows is taken from
    out_labels and may exceed the levels' rows (those rows are 0).  Returns out_labels."""
    batch = int(batch)
    if batch < 1:
        raise RuntimeError("batch must be >= 1")
    _check(coords, "coords", (batch, 4, 2), dtype=torch.int32)
    _on_current_device(coords, "coords")
    if valid4 is not None:
        _check(valid4, "valid4", (batch, 4))
        _on_current_device(valid4, "valid4")
    _check_rows(out_labels, "out_labels", None, 4)
    rows = int(out_labels.shape[0])
    if rows == 0 or rows % batch:
        raise RuntimeError(f"out_labels has {rows} rows: not a positive multiple of the batch size {batch}")
    _check_rows(out_valid, "out_valid", rows, 4, optional=True)
    start, side, n = _level_arrays(levels)
    call("eg_node_labels", coords, valid4, batch, rows // batch, start, side, n, int(frame_size), out_labels, out_valid)
    return out_labels
