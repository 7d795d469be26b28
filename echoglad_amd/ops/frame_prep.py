"""Frame preparation (frame_prep.hip): uint8 -> float / 255, the affine warp, the bilinear resize, gray, the horizontal flip and
the landmarks through the same matrix, in one launch."""
from __future__ import annotations

from typing import Optional

import torch

from ._core import _check, _on_current_device, call


def frame_prep(src: torch.Tensor, out: torch.Tensor, *, matrix_inv: Optional[torch.Tensor] = None, warp_size: int = 0,
               flip: Optional[torch.Tensor] = None, gray: bool = False, coords: Optional[torch.Tensor] = None,
               matrix: Optional[torch.Tensor] = None, crop_size: Optional[int] = None,
               out_label_coords: Optional[torch.Tensor] = None, out_coord_y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src uint8 or float32 [B, C, Hs, Ws] (C 1 or 3) -> out float32 [B, C_out, F, F], written in place by eg_frame_prep
    (include/echoglad_hip.h has the rule): src / 255 for uint8, the affine warp to warp_size^2 driven by matrix_inv [B, 2, 3]
    (grid_sample: bilinear, zeros, align_corners=False; warp_size 0: no warp stage), the non-antialiased bilinear resize to F, gray
    (C = 3 only: C_out = 1), and out[b, :, i, F - 1 - j] where flip [B] uint8 is set.  coords float32 [B, 4, 2] (h, w): the landmarks
    go through `matrix` [B, 2, 3] from crop_size pixels to F (no warp stage: they are F-space integers already), are truncated,
    flipped with their frame and written to out_label_coords int32 [B, 4, 2] and, if given, out_coord_y float32 [B * 4, 2].
    Returns out."""
    warp_size = int(warp_size)
    if warp_size < 0:
        raise RuntimeError("warp_size must be >= 0 (0: no warp stage)")
    if warp_size > 0 and matrix_inv is None:
        raise RuntimeError("a warp stage (warp_size > 0) needs matrix_inv")
    if warp_size == 0 and matrix_inv is not None:
        raise RuntimeError("matrix_inv without a warp stage: pass warp_size")
    if src.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"src must be a uint8 or float32 tensor, got {src.dtype}")
    if src.dim() != 4:
        raise RuntimeError(f"src must be [B, C, Hs, Ws], got {tuple(src.shape)}")
    _check(src, "src", (None, None, None, None), dtype=src.dtype)
    _on_current_device(src, "src")
    B, C, Hs, Ws = (int(v) for v in src.shape)
    if B < 1 or Hs < 1 or Ws < 1:
        raise RuntimeError(f"src {tuple(src.shape)} is empty")
    if C not in (1, 3):
        raise RuntimeError(f"src must have 1 or 3 channels, got {C}")
    gray = bool(gray)
    if gray and C != 3:
        raise RuntimeError("gray needs a 3-channel source")
    if out.dim() != 4 or out.shape[2] != out.shape[3]:
        raise RuntimeError(f"out must be [B, C_out, F, F], got {tuple(out.shape)}")
    F = int(out.shape[3])
    _check(out, "out", (B, 1 if gray else C, F, F))
    _on_current_device(out, "out")
    if matrix_inv is not None:
        _check(matrix_inv, "matrix_inv", (B, 2, 3))
        _on_current_device(matrix_inv, "matrix_inv")
    if flip is not None:
        _check(flip, "flip", (B,), dtype=torch.uint8)
        _on_current_device(flip, "flip")
    if coords is None:
        if out_label_coords is not None or out_coord_y is not None:
            raise RuntimeError("out_label_coords / out_coord_y without coords")
        matrix, crop = None, 0
    else:
        _check(coords, "coords", (B, 4, 2))
        _on_current_device(coords, "coords")
        if out_label_coords is None:
            raise RuntimeError("coords needs out_label_coords")
        _check(out_label_coords, "out_label_coords", (B, 4, 2), dtype=torch.int32)
        _on_current_device(out_label_coords, "out_label_coords")
        if out_coord_y is not None:
            _check(out_coord_y, "out_coord_y", (4 * B, 2))
            _on_current_device(out_coord_y, "out_coord_y")
        crop = 0
        if warp_size > 0:
            if matrix is None or crop_size is None or int(crop_size) < 1:
                raise RuntimeError("coords with a warp stage need matrix and crop_size >= 1")
            _check(matrix, "matrix", (B, 2, 3))
            _on_current_device(matrix, "matrix")
            crop = int(crop_size)
        elif matrix is not None:
            raise RuntimeError("matrix without a warp stage: the coordinates are frame-space integers already")
    call("eg_frame_prep", src, int(src.dtype == torch.uint8), B, C, Hs, Ws, matrix_inv, warp_size, F, flip, int(gray), out,
         coords, matrix, crop, out_label_coords, out_coord_y)
    return out
