"""Coordinate-graph landmark update (models.py:438-473) and resampling: the landmark MLP on the 4 coordinate rows of every frame,
the bilinear samples of the main grid at the landmark positions, and the two fused into one in-place update of the node array."""
from __future__ import annotations

import ctypes as ct

import torch

from ._core import C, _check, _check_rows, call
from .train import _cls_params, _lower_sums

COORD_MLP_GRADS_FLOATS = 5042


def _frame_rows_ptr(h, batch: int, n_per_frame: int, row0: int):
    """(pointer to row `row0` of frame 0, floats between two frames) of a [batch * n_per_frame, 128] node array: where the 4
    coordinate rows of every frame live (eg_*_rows entry points)."""
    _check_rows(h, "h", batch * n_per_frame)
    if row0 < 0 or row0 + 4 > n_per_frame:
        raise RuntimeError("the 4 rows must lie inside a frame")
    return ct.c_void_p(h.data_ptr() + row0 * C * 4), n_per_frame * C


def _check_coords(coords, batch: int, points: int) -> None:
    _check(coords, "coords", numel=batch * points * 2)


def _mlp_fwd_buffers(coords, batch: int, P: dict, want_backward: bool):
    """What coord_mlp_fwd and coord_update_fwd share: the checks of coords and of the 136-32-16-2 head's weights, and the buffers
    (z1, z2, bn, pre | None) the forward fills for the backward."""
    rows = 4 * batch
    _check_coords(coords, batch, 4)
    for k, shape in (("w1", (32, C + 8)), ("w2", (16, 32)), ("w3", (2, 16))):
        if tuple(P[k].shape) != shape:
            raise RuntimeError(f"coordinate MLP {k} must be {shape}, got {tuple(P[k].shape)}")
    f32 = dict(dtype=torch.float32, device=coords.device)
    return (torch.empty(rows, 32, **f32), torch.empty(rows, 16, **f32), torch.empty(96, **f32),
            torch.empty(rows, 2, **f32) if want_backward else None)


def coord_mlp_fwd(lm, coords, batch: int, P: dict, train: bool, frame: int, want_backward: bool, in_rows=None):
    """lm [4*batch,128], coords [4*batch,2] -> (new_coords [4*batch,2], saved = (z1, z2, bn, pre) | None).
    P: the _cls_params dictionary with the 136-32-16-2 head's tensors.
    in_rows = (h, n_per_frame, row0): the landmark rows are rows row0 .. row0 + 3 of every frame of h (no gathered copy); `lm`
    is then an OUTPUT -- the packed copy of those rows the backward needs -- or None."""
    rows = 4 * batch
    _check_rows(lm, "lm", rows, optional=True)
    if lm is None and in_rows is None:
        raise RuntimeError("lm or in_rows")
    z1, z2, bn, pre = _mlp_fwd_buffers(coords, batch, P, want_backward)
    new = torch.empty(rows, 2, dtype=torch.float32, device=coords.device)
    s = _cls_params(P)
    if in_rows is not None:
        ptr, stride = _frame_rows_ptr(in_rows[0], batch, in_rows[1], in_rows[2])
        call("eg_coord_mlp_fwd_rows", ptr, stride, lm, coords, batch, ct.byref(s), train, frame, z1, z2, bn, pre, new)
    else:
        call("eg_coord_mlp_fwd", lm, coords, batch, ct.byref(s), train, frame, z1, z2, bn, pre, new)
    return new, ((z1, z2, bn, pre) if want_backward else None)


def coord_mlp_bwd(dnew, lm, coords, batch: int, P: dict, frame: int, saved, need_dlm: bool, need_dcoords: bool, out_rows=None,
                  accumulate: bool = False):
    """-> (dlm | None, dcoords | None, grads [5042] packed as in include/echoglad_hip.h)
    out_rows = (dh, n_per_frame, row0): dlm is written (accumulate: added) into rows row0 .. row0 + 3 of every frame of dh
    instead of being returned."""
    rows = 4 * batch
    z1, z2, bn, pre = saved
    f32 = dict(dtype=torch.float32, device=lm.device)
    _check(dnew, "dnew", numel=rows * 2)
    scratch = torch.empty(rows, 56, **f32)
    dlm = torch.empty(rows, C, **f32) if (need_dlm and out_rows is None) else None
    dcoords = torch.empty(rows, 2, **f32) if need_dcoords else None
    grads = torch.empty(COORD_MLP_GRADS_FLOATS, **f32)
    s = _cls_params(P)
    common = (dnew, lm, coords, batch, ct.byref(s), frame, z1, z2, bn, pre, scratch)
    if out_rows is not None:
        ptr, stride = _frame_rows_ptr(out_rows[0], batch, out_rows[1], out_rows[2])
        call("eg_coord_mlp_bwd_rows", *common, ptr, stride, accumulate, dcoords, grads)
    else:
        call("eg_coord_mlp_bwd", *common, dlm, dcoords, grads)
    return dlm, dcoords, grads


def coord_update_fwd(h, coords, batch: int, n_per_frame: int, coord_base: int, main_base: int, P: dict, train: bool, frame: int,
                     want_backward: bool, resample: bool = True):
    """The coordinate update of one GNN layer on the node array IN PLACE (eg_coord_update_fwd: models.py:438-473): the landmark MLP on
    the 4 coordinate rows of every frame of h, then (resample) those rows overwritten with the main grid sampled at the new positions.
    One launch up to batch 16.  -> ((new_coords, new_coords_again) [4*batch,2] each: the same coordinates in two tensors -- one to hand
    out, one to keep for the backward, without a copy launch --, lm = packed copy of the rows the MLP read, saved = (z1, z2, bn, pre) | None)"""
    rows = 4 * batch
    _check_rows(h, "h", batch * n_per_frame)
    z1, z2, bn, pre = _mlp_fwd_buffers(coords, batch, P, want_backward)
    f32 = dict(dtype=torch.float32, device=h.device)
    lm = torch.empty(rows, C, **f32)
    new = (torch.empty(rows, 2, **f32), torch.empty(rows, 2, **f32))
    s = _cls_params(P)
    call("eg_coord_update_fwd", h, n_per_frame, coord_base, main_base, coords, batch, ct.byref(s), train, frame, bool(resample),
         lm, z1, z2, bn, pre, new[0], new[1])
    return new, lm, ((z1, z2, bn, pre) if want_backward else None)


def coord_update_bwd(dx, dnew, h, new, lm, coords, batch: int, n_per_frame: int, coord_base: int, main_base: int, P: dict, frame: int,
                     saved, need_dcoords: bool, lower=None):
    """Backward of coord_update_fwd(resample=True) on the gradient array dx IN PLACE (eg_coord_update_bwd): dx is the gradient w.r.t. the
    tensor after the update and leaves as the gradient w.r.t. the tensor before it.  dnew: d new_coords from downstream or None;
    h: the tensor the samples were taken from (after the update); lower as in bilinear4_bwd.
    -> (dcoords | None, grads [5042], taps [batch,2,128] | None).  One launch up to batch 16."""
    rows = 4 * batch
    z1, z2, bn, pre = saved
    _check_rows(dx, "dx", batch * n_per_frame)
    _check_rows(h, "h", batch * n_per_frame)
    if dnew is not None:
        _check(dnew, "dnew", numel=rows * 2)
    f32 = dict(dtype=torch.float32, device=dx.device)
    scratch = torch.empty(rows, 56, **f32)
    dbil = torch.empty(rows, 2, **f32)
    dcoords = torch.empty(rows, 2, **f32) if need_dcoords else None
    grads = torch.empty(COORD_MLP_GRADS_FLOATS, **f32)
    taps, ls = None, None
    if lower is not None:
        ls = _lower_sums(lower, batch * n_per_frame)
        taps = torch.empty(batch, 2, C, **f32)
    s = _cls_params(P)
    call("eg_coord_update_bwd", dx, n_per_frame, coord_base, main_base, h, new, dnew, lm, coords, batch, ct.byref(s), frame,
         z1, z2, bn, pre, scratch, dbil, None if ls is None else ct.byref(ls), taps, dcoords, grads)
    return dcoords, grads, taps


# ---------------------------------------------------------------------------
# coordinate-graph resampling
# ---------------------------------------------------------------------------
def bilinear4_fwd(h, coords, batch, n_per_frame, main_base, frame, points=4, out_rows=None) -> torch.Tensor:
    """out_rows = (dst, n_per_frame, row0): the samples are written into rows row0 .. of every frame of dst (None is returned)."""
    _check_rows(h, "h", batch * n_per_frame)
    _check_coords(coords, batch, points)
    if out_rows is not None:
        ptr, stride = _frame_rows_ptr(out_rows[0], batch, out_rows[1], out_rows[2])
        call("eg_bilinear4_fwd_rows", h, coords, batch, points, n_per_frame, main_base, frame, ptr, stride)
        return None
    out = torch.empty(batch * points, C, dtype=torch.float32, device=h.device)
    call("eg_bilinear4_fwd", h, coords, batch, points, n_per_frame, main_base, frame, out)
    return out


def bilinear4_bwd(dout, h, coords, batch, n_per_frame, main_base, frame, dh=None, want_dcoords=True, points=4, dout_rows=None,
                  lower=None):
    """dout_rows = (src, n_per_frame, row0): the samples' gradient is read from rows row0 .. of every frame of src (dout is None).
    lower = (z, bn, relu, dropout_p, seed, ...) of the layer whose dy ``dh`` is, when that layer's BatchNorm-backward sums were taken
    before this call (gcn_layer_bwd(..., lower=)): -> (dcoords, taps [batch, 2, 128]), the sums of what is added here."""
    _check_rows(h, "h", batch * n_per_frame)
    _check_coords(coords, batch, points)
    dcoords = torch.empty(batch * points, 2, dtype=torch.float32, device=h.device) if want_dcoords else None
    where = (h, coords, batch, points, n_per_frame, main_base, frame, dh, dcoords)
    if lower is not None:
        if dout_rows is None or dh is None:
            raise RuntimeError("tap sums go with the in-place form (dout_rows, dh)")
        ls = _lower_sums(lower, batch * n_per_frame)
        taps = torch.empty(batch, 2, C, dtype=torch.float32, device=h.device)
        ptr, stride = _frame_rows_ptr(dout_rows[0], batch, dout_rows[1], dout_rows[2])
        call("eg_bilinear4_bwd_rows_sums", ptr, stride, *where, ct.byref(ls), taps)
        return dcoords, taps
    if dout_rows is not None:
        ptr, stride = _frame_rows_ptr(dout_rows[0], batch, dout_rows[1], dout_rows[2])
        call("eg_bilinear4_bwd_rows", ptr, stride, *where)
        return dcoords
    call("eg_bilinear4_bwd", dout.contiguous(), *where)
    return dcoords


class _Bilinear4Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, coords, batch, n_per_frame, main_base, frame):
        coords = coords.contiguous()
        ctx.save_for_backward(h, coords)
        ctx.dims = (batch, n_per_frame, main_base, frame)
        return bilinear4_fwd(h, coords, batch, n_per_frame, main_base, frame)

    @staticmethod
    def backward(ctx, dout):
        h, coords = ctx.saved_tensors
        batch, n_per_frame, main_base, frame = ctx.dims
        dh = torch.zeros_like(h) if ctx.needs_input_grad[0] else None
        dcoords = bilinear4_bwd(dout, h, coords, batch, n_per_frame, main_base, frame, dh=dh,
                                want_dcoords=ctx.needs_input_grad[1])
        if dcoords is not None:
            dcoords = dcoords.view_as(coords)
        return dh, dcoords, None, None, None, None


def bilinear4(h, coords, batch, n_per_frame, main_base, frame) -> torch.Tensor:
    """[batch*4, 128] features at the landmark coordinates (differentiable wrt h and coords)."""
    c = coords.reshape(batch * 4, 2)
    if torch.is_grad_enabled() and (h.requires_grad or c.requires_grad):
        return _Bilinear4Fn.apply(h, c, batch, n_per_frame, main_base, frame)
    return bilinear4_fwd(h, c.contiguous(), batch, n_per_frame, main_base, frame)


def scatter_coord_rows(h, new_feats, batch, n_per_frame, coord_base) -> torch.Tensor:
    """h[type==1 rows] = new_feats (models.py:473).  The coordinate rows are the last 4 rows of every frame, so
    this is a strided slice assignment; under autograd a copy keeps the saved forward values intact."""
    need_grad = torch.is_grad_enabled() and (h.requires_grad or new_feats.requires_grad)
    tgt = h.clone() if need_grad else h
    tgt.view(batch, n_per_frame, C)[:, coord_base:coord_base + 4, :] = new_feats.view(batch, 4, C)
    return tgt
