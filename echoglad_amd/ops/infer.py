"""Inference layers and heads: the fused GCN layer in its plain / chained / running-maximum forms, the layer with the
classifier heads folded in, and the pieces they are made of."""
from __future__ import annotations

from typing import Optional

import torch

from ._core import C, _check, _check_rows, _check_vec, call
from .graph import Graph
from .pack import _addresses, _conv_levels, _ints

_HEAD_KEYS = ("w1", "s1", "t1", "w2", "s2", "t2", "w3", "b3")       # the packed inference parameters of the 4 heads, in call order


def _check_layer_args(rows: int, x, weight, scale, shift, residual) -> None:
    _check_rows(x, "x", rows)
    _check(weight, "weight", (C, C))
    _check_vec(scale, "scale", C)
    _check_vec(shift, "shift", C)
    _check_rows(residual, "residual", rows, optional=True)


def gcn_layer_fwd(graph: Graph, batch: int, x: torch.Tensor, weight: torch.Tensor,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                  residual: Optional[torch.Tensor] = None, relu: bool = False, transpose_w: bool = False,
                  out: Optional[torch.Tensor] = None, kidsum_in: Optional[torch.Tensor] = None,
                  kidsum_out: Optional[torch.Tensor] = None, jk_in: Optional[torch.Tensor] = None,
                  jk_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act((A_hat x) W^T * scale + shift) + residual in one kernel.

    kidsum_in / kidsum_out: child-sum side buffers of a chained stack of layers (see `new_kidsum`,
    include/echoglad_hip.h eg_gcn_layer_fwd_chain).  jk_in / jk_out: running JumpingKnowledge('max') maximum,
    jk_out = max(jk_in, result) (eg_gcn_layer_fwd_jk; the first layer passes x as jk_in)."""
    rows = graph.num_nodes * batch
    _check_layer_args(rows, x, weight, scale, shift, residual)
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_rows(out, "out", rows)
    jk = jk_in is not None or jk_out is not None
    if jk:
        if jk_in is None or jk_out is None or transpose_w:
            raise RuntimeError("jk_in and jk_out go together (and not with transpose_w)")
        _check_rows(jk_in, "jk_in", rows)
        _check_rows(jk_out, "jk_out", rows)
    chained = kidsum_in is not None or kidsum_out is not None
    if chained and graph.kidsum_rows == 0 and not jk:
        raise RuntimeError("this graph handle has no child-sum side buffer (kidsum_rows == 0)")
    _check_rows(kidsum_in, "kidsum_in", graph.kidsum_rows * batch, optional=True)
    _check_rows(kidsum_out, "kidsum_out", graph.kidsum_rows * batch, optional=True)
    common = (graph._h, batch, x, weight, scale, shift, residual, relu)
    if jk:
        call("eg_gcn_layer_fwd_jk", *common, out, kidsum_in, kidsum_out, jk_in, jk_out)
    elif chained:
        call("eg_gcn_layer_fwd_chain", *common, transpose_w, out, kidsum_in, kidsum_out)
    else:
        call("eg_gcn_layer_fwd", *common, transpose_w, out)
    return out


def gcn_layer_cls_fwd(graph: Graph, batch: int, x: torch.Tensor, weight: torch.Tensor, scale, shift, residual, relu: bool,
                      packed: dict, sigmoid: bool = False, kidsum_in: Optional[torch.Tensor] = None,
                      jk_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Last layer + node-type filter + 4 classifier heads in one kernel -> logits [batch * (num_nodes - num_conn), 4] (the
    connection nodes at the head of every frame have no logits row).
    jk_in: running JumpingKnowledge('max') maximum of the earlier embeddings: the heads then see max(jk_in, layer output)."""
    rows = graph.num_nodes * batch
    _check_layer_args(rows, x, weight, scale, shift, residual)
    _check_rows(kidsum_in, "kidsum_in", graph.kidsum_rows * batch, optional=True)
    _check_rows(jk_in, "jk_in", rows, optional=True)
    out = torch.empty((graph.num_nodes - graph.num_conn) * batch, 4, dtype=torch.float32, device=x.device)
    call("eg_gcn_layer_cls_fwd", graph._h, batch, x, weight, scale, shift, residual, relu, kidsum_in, jk_in,
         *[packed[k] for k in _HEAD_KEYS], sigmoid, out)
    return out


def split3_planes(w: torch.Tensor):
    """The exact 3-piece bf16 split of the kernels (csrc/tile.h split3), on the host side: float32 tensors hi, mid, lo whose low 16
    bits are zero, hi + mid + lo == w bit for bit (|w| >= 2^-110; integer masks and two exact subtractions)."""
    def top16(v):
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    w = w.detach().to(torch.float32)
    hi = top16(w)
    r = w - hi
    mid = top16(r)
    return hi, mid, top16(r - mid)


_KOFF = (0, 64, 32, 96)          # csrc/tile.h koff16: the k quarter a lane group kq reads


def fold_lo_index(device=None):
    """(channel, k) index tensors of the lo-plane table's layout [k-step 4][wave 4][column block 2][kq 4][i 16][e 8]: entry
    = W[32 wave + 16 cb + i][koff(kq) + 8 step + e], the order in which the lanes of eg_gcn_layer_cls_fold_split_fwd fetch it."""
    ar = lambda n: torch.arange(n, device=device)          # (made on `device`: no host-to-device copy, legal under stream capture)
    s, wv, cb, kq, i, e = torch.meshgrid(ar(4), ar(4), ar(2), ar(4), ar(16), ar(8), indexing="ij")
    ch = 32 * wv + 16 * cb + i
    k = 64 * (kq & 1) + 32 * (kq >> 1) + 8 * s + e          # koff(kq) of _KOFF
    return ch, k


def fold_lo_table(m1: torch.Tensor, w1s: torch.Tensor) -> torch.Tensor:
    """The lo planes of m1 and w1s as bf16 bit patterns (int16 [2, 4, 4, 2, 4, 16, 8], 64 KB) in the kernel's fetch order."""
    ch, k = fold_lo_index(m1.device)
    planes = [(split3_planes(w)[2].view(torch.int32) >> 16).to(torch.int16)[ch, k] for w in (m1, w1s)]
    return torch.stack(planes).contiguous()


_LO_TABLES: dict = {}            # (m1 ptr, version, w1s ptr, version) -> (m1, w1s, table): the table of bare tensors, built once


def _fold_lo_cached(m1: torch.Tensor, w1s: torch.Tensor) -> torch.Tensor:
    key = (m1.data_ptr(), m1._version, w1s.data_ptr(), w1s._version)
    hit = _LO_TABLES.get(key)
    if hit is None:
        # Entries are dropped only while no stream is capturing, oldest first, and never the one in use.  A graph captured with bare
        # tensors holds the table's ADDRESS, not the tensor: a caller that replays such a graph after 64 other weight pairs have
        # passed through here must pass the table itself (folded[3]), as the model's cache does.
        if len(_LO_TABLES) >= 64 and not torch.cuda.is_current_stream_capturing():
            _LO_TABLES.pop(next(iter(_LO_TABLES)))
        hit = (m1, w1s, fold_lo_table(m1, w1s))      # (the operands are held: their addresses cannot be reused under the key)
        _LO_TABLES[key] = hit
    return hit[2]


def gcn_layer_cls_fold_fwd(graph: Graph, batch: int, x: torch.Tensor, folded, residual: bool, packed: dict, sigmoid: bool = False,
                           kidsum_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gcn_layer_cls_fwd for a last layer without ReLU and without jk_in, from ``folded`` = (m1, w1s, c1) of
    nn._heads.fold_last_into_heads (the layer's weight, scale and shift and the heads' w1, s1, t1 in one); ``residual``: the
    layer adds its input.  Same logits to rounding; the layer's output tile is never formed.  The products run on the bf16 matrix
    path from exact splits (eg_gcn_layer_cls_fold_split_fwd; a handle created under EG_LAYER_SPLIT=0 runs the fp32 body of
    eg_gcn_layer_cls_fold_fwd); ``folded`` may carry the lo-plane table of fold_lo_table as a fourth element, otherwise it is built
    here once per (address, version) of m1 and w1s."""
    rows = graph.num_nodes * batch
    m1, w1s, c1 = folded[:3]
    lo = folded[3] if len(folded) > 3 else _fold_lo_cached(m1, w1s)      # (the model's cache brings the table along)
    _check_rows(x, "x", rows)
    _check(m1, "m1", (C, C))
    _check(w1s, "w1s", (C, C))
    _check(c1, "c1", numel=C)
    _check_rows(kidsum_in, "kidsum_in", graph.kidsum_rows * batch, optional=True)
    out = torch.empty((graph.num_nodes - graph.num_conn) * batch, 4, dtype=torch.float32, device=x.device)
    _check(lo, "lo planes", (2, 4, 4, 2, 4, 16, 8), dtype=torch.int16)
    call("eg_gcn_layer_cls_fold_split_fwd", graph._h, batch, x, bool(residual), kidsum_in, m1, w1s, c1, lo,
         *[packed[k] for k in _HEAD_KEYS[3:]], sigmoid, out)
    return out


def new_kidsum(graph: Graph, batch: int) -> Optional[torch.Tensor]:
    """Zero-filled child-sum side buffer [batch * kidsum_rows, 128] for chained layers, or None when the
    topology does not qualify (generic CSR handles, irregular frames)."""
    rows = graph.kidsum_rows
    if rows == 0:
        return None
    return torch.zeros(rows * batch, C, device=graph.device, dtype=torch.float32)


def gcn_aggregate(graph: Graph, batch: int, x: torch.Tensor) -> torch.Tensor:
    """A_hat x (symmetric-normalised adjacency with self loops)."""
    _check_rows(x, "x", graph.num_nodes * batch)
    out = torch.empty_like(x)
    call("eg_gcn_aggregate", graph._h, batch, x, out)
    return out


def linear128_fwd(x: torch.Tensor, weight: torch.Tensor, scale=None, shift=None, residual=None, relu: bool = False,
                  transpose_w: bool = False) -> torch.Tensor:
    _check_rows(x, "x")
    _check_vec(scale, "scale", C)
    _check_vec(shift, "shift", C)
    _check_rows(residual, "residual", x.shape[0], optional=True)
    out = torch.empty_like(x)
    call("eg_linear128_fwd", x, x.shape[0], weight.contiguous(), scale, shift, residual, relu, transpose_w, out)
    return out


def classifier_fwd(h: torch.Tensor, batch: int, n_per_frame: int, row_lo: int, n_valid: int, packed: dict,
                   sigmoid: bool = False) -> torch.Tensor:
    """node-type filter (contiguous row range per frame) + the 4 heads -> [batch*n_valid, 4]."""
    _check_rows(h, "h", batch * n_per_frame)
    out = torch.empty(batch * n_valid, 4, dtype=torch.float32, device=h.device)
    call("eg_classifier_fwd", h, batch, n_per_frame, row_lo, n_valid, *[packed[k] for k in _HEAD_KEYS], sigmoid, out)
    return out


_HEAD_SHAPES = {"w1": (C, C), "s1": (C,), "t1": (C,), "w2": (4, 16, 32), "s2": (64,), "t2": (64,), "w3": (4, 16), "b3": (4,)}


def conv1x1_relu_heads(feats, weights, biases, batch: int, packed: dict, sigmoid: bool = False) -> torch.Tensor:
    """``classifier_fwd(conv1x1_relu_pack_levels(feats, weights, biases, batch, sum p_l^2), ...)`` in ONE launch
    (eg_conv1x1_relu_heads_fwd), bit for bit: relu(Conv2d(C_l, 128, 1)(feats[l])) of every level (coarse to fine) goes from LDS
    straight into the 4 heads, the node-major [batch * N, 128] rows are never written.  -> logits [batch * sum p_l^2, 4]; row
    b * sum + sum_{k<l} p_k^2 + pos is position pos of level l of frame b.  Inference only: nothing here is differentiable."""
    batch = int(batch)
    feats = [f.detach().contiguous() for f in feats]
    weights = [w.detach().contiguous() for w in weights]
    biases = [b.detach().contiguous() if b is not None else None for b in biases]
    feats, biases, chans, sides = _conv_levels(feats, weights, biases, batch)
    for k in _HEAD_KEYS:
        _check(packed[k], k, _HEAD_SHAPES[k])
    out = torch.empty(batch * sum(p * p for p in sides), 4, dtype=torch.float32, device=feats[0].device)
    call("eg_conv1x1_relu_heads_fwd", _addresses(feats), _addresses(weights), _addresses(biases), _ints(chans), _ints(sides), len(feats),
         batch, *[packed[k] for k in _HEAD_KEYS], bool(sigmoid), out)
    return out
