"""Pooling and packing: the average-pool pyramid (pool.hip) and the node-feature packing of level maps, with or without the
1 x 1 convolution in front (pack.hip; its fixed-order backward: pack_train.hip)."""
from __future__ import annotations

import ctypes as ct
import sys
from typing import Optional

import torch

from ._core import C, _check, _check_rows, _check_vec, _scratch, call, raw


def _addresses(tensors):
    """void*[n] of the tensors' addresses (None: a null pointer)."""
    return (ct.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _ints(values):
    return (ct.c_int * len(values))(*values)


def pyramid_supported(x: torch.Tensor, sides) -> bool:
    """eg_avg_pool_pyramid_* cover square float32 CUDA planes up to 512 x 512 and strictly ascending sides <= the frame."""
    sides = list(sides)
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] <= 512 and
            1 <= len(sides) <= 16 and all(1 <= a < b for a, b in zip(sides, sides[1:])) and sides[-1] <= x.shape[2] and sides[0] >= 1)


def _pool_fwd(x: torch.Tensor, sides):
    B, Cn, Fr, _ = x.shape
    maps = [torch.empty(B, Cn, p, p, dtype=torch.float32, device=x.device) for p in sides]
    call("eg_avg_pool_pyramid_fwd", x, B * Cn, Fr, _ints(sides), len(sides), _addresses(maps))
    return maps


def _pool_bwd(grads, frame_grad, sides, shape, device):
    B, Cn, Fr, _ = shape
    dx = torch.empty(shape, dtype=torch.float32, device=device)
    call("eg_avg_pool_pyramid_bwd", _addresses(grads), frame_grad, B * Cn, Fr, _ints(sides), len(sides), dx)
    return dx


class _AvgPoolPyramidFn(torch.autograd.Function):
    """[B, C, F, F] -> tuple of F.adaptive_avg_pool2d(x, p) for every side p, one launch each way."""

    @staticmethod
    def forward(ctx, x, *sides):
        x = x.contiguous()
        ctx.meta = (tuple(sides), tuple(x.shape), x.device)
        return tuple(_pool_fwd(x, list(sides)))

    @staticmethod
    def backward(ctx, *grads):
        sides, shape, device = ctx.meta
        gs = [g.contiguous() if g is not None else None for g in grads]
        return (_pool_bwd(gs, None, list(sides), shape, device),) + (None,) * len(sides)


def avg_pool_pyramid(x: torch.Tensor, sides):
    """[F.adaptive_avg_pool2d(x, (p, p)) for p in sides] (strictly ascending) in one launch; differentiable w.r.t. x."""
    if not pyramid_supported(x, sides):
        raise RuntimeError("avg_pool_pyramid: square float32 CUDA planes up to 512 x 512, strictly ascending sides <= the frame")
    return list(_AvgPoolPyramidFn.apply(x, *[int(p) for p in sides]))


def _alloc_nodes(batch: int, n_rows: int, row_offset: int, used: int, device) -> torch.Tensor:
    """[batch * n_rows, 128] for a packing call: rows no level covers (connection / coordinate nodes) read as zero."""
    alloc = torch.empty if (row_offset == 0 and used == n_rows) else torch.zeros
    return alloc(batch * n_rows, C, dtype=torch.float32, device=device)


def _rows_used(maps) -> int:
    return sum(int(m.shape[2]) ** 2 for m in maps)


# ---------------------------------------------------------------------------
# connection rows: fixed-order means over rows of the node array itself (conn_rows.hip)
# ---------------------------------------------------------------------------
def conn_rows_plan(rows: int):
    """(chunks, rows_per_chunk) a source of `rows` rows is summed in (eg_conn_rows_plan: host arithmetic, a function of `rows` alone)."""
    chunks, rpc = ct.c_int(), ct.c_int()
    call("eg_conn_rows_plan", int(rows), ct.byref(chunks), ct.byref(rpc))
    return chunks.value, rpc.value


def conn_rows_chain(rows: int) -> int:
    """d(rows) of include/echoglad_hip.h: the longest chain of additions a value goes through on its way into a mean over `rows`
    rows (the rows of a row lane, the 8 lane sums, the chunk sums)."""
    chunks, rpc = conn_rows_plan(rows)
    return (-(-min(int(rows), rpc) // 8) - 1) + 7 + (chunks - 1)


def _i64(values):
    return (ct.c_int64 * len(values))(*[int(v) for v in values])


def _conn_fwd(nodes: torch.Tensor, batch: int, n_rows: int, table) -> None:
    """eg_conn_rows_fwd in place on `nodes` (checked, contiguous); `table` = (src_base, src_rows)."""
    base, rows = table
    n_conn = len(base)
    b64, r64 = _i64(base), _i64(rows)
    at = nodes.clone() if _off16(nodes) else nodes
    nbytes = int(raw("eg_conn_rows_workspace_bytes", b64, r64, n_conn, batch, n_rows))
    ws = _scratch("conn_rows", nodes.device, nbytes) if nbytes else None
    call("eg_conn_rows_fwd", at, batch, n_rows, n_conn, b64, r64, ws)
    if at is not nodes:
        nodes.copy_(at)


def _conn_bwd(d_nodes: torch.Tensor, batch: int, n_rows: int, table) -> None:
    base, rows = table
    call("eg_conn_rows_bwd", d_nodes, batch, n_rows, len(base), _i64(base), _i64(rows))


def conn_rows_fwd(nodes: torch.Tensor, batch: int, n_rows: int, src_base, src_rows) -> torch.Tensor:
    """In place on nodes [batch * n_rows, 128]: row j < len(src_base) of every frame becomes the mean over rows
    [src_base[j], src_base[j] + src_rows[j]) of that frame, in the fixed order of eg_conn_rows_fwd.  The table is free (equal or
    disjoint sources behind the connection rows).  No autograd; returns `nodes`."""
    if len(src_base) != len(src_rows):
        raise RuntimeError("one src_rows per src_base")
    _check_rows(nodes, "nodes", int(batch) * int(n_rows))
    _conn_fwd(nodes, int(batch), int(n_rows), (list(src_base), list(src_rows)))
    return nodes


def conn_rows_bwd(d_nodes: torch.Tensor, batch: int, n_rows: int, src_base, src_rows) -> torch.Tensor:
    """In place on d_nodes: the backward of `conn_rows_fwd` (eg_conn_rows_bwd) -- every row of a source range takes
    sum_j d_nodes[b, j] * (1 / src_rows[j]) over the connection rows j that name the range (j ascending; fp32 reciprocal from the
    host, multiply, add).  The connection rows themselves are left as they are.  Returns `d_nodes`."""
    if len(src_base) != len(src_rows):
        raise RuntimeError("one src_rows per src_base")
    _check_rows(d_nodes, "d_nodes", int(batch) * int(n_rows))
    if _off16(d_nodes):
        at = d_nodes.clone()
        _conn_bwd(at, int(batch), int(n_rows), (list(src_base), list(src_rows)))
        d_nodes.copy_(at)
    else:
        _conn_bwd(d_nodes, int(batch), int(n_rows), (list(src_base), list(src_rows)))
    return d_nodes


def _split_conn(args):
    """(args without it, conn_rows): the packing nodes take ``conn_rows`` as an optional trailing string behind their tensors /
    sides, so the call forms without it are the ones they always had.  Their backwards return one more None where it was given."""
    return (args[:-1], args[-1]) if args and isinstance(args[-1], str) else (args, None)


def _conn_table(conn_rows, level_rows, row_offset: int):
    """The level table of a packing call's ``conn_rows=``: None -> None; "level": connection row j = the mean of level j's rows;
    "frame": every connection row = the mean of the last level's rows.  The connection rows are the row_offset rows in front of the
    levels, one per level."""
    if conn_rows is None:
        return None
    if conn_rows not in ("level", "frame"):
        raise ValueError(f'conn_rows must be None, "level" or "frame", got {conn_rows!r}')
    n = len(level_rows)
    if row_offset != n:
        raise RuntimeError(f"conn_rows={conn_rows!r} needs one connection row per level in front of the levels: row_offset "
                           f"{row_offset} != {n} levels")
    base, row = [], row_offset
    for p in level_rows:
        base.append(row)
        row += int(p)
    if conn_rows == "frame":
        return [base[-1]] * n, [int(level_rows[-1])] * n
    return base, [int(p) for p in level_rows]


# The gradient that reaches a packing node is changed IN PLACE by the connection rows' backward only where the buffer is that node's
# alone.  The rule: it is a contiguous tensor that is no view and spans its whole storage, and nobody holds it but autograd's engine
# and the running backward -- its tensor use count, its storage use count and its Python reference count are no higher than those of
# a gradient that a probe node receives from a plain `(y * 3).sum().backward()`, measured once per process in the same call position.
# A tensor hook that kept the gradient (one more Python reference), a producer that handed the same tensor to two inputs or kept it
# (one more use), the user's own `backward(gradient=...)` tensor, a view: all of these count higher, and the add goes to a copy.
# Where the counts cannot be read (another torch), it always goes to a copy.
_grad_baseline = None


def _grad_counts(g: torch.Tensor):
    try:
        return g._use_count(), sys.getrefcount(g), torch._C._storage_Use_Count(g.untyped_storage()._cdata)
    except AttributeError:
        return None


class _GradProbeFn(torch.autograd.Function):
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x * 2.0

    @staticmethod
    def backward(ctx, d_nodes):
        _GradProbeFn.seen = _grad_counts(d_nodes)
        return d_nodes * 2.0


def _baseline():
    global _grad_baseline
    if _grad_baseline is None:
        with torch.enable_grad():
            x = torch.zeros(2, 2, requires_grad=True)
            (_GradProbeFn.apply(x) * 3.0).sum().backward()
        _grad_baseline = _GradProbeFn.seen or ()
    return _grad_baseline


def _grad_is_ours(g: torch.Tensor, counts) -> bool:
    base = _baseline()
    return bool(base) and counts is not None and all(c <= b for c, b in zip(counts, base)) and g._base is None and \
        g.is_contiguous() and g.storage_offset() == 0 and g.untyped_storage().nbytes() == g.numel() * g.element_size()


def _conn_grad(d_nodes: torch.Tensor, counts, batch: int, n_rows: int, table) -> torch.Tensor:
    """d_nodes with the connection rows' gradient added to their source rows (eg_conn_rows_bwd): in place where `_grad_is_ours`,
    else on a copy.  Contiguous and 16-byte aligned either way."""
    _check_rows(d_nodes if d_nodes.is_contiguous() else d_nodes.contiguous(), "d_nodes", batch * n_rows)
    if not (_grad_is_ours(d_nodes, counts) and not _off16(d_nodes)):
        d_nodes = d_nodes.clone(memory_format=torch.contiguous_format)
    _conn_bwd(d_nodes, batch, n_rows, table)
    return d_nodes


class _PyramidPackFn(torch.autograd.Function):
    """create_node_pixels of the base model (models.py:511-523) as ONE autograd node: pooled pyramid of the frame embedding +
    the frame itself -> node-major rows.  Forward: eg_avg_pool_pyramid_fwd + eg_pack_levels; backward: eg_unpack_levels +
    eg_avg_pool_pyramid_bwd (the frame's own rows are added there: no second [B,128,F,F] gradient for autograd to sum)."""

    @staticmethod
    def forward(ctx, x, batch, n_rows, row_offset, out, *sides):
        x = x.contiguous()
        sides, conn = _split_conn(sides)
        sides = list(sides)
        maps = _pool_fwd(x, sides) + [x]
        used = _rows_used(maps)
        table = _conn_table(conn, [int(m.shape[2]) ** 2 for m in maps], row_offset)
        if out is not None:
            nodes = _pack_out(out, [], batch, n_rows, row_offset, used)
        else:
            nodes = _alloc_nodes(batch, n_rows, row_offset, used, x.device)
        _pack_call("eg_pack_levels", maps, nodes, batch, n_rows, row_offset)
        if table is not None:
            _conn_fwd(nodes, batch, n_rows, table)
        ctx.meta = (batch, n_rows, row_offset, sides, tuple(x.shape))
        ctx.conn_table = table
        if out is not None:
            ctx.mark_dirty(out)
        return nodes

    @staticmethod
    def backward(ctx, d_nodes):
        counts = _grad_counts(d_nodes) if ctx.conn_table is not None else None
        batch, n_rows, row_offset, sides, shape = ctx.meta
        if ctx.conn_table is not None:
            d_nodes = _conn_grad(d_nodes, counts, batch, n_rows, ctx.conn_table)
        grads = [torch.empty(shape[0], shape[1], p, p, dtype=torch.float32, device=d_nodes.device) for p in sides]
        g_frame = torch.empty(shape, dtype=torch.float32, device=d_nodes.device)
        _pack_call("eg_unpack_levels", grads + [g_frame], d_nodes.contiguous(), batch, n_rows, row_offset)
        return (_pool_bwd(grads, g_frame, sides, shape, d_nodes.device),) + (None,) * (4 + len(sides) + (ctx.conn_table is not None))


def pyramid_pack(x: torch.Tensor, sides, batch: int, n_rows: int, row_offset: int = 0, out: Optional[torch.Tensor] = None,
                 conn_rows: Optional[str] = None) -> torch.Tensor:
    """Pooled pyramid (sides ascending) of x [batch,128,F,F] + x itself, packed node-major [batch * n_rows, 128] like
    ``pack_levels([adaptive_avg_pool2d(x, p) ...] + [x])``.  Differentiable w.r.t. x (not with ``out=``: written in place).
    ``conn_rows``: as in `pack_levels`."""
    if out is not None and torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("pyramid_pack into out= is not differentiable: call it under torch.no_grad() or without out=")
    _conn_table(conn_rows, [int(p) ** 2 for p in sides] + [int(x.shape[2]) ** 2], int(row_offset))        # refused here, not inside the node
    return _PyramidPackFn.apply(x, int(batch), int(n_rows), int(row_offset), out, *[int(p) for p in sides], *([conn_rows] if conn_rows else []))


# ---------------------------------------------------------------------------
# node-feature packing (pack.hip)
# ---------------------------------------------------------------------------
def _square_sides(tensors, name: str, channels: Optional[int], batch: int):
    """Sides of contiguous CUDA float32 [batch, channels (None: any), side, side] tensors, 1..16 of them."""
    if not 1 <= len(tensors) <= 16:
        raise RuntimeError(f"1..16 {name}s supported")
    for t in tensors:
        _check(t, name, (batch, channels, None, None))
        if t.shape[2] != t.shape[3]:
            raise RuntimeError(f"{name} must be square, got {tuple(t.shape)}")
    return [int(t.shape[2]) for t in tensors]


def _off16(t: Optional[torch.Tensor], side: Optional[int] = None) -> bool:
    """`t` would reach a 16-byte access of pack.hip at an address that is no multiple of 16: the node rows and a bias always move 16
    bytes per lane, a level map / feature does where side * side % 4 == 0 (a contiguous view at an odd element offset of a packed
    buffer; the entry points refuse such a pointer, so it is copied here, as ops.criteria does for eg_bce_*)."""
    return t is not None and t.data_ptr() % 16 != 0 and (side is None or (side * side) % 4 == 0)


def _pack_call(fn_name, maps, nodes, batch, n_rows, row_offset):
    sides = _square_sides(maps, "level map", C, batch)
    side = _ints(sides)
    at = nodes.clone() if _off16(nodes) else nodes
    if fn_name == "eg_pack_levels":
        maps = [m.clone() if _off16(m, p) else m for m, p in zip(maps, sides)]
        call(fn_name, _addresses(maps), side, len(maps), batch, n_rows, row_offset, at)
        if at is not nodes:
            nodes.copy_(at)
    else:
        dst = [torch.empty_like(m) if _off16(m, p) else m for m, p in zip(maps, sides)]
        call(fn_name, at, _addresses(dst), side, len(maps), batch, n_rows, row_offset)
        for m, d in zip(maps, dst):
            if d is not m:
                m.copy_(d)


class _PackLevelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, n_rows, row_offset, *maps):
        maps, conn = _split_conn(maps)
        maps = [m.contiguous() for m in maps]
        nodes = _alloc_nodes(batch, n_rows, row_offset, _rows_used(maps), maps[0].device)
        _pack_call("eg_pack_levels", maps, nodes, batch, n_rows, row_offset)
        ctx.conn_table = _conn_table(conn, [int(m.shape[2]) ** 2 for m in maps], row_offset)
        if ctx.conn_table is not None:
            _conn_fwd(nodes, batch, n_rows, ctx.conn_table)
        ctx.meta = (batch, n_rows, row_offset, [tuple(m.shape) for m in maps])
        return nodes

    @staticmethod
    def backward(ctx, d_nodes):
        counts = _grad_counts(d_nodes) if ctx.conn_table is not None else None
        batch, n_rows, row_offset, shapes = ctx.meta
        if ctx.conn_table is not None:
            d_nodes = _conn_grad(d_nodes, counts, batch, n_rows, ctx.conn_table)
        grads = [torch.empty(s, dtype=torch.float32, device=d_nodes.device) for s in shapes]
        _pack_call("eg_unpack_levels", grads, d_nodes.contiguous(), batch, n_rows, row_offset)
        return (None, None, None, *grads, *([None] if ctx.conn_table is not None else []))


def _pack_out(out: torch.Tensor, inputs, batch: int, n_rows: int, row_offset: int, used: int) -> torch.Tensor:
    """``out=`` of the packing calls: the caller's [batch * n_rows, 128] buffer is written in place (a static node-feature
    buffer that a captured HIP graph reads: nn.HierarchicalPatchModel.enable_hip_graph).  No autograd through it."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        raise RuntimeError("pack into out= is not differentiable: call it under torch.no_grad() or without out=")
    _check_rows(out, "out", batch * n_rows)
    if row_offset > 0 or used < n_rows:              # rows no level covers (connection / coordinate nodes) read as zero, as without out=
        v = out.view(batch, n_rows, C)
        if row_offset > 0:
            v[:, :row_offset].zero_()
        if row_offset + used < n_rows:
            v[:, row_offset + used:].zero_()
    return out


def pack_levels(maps, batch: int, n_rows: int, row_offset: int = 0, out: Optional[torch.Tensor] = None,
                conn_rows: Optional[str] = None) -> torch.Tensor:
    """NCHW level maps [batch,128,p,p] (coarse to fine) -> node-major [batch * n_rows, 128]; level l lands at rows
    row_offset + sum_{k<l} p_k^2 of every frame.  Differentiable w.r.t. the maps (not with ``out=``: written in place).

    ``conn_rows`` (needs row_offset == len(maps), RuntimeError otherwise): the row_offset connection rows in front of the levels
    are filled by eg_conn_rows_fwd inside the same autograd node, right behind the packing launch -- "level": row j = the mean of
    level j's rows; "frame": every row = the mean of the last level's rows (None: they read as zero).  Fixed order of summation,
    bit-reproducible.  The backward adds sum_j d_nodes[b, j] * (1 / rows_j) to the gradient rows of the source levels in front of
    the unpacking (eg_conn_rows_bwd: fp32 reciprocal from the host, multiply, add, j ascending) -- in place where the gradient
    buffer is this node's alone, else on a copy; the rule is written out at `_grad_is_ours`."""
    table = _conn_table(conn_rows, [int(m.shape[2]) ** 2 for m in maps], int(row_offset))
    if out is not None:
        maps = [m.contiguous() for m in maps]
        _pack_out(out, maps, int(batch), int(n_rows), int(row_offset), _rows_used(maps))
        _pack_call("eg_pack_levels", maps, out, int(batch), int(n_rows), int(row_offset))
        if table is not None:
            _conn_fwd(out, int(batch), int(n_rows), table)
        return out
    return _PackLevelsFn.apply(int(batch), int(n_rows), int(row_offset), *maps, *([conn_rows] if conn_rows else []))


def _conv_levels(feats, weights, biases, batch):
    """The level arguments of the 1 x 1 convolution entry points, checked: (features, biases) with the operands that would reach a
    16-byte access off its alignment copied, the channel counts and the sides."""
    n = len(feats)
    if len(weights) != n or len(biases) != n:
        raise RuntimeError("1..16 levels, one weight and one bias (or None) per level")
    sides = _square_sides(feats, "level features", None, batch)
    chans = [int(f.shape[1]) for f in feats]
    for cin, w, b in zip(chans, weights, biases):
        _check(w, "level weight", numel=C * cin)           # [128, cin(, 1, 1)]
        if w.shape[0] != C:
            raise RuntimeError(f"level weight must be [{C}, {cin}(, 1, 1)], got {tuple(w.shape)}")
        _check_vec(b, "level bias", C)
    feats = [f.clone() if _off16(f, p) else f for f, p in zip(feats, sides)]
    biases = [b.clone() if _off16(b) else b for b in biases]
    return feats, biases, chans, sides


def _conv_pack_call(feats, weights, biases, nodes, batch, n_rows, row_offset):
    feats, biases, chans, sides = _conv_levels(feats, weights, biases, batch)
    at = nodes.clone() if _off16(nodes) else nodes
    call("eg_conv1x1_relu_pack_levels", _addresses(feats), _addresses(weights), _addresses(biases), _ints(chans), _ints(sides), len(feats),
         batch, n_rows, row_offset, at)
    if at is not nodes:
        nodes.copy_(at)


class _ConvReluPackFn(torch.autograd.Function):
    """relu(conv1x1(features[l])) of every level, packed node-major, in one launch.  The backward unpacks the node gradient to
    NCHW (eg_unpack_levels) and lets torch differentiate the recomputed relu(conv2d) of each level (the small levels carry the
    wide channel counts; the frame-sized one has 4 input channels)."""

    @staticmethod
    def forward(ctx, batch, n_rows, row_offset, n_levels, *tensors):
        tensors, conn = _split_conn(tensors)
        feats = [t.contiguous() for t in tensors[:n_levels]]
        weights = [t.contiguous() for t in tensors[n_levels:2 * n_levels]]
        biases = list(tensors[2 * n_levels:3 * n_levels])
        nodes = _alloc_nodes(batch, n_rows, row_offset, _rows_used(feats), feats[0].device)
        _conv_pack_call(feats, weights, [b.contiguous() if b is not None else None for b in biases], nodes, batch, n_rows, row_offset)
        ctx.conn_table = _conn_table(conn, [int(f.shape[2]) ** 2 for f in feats], row_offset)
        if ctx.conn_table is not None:
            _conn_fwd(nodes, batch, n_rows, ctx.conn_table)
        ctx.meta = (batch, n_rows, row_offset, n_levels)
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(*feats, *weights, *[b for b in biases if b is not None])
        return nodes

    @staticmethod
    def backward(ctx, d_nodes):
        counts = _grad_counts(d_nodes) if ctx.conn_table is not None else None
        batch, n_rows, row_offset, n = ctx.meta
        if ctx.conn_table is not None:
            d_nodes = _conn_grad(d_nodes, counts, batch, n_rows, ctx.conn_table)
        saved = ctx.saved_tensors
        feats, weights = saved[:n], saved[n:2 * n]
        bl = list(saved[2 * n:])
        biases = [bl.pop(0) if hb else None for hb in ctx.has_bias]
        g_maps = [torch.empty(batch, C, f.shape[2], f.shape[3], dtype=torch.float32, device=d_nodes.device) for f in feats]
        _pack_call("eg_unpack_levels", g_maps, d_nodes.contiguous(), batch, n_rows, row_offset)
        gf, gw, gb = [], [], []
        for l in range(n):
            need = (ctx.needs_input_grad[4 + l], ctx.needs_input_grad[4 + n + l], biases[l] is not None and ctx.needs_input_grad[4 + 2 * n + l])
            if not any(need):
                gf.append(None); gw.append(None); gb.append(None)
                continue
            with torch.enable_grad():
                f = feats[l].detach().requires_grad_(need[0])
                w = weights[l].detach().requires_grad_(need[1])
                b = biases[l].detach().requires_grad_(need[2]) if biases[l] is not None else None
                y = torch.relu(torch.nn.functional.conv2d(f, w.view(C, -1, 1, 1), b))
                ins = [t for t, k in ((f, need[0]), (w, need[1]), (b, need[2])) if k]
                outs = list(torch.autograd.grad(y, ins, g_maps[l]))
            gf.append(outs.pop(0) if need[0] else None)
            gw.append(outs.pop(0).view_as(weights[l]) if need[1] else None)
            gb.append(outs.pop(0) if need[2] else None)
        return (None, None, None, None, *gf, *gw, *gb, *([None] if ctx.conn_table is not None else []))


class _ConvReluPackHipFn(torch.autograd.Function):
    """_ConvReluPackFn with the backward in HIP (eg_conv1x1_relu_pack_bwd: two launches, no atomics, a fixed order of summation,
    so the gradients are bit-reproducible).  The node saves its own output rows: the ReLU's mask is read from them, the product is
    not recomputed and no 128-channel NCHW map is formed."""

    @staticmethod
    def forward(ctx, batch, n_rows, row_offset, n_levels, *tensors):
        tensors, conn = _split_conn(tensors)
        feats = [t.contiguous() for t in tensors[:n_levels]]
        feats = [f.clone() if _off16(f, int(f.shape[2])) else f for f in feats]          # what the backward reads is what is saved
        weights = [t.contiguous() for t in tensors[n_levels:2 * n_levels]]
        biases = list(tensors[2 * n_levels:3 * n_levels])
        nodes = _alloc_nodes(batch, n_rows, row_offset, _rows_used(feats), feats[0].device)
        _conv_pack_call(feats, weights, [b.contiguous() if b is not None else None for b in biases], nodes, batch, n_rows, row_offset)
        ctx.conn_table = _conn_table(conn, [int(f.shape[2]) ** 2 for f in feats], row_offset)
        if ctx.conn_table is not None:                  # before the rows are saved: the ReLU's mask is read from the level rows, which stay as they are
            _conn_fwd(nodes, batch, n_rows, ctx.conn_table)
        ctx.meta = (batch, n_rows, row_offset, n_levels)
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(nodes, *feats, *weights)
        return nodes

    @staticmethod
    def backward(ctx, d_nodes):
        counts = _grad_counts(d_nodes) if ctx.conn_table is not None else None
        batch, n_rows, row_offset, n = ctx.meta
        nodes, feats, weights = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        need = ctx.needs_input_grad
        dev = d_nodes.device
        gf = [torch.empty_like(f) if need[4 + l] else None for l, f in enumerate(feats)]
        gw = [torch.empty_like(w) if need[4 + n + l] else None for l, w in enumerate(weights)]
        gb = [torch.empty(C, dtype=torch.float32, device=dev) if hb and need[4 + 2 * n + l] else None for l, hb in enumerate(ctx.has_bias)]
        if all(g is None for g in gf + gw + gb):
            return (None,) * (4 + 3 * n + (ctx.conn_table is not None))
        if ctx.conn_table is not None:                  # in front of the ReLU's mask: the level rows' gradient is complete before it is gated
            d_nodes = _conn_grad(d_nodes, counts, batch, n_rows, ctx.conn_table)
        d_nodes = d_nodes.contiguous()
        _check_rows(d_nodes, "d_nodes", batch * n_rows)
        d_nodes = d_nodes.clone() if _off16(d_nodes) else d_nodes
        nodes = nodes.clone() if _off16(nodes) else nodes
        sides, chans = [int(f.shape[2]) for f in feats], [int(f.shape[1]) for f in feats]
        side, chan = _ints(sides), _ints(chans)                  # (the gradients are fresh allocations: 16-byte aligned as they are)
        ws = None
        if any(g is not None for g in gw + gb):
            ws = _scratch("tail_bwd", dev, int(raw("eg_conv1x1_relu_pack_bwd_workspace_bytes", chan, side, n, batch)))
        call("eg_conv1x1_relu_pack_bwd", d_nodes, nodes, _addresses(feats), _addresses(weights), chan, side, n, batch, n_rows, row_offset,
             ws, _addresses(gf), _addresses(gw), _addresses(gb))
        return (None, None, None, None, *gf, *gw, *gb, *([None] if ctx.conn_table is not None else []))


def conv1x1_relu_pack_levels(feats, weights, biases, batch: int, n_rows: int, row_offset: int = 0,
                             out: Optional[torch.Tensor] = None, backward: str = "torch", conn_rows: Optional[str] = None) -> torch.Tensor:
    """relu(Conv2d(C_l, 128, 1)(feats[l])) for every level (coarse to fine), written node-major [batch * n_rows, 128] like
    `pack_levels` (models.py:707-710 + :726-756 in one launch).  Differentiable w.r.t. features, weights and biases (not with
    ``out=``: written in place).  ``backward``: "torch" unpacks the node gradient to NCHW and lets torch differentiate the recomputed
    relu(conv2d) of every level (MIOpen's weight gradient: not reproducible bit for bit); "hip" is eg_conv1x1_relu_pack_bwd, a
    fixed-order backward in two launches.  ``conn_rows``: as in `pack_levels` -- the means are taken over the ACTIVATED rows, behind
    the packing launch and before the "hip" node saves its rows; both backwards add the connection rows' gradient to the level
    rows of d_nodes first (for "hip": in front of the ReLU's mask)."""
    if backward not in ("torch", "hip"):
        raise ValueError(f'backward must be "torch" or "hip", got {backward!r}')
    n = len(feats)
    table = _conn_table(conn_rows, [int(f.shape[2]) ** 2 for f in feats], int(row_offset))
    if out is not None:
        feats = [f.contiguous() for f in feats]
        weights = [w.detach().contiguous() for w in weights]
        biases = [b.detach().contiguous() if b is not None else None for b in biases]
        _pack_out(out, list(feats), int(batch), int(n_rows), int(row_offset), _rows_used(feats))
        _conv_pack_call(feats, weights, biases, out, int(batch), int(n_rows), int(row_offset))
        if table is not None:
            _conn_fwd(out, int(batch), int(n_rows), table)
        return out
    fn = _ConvReluPackHipFn if backward == "hip" else _ConvReluPackFn
    return fn.apply(int(batch), int(n_rows), int(row_offset), n, *feats, *weights, *biases, *([conn_rows] if conn_rows else []))
