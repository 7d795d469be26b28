"""-m gpu: the CNN-pyramid block in training mode (csrc/pyramid_conv.hip, csrc/pyramid_train.hip; ops.pyramid_block_train,
nn.CNNHierarchicalPatchModel.enable_hip_pyramid(True, train=True)).  (batch, side, side_out) names a shape.

1. bitwise against the existing entry points where the order of summation is theirs (the forward convolution, the data gradient,
   the p = 0 forward);
2. exact integer sums: inputs from {-1, 0, 1, 2}, every sum exact in fp32 whatever the order, so z, dx and dw3 equal the CPU's;
3. against float64, by test_gpu_embedder.py's rule  max|hip - fp64| <= max(8 max|cpu32 - fp64|, 1e-6 max|fp64|)  (db3, whose true
   value is zero: 8 n 2^-24 max|dz64| as the floor).  The argmax and the ReLU gate are discontinuous: at the two smallest shapes the
   references are asserted to be far from every tie and zero, at the larger ones the kernel's own choices are injected into both
   references and checked at every window;
4. masks and skipped launches;  5. reproducible and capturable;  6. through the model."""
import copy

import pytest
import torch
import torch.nn.functional as F

from echoglad_amd import ops
from echoglad_amd.nn import CNNHierarchicalPatchModel
from echoglad_amd.ops import embedder as E
from echoglad_amd.synthetic import fill_state_dict
from embedder_util import block_fixture, plane_keep
from gpu_util import DEV, graph_tensors
from oracle import gnn_oracle as O
from pyramid_train_reference import pooled_dout, pyramid_block_reference, window_gap, window_max

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MARGIN = 64
C = 128
GRADS = ("dx", "dw3", "db3", "dgamma", "dbeta")


def _new(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def _ints(shape, seed):
    """Values from {-1, 0, 1, 2}."""
    return torch.randint(-1, 3, shape, generator=torch.Generator().manual_seed(seed)).float()


def _within(name, hip, r64, r32, floor=None):
    assert hip is not None and tuple(hip.shape) == tuple(r64.shape), (name, None if hip is None else tuple(hip.shape), tuple(r64.shape))
    e_hip = float((hip.detach().cpu().double() - r64).abs().max())
    e_cpu = float((r32.double() - r64).abs().max())
    tol = max(8 * e_cpu, 1e-6 * float(r64.abs().max()) if floor is None else floor)
    print(f"{name} {tuple(hip.shape)}: hip err {e_hip:.3e}, cpu fp32 err {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}, tol {tol:.3e}")
    assert torch.isfinite(hip).all() and e_hip <= tol, (name, e_hip, e_cpu, tol)


def _dev(t, grad=False):
    return None if t is None else t.detach().to(DEV).requires_grad_(grad)


def _hip_train(fx, side_out, p=0.0, seed=0, need=("x", "w3", "b3", "gamma", "beta"), record=None):
    """The block on the GPU through ops.pyramid_block_train with an nn.BatchNorm2d -> the references' dictionary, and keep.
    record: a list that takes (entry point, arguments) of every library call."""
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(fx["gamma"])
        bn.bias.copy_(fx["beta"])
        bn.running_mean.copy_(fx["rm"])
        bn.running_var.copy_(fx["rv"])
    bn.weight.requires_grad_("gamma" in need)
    bn.bias.requires_grad_("beta" in need)
    x, w3, b3 = _dev(fx["x"], "x" in need), _dev(fx["w3"], "w3" in need), _dev(fx["b3"], "b3" in need)
    inner = E.call
    if record is not None:
        E.call = lambda name, *a: record.append((name, a)) or inner(name, *a)
    try:
        out, keep = ops.pyramid_block_train(x, w3, b3, bn, side_out, p, seed, return_keep=True)
        assert isinstance(out.grad_fn, E._PyramidBlockTrain._backward_cls) and not keep.requires_grad
        (out * pooled_dout(fx, side_out).to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        E.call = inner
    grad = lambda t: None if t is None else t.grad
    return dict(out=out.detach(), rm=bn.running_mean.detach(), rv=bn.running_var.detach(), nbt=int(bn.num_batches_tracked), dx=grad(x),
                dw3=grad(w3), db3=grad(b3), dgamma=grad(bn.weight), dbeta=grad(bn.bias)), keep.detach()


def _arg(record, name, position):
    rows = [a for n, a in record if n == name]
    assert len(rows) == 1, (name, len(rows))
    return rows[0][position]


# ---------------------------------------------------------------------------
# 1. bitwise against the existing entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch,side", [(1, 3), (1, 4),                    # the sides the issue names ...
                                        (2, 7), (2, 8),                    # ... the two sides of the training forward's threshold
                                        (1, 16), (1, 40), (2, 64), (1, 224)], ids=lambda v: str(v))
def test_conv_fwd_equals_embed_conv_fwd_bit_for_bit(batch, side):
    fx = block_fixture(batch, C, C, side, 300 + side)
    x, w, b = _dev(fx["x"]), _dev(fx["w3"]), _dev(fx["b3"])
    for bias in (b, None):
        want, got = _new(batch, C, side, side), _new(batch, C, side, side)
        E.call("eg_embed_conv_fwd", x, batch, C, side, w, bias, C, want)
        E.call("eg_pyramid_conv_fwd", x, batch, side, w, bias, got)
        assert torch.equal(got, want) and float(got.abs().max()) > 0, int((got != want).sum())


@pytest.mark.parametrize("batch,side", [(1, 17),       # the first side on the matrix route, one partial tile
                                        (1, 33),       # crosses the 32-wide tile by one
                                        (2, 40), (2, 64), (1, 224),
                                        (2, 16), (3, 4)],          # the composed route
                         ids=lambda v: str(v))
def test_conv_bwd_data_equals_the_two_existing_calls_bit_for_bit(batch, side):
    fx = block_fixture(batch, C, C, side, 400 + side)
    dz, w, ds = _dev(fx["x"]), _dev(fx["w3"]), _dev(fx["dout"])
    want = _new(batch, C, side, side)
    E.call("eg_conv3x3_bwd_data", dz, w, batch, C, side, C, side, 0, want, None, None)
    got = _new(batch, C, side, side)
    E.call("eg_pyramid_conv_bwd_data", dz, w, None, batch, side, got)
    assert torch.equal(got, want) and float(got.abs().max()) > 0, int((got != want).sum())
    E.call("eg_embed_res_bwd_input", ds, None, batch, C, C, side, want)
    E.call("eg_pyramid_conv_bwd_data", dz, w, ds, batch, side, got)
    assert torch.equal(got, want), int((got != want).sum())


P0_SHAPES = [(2, 40, 17), (1, 64, 32), (1, 33, 33), (2, 20, 1)]


@pytest.mark.parametrize("shape", P0_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_p0_forward_equals_the_embedder_block_then_the_indexed_pool(shape):
    """out bit for bit; idx wherever out > 0 (where out == 0 the pool of the rectified map picks the first zero, this block the
    largest negative of v)."""
    batch, side, side_out = shape
    fx = block_fixture(batch, C, C, side, 500 + side)
    bn = lambda: (_dev(fx["gamma"]), _dev(fx["beta"]), None, None, 1e-5, 0.1)
    x, w, b = _dev(fx["x"]), _dev(fx["w3"]), _dev(fx["b3"])
    record = []
    inner = E.call
    E.call = lambda name, *a: record.append((name, a)) or inner(name, *a)
    try:
        with torch.no_grad():
            got = ops.pyramid_block_train(x, w, b, bn(), side_out, 0.0, 0)
            full = ops.embed_block_train(x, w, b, bn(), None, None, 0.0, 0)
    finally:
        E.call = inner
    want, want_idx = _new(batch, C, side_out, side_out), _new(batch, C, side_out, side_out, dtype=torch.int32)
    E.call("eg_adaptive_max_pool_idx_fwd", full, batch * C, side, side_out, want, want_idx)
    idx = _arg(record, "eg_pyramid_act_fwd", 8)
    assert torch.equal(got, want)
    on = got > 0
    assert 0 < int(on.sum()) < on.numel() or side_out == 1
    assert torch.equal(idx[on], want_idx[on])
    assert int(idx.min()) >= 0 and int(idx.max()) < side * side


# ---------------------------------------------------------------------------
# 2. exact integer sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch,side", [(2, 3), (3, 4), (2, 17), (1, 40)], ids=lambda v: str(v))
def test_integer_forward_and_data_gradient_are_exact(batch, side):
    x, w, b = _ints((batch, C, side, side), 1), _ints((C, C, 3, 3), 2), _ints((C,), 3)
    ds = _ints((batch, C, side, side), 4)
    z = _new(batch, C, side, side)
    E.call("eg_pyramid_conv_fwd", x.to(DEV), batch, side, w.to(DEV), b.to(DEV), z)
    assert torch.equal(z.cpu(), F.conv2d(x, w, b, padding=1))
    dx = _new(batch, C, side, side)
    E.call("eg_pyramid_conv_bwd_data", x.to(DEV), w.to(DEV), ds.to(DEV), batch, side, dx)         # x stands for dz
    assert torch.equal(dx.cpu(), F.conv_transpose2d(x, w, padding=1) + ds)


def _wgrad(x, dz):
    batch, side = int(x.shape[0]), int(x.shape[2])
    nbytes = int(E.raw("eg_pyramid_train_workspace_bytes", batch, side, side))
    assert 0 < nbytes < 40 << 20
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dw = _new(C, C, 3, 3)
    E.call("eg_pyramid_conv_bwd_weight", x.to(DEV), dz.to(DEV), batch, side, ws, dw)
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("batch,side", [(5, 3),        # 45 pixels, five tiles of one frame each, five slices
                                        (2, 17),       # 578 pixels
                                        (3, 40),       # 4800 pixels over three frames, no multiple of 256; 30 tiles, 30 slices
                                        (1, 64),       # 16 full tiles
                                        (1, 224),      # 50176 terms, |sum| < 2^24; 196 tiles in 49 slices of 4: slices of several tiles
                                        (16448, 2)],   # 257 tiles per slice: crosses the fold of 256 tile sums into the next level,
                                                       # which none of the shapes above does (|sum| <= 4 * 65792 < 2^24)
                         ids=lambda v: str(v))
def test_integer_weight_gradient_is_exact(batch, side):
    """The CPU's float32 result is exact as well, whatever its order (every partial sum is an integer below 2^24)."""
    x, dz = _ints((batch, C, side, side), 5), _ints((batch, C, side, side), 6)
    want = torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), dz, padding=1)
    assert float(want.abs().max()) < 2 ** 24 and float(want.abs().max()) > 0
    got = _wgrad(x, dz)
    assert torch.equal(got, want), int((got != want).sum())


def _ramp(batch, side):
    c = torch.arange(C).view(1, C, 1, 1)
    yy, xx = torch.arange(side).view(1, 1, side, 1), torch.arange(side).view(1, 1, 1, side)
    t = (1 + xx + 37 * yy + 1601 * c + 250007 * torch.arange(batch).view(batch, 1, 1, 1)).float()
    assert float(t.max()) * 2 < 2 ** 24
    return t


def test_single_taps_move_planes_exactly_in_the_data_gradient():
    """Nine weights, one per tap, each between a pair (o, c) of its own: dx[c] is dz[o] moved by exactly that tap's offset, zeros
    moving in at every edge; every other plane of dx is zero (then ds alone, added afterwards)."""
    batch, side = 2, 40
    dz, ds = _ramp(batch, side), _ints((batch, C, side, side), 7)
    w = torch.zeros(C, C, 3, 3)
    want = torch.zeros(batch, C, side, side)
    padded = F.pad(dz, (1, 1, 1, 1))
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        o, c = 5 + 11 * tap, 120 - 13 * tap
        w[o, c, ky, kx] = 1.0
        # z[o, y, x] reads x[c, y + ky - 1, x + kx - 1], so dx[c, Y, X] = dz[o, Y - ky + 1, X - kx + 1]
        want[:, c] = padded[:, o, 2 - ky:2 - ky + side, 2 - kx:2 - kx + side]
    got = _new(batch, C, side, side)
    E.call("eg_pyramid_conv_bwd_data", dz.to(DEV), w.to(DEV), None, batch, side, got)
    assert torch.equal(got.cpu(), want)
    E.call("eg_pyramid_conv_bwd_data", dz.to(DEV), w.to(DEV), ds.to(DEV), batch, side, got)
    assert torch.equal(got.cpu(), want + ds)
    assert torch.equal(want, F.conv_transpose2d(dz, w, padding=1))


def test_single_pixels_pick_patches_exactly_in_the_weight_gradient():
    """dz is one 1 per chosen (frame, o) at a corner, an edge or across a tile border: dw3[o][c] is the 3 x 3 patch of x[c] around
    that pixel, tap (ky, kx) at offset (ky - 1, kx - 1), zeros where the patch leaves the map."""
    batch, side = 2, 40
    x = _ramp(batch, side)
    dz = torch.zeros(batch, C, side, side)
    spots = {5: (0, 0, 0), 6: (0, side - 1, side - 1), 7: (1, 0, side - 1), 8: (1, side - 1, 0), 9: (0, 7, 31), 70: (1, 8, 32), 127: (1, 17, 5)}
    padded = F.pad(x, (1, 1, 1, 1))
    want = torch.zeros(C, C, 3, 3)
    for o, (b, y, xx) in spots.items():
        dz[b, o, y, xx] = 1.0
        want[o] = padded[b, :, y:y + 3, xx:xx + 3]
    got = _wgrad(x, dz)
    assert torch.equal(got, want)
    assert torch.equal(want, torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), dz, padding=1))


# ---------------------------------------------------------------------------
# 3. against float64
# ---------------------------------------------------------------------------
def _compare(name, fx, hip, r64, r32):
    n = fx["B"] * fx["side"] ** 2
    for t in ("out", "rm", "rv") + GRADS:
        _within(f"{name} {t}", hip[t], r64[t], r32[t], floor=8 * n * U * float(r64["dz"].abs().max()) if t == "db3" else None)
    assert hip["nbt"] == 1


@pytest.mark.parametrize("shape", [(2, 3, 2),          # the composed routes, overlapping 2-wide windows
                                   (3, 4, 2)],         # one tile, 4 of its 32 columns
                         ids=lambda s: "x".join(map(str, s)))
def test_against_float64_far_from_every_tie(shape):
    """Nothing injected.  On the references alone: the float32 argmax is the float64 argmax, every window's two largest v64 are
    64 max|v32 - v64| apart, and so is every pooled v64 from zero (seed 0; a CPU scan gave gap ratios 2584 and 591 and zero-distance
    ratios 744 and 3058)."""
    batch, side, side_out = shape
    fx = block_fixture(batch, C, C, side, seed=0)
    r64, r32 = pyramid_block_reference(fx, torch.float64, side_out), pyramid_block_reference(fx, torch.float32, side_out)
    err = float((r32["v"].double() - r64["v"]).abs().max())
    gap, zero = float(window_gap(r64["v"], side_out).min()), float(r64["m"].abs().min())
    print(f"{shape}: max|v32 - v64| = {err:.3e}, gap ratio {gap / err:.0f}, zero-distance ratio {zero / err:.0f}")
    assert torch.equal(r32["idx"], r64["idx"]) and gap >= MARGIN * err and zero >= MARGIN * err
    hip, keep = _hip_train(fx, side_out)
    assert torch.equal(keep, torch.ones_like(keep))
    _compare(f"{shape}", fx, hip, r64, r32)


@pytest.mark.parametrize("shape", [(1, 17, 8),
                                   (2, 40, 17),        # irregular overlapping windows, partial tiles both ways
                                   (1, 33, 33),        # no pooling
                                   (2, 20, 1)],        # a global maximum
                         ids=lambda s: "x".join(map(str, s)))
def test_against_float64_with_the_kernels_choices_injected(shape):
    """The margins cannot hold here (the scan gave 29 - 46 at (1, 17, 8) and 6 - 10 at (2, 40, 17)): the kernel's idx and its gate
    out > 0 go into both references, and are themselves checked at EVERY window with t = 8 max|v32 - v64|."""
    batch, side, side_out = shape
    fx = block_fixture(batch, C, C, side, seed=0)
    record = []
    hip, keep = _hip_train(fx, side_out, record=record)
    assert torch.equal(keep, torch.ones_like(keep))
    idx = _arg(record, "eg_pyramid_act_fwd", 8).cpu()
    gate = (hip["out"] > 0).cpu()
    r64 = pyramid_block_reference(fx, torch.float64, side_out, idx=idx, gate=gate)
    r32 = pyramid_block_reference(fx, torch.float32, side_out, idx=idx, gate=gate)
    t = 8 * float((r32["v"].double() - r64["v"]).abs().max())
    assert int(idx.min()) >= 0 and int(idx.max()) < side * side
    assert bool((r64["m"] >= window_max(r64["v"], side_out) - t).all())                         # v64[idx] is a maximum of its window
    sure = r64["m"].abs() > t
    assert torch.equal(gate[sure], (r64["m"] > 0)[sure])
    assert 0 < int(gate.sum()) < gate.numel() or side_out == 1                                  # (a global maximum is positive everywhere)
    print(f"{shape}: t = {t:.3e}, {int((~sure).sum())} of {sure.numel()} pooled values within t of zero")
    _compare(f"{shape}", fx, hip, r64, r32)


# ---------------------------------------------------------------------------
# 4. masks and skipping
# ---------------------------------------------------------------------------
def test_plane_dropout():
    shape, seed, p = (2, 20, 9), 0x1234_5678_9ABC, 0.5
    batch, side, side_out = shape
    fx = block_fixture(batch, C, C, side, seed=11)
    epoch0 = ops.dropout_epoch()
    try:
        ops.dropout_epoch_set(5)
        want = plane_keep(seed + 5, batch * C, p)
        assert 0 < int((want == 0).sum()) < batch * C and set(want.tolist()) == {0.0, 2.0}
        record = []
        hip, keep = _hip_train(fx, side_out, p=p, seed=seed, record=record)
        assert torch.equal(keep.cpu(), want)
        plain, _ = _hip_train(fx, side_out)
        assert torch.equal(hip["out"], plain["out"] * keep.view(batch, C, 1, 1))
        assert torch.equal(hip["rm"], plain["rm"]) and torch.equal(hip["rv"], plain["rv"])
        dropped = (keep == 0).view(batch, C)
        ds = _arg(record, "eg_pyramid_act_bwd", 12)
        assert float(hip["out"][dropped].abs().max()) == 0 and float(ds[dropped].abs().max()) == 0      # zero out, zero gp
        assert float(ds[~dropped].abs().max()) > 0
        ops.dropout_epoch_set(6)
        _, keep6 = _hip_train(fx, side_out, p=p, seed=seed)
        assert torch.equal(keep6.cpu(), plane_keep(seed + 6, batch * C, p)) and not torch.equal(keep6, keep)
    finally:
        ops.dropout_epoch_set(epoch0)


@pytest.mark.parametrize("only", ["x", "w3", "bn"])
def test_a_gradient_that_is_not_asked_for_is_none_and_its_launch_is_skipped(only):
    shape = (2, 40, 17)
    fx = block_fixture(shape[0], C, C, shape[1], seed=0)
    full, _ = _hip_train(fx, shape[2])
    record = []
    hip, _ = _hip_train(fx, shape[2], need={"x": ("x",), "w3": ("w3",), "bn": ("gamma", "beta")}[only], record=record)
    keys = {"x": ("dx",), "w3": ("dw3",), "bn": ("dgamma", "dbeta")}[only]
    for k in GRADS:
        if k in keys:
            assert torch.equal(hip[k], full[k]), k                                    # the same bits as with every gradient asked for
        else:
            assert hip[k] is None, k
    names = [n for n, _ in record]
    forward = ["eg_pyramid_conv_fwd", "eg_bn2d_train_fwd", "eg_pyramid_act_fwd", "eg_pyramid_act_bwd"]
    assert names == forward + {"x": ["eg_pyramid_conv_bwd_data"], "w3": ["eg_pyramid_conv_bwd_weight"], "bn": []}[only]
    bwd = _arg(record, "eg_pyramid_act_bwd", slice(14, 17))                          # dgamma, dbeta, db3
    assert [a is not None for a in bwd] == [only == "bn", only == "bn", False]


def test_double_backward_raises():
    fx = block_fixture(2, C, C, 3, seed=2)
    x = _dev(fx["x"], True)
    y = ops.pyramid_block_train(x, _dev(fx["w3"]), None, (None, None, None, None, 1e-5, 0.1), 2, 0.0, 0)
    gx, = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


# ---------------------------------------------------------------------------
# 5. reproducible and capturable
# ---------------------------------------------------------------------------
def test_reproducible_and_capturable():
    batch, side, side_out, p, seed = 2, 40, 17, 0.3, 99
    fx = block_fixture(batch, C, C, side, seed=21)
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(fx["gamma"])
        bn.bias.copy_(fx["beta"])
    w3, b3 = _dev(fx["w3"], True), _dev(fx["b3"], True)
    params = [w3, b3, bn.weight, bn.bias]
    dout = pooled_dout(fx, side_out).to(DEV)
    state0 = copy.deepcopy(bn.state_dict())
    epoch0 = ops.dropout_epoch()

    def run(x):
        out, keep = ops.pyramid_block_train(x, w3, b3, bn, side_out, p, seed, return_keep=True)
        (out * dout).sum().backward()
        return out, keep

    def snapshot(out, keep, x):
        return [out.detach().clone(), keep.clone(), x.grad.clone()] + [q.grad.clone() for q in params] + [b.clone() for b in bn.buffers()]

    def eager(epoch):
        bn.load_state_dict(state0)
        for q in params:
            q.grad = None
        ops.dropout_epoch_set(epoch)
        x = _dev(fx["x"], True)
        out, keep = run(x)
        torch.cuda.synchronize()
        return snapshot(out, keep, x)

    try:
        first, again = eager(9), eager(9)
        assert len(first) == 3 + 4 + 3 and all(torch.equal(a, b) for a, b in zip(first, again))
        assert all(torch.isfinite(t).all() for t in first) and 0 < int((first[1] == 0).sum()) < batch * C
        want = [eager(10 + k) for k in range(3)]

        static = _dev(fx["x"], True)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):                                   # warm-up on the capture stream: its scratch exists afterwards
            run(static)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        for q in params + [static]:
            q.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.dropout_epoch_add(1)
            out, keep = run(static)
        bn.load_state_dict(state0)
        ops.dropout_epoch_set(9)
        masks = []
        for k in range(3):
            bn.load_state_dict(state0)
            graph.replay()
            torch.cuda.synchronize()
            assert ops.dropout_epoch() == 10 + k
            assert all(torch.equal(a, b) for a, b in zip(snapshot(out, keep, static), want[k])), k
            masks.append(keep.clone())
        assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    finally:
        ops.dropout_epoch_set(epoch0)


# ---------------------------------------------------------------------------
# 6. through the model
# ---------------------------------------------------------------------------
KW = dict(frame_size=32, num_aux_graphs=4, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3,
          output_activation="logit", gnn_dropout_p=0.0, classifier_dropout_p=0.0)


def _cpu_train_step(model, frames, ei, nt, weight, dtype):
    """One training forward + backward of a CPU copy in `dtype`: the pyramid from its torch modules (the parent route), the GNN
    stack from the oracle -> logits and the two gradients."""
    B = frames.shape[0]
    m = copy.deepcopy(model).cpu().to(dtype).train()
    m.enable_hip_pyramid(False)
    ref = O.OracleHierarchicalPatchModel(**KW)
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items() if not k.startswith("conv")}, strict=True)
    ref = ref.to(dtype).train()
    x = frames.cpu().to(dtype)
    outs = m.pyramid_maps(x)
    maps = [outs[len(outs) - 1 - g] for g in range(m.num_aux_graphs)] + [x]
    rows = torch.cat([t[i].permute(1, 2, 0).reshape(-1, 128) for i in range(B) for t in maps], dim=0)
    logits = ref.forward_nodes(rows, ei.cpu(), nt, B)[0]
    (logits * weight.cpu().to(dtype)).sum().backward()
    return dict(logits=logits.detach(), w0=m.conv[0].conv.weight.grad, g3=m.conv[3].bn.weight.grad,
                nbt=int(m.conv[0].bn.num_batches_tracked))


def test_through_the_model(monkeypatch):
    """p = 0 everywhere, so no mask needs injecting."""
    B, frame = 2, 32
    model = CNNHierarchicalPatchModel(cnn_layers_out_width=[16, 8, 4, 2], cnn_dropout_p=0.0, **KW)
    fill_state_dict(model, 9)
    model = model.to(DEV).train()
    topo, ei, nt, _ = graph_tensors(frame, 4, B)
    ei = ei.to(DEV)
    g = torch.Generator().manual_seed(13)
    frames = (0.5 * torch.randn(B, 128, frame, frame, generator=g)).to(DEV)
    weight = torch.randn(B * topo.num_valid_nodes, 4, generator=g).to(DEV)
    r64, r32 = (_cpu_train_step(model, frames, ei, nt, weight, dt) for dt in (torch.float64, torch.float32))

    calls, seeds = [], []
    real = E.pyramid_block_train
    monkeypatch.setattr(E, "pyramid_block_train", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert model.enable_hip_pyramid(True, train=True) is model
    model.dropout_seed_hook = lambda kind, where, s: seeds.append((kind, where, s))
    logits = model(x=frames, edge_index=ei)[0]
    (logits * weight).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 4 and [s for s in seeds if s[0] == "pyramid"] == [("pyramid", i, (0,)) for i in range(4)]
    assert int(model.conv[0].bn.num_batches_tracked) == r64["nbt"] == 1
    _within("logits", logits, r64["logits"], r32["logits"])
    _within("conv.0.conv.weight.grad", model.conv[0].conv.weight.grad, r64["w0"], r32["w0"])
    _within("conv.3.bn.weight.grad", model.conv[3].bn.weight.grad, r64["g3"], r32["g3"])
    # eval under no_grad stays on the eval route; training without autograd on the torch modules
    del calls[:]
    with torch.no_grad():
        model.pyramid_maps(frames)
    assert not calls and int(model.conv[0].bn.num_batches_tracked) == 2
