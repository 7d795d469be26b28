"""-m gpu: the CNN-pyramid block (csrc/pyramid_conv.hip; ops.pyramid_block, nn.CNNHierarchicalPatchModel.enable_hip_pyramid).

The convolution on the f32-input matrix instruction sums in the order of the embedder's vector kernel (k = c * 9 + 3 dy + dx
ascending, one fmaf chain per output) and repeats its epilogue, so ops.embed_block -- tested against float64 in
test_gpu_embedder.py -- is the oracle here and the comparison is torch.equal.  Against float64 the rule is that file's:
    max|hip - fp64| <= max(8 max|cpu32 - fp64|, 1e-6 max|fp64|)
with the same block from torch modules on the CPU in float64 as the truth and in float32 as the yardstick."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from echoglad_amd import ops
from echoglad_amd.nn import CNNHierarchicalPatchModel
from echoglad_amd.ops import embedder as E_ops
from echoglad_amd.synthetic import fill_state_dict
from embedder_util import block_fixture, block_module
from gpu_util import DEV, graph_tensors
from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu


def _args(fx, bias=True, gamma=True):
    d = lambda t: t.to(DEV)
    bn = (d(fx["gamma"]) if gamma else None, d(fx["beta"]), d(fx["rm"]), d(fx["rv"]), 1e-5)
    return d(fx["x"]), d(fx["w3"]), d(fx["b3"]) if bias else None, bn


def _within(name, hip, r64, r32):
    e_hip = float((hip.detach().cpu().double() - r64).abs().max())
    e_cpu = float((r32.double() - r64).abs().max())
    tol = max(8 * e_cpu, 1e-6 * float(r64.abs().max()))
    print(f"{name} {tuple(hip.shape)}: hip err {e_hip:.3e}, cpu fp32 err {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}, tol {tol:.3e}")
    assert torch.isfinite(hip).all() and e_hip <= tol, (name, e_hip, e_cpu, tol)


# ---------------------------------------------------------------------------
# bitwise against the existing kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch,side", [(1, 32),       # one tile
                                        (1, 40),       # partial tiles in x and y: the masking, the zero padding at a non-tile edge
                                        (2, 64),       # halos between tiles, the batch stride
                                        (1, 16),       # one tile, half of its columns masked (the issue had this side on the fallback route;
                                                       # the measured threshold is lower: DESIGN 3.6d)
                                        (3, 4),        # the smallest side on the matrix route: 4 of 32 columns, 4 of 8 rows
                                        (2, 3)])       # the fallback route
def test_no_pool_equals_embed_block_bit_for_bit(batch, side):
    x, w, b, bn = _args(block_fixture(batch, 128, 128, side, 100 + side))
    with torch.no_grad():
        want = ops.embed_block(x, w, b, bn)
        got = ops.pyramid_block(x, w, b, bn, side)
    assert got.shape == want.shape == (batch, 128, side, side)
    assert torch.equal(got, want), int((got != want).sum())


def test_without_conv_bias_and_bn_weight():
    x, w, b, bn = _args(block_fixture(1, 128, 128, 40, 7), bias=False, gamma=False)
    assert b is None and bn[0] is None
    with torch.no_grad():
        assert torch.equal(ops.pyramid_block(x, w, b, bn, 40), ops.embed_block(x, w, b, bn))


@pytest.mark.parametrize("batch,side,side_out", [(2, 40, 17),       # irregular, overlapping windows
                                                 (1, 64, 32),       # exactly 2 x 2
                                                 (1, 224, 128)])    # the real shape of the first block: 14.8 GFLOP
def test_with_the_pool_equals_embed_block_then_torchs_pool(batch, side, side_out):
    x, w, b, bn = _args(block_fixture(batch, 128, 128, side, 200 + side))
    with torch.no_grad():
        want = F.adaptive_max_pool2d(ops.embed_block(x, w, b, bn), side_out)
        got = ops.pyramid_block(x, w, b, bn, side_out)
    assert got.shape == want.shape == (batch, 128, side_out, side_out)
    assert torch.equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------
def test_against_float64():
    """The CPU CNNResBlock (pool, then ReLU: the reference's order) in float64 is the truth, the same block in float32 the
    yardstick.  ReLU and max are 1-Lipschitz: no margin condition on the fixture."""
    fx = block_fixture(2, 128, 128, 40, 31)
    refs = []
    for dtype in (torch.float64, torch.float32):
        blk = block_module(fx, dtype, training=False)
        blk.pool = nn.AdaptiveMaxPool2d((17, 17))
        with torch.no_grad():
            refs.append(blk(fx["x"].to(dtype)))
    x, w, b, bn = _args(fx)
    with torch.no_grad():
        got = ops.pyramid_block(x, w, b, bn, 17)
    _within("block 40 -> 17", got, refs[0], refs[1])


# ---------------------------------------------------------------------------
# the layout trap
# ---------------------------------------------------------------------------
def test_single_taps_move_planes_exactly():
    """Weights zero except W[5][77][1][1] = 1 (an asymmetric pair) and W[100][3][0][2] = 1 (an off-centre tap); BatchNorm the
    identity; x a ramp of small integers that differs in x, y, channel and frame, so every sum is exact.  out = relu(conv + x):
    plane 5 is x[5] + x[77], plane 100 is x[100] + x[3] moved by (dy, dx) = (0, 2) - 1 with zeros moving in, every other plane is
    x's own.  A row / column or tap transposition that random data hides behind a tolerance shows here."""
    B, side = 2, 40
    c = torch.arange(128).view(1, 128, 1, 1)
    yy, xx = torch.arange(side).view(1, 1, side, 1), torch.arange(side).view(1, 1, 1, side)
    x = (1 + xx + 37 * yy + 1601 * c + 250007 * torch.arange(B).view(B, 1, 1, 1)).float()
    assert float(x.max()) * 2 < 2 ** 24
    w = torch.zeros(128, 128, 3, 3)
    w[5, 77, 1, 1] = 1.0
    w[100, 3, 0, 2] = 1.0
    bn = (torch.ones(128), torch.zeros(128), torch.zeros(128), torch.ones(128), 0.0)
    want = x.clone()
    want[:, 5] += x[:, 77]
    want[:, 100, 1:, :-1] += x[:, 3, :-1, 1:]                  # out[y][x] += in[y + 0 - 1][x + 2 - 1]
    with torch.no_grad():
        got = ops.pyramid_block(x.to(DEV), w.to(DEV), None, tuple(t.to(DEV) if torch.is_tensor(t) else t for t in bn), side)
        assert torch.equal(got.cpu(), want)
        assert torch.equal(ops.embed_block(x.to(DEV), w.to(DEV), None, tuple(t.to(DEV) if torch.is_tensor(t) else t for t in bn)).cpu(), want)


# ---------------------------------------------------------------------------
# stability
# ---------------------------------------------------------------------------
PYRAMID_32 = [32, 24, 16, 12, 8, 3, 2]          # seven blocks at frame 32: no pool, the matrix route with a pool, the fallback route (side 3)


def _seven_blocks(seed):
    blocks = []
    for i, width in enumerate(PYRAMID_32):
        _, w, b, bn = _args(block_fixture(1, 128, 128, 1, seed + i))
        blocks.append((w, b, bn, width))
    return blocks


def _run(blocks, x):
    outs = []
    for w, b, bn, width in blocks:
        x = ops.pyramid_block(x, w, b, bn, width)
        outs.append(x)
    return outs


def test_two_calls_give_equal_bits_and_a_captured_pyramid_replays():
    blocks = _seven_blocks(50)
    g = torch.Generator().manual_seed(51)
    batches = [torch.randn(2, 128, 32, 32, generator=g).to(DEV) for _ in range(4)]
    with torch.no_grad():
        eager = [[m.clone() for m in _run(blocks, f)] for f in batches]
        again = _run(blocks, batches[0])                                         # (also the warm-up of the capture)
        assert [m.shape[2] for m in again] == PYRAMID_32
        assert all(torch.equal(a, b) for a, b in zip(again, eager[0])) and all(torch.isfinite(m).all() for m in again)
        static = batches[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = _run(blocks, static)
        for k in (1, 2, 3):
            static.copy_(batches[k])
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, eager[k])), k


# ---------------------------------------------------------------------------
# through the model
# ---------------------------------------------------------------------------
KW = dict(frame_size=32, num_aux_graphs=4, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3,
          output_activation="logit", gnn_dropout_p=0.0, classifier_dropout_p=0.0)


def _cpu_rows(model, frames, dtype):
    """create_node_pixels of a CPU copy in `dtype` with torch ops (plain levels: per frame every level coarse to fine, then the frame)."""
    m = copy.deepcopy(model).cpu().to(dtype).eval()
    with torch.no_grad():
        outs = m.pyramid_maps(frames.cpu().to(dtype))
    maps = [outs[len(outs) - 1 - g] for g in range(m.num_aux_graphs)] + [frames.cpu().to(dtype)]
    return torch.cat([t[i].permute(1, 2, 0).reshape(-1, 128) for i in range(frames.shape[0]) for t in maps], dim=0)


def test_through_the_model(monkeypatch):
    B, frame = 2, 32
    model = CNNHierarchicalPatchModel(cnn_layers_out_width=[16, 8, 4, 2], **KW)
    fill_state_dict(model, 9)
    model = model.to(DEV).eval()
    topo, ei, nt, _ = graph_tensors(frame, 4, B)
    ei = ei.to(DEV)
    g = torch.Generator().manual_seed(13)
    batches = [(0.5 * torch.randn(B, 128, frame, frame, generator=g)).to(DEV) for _ in range(3)]
    frames = batches[0]

    calls = []
    real = E_ops.pyramid_block
    monkeypatch.setattr(E_ops, "pyramid_block", lambda *a, **k: calls.append(1) or real(*a, **k))

    # node features: the HIP route against the same model with HIP off and every block's forward = embed_block + torch's pool
    with torch.no_grad():
        on = model.enable_hip_pyramid().create_node_pixels(frames, B).clone()
    assert len(calls) == 4 and on.shape == (B * topo.num_nodes, 128)
    model.enable_hip_pyramid(False)
    for blk in model.conv:
        side_out = blk.pool.output_size[0]
        monkeypatch.setattr(blk, "forward", lambda x, blk=blk, side_out=side_out: F.adaptive_max_pool2d(
            ops.embed_block(x.contiguous(), blk.conv.weight, blk.conv.bias, blk.bn), side_out))
    with torch.no_grad():
        off = model.create_node_pixels(frames, B).clone()
    assert len(calls) == 4 and torch.equal(on, off)
    monkeypatch.undo()
    monkeypatch.setattr(E_ops, "pyramid_block", lambda *a, **k: calls.append(1) or real(*a, **k))
    _within("node features", on, _cpu_rows(model, frames, torch.float64), _cpu_rows(model, frames, torch.float32))

    # logits against the float64 CPU model (the oracle's GNN stack behind the float64 pyramid)
    base = {k: v.cpu() for k, v in model.state_dict().items() if not k.startswith("conv")}
    refs = []
    for dtype in (torch.float64, torch.float32):
        ref = O.OracleHierarchicalPatchModel(**KW)
        ref.load_state_dict(base, strict=True)
        ref = ref.to(dtype).eval()
        with torch.no_grad():
            refs.append(ref.forward_nodes(_cpu_rows(model, frames, dtype), ei.cpu(), nt, B)[0])
    model.enable_hip_pyramid()
    with torch.no_grad():
        logits = model(x=frames, edge_index=ei)[0].clone()
    assert logits.shape == (B * topo.num_valid_nodes, 4)
    _within("logits", logits, refs[0], refs[1])

    # one captured graph serves every batch: the packing behind the pyramid writes the static node-feature buffer
    model.enable_hip_graph()
    del calls[:]
    with torch.no_grad():
        for k, f in enumerate(batches):
            out = model(x=f, edge_index=ei)[0].clone()
            if k == 0:
                assert float((out - logits).abs().max()) <= 1e-5 * float(logits.abs().max())
            else:
                assert not torch.equal(out, logits)
    assert model.hip_graph_captures == 1 and len(calls) == 3 * 4
    model.enable_hip_graph(False)

    # training mode, or gradients on: the torch modules
    del calls[:]
    out = model.pyramid_maps(frames)                                             # eval, autograd on
    assert not calls and out[-1].grad_fn is not None
    model.train()
    with torch.no_grad():
        model.pyramid_maps(frames)
    assert not calls
    out = model.pyramid_maps(frames)
    assert not calls and out[-1].grad_fn is not None and int(model.conv[0].bn.num_batches_tracked) == 2
    model.eval()
    with torch.no_grad():
        model.pyramid_maps(frames)
    assert len(calls) == 4
