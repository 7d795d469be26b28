"""-m gpu: the HIP UNet front-end (csrc/frontend.hip: eg_conv3x3_relu_bn_fwd, eg_adaptive_max_pool_fwd; nn.unet_decoder_maps;
UNetNodeFeatureModel.enable_hip_frontend) against plain torch on the CPU in float64.  Every bound is derived from the number
format or from the CPU float32 result's own error against float64, never from what the kernels return."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from echoglad_amd import ops
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import unet_decoder_maps
from echoglad_amd.topology import HierTopology, TopologySpec
from oracle import gnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _conv_input64(x0, side, x1):
    """What the kernel convolves, in float64 on the CPU: nn.Upsample(size=side)(x0) concatenated with x1."""
    x = x0.double()
    if x.shape[2] != side:
        x = nn.Upsample(size=side)(x)
    return x if x1 is None else torch.cat([x, x1.double()], dim=1)


def _conv_case(B, c0, c_out, side, side0=None, c1=0, seed=0, neg_gamma=False, bare=False):
    """One convolution on the GPU against float64, element by element, within
        s (K + 8) u S + 8 u (s (|r| + |mean|) + |beta|) + 1e-30
    (u = 2^-24, K = 9 (c0 + c1), S = conv(|x|, |w|) + |bias|, r the float64 ReLU output, s = |gamma| rsqrt(var + eps))."""
    g = torch.Generator().manual_seed(1000 + seed)
    side0 = side if side0 is None else side0
    x0 = torch.randn(B, c0, side0, side0, generator=g)
    x1 = torch.randn(B, c1, side, side, generator=g) if c1 else None
    K = 9 * (c0 + c1)
    w = torch.randn(c_out, c0 + c1, 3, 3, generator=g) / K ** 0.5
    bias = None if bare else torch.randn(c_out, generator=g) * 0.5
    gamma = None if bare else torch.rand(c_out, generator=g) + 0.5
    if neg_gamma and gamma is not None:
        gamma[::2] *= -1
    beta = None if bare else torch.randn(c_out, generator=g) * 0.3
    mean = torch.randn(c_out, generator=g) * 0.3
    var = torch.rand(c_out, generator=g) + 0.25
    eps = 1e-5
    xin = _conv_input64(x0, side, x1)
    b64 = torch.zeros(c_out, dtype=torch.float64) if bias is None else bias.double()
    r = F.relu(F.conv2d(xin, w.double(), b64, padding=1))
    S = F.conv2d(xin.abs(), w.double().abs(), b64.abs(), padding=1)
    g64 = torch.ones(c_out, dtype=torch.float64) if gamma is None else gamma.double()
    be64 = torch.zeros(c_out, dtype=torch.float64) if beta is None else beta.double()
    inv = (var.double() + eps).rsqrt()
    v = lambda t: t.view(1, -1, 1, 1)
    ref = (r - v(mean.double())) * v(inv) * v(g64) + v(be64)
    s = v(g64.abs() * inv)
    bound = s * (K + 8) * U * S + 8 * U * (s * (r.abs() + v(mean.double().abs())) + v(be64.abs())) + 1e-30
    dev = lambda t: None if t is None else t.to(DEV)
    out = ops.conv3x3_relu_bn(dev(x0), dev(w), dev(bias), (dev(gamma), dev(beta), dev(mean), dev(var), eps), side=side, x1=dev(x1))
    assert out.shape == ref.shape and out.dtype == torch.float32
    err = (out.cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"conv B={B} {c0}+{c1}->{c_out} side {side0}->{side}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(out).all() and ratio <= 1.0


# the issue's cases, then the launcher's other paths: the tile kernel's 8-channel instantiation (>= 512 workgroups) with a channel
# remainder, and the tile kernel with a resize, a concatenation and channel counts that divide nothing (sides just past the threshold)
CONV_CASES = {
    "odd_side_below_a_tile": dict(B=2, c0=4, c_out=8, side=7),
    "channels_divide_nothing": dict(B=1, c0=3, c_out=5, side=9),
    "concat": dict(B=2, c0=4, c1=4, c_out=4, side=6),
    "resize_4_to_7": dict(B=1, c0=8, c_out=4, side=7, side0=4),
    "resize_128_to_224": dict(B=1, c0=8, c_out=4, side=224, side0=128),
    "deep_512_side2": dict(B=1, c0=512, c_out=512, side=2),
    "deep_concat_256_256_side4": dict(B=1, c0=256, c1=256, c_out=256, side=4),
    "deep_batch3_side8": dict(B=3, c0=64, c_out=128, side=8),
    "negative_gamma": dict(B=2, c0=5, c_out=6, side=11, neg_gamma=True),
    "no_bias_no_affine": dict(B=2, c0=5, c_out=6, side=11, bare=True),
    "negative_gamma_tile": dict(B=1, c0=6, c_out=7, side=19, neg_gamma=True),
    "threshold_16": dict(B=2, c0=9, c1=3, c_out=6, side=16, side0=5),
    "threshold_17": dict(B=2, c0=9, c1=3, c_out=6, side=17, side0=5),
    "tile_resize_concat_odd": dict(B=2, c0=5, c1=6, c_out=9, side=40, side0=17),
    "tile_wide_remainder": dict(B=3, c0=4, c_out=10, side=224),
    "tile_partial_tiles": dict(B=1, c0=17, c_out=3, side=33),
}


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_one_convolution_against_float64(name):
    _conv_case(seed=sorted(CONV_CASES).index(name), **CONV_CASES[name])


@pytest.mark.parametrize("c_in", [3, 20])
@pytest.mark.parametrize("side", [1, 2, 3, 16, 17, 33, 224])
def test_borders_exactly(side, c_in):
    """x = 1, w = 1, no bias, identity BatchNorm (var 1, eps 0): every output is c_in times the number of taps inside the map --
    4 at corners, 6 at edges, 9 inside -- as exact integers."""
    c_out = 2
    x = torch.ones(1, c_in, side, side, device=DEV)
    w = torch.ones(c_out, c_in, 3, 3, device=DEV)
    bn = (None, None, torch.zeros(c_out, device=DEV), torch.ones(c_out, device=DEV), 0.0)
    out = ops.conv3x3_relu_bn(x, w, None, bn).cpu()
    taps = F.conv2d(torch.ones(1, 1, side, side, dtype=torch.float64), torch.ones(1, 1, 3, 3, dtype=torch.float64), padding=1)
    assert torch.equal(out.double(), (c_in * taps).expand(1, c_out, side, side))
    if side >= 3:
        assert out[0, 0, 0, 0] == 4 * c_in and out[0, 1, -1, -1] == 4 * c_in and out[0, 0, 0, -1] == 4 * c_in
        assert out[0, 0, 0, 1] == 6 * c_in and out[0, 1, side // 2, -1] == 6 * c_in and out[0, 0, -1, 1] == 6 * c_in
        assert out[0, 0, 1, 1] == 9 * c_in and out[0, 1, side // 2, side // 2] == 9 * c_in


@pytest.mark.parametrize("side0,side", [(128, 224), (4, 7), (2, 4), (5, 16), (7, 40)])
def test_resize_rule_is_nn_upsample(side0, side):
    """A centre-tap identity weight with positive input and an identity BatchNorm copies the resized input: bit-equal to
    nn.Upsample(size=side) on the CPU."""
    g = torch.Generator().manual_seed(side)
    x = torch.rand(2, 4, side0, side0, generator=g) + 0.1
    w = torch.zeros(4, 4, 3, 3)
    for c in range(4):
        w[c, c, 1, 1] = 1.0
    bn = (None, None, torch.zeros(4, device=DEV), torch.ones(4, device=DEV), 0.0)
    out = ops.conv3x3_relu_bn(x.to(DEV), w.to(DEV), None, bn, side=side)
    assert torch.equal(out.cpu(), nn.Upsample(size=side)(x))


@pytest.mark.parametrize("side_in,side_out,planes", [(224, 128, 37), (7, 3, 1), (4, 2, 37), (5, 5, 1), (16, 8, 37), (224, 128, 1)])
def test_adaptive_max_pool_is_torchs(side_in, side_out, planes):
    g = torch.Generator().manual_seed(side_in * 1000 + side_out)
    x = torch.randn(1, planes, side_in, side_in, generator=g)
    x[0, planes // 2] = -x[0, planes // 2].abs() - 0.5                # a plane of all-negative values
    out = ops.adaptive_max_pool(x.to(DEV), side_out)
    assert torch.equal(out.cpu(), F.adaptive_max_pool2d(x, side_out))


# ---------------------------------------------------------------------------
# the whole front-end
# ---------------------------------------------------------------------------
def _randomise_bn(model, seed):
    """Trained-like BatchNorms: random running statistics and affine parameters, every third gamma negative."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in list(model.down_convs.modules()) + list(model.up_convs.modules()):
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                gamma = torch.rand(n, generator=g) + 0.5
                gamma[::3] *= -1
                m.weight.copy_(gamma)
                m.bias.copy_(torch.randn(n, generator=g) * 0.2)


def _torch_maps(down_convs, up_convs, frames):
    """UNetNodeFeatureModel.decoder_maps on plain torch modules (the CPU copies)."""
    x, skips = frames, []
    for down in down_convs:
        skips.append(x)
        x = down(x)
    feats = [x]
    for up in up_convs:
        x = up(x, skips.pop())
        feats.append(x)
    return feats


def _cpu_refs(model, frames):
    """(float64 maps, float32 maps) of CPU deep copies of the model's front-end."""
    with torch.no_grad():
        d64, u64 = copy.deepcopy(model.down_convs).cpu().double().eval(), copy.deepcopy(model.up_convs).cpu().double().eval()
        d32, u32 = copy.deepcopy(model.down_convs).cpu().float().eval(), copy.deepcopy(model.up_convs).cpu().float().eval()
        return _torch_maps(d64, u64, frames.cpu().double()), _torch_maps(d32, u32, frames.cpu().float())


def _assert_within_reference_error(got, ref64, ref32, what):
    """max|hip - fp64| <= max(8 max|cpu32 - fp64|, 1e-6 max|fp64|) for every map."""
    assert len(got) == len(ref64)
    for i, (h, r64, r32) in enumerate(zip(got, ref64, ref32)):
        assert h.shape == r64.shape
        e_hip = float((h.cpu().double() - r64).abs().max())
        e_cpu = float((r32.double() - r64).abs().max())
        tol = max(8 * e_cpu, 1e-6 * float(r64.abs().max()))
        print(f"{what} map {i} {tuple(h.shape)}: hip err {e_hip:.3e}, cpu fp32 err {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}")
        assert torch.isfinite(h).all() and e_hip <= tol, (what, i, e_hip, e_cpu)


SMALL = dict(frame_size=16, num_aux_graphs=3, encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32],
             node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit",
             use_coordinate_graph=False, gnn_dropout_p=0.0, classifier_dropout_p=0.0)


def _small_model(seed=5):
    torch.manual_seed(seed)
    model = UNetNodeFeatureModel(**SMALL)
    _randomise_bn(model, seed)
    return model.to(DEV).eval()


def test_whole_front_end_small():
    model = _small_model()
    frames = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(11)).to(DEV)
    ref64, ref32 = _cpu_refs(model, frames)
    with torch.no_grad():
        got = unet_decoder_maps(model.down_convs, model.up_convs, frames)
    assert [tuple(m.shape) for m in got] == [(2, 32, 2, 2), (2, 16, 4, 4), (2, 8, 8, 8), (2, 4, 16, 16)]
    _assert_within_reference_error(got, ref64, ref32, "small")


@pytest.fixture(scope="module")
def default_model():
    torch.manual_seed(7)
    model = UNetNodeFeatureModel(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                 num_gnn_layers=3, output_activation="logit", use_coordinate_graph=True, gnn_dropout_p=0.5,
                                 classifier_dropout_p=0.5)
    _randomise_bn(model, 7)
    return model.to(DEV).eval()


def test_whole_front_end_at_the_default_shape(default_model, golden_dir):
    model = default_model.enable_hip_frontend(True)
    assert set(model.state_dict()) == set(json.load(open(os.path.join(golden_dir, "unet_state_keys.json")))["state_dict"])
    frames = torch.randn(1, 4, 224, 224, generator=torch.Generator().manual_seed(12)).to(DEV)
    ref64, ref32 = _cpu_refs(model, frames)
    with torch.no_grad():
        got = model.decoder_maps(frames)
    assert [m.shape[2] for m in got] == [2, 4, 8, 16, 32, 64, 128, 224] and [m.shape[1] for m in got] == [512, 256, 128, 64, 32, 16, 8, 4]
    _assert_within_reference_error(got, ref64, ref32, "default")


def _node_pixels_cpu(model, maps, dtype):
    """The UNet variant's tail (relu(linears[i](map_i)), node-major, per frame) on the CPU in `dtype`."""
    lin = copy.deepcopy(model.linears).cpu().to(dtype)
    with torch.no_grad():
        acts = [F.relu(m(f)) for f, m in zip(maps, lin)]
    B = maps[0].shape[0]
    return torch.cat([a[i].permute(1, 2, 0).reshape(-1, 128) for i in range(B) for a in acts], dim=0)


def test_through_the_model():
    B, frame, naux = 2, 16, 3
    model = _small_model(seed=9)
    topo = HierTopology(TopologySpec(frame, naux, False, False))
    ei = torch.from_numpy(topo.batched_edge_index(B)).to(DEV)
    g = torch.Generator().manual_seed(13)
    frames = torch.randn(B, 4, frame, frame, generator=g) * 0.3
    frames[:, :, 5:8, 9:12] += 4.0                                    # a bright blob: a peaked fixture
    frames = frames.to(DEV)
    ref64, ref32 = _cpu_refs(model, frames)
    px64, px32 = _node_pixels_cpu(model, ref64, torch.float64), _node_pixels_cpu(model, ref32, torch.float32)
    with torch.no_grad():
        off_logits = model(x=frames, edge_index=ei)[0].clone()
        model.enable_hip_frontend(True)
        px = model.create_node_pixels(frames, B).clone()
        on_logits = model(x=frames, edge_index=ei)[0].clone()
    _assert_within_reference_error([px.view(-1, 128)], [px64], [px32], "node pixels")
    assert on_logits.shape == off_logits.shape and torch.isfinite(on_logits).all()
    # the fixture is peaked: on the flag-off route the two largest main-grid logits of every (frame, channel) are further apart
    # than 100 times the largest difference between the two routes
    route = float((on_logits - off_logits).abs().max())
    per = off_logits.cpu().view(B, -1, 4)[:, -frame * frame:, :]
    top2 = per.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    print(f"route difference {route:.3e}, smallest top-two gap {gap:.3e}")
    assert gap >= 100 * route
    assert torch.equal(O.landmark_argmax(on_logits.cpu(), B, frame), O.landmark_argmax(off_logits.cpu(), B, frame))

    # flag on, but training or autograd: the torch path, bit for bit, with a graph behind it
    def maps_with(flag, train):
        model.enable_hip_frontend(flag)
        model.train(train)
        state = copy.deepcopy(model.state_dict())                     # (train-mode BatchNorms move their running statistics)
        with torch.enable_grad():
            out = model.decoder_maps(frames)
        model.load_state_dict(state)
        return out

    assert all(p.requires_grad for p in model.down_convs.parameters())
    for train in (True, False):
        off = maps_with(False, train)
        on = maps_with(True, train)
        assert all(torch.equal(a, b) for a, b in zip(on, off)) and all(m.grad_fn is not None for m in on)
    model.eval().enable_hip_frontend(True)

    # no cache: an in-place edit of a running statistic and a load_state_dict show in the next output, as float64 says
    with torch.no_grad():
        before = model.decoder_maps(frames)
        model.down_convs[0].BN1.running_var.mul_(4.0)
        edited = model.decoder_maps(frames)
    assert not torch.equal(edited[-1], before[-1])
    _assert_within_reference_error(edited, *_cpu_refs(model, frames), "edited running_var")
    other = _small_model(seed=21)
    model.load_state_dict(other.state_dict())
    with torch.no_grad():
        loaded = model.decoder_maps(frames)
    assert not torch.equal(loaded[-1], edited[-1])
    _assert_within_reference_error(loaded, *_cpu_refs(other, frames), "after load_state_dict")


def test_reproducible_and_capturable():
    model = _small_model(seed=15)
    g = torch.Generator().manual_seed(17)
    batches = [torch.randn(2, 4, 16, 16, generator=g).to(DEV) for _ in range(4)]
    with torch.no_grad():
        eager = [[m.clone() for m in unet_decoder_maps(model.down_convs, model.up_convs, f)] for f in batches]
        again = unet_decoder_maps(model.down_convs, model.up_convs, batches[0])              # (also the warm-up of the capture)
        assert all(torch.equal(a, b) for a, b in zip(again, eager[0]))
        static = batches[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = unet_decoder_maps(model.down_convs, model.up_convs, static)
        for k in (1, 2, 3):
            static.copy_(batches[k])
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, eager[k])), k
