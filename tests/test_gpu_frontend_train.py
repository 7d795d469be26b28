"""-m gpu: the training-mode HIP UNet front-end (csrc/frontend_train.hip; ops.conv3x3_relu_bn_train, ops.adaptive_max_pool_train,
nn.unet_decoder_maps_train, UNetNodeFeatureModel.enable_hip_frontend(train=True)) against the same block built from torch modules
on the CPU in float64, with CPU float32 as the yardstick: per tensor

    max|hip - fp64| <= max(8 max|cpu32 - fp64|, 1e-6 max|fp64|)

The ReLU and the pools' argmax are discontinuous, so every fixture with random signs asserts on the float64 reference that no
pre-activation is within 64 (K + 8) 2^-24 S of zero (K = 9 c_in, S = conv(|x|, |w|) + |bias|) and that the CPU float32 mask is the
float64 mask.  The single-block fixtures get there by construction: x = s |randn| with a sign map s that is +1 left of a band of
zeros (two destination pixels wide) and -1 right of it, flipped in every second frame, and w = t_o |randn| / sqrt(K) with one sign
per output channel -- no 3 x 3 window sees both signs, so a pre-activation is +-conv(|x|, |w|) + bias with a small bias, while the
mask is mixed inside every channel and dy, and with it every gradient sum, has random signs."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from echoglad_amd import ops
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import unet_decoder_maps, unet_decoder_maps_train
from echoglad_amd.ops.frontend import _AdaptiveMaxPoolTrain, _Conv3x3ReluBnTrain
from echoglad_amd.topology import HierTopology, TopologySpec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
MARGIN = 64


def _within(name, hip, r64, r32):
    """The 8x rule for one tensor; prints the ratio."""
    assert hip is not None and tuple(hip.shape) == tuple(r64.shape), (name, None if hip is None else tuple(hip.shape), tuple(r64.shape))
    e_hip = float((hip.detach().cpu().double() - r64).abs().max())
    e_cpu = float((r32.double() - r64).abs().max())
    tol = max(8 * e_cpu, 1e-6 * float(r64.abs().max()))
    print(f"{name} {tuple(hip.shape)}: hip err {e_hip:.3e}, cpu fp32 err {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}, tol {tol:.3e}")
    assert torch.isfinite(hip).all() and e_hip <= tol, (name, e_hip, e_cpu, tol)


# ---------------------------------------------------------------------------
# one block
# ---------------------------------------------------------------------------
class _Block(nn.Module):
    """conv3x3 -> ReLU -> BatchNorm2d on cat([Upsample(x0), x1]) from torch modules."""

    def __init__(self, c_in, c_out, side, bias=True, affine=True):
        super().__init__()
        self.up = nn.Upsample(size=side)
        self.conv = nn.Conv2d(c_in, c_out, 3, padding=1, bias=bias)
        self.bn = nn.BatchNorm2d(c_out, affine=affine)

    def forward(self, x0, x1=None):
        x = x0 if x0.shape[2] == self.up.size else self.up(x0)
        x = x if x1 is None else torch.cat([x, x1], dim=1)
        self.z = self.conv(x)
        self.xin = x
        return self.bn(F.relu(self.z))


def _sign_map(B, side0, side):
    """[B, 1, side0, side0] of +1 / 0 / -1: see the module docstring (all +1 where the map is too small for a band)."""
    s = torch.ones(B, 1, side0, side0)
    band = 2 if side // side0 < 2 else 1                      # source pixels that make two destination pixels
    if side0 >= band + 2:
        a = (side0 - band) // 2
        s[:, :, :, a:a + band] = 0.0
        s[:, :, :, a + band:] = -1.0
    s[1::2] *= -1.0
    return s


def _fixture(B, c0, c_out, side, side0=None, c1=0, seed=0, neg_gamma=False, bare=False, positive=False):
    g = torch.Generator().manual_seed(2000 + seed)
    side0 = side if side0 is None else side0
    K = 9 * (c0 + c1)
    s0 = torch.ones(B, 1, side0, side0) if positive else _sign_map(B, side0, side)
    x0 = torch.randn(B, c0, side0, side0, generator=g).abs() * s0
    s1 = s0 if side0 == side else nn.Upsample(size=side)(s0)
    x1 = torch.randn(B, c1, side, side, generator=g).abs() * s1 if c1 else None
    w = torch.randn(c_out, c0 + c1, 3, 3, generator=g).abs() / K ** 0.5
    if not positive:
        w = w * (torch.randint(0, 2, (c_out, 1, 1, 1), generator=g) * 2.0 - 1.0)
    bias = None if bare else (torch.ones(c_out) if positive else torch.randn(c_out, generator=g) * 0.05)
    gamma = None if bare else torch.rand(c_out, generator=g) + 0.5
    if neg_gamma and gamma is not None:
        gamma[1::2] *= -1
    beta = None if bare else torch.randn(c_out, generator=g) * 0.3
    rm, rv = torch.randn(c_out, generator=g) * 0.3, torch.rand(c_out, generator=g) + 0.25
    dy = torch.randn(B, c_out, side, side, generator=g)
    return dict(x0=x0, x1=x1, w=w, bias=bias, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy, side=side, K=K)


def _reference(fx, dtype, need=("x0", "x1", "w")):
    """The block on the CPU in `dtype` -> every output and gradient, and the pre-activations."""
    c_out, c_in = fx["w"].shape[0], fx["w"].shape[1]
    blk = _Block(c_in, c_out, fx["side"], bias=fx["bias"] is not None, affine=fx["gamma"] is not None).to(dtype).train()
    with torch.no_grad():
        blk.conv.weight.copy_(fx["w"])
        if fx["bias"] is not None:
            blk.conv.bias.copy_(fx["bias"])
        if fx["gamma"] is not None:
            blk.bn.weight.copy_(fx["gamma"])
            blk.bn.bias.copy_(fx["beta"])
        blk.bn.running_mean.copy_(fx["rm"])
        blk.bn.running_var.copy_(fx["rv"])
    x0 = fx["x0"].clone().to(dtype).requires_grad_("x0" in need)
    x1 = None if fx["x1"] is None else fx["x1"].clone().to(dtype).requires_grad_("x1" in need)
    y = blk(x0, x1)
    (y * fx["dy"].to(dtype)).sum().backward()
    out = dict(y=y.detach(), rm=blk.bn.running_mean.clone(), rv=blk.bn.running_var.clone(), dx0=x0.grad, dx1=None if x1 is None else x1.grad,
               dw=blk.conv.weight.grad, dbias=None if fx["bias"] is None else blk.conv.bias.grad,
               dgamma=None if fx["gamma"] is None else blk.bn.weight.grad, dbeta=None if fx["gamma"] is None else blk.bn.bias.grad,
               z=blk.z.detach(), nbt=int(blk.bn.num_batches_tracked))
    with torch.no_grad():
        b = torch.zeros(c_out, dtype=dtype) if fx["bias"] is None else fx["bias"].to(dtype).abs()
        out["S"] = F.conv2d(blk.xin.detach().abs(), fx["w"].to(dtype).abs(), b, padding=1)
    return out


def _precondition(z64, S64, z32, K, what):
    need = MARGIN * (K + 8) * U * S64
    room = float((z64.abs() / need)[S64 > 0].min())           # (S = 0: an all-zero window without a bias, z = 0 in every precision)
    print(f"{what}: smallest |z| / (64 (K + 8) u S) = {room:.2f}")
    assert bool((z64.abs() >= need).all()), (what, room)
    assert torch.equal(z32 > 0, z64 > 0), what


def _hip_block(fx, need=("x0", "x1", "w", "bias", "gamma", "beta"), module=True):
    """The block on the GPU -> the same dictionary."""
    c_out = fx["w"].shape[0]
    dev = lambda t, name: None if t is None else t.detach().to(DEV).requires_grad_(name in need)
    x0, x1, w, bias = dev(fx["x0"], "x0"), dev(fx["x1"], "x1"), dev(fx["w"], "w"), dev(fx["bias"], "bias")
    if module:
        bn = nn.BatchNorm2d(c_out, affine=fx["gamma"] is not None).to(DEV).train()
        with torch.no_grad():
            if fx["gamma"] is not None:
                bn.weight.copy_(fx["gamma"])
                bn.bias.copy_(fx["beta"])
                bn.weight.requires_grad_("gamma" in need)
                bn.bias.requires_grad_("beta" in need)
            bn.running_mean.copy_(fx["rm"])
            bn.running_var.copy_(fx["rv"])
        gamma, beta, rm, rv = bn.weight, bn.bias, bn.running_mean, bn.running_var
        y = ops.conv3x3_relu_bn_train(x0, w, bias, bn, side=fx["side"], x1=x1)
        nbt = int(bn.num_batches_tracked)
    else:
        gamma, beta, rm, rv = dev(fx["gamma"], "gamma"), dev(fx["beta"], "beta"), fx["rm"].to(DEV), fx["rv"].to(DEV)
        y = ops.conv3x3_relu_bn_train(x0, w, bias, (gamma, beta, rm, rv, 1e-5, 0.1), side=fx["side"], x1=x1)
        nbt = None
    assert isinstance(y.grad_fn, _Conv3x3ReluBnTrain._backward_cls)
    (y * fx["dy"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grad = lambda t: None if t is None else t.grad
    return dict(y=y.detach(), rm=rm.detach(), rv=rv.detach(), dx0=grad(x0), dx1=grad(x1), dw=grad(w), dbias=grad(bias),
                dgamma=grad(gamma), dbeta=grad(beta), nbt=nbt)


TENSORS = ("y", "rm", "rv", "dx0", "dx1", "dw", "dbias", "dgamma", "dbeta")


def _block_case(name, positive=False, **shape):
    fx = _fixture(positive=positive, **shape)
    r64, r32 = _reference(fx, torch.float64), _reference(fx, torch.float32)
    if positive:
        assert float(r64["z"].min()) >= 1.0                   # the ReLU is inactive: nothing to precondition
    else:
        _precondition(r64["z"], r64["S"], r32["z"], fx["K"], name)
        frac = float((r64["z"] > 0).double().mean())
        assert 0.05 < frac < 0.95, frac                       # a mixed mask
    hip = _hip_block(fx)
    for t in TENSORS:
        if r64[t] is None:
            assert hip[t] is None, t
        else:
            _within(f"{name} {t}", hip[t], r64[t], r32[t])
    assert hip["nbt"] == r64["nbt"] == 1


BLOCK_CASES = {
    "deep_odd_side": dict(B=2, c0=4, c_out=8, side=7),
    "channels_divide_nothing": dict(B=1, c0=3, c_out=5, side=9),
    "concat": dict(B=2, c0=4, c1=4, c_out=4, side=6),
    "uneven_nearest_blocks_4_to_7": dict(B=1, c0=8, c_out=4, side=7, side0=4),
    "deep_512_side2": dict(B=1, c0=512, c_out=512, side=2),
    "deep_concat_256_256_side4": dict(B=1, c0=256, c1=256, c_out=256, side=4),
    "deep_batch3_side8": dict(B=3, c0=64, c_out=128, side=8),
    "negative_gamma": dict(B=2, c0=5, c_out=6, side=11, neg_gamma=True),
    "no_bias_no_affine": dict(B=2, c0=5, c_out=6, side=11, bare=True),
    "boundary_16": dict(B=2, c0=9, c1=3, c_out=6, side=16, side0=5),
    "boundary_17": dict(B=2, c0=9, c1=3, c_out=6, side=17, side0=5),
    "tile_resize_concat_odd": dict(B=2, c0=5, c1=6, c_out=9, side=40, side0=17),
    "tile_partial_tiles": dict(B=1, c0=17, c_out=3, side=33),
}


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_one_block_forward_and_every_gradient(name):
    _block_case(name, seed=sorted(BLOCK_CASES).index(name), **BLOCK_CASES[name])


@pytest.mark.parametrize("only", ["w", "x0"])
def test_a_gradient_that_is_not_needed_is_none(only, monkeypatch):
    returned = []
    inner = _Conv3x3ReluBnTrain.backward
    monkeypatch.setattr(_Conv3x3ReluBnTrain, "backward", staticmethod(lambda ctx, dy: returned.append(inner(ctx, dy)) or returned[-1]))
    fx = _fixture(B=2, c0=4, c1=4, c_out=4, side=6, seed=40)
    r64, r32 = _reference(fx, torch.float64), _reference(fx, torch.float32)
    _precondition(r64["z"], r64["S"], r32["z"], fx["K"], only)
    hip = _hip_block(fx, need=(only,), module=False)
    key = {"w": "dw", "x0": "dx0"}[only]
    _within(f"only {only}: {key}", hip[key], r64[key], r32[key])
    _within(f"only {only}: y", hip["y"], r64["y"], r32["y"])
    for t in ("dx0", "dx1", "dw", "dbias", "dgamma", "dbeta"):
        if t != key:
            assert hip[t] is None, t
    assert len(returned) == 1 and [g is not None for g in returned[0]] == [only == "x0", False, only == "w"] + [False] * 7


def test_double_backward_raises():
    fx = _fixture(B=2, c0=4, c_out=4, side=6, seed=41)
    x0 = fx["x0"].to(DEV).requires_grad_()
    y = ops.conv3x3_relu_bn_train(x0, fx["w"].to(DEV), None, (None, None, None, None, 1e-5, 0.1))
    gx, = torch.autograd.grad((y * y).sum(), x0, create_graph=True)       # dy = 2 y is itself part of the graph
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


def test_the_long_reductions_at_the_real_side():
    """B = 1, 4 -> 8, side 224 from 128: x = |randn|, w = |randn| / sqrt(K), bias = 1, so every pre-activation is >= 1 (asserted)."""
    _block_case("real side", positive=True, B=1, c0=4, c_out=8, side=224, side0=128, seed=50)


# ---------------------------------------------------------------------------
# exact structure
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c_in", [3, 20])
@pytest.mark.parametrize("side", [1, 2, 3, 16, 17, 33])
def test_exact_structure(side, c_in):
    """x = 1, w = 1, bias = 1, gamma = 1 (a 6-tuple bn without affine parameters), B = 2, dy a map of non-zero integers in -3 .. 3.
    The BatchNorm is taken out of the check by construction: pixels with the same number of taps inside the map (corner, edge,
    interior) share their pre-activation, and dy sums to zero over each such class in every channel, so sum dy = 0 exactly and
    sum dy xhat = 0 up to rounding; eps = 2^40 makes 1 / sqrt(var + eps) = 2^-20 exactly in float32 (var < 2^16).  Then
    dz = 2^-20 dy exactly, and dW, dbias and dx are 2^-20 times sums of integers: they must equal, bit for bit, what float64
    autograd of the convolution gives for the upstream gradient 2^-20 dy."""
    B, c_out = 2, 2
    g = torch.Generator().manual_seed(side * 100 + c_in)
    taps = F.conv2d(torch.ones(1, 1, side, side), torch.ones(1, 1, 3, 3), padding=1).expand(B, 1, side, side).reshape(-1)
    dy = torch.zeros(c_out, B * side * side)
    for o in range(c_out):
        for cls in taps.unique():
            where = (taps == cls).nonzero().flatten()
            assert len(where) % 2 == 0
            where = where[torch.randperm(len(where), generator=g)]
            a = torch.randint(1, 4, (len(where) // 2,), generator=g).float()
            dy[o, where[0::2]], dy[o, where[1::2]] = a, -a
    dy = dy.view(c_out, B, side, side).transpose(0, 1).contiguous()
    x = torch.ones(B, c_in, side, side, device=DEV, requires_grad=True)
    w = torch.ones(c_out, c_in, 3, 3, device=DEV, requires_grad=True)
    bias = torch.ones(c_out, device=DEV, requires_grad=True)
    y = ops.conv3x3_relu_bn_train(x, w, bias, (None, None, None, None, 2.0 ** 40, 0.1))
    y.backward(dy.to(DEV))
    x64 = torch.ones(B, c_in, side, side, dtype=torch.float64, requires_grad=True)
    w64 = torch.ones(c_out, c_in, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.ones(c_out, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w64, b64, padding=1).backward(dy.double() * 2.0 ** -20)
    assert torch.equal(w.grad.cpu().double(), w64.grad) and (side == 1 or float(w64.grad.abs().max()) > 0)      # (side 1: dW = sum dy = 0)
    assert torch.equal(bias.grad.cpu().double(), b64.grad)
    assert torch.equal(x.grad.cpu().double(), x64.grad)


# ---------------------------------------------------------------------------
# pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("side_in,side_out,planes,ties", [(224, 128, 3, False), (7, 3, 1, False), (4, 2, 37, False), (5, 5, 1, False),
                                                         (16, 8, 37, False), (9, 4, 5, True)])
def test_pool_backward_is_torchs(side_in, side_out, planes, ties):
    g = torch.Generator().manual_seed(side_in * 1000 + side_out)
    if ties:
        x = torch.randint(0, 3, (2, planes, side_in, side_in), generator=g).float()
    else:
        x = torch.randn(2, planes, side_in, side_in, generator=g)
    dy = torch.randint(-3, 4, (2, planes, side_out, side_out), generator=g).float()
    xc = x.clone().requires_grad_()
    want = F.adaptive_max_pool2d(xc, side_out)
    want.backward(dy)
    xd = x.to(DEV).requires_grad_()
    got = ops.adaptive_max_pool_train(xd, side_out)
    assert isinstance(got.grad_fn, _AdaptiveMaxPoolTrain._backward_cls)
    got.backward(dy.to(DEV))
    assert torch.equal(got.detach(), ops.adaptive_max_pool(x.to(DEV), side_out)) and torch.equal(got.detach().cpu(), want.detach())
    assert torch.equal(xd.grad.cpu(), xc.grad)


@pytest.mark.parametrize("side_in,side_out,planes", [(7, 3, 1), (5, 5, 1), (4, 2, 37), (17, 16, 3)])
def test_both_pools_are_one_kernel(side_in, side_out, planes):
    """The eval and the training pool are two instantiations of one kernel: the same bits out (compared as int32, since
    torch.equal calls a NaN unequal to itself), and the saved indices are those of torch's CPU pool.  In every plane the first
    window holds its maximum twice, at its first and its last element (not at 5 -> 5, where a window is one pixel), the last
    window holds a NaN, and in plane 0 the window before it holds two.  Checked on the CPU: torch lets every NaN take over
    (`val > max || isnan(val)`), so a NaN window's index is its LAST NaN -- the first where there is one -- which is the kernel's
    rule as well: all windows are compared, the NaN windows included."""
    g = torch.Generator().manual_seed(side_in * 100 + side_out)
    x = torch.randn(2, planes, side_in, side_in, generator=g)
    lo = lambda i: (i * side_in) // side_out
    hi = lambda i: -(-(i + 1) * side_in // side_out)
    tied = hi(0) - lo(0) > 1
    if tied:
        x[:, :, 0, 0] = x[:, :, hi(0) - 1, hi(0) - 1] = 50.0
    last, nan = side_out - 1, float("nan")
    x[:, :, hi(last) - 1, hi(last) - 1] = nan
    x[0, 0, lo(last - 1), lo(last)] = x[0, 0, lo(last - 1), hi(last) - 1 if tied else lo(last)] = nan     # window (last - 1, last)
    want, want_idx = F.adaptive_max_pool2d(x, side_out, return_indices=True)
    assert bool(want[:, :, last, last].isnan().all()) and bool(want[0, 0, last - 1, last].isnan())
    assert bool((want_idx[:, :, last, last] == (hi(last) - 1) * side_in + hi(last) - 1).all())
    assert int(want_idx[0, 0, last - 1, last]) == lo(last - 1) * side_in + (hi(last) - 1 if tied else lo(last))       # the last NaN
    if tied:
        assert bool((want[:, :, 0, 0] == 50.0).all()) and bool((want_idx[:, :, 0, 0] == 0).all())      # the first of the two
    xd = x.to(DEV)
    got = ops.adaptive_max_pool_train(xd.clone().requires_grad_(), side_out)
    with torch.no_grad():
        plain = ops.adaptive_max_pool(xd, side_out)
    idx, = got.grad_fn.saved_tensors
    assert got.dtype == plain.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(got.detach().view(torch.int32), plain.view(torch.int32))
    assert torch.equal(plain.cpu().isnan(), want.isnan()) and torch.equal(plain.cpu().nan_to_num(nan=0.0), want.nan_to_num(nan=0.0))
    assert torch.equal(idx.cpu().long(), want_idx)


# ---------------------------------------------------------------------------
# the whole front-end
# ---------------------------------------------------------------------------
SMALL = dict(frame_size=16, num_aux_graphs=3, encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32],
             node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit",
             use_coordinate_graph=False, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
STACK_SEED = 0          # chosen on the CPU so that the preconditions of test_whole_front_end_small hold


def _small_model(seed):
    """SMALL with trained-like BatchNorms (every third gamma negative) and convolution biases far from zero: with random signs
    after every BatchNorm, some pre-activation of 24 k lands within the precondition's margin of zero for every seed otherwise."""
    torch.manual_seed(seed)
    model = UNetNodeFeatureModel(**SMALL)
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
            elif isinstance(m, nn.Conv2d):            # +-(3 .. 4), three in four positive: a channel is alive or dead as a whole
                sign = (torch.rand(m.out_channels, generator=g) < 0.75).float() * 2.0 - 1.0
                m.bias.copy_((torch.rand(m.out_channels, generator=g) + 3.0) * sign)
    return model.to(DEV).train()


def _torch_maps(down_convs, up_convs, frames):
    x, skips = frames, []
    for down in down_convs:
        skips.append(x)
        x = down(x)
    feats = [x]
    for up in up_convs:
        x = up(x, skips.pop())
        feats.append(x)
    return feats


def _loss_weights(maps, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(m.shape, generator=g) for m in maps]


def _cpu_stack(model, frames, dtype, hooks=False):
    """Forward + backward of CPU copies of the model's front-end in `dtype` -> (maps, d frames, the modules, hook records)."""
    down, up = copy.deepcopy(model.down_convs).cpu().to(dtype).train(), copy.deepcopy(model.up_convs).cpu().to(dtype).train()
    records = []
    if hooks:
        for blocks in (down, up):
            for m in blocks.modules():
                if isinstance(m, nn.Conv2d):
                    m.register_forward_hook(lambda mod, inp, out: records.append(("conv", mod, inp[0].detach(), out.detach())))
                elif isinstance(m, nn.AdaptiveMaxPool2d):
                    m.register_forward_hook(lambda mod, inp, out: records.append(("pool", mod, inp[0].detach(), out.detach())))
    x = frames.detach().cpu().clone().to(dtype).requires_grad_()
    maps = _torch_maps(down, up, x)
    sum((m * w.to(dtype)).sum() for m, w in zip(maps, _loss_weights(maps))).backward()
    return [m.detach() for m in maps], x.grad, (down, up), records


def _window_top_two(x, x32, side_out):
    """Smallest gap between the two largest values of any pool window of x [B, C, s, s], leaving out the windows whose two
    largest values are equal in float64 AND in float32 (a dead channel: relu = 0 everywhere, so every value is the BatchNorm's
    bias in every precision, and the first in scan order takes the gradient)."""
    side_in, worst = x.shape[2], float("inf")
    for i in range(side_out):
        y0, y1 = (i * side_in) // side_out, -(-(i + 1) * side_in // side_out)
        for j in range(side_out):
            x0, x1 = (j * side_in) // side_out, -(-(j + 1) * side_in // side_out)
            top = x[:, :, y0:y1, x0:x1].flatten(2).topk(2, dim=2).values
            top32 = x32[:, :, y0:y1, x0:x1].flatten(2).topk(2, dim=2).values
            gap = top[..., 0] - top[..., 1]
            tied = (gap == 0) & (top32[..., 0] == top32[..., 1])
            if not bool(tied.all()):
                worst = min(worst, float(gap[~tied].min()))
    return worst


def _stack_preconditions(rec64, rec32):
    assert len(rec64) == len(rec32) > 0
    for (kind, mod, inp, out), (_, _, inp32, out32) in zip(rec64, rec32):
        if kind == "conv":
            K = 9 * mod.in_channels
            S = F.conv2d(inp.abs(), mod.weight.detach().abs(), mod.bias.detach().abs(), padding=1)
            _precondition(out, S, out32, K, f"conv {mod.in_channels}->{mod.out_channels} side {out.shape[2]}")
        else:
            side_out = mod.output_size if isinstance(mod.output_size, int) else mod.output_size[0]
            gap, err = _window_top_two(inp, inp32, side_out), float((inp32.double() - inp).abs().max())
            print(f"pool {inp.shape[2]}->{side_out}: smallest top-two gap {gap:.3e}, cpu fp32 error of its input {err:.3e}")
            assert gap >= MARGIN * err                        # the margin of the ReLU precondition on the reference's own error


def _named_grads(down, up):
    return {f"{tag}.{n}": p.grad for tag, blocks in (("down", down), ("up", up)) for n, p in blocks.named_parameters()}


def _named_stats(down, up):
    return {f"{tag}.{n}": b for tag, blocks in (("down", down), ("up", up)) for n, b in blocks.named_buffers() if "running" in n}


def test_whole_front_end_small():
    model = _small_model(STACK_SEED)
    frames = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(11 + STACK_SEED))
    m64, df64, (d64, u64), rec64 = _cpu_stack(model, frames, torch.float64, hooks=True)
    m32, df32, (d32, u32), rec32 = _cpu_stack(model, frames, torch.float32, hooks=True)
    _stack_preconditions(rec64, rec32)
    x = frames.detach().to(DEV).requires_grad_()
    maps = unet_decoder_maps_train(model.down_convs, model.up_convs, x)
    assert [tuple(m.shape) for m in maps] == [(2, 32, 2, 2), (2, 16, 4, 4), (2, 8, 8, 8), (2, 4, 16, 16)]
    sum((m * w.to(DEV)).sum() for m, w in zip(maps, _loss_weights(maps))).backward()
    for i, m in enumerate(maps):
        _within(f"small map {i}", m, m64[i], m32[i])
    _within("small d frames", x.grad, df64, df32)
    g64, g32, got = _named_grads(d64, u64), _named_grads(d32, u32), _named_grads(model.down_convs, model.up_convs)
    assert len(got) == 2 * 3 * 8
    for name in g64:
        _within(f"small grad {name}", got[name], g64[name], g32[name])
    s64, s32, got = _named_stats(d64, u64), _named_stats(d32, u32), _named_stats(model.down_convs, model.up_convs)
    for name in s64:
        _within(f"small stat {name}", got[name], s64[name], s32[name])
    assert all(int(m.num_batches_tracked) == 1 for m in model.down_convs.modules() if isinstance(m, nn.BatchNorm2d))


def _with_state(model, fn):
    """fn() from the model's current state, which is put back afterwards (train-mode BatchNorms move their statistics)."""
    state = copy.deepcopy(model.state_dict())
    try:
        return fn()
    finally:
        model.load_state_dict(state)


def test_through_the_model():
    B, frame, naux = 2, 16, 3
    model = _small_model(9)
    frames = torch.randn(B, 4, frame, frame, generator=torch.Generator().manual_seed(13)).to(DEV)
    maps = lambda: [m for m in model.decoder_maps(frames)]
    model.enable_hip_frontend(False)
    torch_train = _with_state(model, maps)
    model.enable_hip_frontend(True)                                       # without train: as today, torch in training mode
    assert all(torch.equal(a, b) for a, b in zip(_with_state(model, maps), torch_train))
    model.enable_hip_frontend(True, train=True)
    new = _with_state(model, maps)
    direct = _with_state(model, lambda: unet_decoder_maps_train(model.down_convs, model.up_convs, frames))
    hip_nodes = (_Conv3x3ReluBnTrain._backward_cls, _AdaptiveMaxPoolTrain._backward_cls)       # (the coarsest map leaves a pool)
    assert all(isinstance(m.grad_fn, hip_nodes) for m in new)
    assert all(torch.equal(a, b) for a, b in zip(new, direct))
    for a, b in zip(new, torch_train):
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
    model.eval()
    with torch.no_grad():                                                 # eval + no_grad: the eval HIP route
        assert all(torch.equal(a, b) for a, b in zip(model.decoder_maps(frames), unet_decoder_maps(model.down_convs, model.up_convs, frames)))
    with torch.enable_grad():                                             # eval with autograd: torch, bit for bit
        on = model.decoder_maps(frames)
        model.enable_hip_frontend(False)
        off = model.decoder_maps(frames)
    assert all(torch.equal(a, b) for a, b in zip(on, off)) and all(not isinstance(m.grad_fn, hip_nodes) for m in on)
    # one full step in training mode
    model.train().enable_hip_frontend(True, train=True)
    topo = HierTopology(TopologySpec(frame, naux, False, False))
    ei = torch.from_numpy(topo.batched_edge_index(B)).to(DEV)
    logits = model(x=frames, edge_index=ei)[0]
    target = (torch.rand(logits.shape, generator=torch.Generator().manual_seed(1)) > 0.9).float().to(DEV)
    F.binary_cross_entropy_with_logits(logits, target).backward()
    params = dict(model.down_convs.named_parameters(prefix="down_convs"), **dict(model.up_convs.named_parameters(prefix="up_convs")))
    assert len(params) == 48
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert any(float(p.grad.abs().max()) > 0 for p in params.values())


def _run(model, frames):
    """Forward + backward of the HIP stack -> (maps, d frames); parameter gradients land in .grad."""
    maps = unet_decoder_maps_train(model.down_convs, model.up_convs, frames)
    sum((m * w).sum() for m, w in zip(maps, model._loss_w)).backward()
    return maps


def _snapshot(model, maps, frames):
    out = [m.detach().clone() for m in maps] + [frames.grad.clone()]
    out += [p.grad.clone() for p in list(model.down_convs.parameters()) + list(model.up_convs.parameters())]
    out += [b.clone() for b in list(model.down_convs.buffers()) + list(model.up_convs.buffers())]
    return out


def test_reproducible_and_capturable():
    model = _small_model(15)
    params = list(model.down_convs.parameters()) + list(model.up_convs.parameters())
    g = torch.Generator().manual_seed(17)
    batches = [torch.randn(2, 4, 16, 16, generator=g).to(DEV) for _ in range(4)]
    model._loss_w = [w.to(DEV) for w in _loss_weights([torch.empty(2, 32, 2, 2), torch.empty(2, 16, 4, 4), torch.empty(2, 8, 8, 8),
                                                       torch.empty(2, 4, 16, 16)])]
    state0 = copy.deepcopy(model.state_dict())

    def eager(frames):
        model.load_state_dict(state0)
        for p in params:
            p.grad = None
        x = frames.clone().requires_grad_()
        return _snapshot(model, _run(model, x), x)

    first = [eager(f) for f in batches]
    again = eager(batches[0])
    assert len(again) == 4 + 1 + 48 + 36 and all(torch.equal(a, b) for a, b in zip(again, first[0]))

    static = batches[0].clone().requires_grad_()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                      # warm-up on the capture stream: its scratch exists afterwards
        model.load_state_dict(state0)
        _run(model, static)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for p in params + [static]:
        p.grad = None                                                     # .grad is allocated inside the capture: static buffers
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        maps = _run(model, static)
    for k in (1, 2, 3):
        model.load_state_dict(state0)
        with torch.no_grad():
            static.copy_(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(model, maps, static)
        assert all(torch.equal(a, b) for a, b in zip(got, first[k])), k
