"""-m gpu: the HIP CNN embedder (csrc/embedder.hip; ops.embed_block, ops.embed_block_train, nn.CNN.enable_hip) against the same block
built from torch modules on the CPU in float64, with CPU float32 as the yardstick: per tensor

    max|hip - fp64| <= max(8 max|cpu32 - fp64|, 1e-6 max|fp64|)

(db3, whose true value is zero: 8 n 2^-24 max|dz64| in place of the 1e-6 term, the worst-case rounding of an n-term sum).  The
backward's gate [s > 0] is discontinuous, so every training case asserts on the references alone that the float32 mask is the
float64 mask and that min|s64| >= 64 max|s32 - s64|; each case's seed was chosen on the CPU so that this holds."""
import copy

import pytest
import torch

from echoglad_amd import ops
from echoglad_amd.nn import CNN
from echoglad_amd.ops import embedder as E
from embedder_util import block_fixture, block_reference, plane_keep, relu_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
MARGIN = 64

# (B, c_in, c_out, side) -> the fixture's seed
SHAPES = {
    (2, 1, 4, 1): 0,          # one pixel, all halo, n = 2
    (1, 1, 4, 2): 0,          # side 2
    (2, 4, 4, 3): 2,          # identity residual
    (3, 3, 5, 16): 2,         # one partial tile, odd channel counts
    (2, 1, 4, 17): 7,         # side 17
    (1, 4, 8, 33): 3,         # crosses the 32-wide tile by one
    (2, 5, 4, 40): 6,         # crosses both tile edges, c_in > c_out
    (1, 9, 4, 20): 9,         # more input channels than one LDS stage of 8
}
REAL = (1, 1, 4, 224)
GRADS = ("dx", "dw3", "db3", "dgamma", "dbeta", "dw1", "db1")


def _within(name, hip, r64, r32, floor=None):
    """The 8x rule for one tensor; prints the ratio."""
    assert hip is not None and tuple(hip.shape) == tuple(r64.shape), (name, None if hip is None else tuple(hip.shape), tuple(r64.shape))
    e_hip = float((hip.detach().cpu().double() - r64).abs().max())
    e_cpu = float((r32.double() - r64).abs().max())
    tol = max(8 * e_cpu, 1e-6 * float(r64.abs().max()) if floor is None else floor)
    print(f"{name} {tuple(hip.shape)}: hip err {e_hip:.3e}, cpu fp32 err {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}, tol {tol:.3e}")
    assert torch.isfinite(hip).all() and e_hip <= tol, (name, e_hip, e_cpu, tol)


def _precondition(name, r64, r32):
    same, ratio = relu_margin(r64, r32)
    print(f"{name}: min|s64| / max|s32 - s64| = {ratio:.1f}")
    assert same and ratio >= MARGIN, (name, same, ratio)


def _dev(t, grad=False):
    return None if t is None else t.detach().to(DEV).requires_grad_(grad)


def _hip_train(fx, p=0.0, seed=0, need=("x", "w3", "b3", "gamma", "beta", "w1", "b1")):
    """The block on the GPU through ops.embed_block_train with an nn.BatchNorm2d -> the references' dictionary, and keep."""
    bn = torch.nn.BatchNorm2d(fx["c_out"]).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(fx["gamma"])
        bn.bias.copy_(fx["beta"])
        bn.running_mean.copy_(fx["rm"])
        bn.running_var.copy_(fx["rv"])
    bn.weight.requires_grad_("gamma" in need)
    bn.bias.requires_grad_("beta" in need)
    x, w3, b3 = _dev(fx["x"], "x" in need), _dev(fx["w3"], "w3" in need), _dev(fx["b3"], "b3" in need)
    w1, b1 = _dev(fx["w1"], "w1" in need), _dev(fx["b1"], "b1" in need)
    out, keep = ops.embed_block_train(x, w3, b3, bn, w1, b1, p, seed, return_keep=True)
    assert isinstance(out.grad_fn, E._EmbedBlockTrain._backward_cls) and not keep.requires_grad
    (out * fx["dout"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grad = lambda t: None if t is None else t.grad
    return dict(out=out.detach(), rm=bn.running_mean.detach(), rv=bn.running_var.detach(), nbt=int(bn.num_batches_tracked), dx=grad(x),
                dw3=grad(w3), db3=grad(b3), dgamma=grad(bn.weight), dbeta=grad(bn.bias), dw1=grad(w1), db1=grad(b1)), keep.detach()


def _compare_train(name, fx, hip, r64, r32):
    n = fx["B"] * fx["side"] ** 2
    for t in ("out", "rm", "rv") + GRADS:
        if r64[t] is None:
            assert hip[t] is None, t
        else:
            _within(f"{name} {t}", hip[t], r64[t], r32[t], floor=8 * n * U * float(r64["dz"].abs().max()) if t == "db3" else None)
    assert hip["nbt"] == r64["nbt"] == 1


# ---------------------------------------------------------------------------
# 1. eval
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES) + [REAL], ids=lambda s: "x".join(map(str, s)))
def test_eval_block(shape):
    fx = block_fixture(*shape, seed=SHAPES.get(shape, 0))
    r64, r32 = block_reference(fx, torch.float64, training=False), block_reference(fx, torch.float32, training=False)
    with torch.no_grad():
        out = ops.embed_block(_dev(fx["x"]), _dev(fx["w3"]), _dev(fx["b3"]),
                              (_dev(fx["gamma"]), _dev(fx["beta"]), _dev(fx["rm"]), _dev(fx["rv"]), 1e-5), _dev(fx["w1"]), _dev(fx["b1"]))
    _within(f"eval {shape} out", out, r64["out"], r32["out"])
    frac = float((r64["out"] > 0).double().mean())
    assert 0.05 < frac < 0.95 or shape[3] < 16, frac          # a mixed ReLU (the tiny maps hold a few values)


def _seeded_cnn(out_channels, seed, p=0.1):
    torch.manual_seed(seed)
    model = CNN(out_channels=out_channels, cnn_dropout_p=p)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("running_mean"):
                t.copy_(0.3 * torch.randn(t.shape))
            elif name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape))
            elif name.endswith("bn.weight"):
                t.copy_((0.5 + torch.rand(t.shape)) * torch.tensor([1.0 if o % 2 == 0 else -1.0 for o in range(t.numel())]))
            elif name.endswith("bn.bias"):
                t.copy_(0.3 * torch.randn(t.shape))
    return model


@pytest.mark.parametrize("out_channels", [[4], [8, 8, 4]], ids=["default", "c884"])
def test_eval_through_the_module(out_channels, monkeypatch):
    model = _seeded_cnn(out_channels, 31).eval()
    x = torch.randn(2, 1, 33, 33, generator=torch.Generator().manual_seed(32))
    with torch.no_grad():
        r32 = model(x)
        r64 = copy.deepcopy(model).double()(x.double())
        hip_model = copy.deepcopy(model).to(DEV).enable_hip()
        calls, inner = [], E.call
        monkeypatch.setattr(E, "call", lambda name, *a: calls.append(name) or inner(name, *a))
        out = hip_model(x.to(DEV))
    assert calls == ["eg_embed_block_fwd"] * len(out_channels)             # one launch per block
    _within(f"CNN {out_channels} eval", out, r64, r32)


# ---------------------------------------------------------------------------
# 2. training, p = 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_train_block_forward_and_every_gradient(shape):
    fx = block_fixture(*shape, seed=SHAPES[shape])
    r64, r32 = block_reference(fx, torch.float64), block_reference(fx, torch.float32)
    _precondition(f"train {shape}", r64, r32)
    hip, keep = _hip_train(fx)
    assert torch.equal(keep, torch.ones_like(keep))
    _compare_train(f"train {shape}", fx, hip, r64, r32)


@pytest.mark.parametrize("only", ["w3", "x", "w1"])
def test_a_gradient_that_is_not_asked_for_is_none_and_its_launch_is_skipped(only, monkeypatch):
    shape = (2, 5, 4, 40)
    fx = block_fixture(*shape, seed=SHAPES[shape])
    r64, r32 = block_reference(fx, torch.float64), block_reference(fx, torch.float32)
    _precondition(f"only {only}", r64, r32)
    calls, inner = [], E.call
    monkeypatch.setattr(E, "call", lambda name, *a: calls.append((name, a)) or inner(name, *a))
    hip, _ = _hip_train(fx, need=(only,))
    key = "d" + only
    _within(f"only {only}: {key}", hip[key], r64[key], r32[key])
    assert all(hip[t] is None for t in GRADS if t != key)
    names = [c[0] for c in calls]
    forward = ["eg_embed_conv_fwd", "eg_bn2d_train_fwd", "eg_embed_act_fwd", "eg_embed_act_bwd"]
    assert names == forward + {"w3": ["eg_conv3x3_bwd_weight"], "x": ["eg_conv3x3_bwd_data", "eg_embed_res_bwd_input"], "w1": []}[only]
    bwd = calls[3][1]
    assert [a is not None for a in bwd[15:20]] == [False, False, False, False, only == "w1"]      # dgamma, dbeta, db3, db1, dw1


def test_double_backward_raises():
    fx = block_fixture(2, 4, 4, 3, seed=2)
    x = _dev(fx["x"], True)
    y = ops.embed_block_train(x, _dev(fx["w3"]), None, (None, None, None, None, 1e-5, 0.1), None, None, 0.0, 0)
    gx, = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


# ---------------------------------------------------------------------------
# 3. the real side
# ---------------------------------------------------------------------------
def test_the_long_reductions_at_the_real_side():
    """(1, 1, 4, 224) with x = |randn|, W1 = |randn|, b1 >= 0, beta = 8: every s is >= 0.1 (asserted), the gate is all-on, and the
    50,176-term sums and the 196-tile weight gradient stand under the same rule."""
    fx = block_fixture(*REAL, seed=0, all_on=True)
    r64, r32 = block_reference(fx, torch.float64), block_reference(fx, torch.float32)
    assert float(r64["s"].min()) >= 0.1 and float(r32["s"].min()) > 0
    hip, _ = _hip_train(fx)
    _compare_train("real side", fx, hip, r64, r32)


# ---------------------------------------------------------------------------
# 4. the two residuals are one chain
# ---------------------------------------------------------------------------
def test_identity_residual_equals_the_one_by_one_route_with_the_unit_matrix(monkeypatch):
    fx = block_fixture(2, 4, 4, 17, seed=0)
    fx1 = dict(fx, w1=torch.eye(4).view(4, 4, 1, 1).clone(), b1=torch.zeros(4))
    bn = lambda: (_dev(fx["gamma"]), _dev(fx["beta"]), _dev(fx["rm"]), _dev(fx["rv"]), 1e-5)
    with torch.no_grad():
        a = ops.embed_block(_dev(fx["x"]), _dev(fx["w3"]), _dev(fx["b3"]), bn())
        b = ops.embed_block(_dev(fx["x"]), _dev(fx["w3"]), _dev(fx["b3"]), bn(), _dev(fx1["w1"]), _dev(fx1["b1"]))
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    calls, inner = [], E.call
    monkeypatch.setattr(E, "call", lambda name, *a: calls.append((name, a)) or inner(name, *a))
    ha, _ = _hip_train(fx)
    hb, _ = _hip_train(fx1)
    dz = [c[1][14] for c in calls if c[0] == "eg_embed_act_bwd"]
    assert len(dz) == 2 and torch.equal(dz[0], dz[1]) and float(dz[0].abs().max()) > 0
    for t in ("out", "rm", "rv", "dx", "dw3", "db3", "dgamma", "dbeta"):
        assert torch.equal(ha[t], hb[t]), t


# ---------------------------------------------------------------------------
# 5. Dropout2d
# ---------------------------------------------------------------------------
def test_plane_dropout():
    shape, seed, p = (8, 3, 4, 17), 0x1234_5678_9ABC, 0.5
    fx = block_fixture(*shape, seed=11)
    epoch0 = ops.dropout_epoch()
    try:
        ops.dropout_epoch_set(5)
        want = plane_keep(seed + 5, 8 * 4, p)
        assert 0 < int((want == 0).sum()) < 32 and set(want.tolist()) == {0.0, 2.0}
        r64, r32 = block_reference(fx, torch.float64, keep=want), block_reference(fx, torch.float32, keep=want)
        _precondition("dropout", r64, r32)
        hip, keep = _hip_train(fx, p=p, seed=seed)
        assert torch.equal(keep.cpu(), want)
        plain, _ = _hip_train(fx)
        assert torch.equal(hip["out"], plain["out"] * keep.view(8, 4, 1, 1))
        assert torch.equal(hip["rm"], plain["rm"]) and torch.equal(hip["rv"], plain["rv"])
        _compare_train("dropout", fx, hip, r64, r32)
        ops.dropout_epoch_set(6)
        _, keep6 = _hip_train(fx, p=p, seed=seed)
        assert torch.equal(keep6.cpu(), plane_keep(seed + 6, 32, p)) and not torch.equal(keep6, keep)
        # 4096 planes at side 2, p = 0.1
        many = block_fixture(1024, 1, 4, 2, seed=1)
        _, keep_many = _hip_train(many, p=0.1, seed=seed, need=("w3",))
        want_many = plane_keep(seed + 6, 4096, 0.1)
        assert int((keep_many == 0).sum()) == int((want_many == 0).sum()) and torch.equal(keep_many.cpu(), want_many)
    finally:
        ops.dropout_epoch_set(epoch0)


# ---------------------------------------------------------------------------
# 6. reproducible and capturable
# ---------------------------------------------------------------------------
def test_reproducible_and_capturable():
    model = _seeded_cnn([8, 8, 4], 41).to(DEV).train().enable_hip(True, train=True)
    params = list(model.parameters())
    g = torch.Generator().manual_seed(42)
    frames = torch.randn(2, 1, 33, 33, generator=g).to(DEV)
    weight = torch.randn(2, 4, 33, 33, generator=g).to(DEV)
    state0 = copy.deepcopy(model.state_dict())
    epoch0 = ops.dropout_epoch()
    torch.manual_seed(43)
    rng = torch.get_rng_state()

    def run(x):
        torch.set_rng_state(rng)                                          # the host seeds of the three blocks
        out = model(x)
        (out * weight).sum().backward()
        return out

    def snapshot(out, x):
        return [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params] + [b.clone() for b in model.buffers()]

    def eager():
        model.load_state_dict(state0)
        for p in params:
            p.grad = None
        ops.dropout_epoch_set(9)
        x = frames.clone().requires_grad_()
        return snapshot(run(x), x)

    try:
        first, again = eager(), eager()
        assert len(first) == 2 + 16 + 9 and all(torch.equal(a, b) for a, b in zip(first, again))

        static = frames.clone().requires_grad_()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):                                   # warm-up on the capture stream: its scratch exists afterwards
            model.load_state_dict(state0)
            run(static)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        for p in params + [static]:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run(static)
        for _ in range(3):
            model.load_state_dict(state0)
            ops.dropout_epoch_set(9)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(snapshot(out, static), first))
    finally:
        ops.dropout_epoch_set(epoch0)
