"""CPU: the host side of the HIP CNN embedder -- the new entry points in the header and the binding, the torch route of nn.CNN
against the reference's own CNN (tests/golden/cnn_embedder.npz, made by tests/golden/make_embedder_golden.py), what
ops.embed_block / embed_block_train refuse before they reach the library, the structures CNN.enable_hip refuses, the routing
matrix and the plane mask restated in Python.  No GPU and no built library needed."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from echoglad_amd import _lib, ops
from echoglad_amd.nn import CNN, CNNResBlock
from echoglad_amd.ops import embedder as em
from embedder_util import plane_keep

DECLS = """
size_t eg_embed_workspace_bytes(int batch, int c_in, int c_out, int side);
int eg_embed_block_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, const float* bn_weight,
 const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps, const float* w1, const float* b1,
 int c_out, float* out, eg_stream_t stream);
int eg_embed_conv_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, int c_out, float* z,
 eg_stream_t stream);
int eg_embed_act_fwd(const float* y, const float* x, int batch, int c_in, int side, const float* w1, const float* b1, int c_out, float p,
 uint64_t seed, float* keep, float* out, eg_stream_t stream);
int eg_embed_act_bwd(const float* dout, const float* out, const float* keep, const float* x, const float* z, const float* save_mean,
 const float* save_invstd, const float* gamma, int batch, int c_in, int c_out, int side, void* workspace, float* ds,
 float* dz, float* dgamma, float* dbeta, float* db3, float* db1, float* dw1, eg_stream_t stream);
int eg_embed_res_bwd_input(const float* ds, const float* w1, int batch, int c_in, int c_out, int side, float* dx, eg_stream_t stream);
"""

MODELS = {"default": dict(out_channels=[4], kernel_sizes=[3], pool_sizes=[1], cnn_dropout_p=0.1), "c884": dict(out_channels=[8, 8, 4])}


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_the_embedder_entry_points():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert len(want) == 6
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name != "eg_embed_workspace_bytes")
    assert _lib.ABI_VERSION >= 149
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert ops.embed_block is em.embed_block and ops.embed_block_train is em.embed_block_train


# ---------------------------------------------------------------------------
# the torch route against the reference's own class
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    path = os.path.join(golden_dir, "cnn_embedder.npz")
    assert os.path.getsize(path) < 100 * 1024
    return np.load(path)


def _close(name, got, want):
    want = torch.from_numpy(np.asarray(want))
    assert tuple(got.shape) == tuple(want.shape), name
    err, scale = float((got.detach().double() - want.double()).abs().max()), float(want.double().abs().max())
    assert err <= 1e-5 * scale, (name, err, scale)        # K 2^-24 with K = 72 terms: a CPU convolution may order its sum differently


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_keys_and_the_torch_route_are_the_reference_s(name, golden):
    keys = [str(k) for k in golden[f"{name}/keys"]]
    model = CNN(**MODELS[name])
    assert list(model.state_dict()) == keys
    if name == "c884":
        assert not any(k.startswith("conv.1.0.one_by_one_cnn") for k in keys) and "conv.2.0.one_by_one_cnn.weight" in keys
    state = {k: torch.from_numpy(golden[f"{name}/state/{k}"]) for k in keys}
    model.load_state_dict(state, strict=True)
    x = torch.from_numpy(golden[f"{name}/x"])
    assert tuple(x.shape) == (2, 1, 12, 12)
    model.eval()
    with torch.no_grad():
        _close("eval_out", model(x), golden[f"{name}/eval_out"])
    train = CNN(**dict(MODELS[name], cnn_dropout_p=0.0))
    train.load_state_dict(state, strict=True)
    train.train()
    y = train(x)
    _close("train_out", y, golden[f"{name}/train_out"])
    (y * torch.from_numpy(golden[f"{name}/dout"])).sum().backward()
    grads = [k for k in golden.files if k.startswith(f"{name}/grad/")]
    assert len(grads) == len(list(train.parameters())) > 0
    for key, p in train.named_parameters():
        want = golden[f"{name}/grad/{key}"]
        if key.endswith(".conv.bias"):                    # mathematically zero in front of a training-mode BatchNorm: rounding noise
            assert float(p.grad.abs().max()) <= 1e-4 and float(np.abs(want).max()) <= 1e-4, key
        else:
            _close(f"grad {key}", p.grad, want)
    after = [k for k in golden.files if k.startswith(f"{name}/after/")]
    assert len(after) == 3 * len(MODELS[name]["out_channels"])
    for key, t in train.state_dict().items():
        if f"{name}/after/{key}" in golden.files:
            if key.endswith("num_batches_tracked"):
                assert int(t) == int(golden[f"{name}/after/{key}"]) == 4
            else:
                _close(f"after {key}", t, golden[f"{name}/after/{key}"])


def test_the_torch_route_takes_every_argument_of_the_reference():
    m = CNN(out_channels=[4, 6], kernel_sizes=[5, 3], pool_sizes=[2, 1], fc_output_dim=7, cnn_dropout_p=0.2)
    assert m.conv[0][0].conv.kernel_size == (5, 5) and m.conv[0][0].conv.padding == (2, 2) and m.conv[0][0].pool.kernel_size == (2, 2)
    assert m.conv[0][0].dropout.p == 0.2 and isinstance(m.output_fc[2], nn.Linear)
    blk = CNNResBlock(in_channels=3, padding=1, out_channels=3, out_size=5)
    assert blk.one_by_one_cnn is None and isinstance(blk.pool, nn.AdaptiveMaxPool2d)
    assert tuple(blk(torch.randn(2, 3, 9, 9)).shape) == (2, 3, 5, 5)
    assert tuple(CNN(out_channels=[4], pool_sizes=[2])(torch.randn(1, 1, 8, 8)).shape) == (1, 4, 4, 4)


# ---------------------------------------------------------------------------
# refusals before the library
# ---------------------------------------------------------------------------
def _bn(c, training):
    return (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c), 1e-5) + ((0.1,) if training else ())


def _both(x, w, b, bn_of, one_w=None, one_b=None, p=0.0):
    """The two operators on the same arguments (bn_of(training) -> the BatchNorm for that mode)."""
    def eval_mode():
        with torch.no_grad():
            return em.embed_block(x, w, b, bn_of(False), one_w, one_b)
    yield eval_mode
    yield lambda: em.embed_block_train(x, w, b, bn_of(True), one_w, one_b, p, 1)


def test_both_ops_refuse_what_the_kernels_do_not_take():
    x, w, w1 = torch.randn(2, 3, 6, 6), torch.randn(8, 3, 3, 3), torch.randn(8, 3, 1, 1)
    bn8 = lambda training: _bn(8, training)
    cases = [
        (RuntimeError, "CUDA", _both(x, w, None, bn8, w1)),                                # well-formed, but on the CPU: no fallback
        (RuntimeError, "CUDA", _both(x, w, torch.zeros(8), lambda t: nn.BatchNorm2d(8).train(t), w1, torch.zeros(8))),
        (RuntimeError, "CUDA", _both(torch.randn(2, 8, 6, 6), torch.randn(8, 8, 3, 3), None, bn8)),      # identity residual
        (RuntimeError, "float32", _both(x.double(), w, None, bn8, w1)),
        (RuntimeError, "float32", _both(x, w.half(), None, bn8, w1)),
        (RuntimeError, "one_w must be", _both(x, w, None, bn8, w1.double())),
        (RuntimeError, "contiguous", _both(x.transpose(2, 3), w, None, bn8, w1)),
        (RuntimeError, "square", _both(torch.randn(2, 3, 6, 5), w, None, bn8, w1)),
        (RuntimeError, r"c0 \+ c1 = 3 \+ 0", _both(x, torch.randn(8, 5, 3, 3), None, bn8, w1)),
        (RuntimeError, "one_w must be given", _both(x, w, None, bn8)),
        (RuntimeError, "one_w must be", _both(x, w, None, bn8, torch.randn(8, 4, 1, 1))),
        (RuntimeError, "one_b without one_w", _both(torch.randn(2, 8, 6, 6), torch.randn(8, 8, 3, 3), None, bn8, None, torch.zeros(8))),
        (RuntimeError, "128", _both(torch.randn(1, 129, 4, 4), torch.randn(4, 129, 3, 3), None, lambda t: _bn(4, t), torch.randn(4, 129, 1, 1))),
        (RuntimeError, "tuple", _both(x, w, None, lambda t: _bn(8, not t), w1)),
        (RuntimeError, "mode", _both(x, w, None, lambda t: nn.BatchNorm2d(8).train(not t), w1)),          # the BatchNorm in the other mode
    ]
    for exc, match, calls in cases:
        for fn in calls:
            with pytest.raises(exc, match=match):
                fn()
    # training only
    with pytest.raises(NotImplementedError, match="momentum"):
        em.embed_block_train(x, w, None, nn.BatchNorm2d(8, momentum=None), w1, None, 0.0, 1)
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        em.embed_block_train(x, w, None, nn.BatchNorm2d(8, track_running_stats=False), w1, None, 0.0, 1)
    with pytest.raises(RuntimeError, match="running statistics"):
        em.embed_block(x, w, None, nn.BatchNorm2d(8, track_running_stats=False).eval(), w1, None)
    with pytest.raises(ValueError, match="more than 1 value per channel"):          # torch's own refusal, with its words
        em.embed_block_train(torch.randn(1, 3, 1, 1), w, None, bn8(True), w1, None, 0.0, 1)
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            em.embed_block_train(x, w, None, bn8(True), w1, None, p, 1)
    with pytest.raises(RuntimeError, match="inference-only"):
        em.embed_block(x.clone().requires_grad_(), w, None, bn8(False), w1)
    with pytest.raises(RuntimeError, match="inference-only"):
        em.embed_block(x, w.clone().requires_grad_(), None, bn8(False), w1)


@pytest.mark.parametrize("breakage", ["kernel5", "pool2", "adaptive_pool", "fc", "no_stats", "momentum_none", "eval_bn", "stride2"])
def test_enable_hip_refuses_other_structures(breakage):
    kw = dict(out_channels=[4, 4])
    if breakage == "kernel5":
        kw["kernel_sizes"] = [3, 5]
    elif breakage == "pool2":
        kw["pool_sizes"] = [2, 1]
    elif breakage == "fc":
        kw["fc_output_dim"] = 8
    m = CNN(**kw)
    where = {"kernel5": r"conv\[1\]\[0\]\.conv", "pool2": r"conv\[0\]\[0\]\.pool", "fc": "output_fc"}.get(breakage)
    if breakage == "adaptive_pool":
        m.conv[1][0].pool, where = nn.AdaptiveMaxPool2d(4), r"conv\[1\]\[0\]\.pool"
    elif breakage == "no_stats":
        m.conv[0][0].bn, where = nn.BatchNorm2d(4, track_running_stats=False), r"conv\[0\]\[0\]\.bn.*running statistics"
    elif breakage == "momentum_none":
        m.conv[1][0].bn, where = nn.BatchNorm2d(4, momentum=None), r"conv\[1\]\[0\]\.bn.*momentum"
    elif breakage == "eval_bn":
        m.conv[1][0].bn.eval()
        where = r"conv\[1\]\[0\]\.bn.*eval mode"
    elif breakage == "stride2":
        m.conv[0][0].conv, where = nn.Conv2d(1, 4, 3, padding=1, stride=2), r"conv\[0\]\[0\]\.conv: stride"
    keys = list(m.state_dict())
    with pytest.raises(NotImplementedError, match="CNN.enable_hip: " + where):
        m.enable_hip(True, train=True)
    assert m._hip is False and m._hip_train is False and list(m.state_dict()) == keys
    if breakage in ("no_stats", "momentum_none", "eval_bn", "kernel5"):
        assert m(torch.randn(2, 1, 8, 8)).grad_fn is not None             # still the torch route


def test_a_block_that_changes_after_enable_hip_is_refused_at_the_call():
    m = CNN(out_channels=[4]).enable_hip(True, train=True)
    m.conv[0][0].bn.eval()
    with pytest.raises(NotImplementedError, match=r"conv\[0\]\[0\]\.bn"):
        m(torch.randn(2, 1, 8, 8))


def test_the_routing_matrix_and_the_state_dict():
    x = torch.randn(2, 1, 8, 8)
    for flag, train in itertools.product((False, True), repeat=2):
        m = CNN(out_channels=[4], cnn_dropout_p=0.1)
        keys = list(m.state_dict())
        assert m.enable_hip(flag, train=train) is m and list(m.state_dict()) == keys
        assert (m._hip, m._hip_train) == (flag, flag and train)
        for training, grad in itertools.product((False, True), repeat=2):
            m.train(training)
            hip = (flag and not training and not grad) or (flag and train and training and grad)
            with torch.set_grad_enabled(grad):
                if hip:
                    with pytest.raises(RuntimeError, match="CUDA"):       # the HIP routes have no CPU fallback
                        m(x)
                else:
                    assert (m(x).grad_fn is not None) == grad             # torch modules
    m = CNN(out_channels=[4]).enable_hip(True, train=True)
    m.enable_hip(False)
    assert (m._hip, m._hip_train) == (False, False) and m(x).grad_fn is not None


def test_seeds_are_drawn_per_block_and_reported(monkeypatch):
    seen, seeds = [], []
    m = CNN(out_channels=[4, 4], cnn_dropout_p=0.1).enable_hip(True, train=True)
    m.dropout_seed_hook = lambda what, block, s: seen.append((what, block, s))
    monkeypatch.setattr(em, "embed_block_train", lambda x, w, b, bn, w1, b1, p, seed: seeds.append((p, seed)) or torch.zeros(2, 4, 8, 8))
    torch.manual_seed(3)
    want = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2)]
    torch.manual_seed(3)
    m(torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(0)))
    assert seeds == [(0.1, want[0]), (0.1, want[1])] and seen == [("embedder", 0, (want[0],)), ("embedder", 1, (want[1],))]
    m0 = CNN(out_channels=[4], cnn_dropout_p=0.0).enable_hip(True, train=True)
    m0(torch.randn(2, 1, 8, 8))
    assert seeds[-1] == (0.0, 0)                                          # p == 0: no draw


# ---------------------------------------------------------------------------
# the plane mask
# ---------------------------------------------------------------------------
MASK_SEED = 0x5EED_0000_0000_2023


def test_plane_mask_restated_in_python():
    keep = plane_keep(MASK_SEED, 4096, 0.1)
    dropped = int((keep == 0).sum())
    assert 294 <= dropped <= 525, dropped                                 # 409.6 +- 6 sigma, sigma = 19.2
    kept = keep[keep != 0]
    assert torch.equal(kept, torch.full_like(kept, float(np.float32(1) / (np.float32(1) - np.float32(0.1)))))
    assert torch.equal(plane_keep(MASK_SEED, 4096, 0.0), torch.ones(4096))
    assert not torch.equal(plane_keep(MASK_SEED + 1, 4096, 0.1), keep)                     # the epoch moves the mask
    assert torch.equal(plane_keep(MASK_SEED + (1 << 64), 64, 0.5), plane_keep(MASK_SEED, 64, 0.5))       # uint64 arithmetic
