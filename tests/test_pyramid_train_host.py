"""CPU: the host side of the CNN pyramid's training mode -- the entry points in the header and the binding, the error codes they
return before anything is launched, the bounded workspace, ops.pyramid_block_train's refusals, the routing of
nn.CNNHierarchicalPatchModel.enable_hip_pyramid(True, train=True), and the reference helper of the GPU tests
(tests/pyramid_train_reference.py) against CNNResBlock from torch modules in float64.  No GPU needed."""
import ctypes as ct
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from echoglad_amd import _lib, ops
from echoglad_amd.nn import CNNHierarchicalPatchModel, CNNResBlock
from echoglad_amd.ops import embedder as em
from embedder_util import block_fixture
from pyramid_train_reference import pooled_dout, pyramid_block_reference, window_gap

DECLS = """
size_t eg_pyramid_train_workspace_bytes(int batch, int side, int side_out);
int eg_pyramid_conv_fwd(const float* x, int batch, int side, const float* w3, const float* b3, float* z, eg_stream_t stream);
int eg_pyramid_act_fwd(const float* y, const float* x, int batch, int side, int side_out, float p, uint64_t seed, float* keep, int* idx,
 float* out, eg_stream_t stream);
int eg_pyramid_act_bwd(const float* dout, const float* out, const float* keep, const int* idx, const float* z, const float* save_mean,
 const float* save_invstd, const float* gamma, int batch, int side, int side_out, void* workspace, float* ds,
 float* dz, float* dgamma, float* dbeta, float* db3, eg_stream_t stream);
int eg_pyramid_conv_bwd_data(const float* dz, const float* w3, const float* ds, int batch, int side, float* dx, eg_stream_t stream);
int eg_pyramid_conv_bwd_weight(const float* x, const float* dz, int batch, int side, void* workspace, float* dw3, eg_stream_t stream);
"""
NAMES = ["eg_pyramid_act_bwd", "eg_pyramid_act_fwd", "eg_pyramid_conv_bwd_data", "eg_pyramid_conv_bwd_weight", "eg_pyramid_conv_fwd",
         "eg_pyramid_train_workspace_bytes"]
SMALL = dict(frame_size=32, num_aux_graphs=4, cnn_layers_out_width=[16, 8, 4, 2], node_embedding_dim=128, node_hidden_dim=128,
             classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit")
MIB = 1 << 20


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_the_training_entry_points():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert sorted(want) == NAMES
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name != "eg_pyramid_train_workspace_bytes")
    assert _lib.ABI_VERSION >= 151
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 151: .*eg_pyramid_conv_bwd_weight", _flat(text))            # the ABI history line
    assert "POOL, THEN ReLU, THEN DROPOUT" in text
    assert ops.pyramid_block_train is em.pyramid_block_train


def test_bad_arguments_return_error_codes_with_nothing_launched(built_lib):
    """Without a GPU a launch would come back as EG_ERR_HIP: EG_ERR_ARG / EG_ERR_UNSUPPORTED show that the check came first."""
    lib = _lib.load()
    mem = (ct.c_float * 256)()                       # never dereferenced: every call below is refused
    p = [ct.c_void_p(ct.addressof(mem) + 16 * i) for i in range(16)]
    ARG, UNS = _lib.EG_ERR_ARG, _lib.EG_ERR_UNSUPPORTED

    def conv_fwd(x=p[0], batch=1, side=64, w=p[1], b=None, z=p[2]):
        return lib.eg_pyramid_conv_fwd(x, batch, side, w, b, z, None)

    def act_fwd(y=p[0], x=p[1], batch=1, side=64, side_out=32, prob=0.0, keep=p[2], idx=p[3], out=p[4]):
        return lib.eg_pyramid_act_fwd(y, x, batch, side, side_out, prob, 0, keep, idx, out, None)

    def act_bwd(dout=p[0], out=p[1], keep=p[2], idx=p[3], z=p[4], mean=p[5], invstd=p[6], batch=1, side=64, side_out=32, ws=p[7],
                ds=p[8], dz=p[9]):
        return lib.eg_pyramid_act_bwd(dout, out, keep, idx, z, mean, invstd, None, batch, side, side_out, ws, ds, dz, None, None, None, None)

    def dgrad(dz=p[0], w=p[1], ds=None, batch=1, side=64, dx=p[2]):
        return lib.eg_pyramid_conv_bwd_data(dz, w, ds, batch, side, dx, None)

    def wgrad(x=p[0], dz=p[1], batch=1, side=64, ws=p[2], dw=p[3]):
        return lib.eg_pyramid_conv_bwd_weight(x, dz, batch, side, ws, dw, None)

    shapes = [(dict(batch=0), ARG, "batch"), (dict(side=0), ARG, ">= 1"), (dict(side=513), UNS, "512"),
              (dict(batch=70000), UNS, "batch too large"), (dict(batch=65535, side=512), UNS, "batch too large")]
    pool = [(dict(side_out=65), ARG, "side_out must not exceed side"), (dict(side_out=0), ARG, ">= 1")]
    cases = [(conv_fwd, [(dict(x=None), ARG, "NULL"), (dict(w=None), ARG, "NULL"), (dict(z=None), ARG, "NULL"),
                         (dict(z=p[0]), ARG, "alias")] + shapes),
             (act_fwd, [(dict(y=None), ARG, "NULL"), (dict(x=None), ARG, "NULL"), (dict(keep=None), ARG, "NULL"),
                        (dict(idx=None), ARG, "NULL"), (dict(out=None), ARG, "NULL"), (dict(out=p[1]), ARG, "alias"),
                        (dict(idx=p[4]), ARG, "alias"), (dict(prob=1.0), ARG, "[0, 1)"), (dict(prob=-0.1), ARG, "[0, 1)")] + shapes + pool),
             (act_bwd, [(dict(dout=None), ARG, "NULL"), (dict(idx=None), ARG, "NULL"), (dict(ws=None), ARG, "NULL"),
                        (dict(ds=None), ARG, "NULL"), (dict(dz=None), ARG, "NULL"), (dict(dz=p[8]), ARG, "alias"),
                        (dict(ds=p[4]), ARG, "alias"), (dict(side=1, side_out=1), ARG, "Expected more than 1 value per channel")]
              + shapes + pool),
             (dgrad, [(dict(dz=None), ARG, "NULL"), (dict(w=None), ARG, "NULL"), (dict(dx=None), ARG, "NULL"),
                      (dict(dx=p[0]), ARG, "alias"), (dict(ds=p[2]), ARG, "alias")] + shapes),
             (wgrad, [(dict(x=None), ARG, "NULL"), (dict(dz=None), ARG, "NULL"), (dict(dw=None), ARG, "NULL"),
                      (dict(ws=None), ARG, "workspace"), (dict(dw=p[1]), ARG, "alias")] + shapes)]
    for fn, rows in cases:
        for kw, rc, words in rows:
            assert fn(**kw) == rc, (fn.__name__, kw)
            assert words in _lib.last_error(), (fn.__name__, kw, _lib.last_error())


def test_the_workspace_does_not_grow_with_the_pixel_count(built_lib):
    nbytes = _lib.load().eg_pyramid_train_workspace_bytes
    slices = 64 * 128 * 128 * 9 * 4                                                  # 64 slices x 589,824 B
    chunk_sums = lambda batch, side: -(-batch * side * side // (256 * 32)) * 128 * (8 + 4)
    big, small = nbytes(32, 224, 128), nbytes(8, 224, 128)
    assert slices < big < 40 * MIB
    assert abs(big - slices - chunk_sums(32, 224)) <= 512 and abs(small - slices - chunk_sums(8, 224)) <= 512      # (rounded to 256 B)
    assert nbytes(32, 224, 128) == nbytes(32, 224, 1)
    assert 0 < nbytes(1, 3, 2) < 64 * 1024                                           # one tile: dw3 is written directly
    # close to the largest pixel count there is: the chunk sums (chunks of 256 * 128 values above 2^29) grow, the slices do not
    huge = -(-65535 * 181 * 181 // (256 * 128)) * 128 * (8 + 4)
    assert abs(nbytes(65535, 181, 1) - slices - huge) <= 512
    for batch, side, side_out in ((0, 32, 16), (1, 0, 0), (1, 513, 2), (1, 32, 33), (1, 32, 0), (70000, 8, 4), (65535, 512, 2)):
        assert nbytes(batch, side, side_out) == 0, (batch, side, side_out)


def test_op_refuses_before_the_library():
    x, w = torch.randn(2, 128, 8, 8), torch.randn(128, 128, 3, 3)
    bn = (None, None, None, None, 1e-5, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):                                   # well-formed, but on the CPU: no fallback
        em.pyramid_block_train(x, w, None, bn, 4, 0.0, 0)
    with pytest.raises(RuntimeError, match="128 -> 128"):
        em.pyramid_block_train(torch.randn(1, 64, 8, 8), torch.randn(64, 64, 3, 3), None, (None, None, None, None, 1e-5, 0.1), 4, 0.0, 0)
    for side_out in (0, 9):
        with pytest.raises(RuntimeError, match="side_out must be in 1 .. side = 8"):
            em.pyramid_block_train(x, w, None, bn, side_out, 0.0, 0)
    with pytest.raises(RuntimeError, match="float32"):
        em.pyramid_block_train(x.double(), w, None, bn, 4, 0.0, 0)
    with pytest.raises(RuntimeError, match="eval mode"):
        em.pyramid_block_train(x, w, None, nn.BatchNorm2d(128).eval(), 4, 0.0, 0)
    with pytest.raises(NotImplementedError, match="momentum=None"):
        em.pyramid_block_train(x, w, None, nn.BatchNorm2d(128, momentum=None).train(), 4, 0.0, 0)
    for p in (1.0, -0.1):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            em.pyramid_block_train(x, w, None, bn, 4, p, 0)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        em.pyramid_block_train(torch.randn(1, 128, 1, 1), w, None, bn, 1, 0.0, 0)


def test_routing_on_the_cpu(monkeypatch):
    """The training route needs training mode, autograd, CUDA float32 frames; CPU frames never route."""
    calls = []
    monkeypatch.setattr(em, "pyramid_block_train", lambda *a, **k: calls.append(a) or torch.zeros(1))
    monkeypatch.setattr(em, "pyramid_block", lambda *a, **k: calls.append(a) or torch.zeros(1))
    m = CNNHierarchicalPatchModel(**SMALL)
    keys = list(m.state_dict())
    assert m.hip_pyramid_train is False
    assert m.enable_hip_pyramid(True, train=True) is m and m.hip_pyramid is True and m.hip_pyramid_train is True
    assert list(m.state_dict()) == keys
    x = torch.randn(2, 128, 32, 32)
    for training in (False, True):
        m.train(training)
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                outs = m.pyramid_maps(x)
            assert [tuple(o.shape) for o in outs] == [(2, 128, w, w) for w in (16, 8, 4, 2)]
    assert not calls and int(m.conv[0].bn.num_batches_tracked) == 2
    assert m._hip_route(x) is None
    assert m.enable_hip_pyramid().hip_pyramid_train is False and m.hip_pyramid is True         # no further argument: eval only
    assert m.enable_hip_pyramid(False, train=True).hip_pyramid_train is False


def test_enable_refuses_a_cumulative_average_and_a_batchnorm_in_another_mode():
    m = CNNHierarchicalPatchModel(**SMALL).train()
    m.conv[2].bn = nn.BatchNorm2d(128, momentum=None)
    with pytest.raises(NotImplementedError, match=r"enable_hip_pyramid: conv\[2\]\.bn: .*momentum=None"):
        m.enable_hip_pyramid(True, train=True)
    assert m.hip_pyramid is False and m.hip_pyramid_train is False
    m = CNNHierarchicalPatchModel(**SMALL).train()
    m.conv[1].bn.eval()
    with pytest.raises(NotImplementedError, match=r"enable_hip_pyramid: conv\[1\]\.bn: .*eval mode, the module in training mode"):
        m.enable_hip_pyramid(True, train=True)


# ---------------------------------------------------------------------------
# the reference helper
# ---------------------------------------------------------------------------
def _module_reference(fx, side_out):
    """CNNResBlock(..., out_size=side_out) from torch modules in float64 -> the helper's dictionary."""
    blk = CNNResBlock(in_channels=128, padding=1, out_channels=128, kernel_size=3, out_size=side_out, cnn_dropout_p=0.0).double().train()
    with torch.no_grad():
        for t, k in ((blk.conv.weight, "w3"), (blk.conv.bias, "b3"), (blk.bn.weight, "gamma"), (blk.bn.bias, "beta"),
                     (blk.bn.running_mean, "rm"), (blk.bn.running_var, "rv")):
            t.copy_(fx[k])
    x = fx["x"].double().requires_grad_()
    out = blk(x)
    (out * pooled_dout(fx, side_out).double()).sum().backward()
    return dict(out=out.detach(), rm=blk.bn.running_mean, rv=blk.bn.running_var, dx=x.grad, dw3=blk.conv.weight.grad,
                db3=blk.conv.bias.grad, dgamma=blk.bn.weight.grad, dbeta=blk.bn.bias.grad)


@pytest.mark.parametrize("shape", [(2, 5, 2), (1, 9, 4), (2, 6, 6)], ids=lambda s: "x".join(map(str, s)))
def test_the_helper_is_the_block_from_torch_modules(shape):
    B, side, side_out = shape
    fx = block_fixture(B, 128, 128, side, seed=3)
    want = _module_reference(fx, side_out)
    plain = pyramid_block_reference(fx, torch.float64, side_out)
    _, torch_idx = F.adaptive_max_pool2d(plain["v"], side_out, return_indices=True)
    injected = pyramid_block_reference(fx, torch.float64, side_out, idx=torch_idx.to(torch.int32), gate=(plain["m"] > 0))
    assert torch.equal(plain["idx"], torch_idx)
    assert 0 < int((plain["m"] > 0).sum()) < plain["m"].numel()                      # a mixed gate
    for got in (plain, injected):
        for k, w in want.items():
            scale = float(w.abs().max())
            if k == "db3":                                                           # zero but for rounding
                assert float((got[k] - w).abs().max()) <= 1e-12 * float(plain["dz"].abs().max()) * B * side * side
            else:
                assert float((got[k] - w).abs().max()) <= 1e-12 * scale, k
    if side_out < side:
        assert torch.isfinite(window_gap(plain["v"], side_out)).all() and float(window_gap(plain["v"], side_out).min()) > 0
