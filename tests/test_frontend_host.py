"""CPU: the host side of the HIP UNet front-end -- the two entry points in the header and the binding, what ops.frontend refuses
before it reaches the library, and the structures nn.unet_decoder_maps refuses.  No GPU and no built library needed."""
import re

import pytest
import torch
import torch.nn as nn

from echoglad_amd import _lib
from echoglad_amd.examples import UNetNodeFeatureModel, _Down, _Up
from echoglad_amd.nn import unet_decoder_maps
from echoglad_amd.ops import frontend as fe

CONV_DECL = """int eg_conv3x3_relu_bn_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side,
 const float* weight, const float* bias, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
 float bn_eps, int c_out, float* out, eg_stream_t stream);"""
POOL_DECL = "int eg_adaptive_max_pool_fwd(const float* x, int planes, int side_in, int side_out, float* out, eg_stream_t stream);"


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_both_entry_points_with_the_agreed_signatures():
    header = _flat(re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S))
    assert _flat(CONV_DECL) in header
    assert _flat(POOL_DECL) in header
    want = _lib.parse_header(CONV_DECL + "\n" + POOL_DECL)
    for name in ("eg_conv3x3_relu_bn_fwd", "eg_adaptive_max_pool_fwd"):
        assert _lib.SIGNATURES[name] == want[name][:2]
        assert name in _lib.TAKES_STREAM
    assert _lib.ABI_VERSION >= 145


def _bn(c):
    return (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c), 1e-5)


def test_ops_refuse_what_the_kernels_do_not_take():
    x = torch.randn(2, 4, 6, 6)
    w = torch.randn(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="CUDA"):                       # well-formed, but on the CPU: no fallback
        fe.conv3x3_relu_bn(x, w, None, _bn(8))
    with pytest.raises(RuntimeError, match="CUDA"):
        fe.adaptive_max_pool(x, 3)
    with pytest.raises(RuntimeError, match="float32"):
        fe.conv3x3_relu_bn(x.double(), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="float32"):
        fe.conv3x3_relu_bn(x, w.half(), None, _bn(8))
    with pytest.raises(RuntimeError, match="float32"):
        fe.adaptive_max_pool(x.to(torch.bfloat16), 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        fe.conv3x3_relu_bn(x.transpose(2, 3), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="contiguous"):
        fe.adaptive_max_pool(x.transpose(2, 3), 3)
    with pytest.raises(RuntimeError, match="square"):
        fe.conv3x3_relu_bn(torch.randn(2, 4, 6, 5), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="square"):
        fe.adaptive_max_pool(torch.randn(2, 4, 6, 5), 3)
    with pytest.raises(RuntimeError, match=r"c0 \+ c1 = 4 \+ 3"):
        fe.conv3x3_relu_bn(x, w, None, _bn(8), x1=torch.randn(2, 3, 6, 6))
    with pytest.raises(RuntimeError, match=r"c0 \+ c1 = 4 \+ 0"):
        fe.conv3x3_relu_bn(x, torch.randn(8, 5, 3, 3), None, _bn(8))
    with pytest.raises(RuntimeError, match="x1 must be"):                 # the skip map's side is the output's
        fe.conv3x3_relu_bn(x, torch.randn(8, 8, 3, 3), None, _bn(8), side=7, x1=torch.randn(2, 4, 6, 6))
    with pytest.raises(RuntimeError, match="3, 3"):
        fe.conv3x3_relu_bn(x, torch.randn(8, 4, 5, 5), None, _bn(8))
    with pytest.raises(RuntimeError, match="side_out"):
        fe.adaptive_max_pool(x, 7)
    with pytest.raises(RuntimeError, match="5-tuple"):
        fe.conv3x3_relu_bn(x, w, None, (torch.ones(8), torch.zeros(8)))
    with pytest.raises(RuntimeError, match="running"):
        fe.conv3x3_relu_bn(x, w, None, nn.BatchNorm2d(8, track_running_stats=False).eval())
    with pytest.raises(RuntimeError, match="training mode"):
        fe.conv3x3_relu_bn(x, w, None, nn.BatchNorm2d(8))


def test_ops_are_inference_only():
    x = torch.randn(1, 4, 6, 6)
    w = torch.randn(8, 4, 3, 3)
    for args in ((x.clone().requires_grad_(), w), (x, w.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="inference-only"):
            fe.conv3x3_relu_bn(*args, None, _bn(8))
    with pytest.raises(RuntimeError, match="inference-only"):             # a module's parameters require grad by default
        fe.conv3x3_relu_bn(x, w, None, nn.BatchNorm2d(8).eval())
    with pytest.raises(RuntimeError, match="inference-only"):
        fe.adaptive_max_pool(x.clone().requires_grad_(), 3)
    with torch.no_grad():                                                 # without autograd the same call gets as far as the device check
        with pytest.raises(RuntimeError, match="CUDA"):
            fe.conv3x3_relu_bn(x, w.clone().requires_grad_(), None, nn.BatchNorm2d(8).eval())


def _blocks():
    return nn.ModuleList([_Down(4, 8, 8), _Down(8, 16, 4)]).eval(), nn.ModuleList([_Up(16, 8, 8), _Up(8, 4, 16)]).eval()


@pytest.mark.parametrize("breakage", ["kernel5", "stride2", "padding0", "dilation2", "groups2", "no_stats", "bilinear", "rect"])
def test_unet_decoder_maps_refuses_other_structures(breakage):
    down, up = _blocks()
    frames = torch.randn(1, 4, 16, 16)
    if breakage == "kernel5":
        down[1].conv1 = nn.Conv2d(8, 16, 5, padding=2)
    elif breakage == "stride2":
        down[0].conv2 = nn.Conv2d(8, 8, 3, padding=1, stride=2)
    elif breakage == "padding0":
        up[0].conv1 = nn.Conv2d(16, 8, 3, padding=0)
    elif breakage == "dilation2":
        up[1].conv2 = nn.Conv2d(8, 4, 3, padding=1, dilation=2)
    elif breakage == "groups2":
        down[0].conv1 = nn.Conv2d(4, 8, 3, padding=1, groups=2)
    elif breakage == "no_stats":
        down[0].BN1 = nn.BatchNorm2d(8, track_running_stats=False).eval()
    elif breakage == "bilinear":
        up[0].upsample = nn.Upsample(size=8, mode="bilinear")
    elif breakage == "rect":
        frames = torch.randn(1, 4, 16, 12)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="unet_decoder_maps"):
        unet_decoder_maps(down, up, frames)


def test_a_well_formed_stack_gets_as_far_as_the_device_check():
    down, up = _blocks()
    with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA"):
        unet_decoder_maps(down, up, torch.randn(1, 4, 16, 16))


def test_the_flag_is_off_by_default_and_leaves_the_state_dict_alone():
    kw = dict(frame_size=16, num_aux_graphs=3, encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32],
              node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit",
              use_coordinate_graph=False, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    torch.manual_seed(0)
    m = UNetNodeFeatureModel(**kw).eval()
    keys = list(m.state_dict())
    frames = torch.randn(1, 4, 16, 16)
    with torch.no_grad():
        before = m.decoder_maps(frames)
    assert m.hip_frontend is False
    assert m.enable_hip_frontend() is m and m.hip_frontend is True
    assert list(m.state_dict()) == keys
    with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA"):      # on: eval + no_grad takes the HIP route (no CPU fallback)
        m.decoder_maps(frames)
    with torch.enable_grad():                                             # eval with autograd on: the torch path, bit for bit
        again = m.decoder_maps(frames)
    assert all(torch.equal(a, b) for a, b in zip(before, again)) and again[-1].grad_fn is not None
    m.enable_hip_frontend(False)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(before, m.decoder_maps(frames)))
