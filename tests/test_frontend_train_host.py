"""CPU: the host side of the training-mode HIP UNet front-end -- the new entry points in the header and the binding, what
ops.conv3x3_relu_bn_train / adaptive_max_pool_train refuse before they reach the library, the structures
nn.unet_decoder_maps_train refuses, and the model's second opt-in.  No GPU and no built library needed."""
import json
import os
import re

import pytest
import torch
import torch.nn as nn

from echoglad_amd import _lib
from echoglad_amd.examples import UNetNodeFeatureModel, _Down, _Up
from echoglad_amd.nn import unet_decoder_maps_train
from echoglad_amd.ops import frontend as fe

DECLS = """
size_t eg_frontend_train_workspace_bytes(int batch, int c_in, int c_out, int side);
int eg_conv3x3_relu_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* weight,
 const float* bias, int c_out, float* r, eg_stream_t stream);
int eg_bn2d_train_fwd(const float* r, int batch, int channels, int side, const float* gamma, const float* beta, float eps,
 float momentum, float* running_mean, float* running_var, void* workspace, float* y, float* save_mean, float* save_invstd,
 eg_stream_t stream);
int eg_relu_bn2d_bwd(const float* dy, const float* r, const float* save_mean, const float* save_invstd, const float* gamma, int batch,
 int channels, int side, void* workspace, float* dz, float* dgamma, float* dbeta, float* dbias, eg_stream_t stream);
int eg_conv3x3_bwd_data(const float* dz, const float* weight, int batch, int c_out, int side, int c0, int side0, int c1, float* dx0,
 float* dx1, float* full, eg_stream_t stream);
int eg_conv3x3_bwd_weight(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* dz, int c_out,
 void* workspace, float* dweight, eg_stream_t stream);
int eg_adaptive_max_pool_idx_fwd(const float* x, int planes, int side_in, int side_out, float* out, int* idx, eg_stream_t stream);
int eg_adaptive_max_pool_bwd(const float* dy, const int* idx, int planes, int side_in, int side_out, float* dx, eg_stream_t stream);
"""


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_the_training_entry_points():
    header = _flat(re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S))
    want = _lib.parse_header(DECLS)
    assert len(want) == 8
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name != "eg_frontend_train_workspace_bytes")
    assert _lib.ABI_VERSION >= 146
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in open(_lib.HEADER_PATH).read()


def _bn(c):
    return (torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c), 1e-5, 0.1)


def test_train_ops_refuse_what_the_kernels_do_not_take():
    x = torch.randn(2, 4, 6, 6)
    w = torch.randn(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="CUDA"):                       # well-formed, but on the CPU: no fallback
        fe.conv3x3_relu_bn_train(x, w, None, _bn(8))
    with pytest.raises(RuntimeError, match="CUDA"):
        fe.conv3x3_relu_bn_train(x, w, torch.zeros(8), nn.BatchNorm2d(8))
    with pytest.raises(RuntimeError, match="CUDA"):
        fe.adaptive_max_pool_train(x, 3)
    with pytest.raises(RuntimeError, match="float32"):
        fe.conv3x3_relu_bn_train(x.double(), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="float32"):
        fe.conv3x3_relu_bn_train(x, w.half(), None, _bn(8))
    with pytest.raises(RuntimeError, match="float32"):
        fe.adaptive_max_pool_train(x.to(torch.bfloat16), 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        fe.conv3x3_relu_bn_train(x.transpose(2, 3), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="contiguous"):
        fe.adaptive_max_pool_train(x.transpose(2, 3), 3)
    with pytest.raises(RuntimeError, match="square"):
        fe.conv3x3_relu_bn_train(torch.randn(2, 4, 6, 5), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="square"):
        fe.adaptive_max_pool_train(torch.randn(2, 4, 6, 5), 3)
    with pytest.raises(RuntimeError, match=r"c0 \+ c1 = 4 \+ 3"):
        fe.conv3x3_relu_bn_train(x, w, None, _bn(8), x1=torch.randn(2, 3, 6, 6))
    with pytest.raises(RuntimeError, match=r"c0 \+ c1 = 4 \+ 0"):
        fe.conv3x3_relu_bn_train(x, torch.randn(8, 5, 3, 3), None, _bn(8))
    with pytest.raises(RuntimeError, match="x1 must be"):
        fe.conv3x3_relu_bn_train(x, torch.randn(8, 8, 3, 3), None, _bn(8), side=7, x1=torch.randn(2, 4, 6, 6))
    with pytest.raises(RuntimeError, match="side_out"):
        fe.adaptive_max_pool_train(x, 7)
    with pytest.raises(RuntimeError, match="6-tuple"):
        fe.conv3x3_relu_bn_train(x, w, None, (torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8), 1e-5))
    with pytest.raises(RuntimeError, match="eval mode"):
        fe.conv3x3_relu_bn_train(x, w, None, nn.BatchNorm2d(8).eval())
    with pytest.raises(NotImplementedError, match="momentum"):
        fe.conv3x3_relu_bn_train(x, w, None, nn.BatchNorm2d(8, momentum=None))
    with pytest.raises(NotImplementedError, match="momentum"):
        fe.conv3x3_relu_bn_train(x, w, None, (None, None, None, None, 1e-5, None))
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        fe.conv3x3_relu_bn_train(x, w, None, nn.BatchNorm2d(8, track_running_stats=False))
    with pytest.raises(ValueError, match="more than 1 value per channel"):       # torch's own refusal, with its words
        fe.conv3x3_relu_bn_train(torch.randn(1, 4, 1, 1), w, None, _bn(8))
    with pytest.raises(RuntimeError, match="16 x"):
        fe.conv3x3_relu_bn_train(torch.randn(1, 4, 2, 2), w, None, _bn(8), side=40)


def test_the_eval_operators_stay_inference_only():
    x = torch.randn(1, 4, 6, 6)
    w = torch.randn(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="training mode"):
        fe.conv3x3_relu_bn(x, w, None, nn.BatchNorm2d(8))
    with pytest.raises(RuntimeError, match="inference-only"):
        fe.conv3x3_relu_bn(x.clone().requires_grad_(), w, None, (None, None, torch.zeros(8), torch.ones(8), 1e-5))


def _blocks():
    return nn.ModuleList([_Down(4, 8, 8), _Down(8, 16, 4)]).train(), nn.ModuleList([_Up(16, 8, 8), _Up(8, 4, 16)]).train()


@pytest.mark.parametrize("breakage", ["kernel5", "stride2", "padding0", "dilation2", "groups2", "no_stats", "bilinear", "rect",
                                      "eval_bn", "momentum_none"])
def test_unet_decoder_maps_train_refuses_other_structures(breakage):
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
        down[0].BN1 = nn.BatchNorm2d(8, track_running_stats=False)
    elif breakage == "bilinear":
        up[0].upsample = nn.Upsample(size=8, mode="bilinear")
    elif breakage == "rect":
        frames = torch.randn(1, 4, 16, 12)
    elif breakage == "eval_bn":
        up[1].BN2.eval()
    elif breakage == "momentum_none":
        down[1].BN2 = nn.BatchNorm2d(16, momentum=None)
    with pytest.raises(NotImplementedError, match="unet_decoder_maps"):
        unet_decoder_maps_train(down, up, frames)


def test_a_well_formed_training_stack_gets_as_far_as_the_device_check():
    down, up = _blocks()
    with pytest.raises(RuntimeError, match="CUDA"):
        unet_decoder_maps_train(down, up, torch.randn(1, 4, 16, 16))


def test_train_is_a_second_opt_in_and_leaves_the_state_dict_alone(golden_dir):
    kw = dict(frame_size=16, num_aux_graphs=3, encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32],
              node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit",
              use_coordinate_graph=False, gnn_dropout_p=0.0, classifier_dropout_p=0.0)
    torch.manual_seed(0)
    m = UNetNodeFeatureModel(**kw).train()
    keys = list(m.state_dict())
    frames = torch.randn(2, 4, 16, 16)
    assert m.hip_frontend is False and m.hip_frontend_train is False
    assert m.enable_hip_frontend(True) is m and m.hip_frontend is True and m.hip_frontend_train is False     # train stays off
    state = {k: v.clone() for k, v in m.state_dict().items()}
    on = m.decoder_maps(frames)                                           # training + autograd with train off: torch, as before
    m.load_state_dict(state)
    m.enable_hip_frontend(False)
    off = m.decoder_maps(frames)
    assert all(torch.equal(a, b) for a, b in zip(on, off)) and on[-1].grad_fn is not None
    m.enable_hip_frontend(True, train=True)
    assert m.hip_frontend is True and m.hip_frontend_train is True and list(m.state_dict()) == keys
    with pytest.raises(RuntimeError, match="CUDA"):                       # training + autograd: the new route (no CPU fallback)
        m.decoder_maps(frames)
    m.eval()
    with torch.enable_grad():                                             # eval with autograd on: still torch
        assert m.decoder_maps(frames)[-1].grad_fn is not None
    with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA"):      # eval + no_grad: the eval HIP route
        m.decoder_maps(frames)
    m.train()
    with torch.no_grad():                                                 # training without autograd: torch
        assert m.decoder_maps(frames)[-1].grad_fn is None
    m.enable_hip_frontend(False, train=True)
    assert m.hip_frontend is False and m.hip_frontend_train is False
    torch.manual_seed(7)
    default = UNetNodeFeatureModel(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                   num_gnn_layers=3, output_activation="logit", use_coordinate_graph=True, gnn_dropout_p=0.5,
                                   classifier_dropout_p=0.5).enable_hip_frontend(True, train=True)
    assert set(default.state_dict()) == set(json.load(open(os.path.join(golden_dir, "unet_state_keys.json")))["state_dict"])
