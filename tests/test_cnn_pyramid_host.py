"""CPU: the host side of the CNN-pyramid variant -- the two entry points in the header and the binding, the error codes
eg_pyramid_block_fwd returns before anything is launched, nn.CNNHierarchicalPatchModel's state_dict against the reference's key
list, its constructor and enable_hip_pyramid refusals, the routing, and create_node_pixels on the torch route in float64 against
the reference's per-sample loop (models.py:599-636) restated here with torch ops.  No GPU needed.

tests/golden/cnn_pyramid_state_keys.json was made by tests/golden/make_cnn_pyramid_keys.py, which runs the reference's own class;
torchvision is not installed where the fixtures are made, so its IntermediateLayerGetter is restated there from its documentation
(a ModuleDict of the Sequential's children up to the last returned one) -- that one stand-in is why both key prefixes
(conv.{i}.*, conv_hierarchical_grids.{i}.*) are also checked by hand below against models.py:560-588."""
import ctypes as ct
import json
import os
import re

import pytest
import torch
import torch.nn as nn

from echoglad_amd import _lib, ops
from echoglad_amd.nn import CNNHierarchicalPatchModel, CNNResBlock
from echoglad_amd.ops import embedder as em

DECLS = """
size_t eg_pyramid_block_scratch_bytes(int batch, int side, int side_out);
int eg_pyramid_block_fwd(const float* x, int batch, int side, const float* w3, const float* b3, const float* bn_weight,
 const float* bn_bias, const float* running_mean, const float* running_var, float eps, int side_out, float* scratch, float* out,
 eg_stream_t stream);
"""

DEFAULT = dict(frame_size=224, gnn_dropout_p=0.5, classifier_dropout_p=0.5, node_embedding_dim=128, node_hidden_dim=128,
               num_output_channels=4, num_gnn_layers=3, num_aux_graphs=7, gnn_jk_mode="last", classifier_hidden_dim=32, residual=True,
               use_coordinate_graph=True, output_activation="logit", use_connection_nodes=False, use_main_graph_only=False)
SMALL = dict(frame_size=32, num_aux_graphs=4, cnn_layers_out_width=[16, 8, 4, 2], node_embedding_dim=128, node_hidden_dim=128,
             classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit")


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_the_pyramid_entry_points():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert sorted(want) == ["eg_pyramid_block_fwd", "eg_pyramid_block_scratch_bytes"]
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name == "eg_pyramid_block_fwd")
    assert _lib.ABI_VERSION >= 150
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert ops.pyramid_block is em.pyramid_block


def test_bad_arguments_return_error_codes_with_nothing_launched(built_lib):
    """Without a GPU a launch would come back as EG_ERR_HIP: EG_ERR_ARG / EG_ERR_UNSUPPORTED show that the check came first."""
    lib = _lib.load()
    mem = (ct.c_float * 64)()                        # never dereferenced: every call below is refused
    base = ct.addressof(mem)
    x, w, m, v, s, o = (ct.c_void_p(base + 16 * i) for i in range(6))
    fwd = lib.eg_pyramid_block_fwd

    def call(x=x, batch=1, side=64, w=w, mean=m, var=v, eps=1e-5, side_out=32, scratch=s, out=o):
        return fwd(x, batch, side, w, None, None, None, mean, var, eps, side_out, scratch, out, None)

    for kw, rc, words in [(dict(x=None), _lib.EG_ERR_ARG, "must not be NULL"), (dict(out=None), _lib.EG_ERR_ARG, "must not be NULL"),
                          (dict(w=None), _lib.EG_ERR_ARG, "must not be NULL"), (dict(mean=None), _lib.EG_ERR_ARG, "must not be NULL"),
                          (dict(var=None), _lib.EG_ERR_ARG, "must not be NULL"),
                          (dict(side_out=65), _lib.EG_ERR_ARG, "side_out must not exceed side"),
                          (dict(side_out=0), _lib.EG_ERR_ARG, ">= 1"), (dict(side=0, side_out=0), _lib.EG_ERR_ARG, ">= 1"),
                          (dict(batch=0), _lib.EG_ERR_ARG, "batch"), (dict(eps=-1.0), _lib.EG_ERR_ARG, "eps"),
                          (dict(side=513, side_out=513), _lib.EG_ERR_UNSUPPORTED, "512"),
                          (dict(side=513, side_out=2), _lib.EG_ERR_UNSUPPORTED, "512"),
                          (dict(batch=70000), _lib.EG_ERR_UNSUPPORTED, "batch too large"),
                          (dict(batch=65535, side=512, side_out=512), _lib.EG_ERR_UNSUPPORTED, "batch too large"),
                          (dict(scratch=None), _lib.EG_ERR_ARG, "scratch must be given"),        # side_out != side
                          (dict(out=x), _lib.EG_ERR_ARG, "alias"), (dict(scratch=x), _lib.EG_ERR_ARG, "alias"),
                          (dict(scratch=o), _lib.EG_ERR_ARG, "alias")]:
        assert call(**kw) == rc, kw
        assert words in _lib.last_error(), (kw, _lib.last_error())
    nbytes = lib.eg_pyramid_block_scratch_bytes
    assert nbytes(8, 224, 128) == 8 * 128 * 224 * 224 * 4 == 205520896
    assert nbytes(1, 40, 17) == 128 * 1600 * 4
    assert nbytes(8, 224, 224) == 0 and nbytes(1, 32, 32) == 0                       # no pool: no scratch
    assert nbytes(1, 513, 2) == 0 and nbytes(0, 32, 16) == 0 and nbytes(1, 32, 33) == 0 and nbytes(1, 32, 0) == 0


def test_op_refuses_before_the_library():
    x, w = torch.randn(1, 128, 8, 8), torch.randn(128, 128, 3, 3)
    bn = (None, None, torch.zeros(128), torch.ones(128), 1e-5)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):                               # well-formed, but on the CPU: no fallback
            em.pyramid_block(x, w, None, bn, 4)
        with pytest.raises(RuntimeError, match="128 -> 128"):
            em.pyramid_block(torch.randn(1, 64, 8, 8), torch.randn(64, 64, 3, 3), None, (None, None, torch.zeros(64), torch.ones(64), 1e-5), 4)
        with pytest.raises(RuntimeError, match="one_w must be given"):                # embed_block's checker: no identity residual
            em.pyramid_block(torch.randn(1, 64, 8, 8), torch.randn(128, 64, 3, 3), None, bn, 4)
        for side_out in (0, 9):
            with pytest.raises(RuntimeError, match="side_out must be in 1 .. side = 8"):
                em.pyramid_block(x, w, None, bn, side_out)
        with pytest.raises(RuntimeError, match="float32"):
            em.pyramid_block(x.double(), w, None, bn, 4)
        with pytest.raises(RuntimeError, match="mode"):
            em.pyramid_block(x, w, None, nn.BatchNorm2d(128).train(), 4)
    with pytest.raises(RuntimeError, match="inference-only"):
        em.pyramid_block(x.clone().requires_grad_(), w, None, bn, 4)


# ---------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_s(golden_dir):
    path = os.path.join(golden_dir, "cnn_pyramid_state_keys.json")
    assert os.path.getsize(path) < 100 * 1024
    ref = json.load(open(path))
    model = CNNHierarchicalPatchModel(**DEFAULT)
    state = model.state_dict()
    assert list(state) == ref["keys"]
    assert {k: list(v.shape) for k, v in state.items()} == ref["state_dict"]
    assert sum(p.numel() for p in model.parameters()) == ref["n_parameters"]              # shared blocks counted once
    # by hand from models.py:560-588: seven blocks under `conv`, the same seven once more under `conv_hierarchical_grids`
    per_block = ["conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    for prefix in ("conv", "conv_hierarchical_grids"):
        assert [k for k in state if k.startswith(prefix + ".")] == [f"{prefix}.{i}.{t}" for i in range(7) for t in per_block]
    assert not any("one_by_one" in k for k in state)
    assert model.conv_hierarchical_grids["3"] is model.conv[3]
    assert [b.pool.output_size for b in model.conv] == [(w, w) for w in (128, 64, 32, 16, 8, 4, 2)]
    assert all(isinstance(b, CNNResBlock) and b.conv.in_channels == b.conv.out_channels == 128 for b in model.conv)
    # fewer levels than layers: the getter still holds every block (the coarsest level is the last one)
    few = CNNHierarchicalPatchModel(**dict(DEFAULT, num_aux_graphs=3, use_coordinate_graph=False))
    assert list(few.conv_hierarchical_grids) == [str(i) for i in range(7)]
    assert CNNHierarchicalPatchModel(cnn_dropout_p=0.25, **dict(DEFAULT, use_coordinate_graph=False)).conv[2].dropout.p == 0.25


def test_state_dict_round_trip_is_strict():
    torch.manual_seed(0)
    a, b = CNNHierarchicalPatchModel(**SMALL), CNNHierarchicalPatchModel(**SMALL)
    with torch.no_grad():
        for blk in a.conv:
            blk.bn.running_mean.normal_()
            blk.bn.running_var.uniform_(0.5, 1.5)
            blk.bn.num_batches_tracked.fill_(7)
    state = a.state_dict()
    assert sum(k.startswith("conv.") for k in state) == sum(k.startswith("conv_hierarchical_grids.") for k in state) == 4 * 7
    result = b.load_state_dict(state, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    assert int(b.conv[3].bn.num_batches_tracked) == 7
    partial = {k: v for k, v in state.items() if not k.startswith("conv_hierarchical_grids.")}
    with pytest.raises(RuntimeError, match="conv_hierarchical_grids"):
        b.load_state_dict(partial, strict=True)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="num_aux_graphs=5"):
        CNNHierarchicalPatchModel(**dict(SMALL, num_aux_graphs=5))                        # more levels than layers
    with pytest.raises(ValueError, match="widths"):
        CNNHierarchicalPatchModel(**dict(SMALL, cnn_layers_out_width=[16, 8, 4, 3]))
    with pytest.raises(ValueError, match="widths"):
        CNNHierarchicalPatchModel(**dict(SMALL, cnn_layers_out_width=[2, 4, 8, 16]))      # fine to coarse is the order
    with pytest.raises(ValueError, match="num_aux_graphs=8"):
        CNNHierarchicalPatchModel(frame_size=512, num_aux_graphs=8)                       # the default widths are seven layers
    with pytest.raises(ValueError, match="at least one layer"):
        CNNHierarchicalPatchModel(**dict(SMALL, cnn_layers_out_width=[], num_aux_graphs=0, use_main_graph_only=True))
    CNNHierarchicalPatchModel(**dict(SMALL, cnn_layers_out_width=[24, 20, 16, 8, 4, 2]))   # layers in front of the levels: any width
    CNNHierarchicalPatchModel(**dict(SMALL, cnn_layers_out_width=[16, 8, 4, 3], use_main_graph_only=True))      # no level is taken


@pytest.mark.parametrize("breakage", ["max_pool", "stride2", "kernel5", "no_stats", "residual", "rect_pool", "channels"])
def test_enable_hip_pyramid_refuses_other_structures(breakage):
    m = CNNHierarchicalPatchModel(**SMALL).eval()
    if breakage == "max_pool":
        m.conv[1].pool, where = nn.MaxPool2d(2), r"conv\[1\]\.pool: MaxPool2d"
    elif breakage == "stride2":
        m.conv[0].conv, where = nn.Conv2d(128, 128, 3, padding=1, stride=2), r"conv\[0\]\.conv: stride"
    elif breakage == "kernel5":
        m.conv[2].conv, where = nn.Conv2d(128, 128, 5, padding=2), r"conv\[2\]\.conv: kernel_size"
    elif breakage == "no_stats":
        m.conv[3].bn, where = nn.BatchNorm2d(128, track_running_stats=False), r"conv\[3\]\.bn.*running statistics"
    elif breakage == "residual":
        m.conv[1].one_by_one_cnn, where = nn.Conv2d(128, 128, 1), r"conv\[1\]\.one_by_one_cnn"
    elif breakage == "rect_pool":
        m.conv[0].pool, where = nn.AdaptiveMaxPool2d((16, 8)), r"conv\[0\]\.pool: output_size"
    else:
        m.conv[0].conv, where = nn.Conv2d(64, 128, 3, padding=1), r"conv\[0\]\.conv: in_channels"
    keys = list(m.state_dict())
    with pytest.raises(NotImplementedError, match="CNNHierarchicalPatchModel.enable_hip_pyramid: " + where):
        m.enable_hip_pyramid()
    assert m.hip_pyramid is False and list(m.state_dict()) == keys


def test_routing_on_the_cpu(monkeypatch):
    """The HIP route needs eval mode, no autograd, CUDA float32 frames; everything else is the torch modules."""
    calls = []
    monkeypatch.setattr(em, "pyramid_block", lambda *a: calls.append(a) or torch.zeros(1))
    m = CNNHierarchicalPatchModel(**SMALL)
    keys = list(m.state_dict())
    assert m.enable_hip_pyramid() is m and m.hip_pyramid is True and list(m.state_dict()) == keys
    x = torch.randn(2, 128, 32, 32)
    for training in (False, True):
        m.train(training)
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                outs = m.pyramid_maps(x)                                           # CPU frames: never the HIP route
            assert [tuple(o.shape) for o in outs] == [(2, 128, w, w) for w in (16, 8, 4, 2)]
            assert (outs[-1].grad_fn is not None) == grad
    assert not calls
    assert m.enable_hip_pyramid(False).hip_pyramid is False


# ---------------------------------------------------------------------------
# create_node_pixels on the torch route, float64, against the reference's loop
# ---------------------------------------------------------------------------
def _cpu_pack(level_maps, B, node_coords=None, connection_embed=None):
    """What pack_node_features documents, with torch ops in the maps' own dtype: per frame the connection rows, then every level
    (coarse to fine) as map.permute(1, 2, 0).reshape(-1, 128)."""
    rows = []
    for i in range(B):
        rows += ([] if connection_embed is None else [connection_embed[i]]) + [m[i].permute(1, 2, 0).reshape(-1, 128) for m in level_maps]
    return torch.cat(rows, dim=0)


def _reference_rows(model, frames, B):
    """models.py:599-636 with torch ops: feature_grids[g] = output of block L - 1 - g, then the per-sample loop."""
    L, naux = len(model.conv), model.num_aux_graphs
    grids, x = {}, frames
    for i, blk in enumerate(model.conv):
        x = blk(x)
        if L - 1 - i < naux:
            grids[str(L - 1 - i)] = x
    all_x = []
    for i in range(B):
        x, conn = torch.zeros(0, 128, dtype=frames.dtype), torch.zeros(0, 128, dtype=frames.dtype)
        if not model.use_main_graph_only:
            for g in range(naux):
                x = torch.cat([x, torch.reshape(grids[str(g)][i].permute(1, 2, 0), (-1, 128))], dim=0)
                if model.use_connection_nodes:
                    conn = torch.cat([conn, torch.reshape(grids[str(g)][i].mean(dim=(1, 2)), (-1, 128))], dim=0)
        x = torch.cat([x, torch.reshape(frames[i].permute(1, 2, 0), (-1, 128))], dim=0)
        if model.use_connection_nodes:
            conn = torch.cat([conn, torch.reshape(frames[i].mean(dim=(1, 2)), (-1, 128))], dim=0)
            x = torch.cat([conn, x], dim=0)
        all_x.append(x)
    return torch.cat(all_x, dim=0), grids


@pytest.fixture(scope="module")
def frames64():
    return torch.randn(2, 128, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(5))


def _model64(seed, **extra):
    torch.manual_seed(seed)
    m = CNNHierarchicalPatchModel(**dict(SMALL, **extra)).double().eval()
    with torch.no_grad():
        for blk in m.conv:
            blk.bn.running_mean.normal_(0, 0.3)
            blk.bn.running_var.uniform_(0.5, 1.5)
            blk.bn.weight.uniform_(0.5, 1.5)
            blk.bn.bias.normal_(0, 0.3)
    return m


@pytest.mark.parametrize("conn", [False, True])
def test_create_node_pixels_is_the_reference_loop_in_float64(conn, frames64, monkeypatch):
    B = 2
    m = _model64(3, use_connection_nodes=conn)
    seen = {}

    def pack(level_maps, num_samples_per_batch, node_coords=None, connection_embed=None):
        seen.update(maps=level_maps, conn=connection_embed)
        return _cpu_pack(level_maps, num_samples_per_batch, node_coords, connection_embed)
    monkeypatch.setattr(m, "pack_node_features", pack)
    with torch.no_grad():
        got = m.create_node_pixels(frames64, B)
        want, grids = _reference_rows(m, frames64, B)
    assert [tuple(t.shape) for t in seen["maps"]] == [(B, 128, s, s) for s in (2, 4, 8, 16, 32)]           # coarse to fine, then the frame
    for g in range(4):
        assert torch.equal(seen["maps"][g], grids[str(g)]), g                          # level g is the output of block L - 1 - g
    assert seen["maps"][4] is frames64
    n_conn = 5 if conn else 0
    assert got.dtype == torch.float64 and got.shape == want.shape == (B * (n_conn + 4 + 16 + 64 + 256 + 1024), 128)
    per = got.shape[0] // B
    g3, w3 = got.view(B, per, 128), want.view(B, per, 128)
    assert torch.equal(g3[:, n_conn:], w3[:, n_conn:])
    if conn:
        assert tuple(seen["conn"].shape) == (B, 5, 128)
        # (a mean over (2, 3) of the batch against a mean over (1, 2) of one sample: the same sums, perhaps in another order)
        assert float((g3[:, :n_conn] - w3[:, :n_conn]).abs().max()) <= 1e-14 * float(w3[:, :n_conn].abs().max()) + 1e-300
    else:
        assert seen["conn"] is None


def test_main_graph_only_skips_the_pyramid_in_eval_and_runs_it_in_training(frames64, monkeypatch):
    m = _model64(4, use_main_graph_only=True)
    monkeypatch.setattr(m, "pack_node_features", lambda maps, B, node_coords=None, connection_embed=None: _cpu_pack(maps, B))
    ran = []
    m.conv[0].register_forward_hook(lambda *a: ran.append(1))
    want = torch.cat([frames64[i].permute(1, 2, 0).reshape(-1, 128) for i in range(2)], dim=0)
    with torch.no_grad():
        assert torch.equal(m.create_node_pixels(frames64, 2), want) and not ran      # eval: its outputs are unused
    m.train()
    before = m.conv[0].bn.running_mean.clone()
    assert torch.equal(m.create_node_pixels(frames64, 2), want) and ran == [1]       # training: the reference runs it
    assert not torch.equal(m.conv[0].bn.running_mean, before) and int(m.conv[0].bn.num_batches_tracked) == 1
