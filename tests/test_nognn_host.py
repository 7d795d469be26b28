"""CPU: the host side of the no-GNN baselines -- the ABI of eg_conv1x1_relu_heads_fwd (csrc/tail_heads.hip), its refusals before any
launch, the state_dict of UNetNoGNN / UNet, the model registry and builder (echoglad_amd/models.py) and the model's switch between
the fused launch and the composed route.  No GPU needed."""
import copy
import ctypes as ct
import json
import os
import re

import pytest
import torch

from echoglad_amd import _lib, models, nn, ops
from echoglad_amd.examples import UNet, UNetNoGNN, UNetNodeFeatureModel

DECLS = """
int eg_conv1x1_relu_heads_fwd(const float* const* level_feats, const float* const* level_weights,
 const float* const* level_biases, const int* level_channels, const int* level_side, int n_levels,
 int batch, const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
 const float* t2, const float* w3, const float* b3, int sigmoid, float* logits, eg_stream_t stream);
"""
NAME = "eg_conv1x1_relu_heads_fwd"


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def _ints(v):
    return (ct.c_int * len(v))(*v)


def test_header_and_binding_declare_abi_154():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert list(want) == [NAME]
    assert _flat(DECLS) in header
    res, args, takes_stream = want[NAME]
    assert _lib.SIGNATURES[NAME] == (res, args) and takes_stream and NAME in _lib.TAKES_STREAM
    assert len(args) == 18
    assert _lib.ABI_VERSION >= 154
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 154: eg_conv1x1_relu_heads_fwd", _flat(text))                   # the ABI history line


def test_library_reports_the_abi_and_exports_the_entry_point(built_lib):
    lib = _lib.load()
    assert lib.eg_version() == _lib.ABI_VERSION >= 154
    assert hasattr(lib, NAME) and not _lib.check_exports()


def test_bad_arguments_return_eg_err_arg_with_nothing_launched(built_lib):
    """Without a GPU a launch would come back as EG_ERR_HIP: EG_ERR_ARG shows that the check came first."""
    lib = _lib.load()
    mem = (ct.c_float * 64)()                              # never dereferenced: every call below is refused
    p = [ct.c_void_p(ct.addressof(mem) // 16 * 16 + 16 * (i + 1)) for i in range(12)]
    arr = lambda *v: (ct.c_void_p * len(v))(*v)
    heads = ("w1", "s1", "t1", "w2", "s2", "t2", "w3", "b3")

    def fwd(feats=arr(p[0]), ws=arr(p[1]), bs=arr(p[2]), chans=(8,), sides=(4,), n=1, batch=1, logits=p[3], **kw):
        hp = [kw.get(k, p[4 + i]) for i, k in enumerate(heads)]
        return lib.eg_conv1x1_relu_heads_fwd(feats, ws, bs, None if chans is None else _ints(chans), None if sides is None else _ints(sides),
                                             n, batch, *hp, 0, logits, None)

    odd = ct.c_void_p(p[0].value + 4)
    rows = [(dict(feats=None), "NULL"), (dict(ws=None), "NULL"), (dict(chans=None), "NULL"), (dict(sides=None), "NULL"), (dict(logits=None), "NULL")]
    rows += [({k: None}, "NULL") for k in heads]
    rows += [(dict(n=0), "bad argument"), (dict(batch=0), "bad argument"), (dict(batch=-3), "bad argument"),
             (dict(n=17, chans=(8,) * 17, sides=(1,) * 17, feats=arr(*[p[0]] * 17), ws=arr(*[p[1]] * 17), bs=None), "bad argument"),
             (dict(feats=arr(None)), "NULL level map"), (dict(ws=arr(None)), "NULL level map"),
             (dict(sides=(0,)), "bad side"), (dict(chans=(0,)), "bad side"), (dict(sides=(-2,)), "bad side"),
             (dict(batch=1 << 16, sides=(256,)), "exceeds int32"), (dict(batch=1 << 15, sides=(256,), chans=(8,)), "exceeds int32"),
             (dict(sides=(46341,)), "exceeds int32"), (dict(n=2, sides=(300, 46340), chans=(8, 8), feats=arr(p[0], p[0]), ws=arr(p[1], p[1]), bs=None),
                                                       "exceeds int32"),
             (dict(logits=odd), "16-byte"), (dict(bs=arr(odd)), "16-byte"), (dict(feats=arr(odd)), "16-byte"),
             (dict(feats=arr(odd), sides=(6,)), "16-byte")]
    for kw, words in rows:
        assert fwd(**kw) == _lib.EG_ERR_ARG, kw
        assert words in _lib.last_error(), (kw, _lib.last_error())
    # a level with side^2 % 4 != 0 goes element by element: its map needs 4 bytes, so an odd address gets past the checks -- and the
    # launch is what fails without a device
    if not torch.cuda.is_available():
        assert fwd(feats=arr(odd), sides=(3,)) == _lib.EG_ERR_HIP
        assert fwd(bs=None) == _lib.EG_ERR_HIP and fwd(bs=arr(None)) == _lib.EG_ERR_HIP                 # biases are optional


DEFAULT = dict(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=3,
               output_activation="logit", use_coordinate_graph=True, gnn_dropout_p=0.5, classifier_dropout_p=0.5)


@pytest.mark.parametrize("cls", [UNetNoGNN, UNet])
def test_state_dict_is_the_unet_variants(cls, golden_dir):
    """The reference's ablations construct the parent's modules, the unused gnn_layers included: same keys, same order, same shapes,
    so a reference checkpoint loads strict=True."""
    ref = json.load(open(os.path.join(golden_dir, "unet_state_keys.json")))
    m = cls(**DEFAULT)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["state_dict"]
    assert list(m.state_dict()) == list(UNetNodeFeatureModel(**DEFAULT).state_dict())
    assert sum(q.numel() for q in m.parameters()) == ref["n_parameters"]
    assert isinstance(m, UNetNodeFeatureModel) and issubclass(UNet, UNetNoGNN) and m.fuse_tail in (True, False)


def _config(golden_dir):
    return json.load(open(os.path.join(golden_dir, "model_config_default.json")))


def test_builder_builds_the_default_config_and_every_registry_name(golden_dir):
    cfg = _config(golden_dir)
    assert set(cfg) == {"checkpoint_path", "embedder", "landmark"}
    keep = copy.deepcopy(cfg)
    built = models.build(cfg)
    assert cfg == keep                                                                     # the caller's config is not mutated
    assert list(built) == ["embedder", "landmark"]
    assert type(built["embedder"]) is nn.CNN and type(built["landmark"]) is UNetNodeFeatureModel
    assert list(models.MODELS) == ["cnn", "identical", "hierarchicalpatch", "cnn_hierarchical_patch", "unet_hierarchical_patch", "unet_noGNN", "unet"]
    for name, cls in (("unet_noGNN", UNetNoGNN), ("unet", UNet)):
        c = copy.deepcopy(keep)
        c["landmark"]["name"] = name
        assert type(models.build(c, logger=None)["landmark"]) is cls
    small = dict(frame_size=16, num_aux_graphs=2, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2,
                 output_activation="logit")
    for name, cls in (("hierarchicalpatch", nn.HierarchicalPatchModel), ("cnn_hierarchical_patch", nn.CNNHierarchicalPatchModel)):
        assert type(models.build({"checkpoint_path": "", "landmark": dict(small, name=name)})["landmark"]) is cls
    ident = models.build({"checkpoint_path": None, "embedder": {"name": "identical"}})["embedder"]
    x = torch.randn(2, 3)
    assert isinstance(ident, torch.nn.Module) and ident(x) is x and not list(ident.parameters())
    said = []
    models.build({"checkpoint_path": None, "embedder": {"name": "identical"}}, logger=type("L", (), {"infov": lambda self, m: said.append(m)})())
    assert said == ["Model is created."]


def test_builder_refuses_an_unknown_name(golden_dir):
    cfg = _config(golden_dir)
    cfg["landmark"]["name"] = "unet_plus_plus"
    with pytest.raises(KeyError, match="unet_noGNN"):
        models.build(cfg)


SMALL = dict(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=16, num_aux_graphs=3, node_embedding_dim=128,
             node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit")


@pytest.mark.parametrize("flags", [{}, {"use_coordinate_graph": True}, {"use_connection_nodes": True}, {"use_main_graph_only": True}], ids=str)
def test_model_switch(monkeypatch, flags):
    """The fused launch only in eval mode with autograd off; the composed route in training mode, with autograd on and with
    fuse_tail = False; the graph resolver is never asked."""
    m = UNetNoGNN(**SMALL, **flags)
    assert m.fuse_tail is True and "fuse_tail" not in m.state_dict()
    n, _, n_valid, _, _ = m._row_ranges()
    B = 2
    seen = []

    def fused(feats, weights, biases, batch, packed, sigmoid=False):
        seen.append(("fused", [tuple(f.shape[1:]) for f in feats], len(weights), len(biases), batch, sorted(packed), sigmoid))
        return torch.zeros(batch * sum(f.shape[2] ** 2 for f in feats), 4)

    monkeypatch.setattr(ops, "conv1x1_relu_heads", fused)
    monkeypatch.setattr(m, "create_node_pixels", lambda x, b, nc=None: seen.append(("pixels", b, nc is not None)) or torch.zeros(b * n, 128))
    monkeypatch.setattr(m, "forward_heads", lambda h, b: seen.append(("heads", tuple(h.shape), b)) or torch.zeros(b * n_valid, 4))

    def no_graph(*a, **k):
        raise AssertionError("the graph resolver was asked")
    monkeypatch.setattr(m._resolver, "resolve", no_graph)
    x = torch.randn(B, 4, 16, 16)
    coords = torch.rand(B * 4, 2) * 15 if flags.get("use_coordinate_graph") else None
    kw = dict(x=x, node_coords=coords, edge_index="never read")
    levels = [(4, 16, 16)] if flags.get("use_main_graph_only") else [(32, 2, 2), (16, 4, 4), (8, 8, 8), (4, 16, 16)]
    composed = [("pixels", B, coords is not None), ("heads", (B * n, 128), B)]
    m.eval()
    with torch.no_grad():
        out, none = m(**kw)
    assert none is None and out.shape == (B * n_valid, 4)
    assert seen == [("fused", levels, len(levels), len(levels), B, ["b3", "s1", "s2", "t1", "t2", "w1", "w2", "w3"], False)]
    del seen[:]
    m(**kw)                                                # eval mode, autograd on
    assert seen == composed
    del seen[:]
    m.train()
    with torch.no_grad():
        m(**kw)
    m(**kw)
    assert seen == composed * 2
    del seen[:]
    m.eval()
    m.fuse_tail = False
    with torch.no_grad():
        out, none = m(**kw)
    assert seen == composed and none is None and out.shape == (B * n_valid, 4)
    # a PyG-style batch object: x (and node_coords) are read from it
    del seen[:]
    m.fuse_tail = True
    batch = type("Batch", (), dict(x=x, edge_index=None, batch=None, node_type=None, node_coords=coords))()
    with torch.no_grad():
        m(batch)
    assert [s[0] for s in seen] == ["fused"]


def test_sigmoid_reaches_the_fused_launch(monkeypatch):
    m = UNet(**dict(SMALL, output_activation="sigmoid")).eval()
    seen = []
    monkeypatch.setattr(ops, "conv1x1_relu_heads", lambda f, w, b, batch, packed, sigmoid=False: seen.append(sigmoid) or torch.zeros(batch * 340, 4))
    with torch.no_grad():
        m(x=torch.randn(1, 4, 16, 16))
    assert seen == [True]
