"""CPU: the host side of the UNet tail's HIP backward (csrc/pack_train.hip) -- the ABI, the slice plan and the workspace bound as
include/echoglad_hip.h documents them, the refusals that come before any launch, and the model switch.  No GPU needed."""
import ctypes as ct
import re

import pytest

from echoglad_amd import _lib
from echoglad_amd.examples import UNetNodeFeatureModel

DECLS = """
size_t eg_conv1x1_relu_pack_bwd_workspace_bytes(const int* level_channels, const int* level_side, int n_levels, int batch);
int eg_conv1x1_relu_pack_bwd_plan(const int* level_channels, const int* level_side, int n_levels, int batch, int* level_slices,
 int* level_tiles_per_slice);
int eg_conv1x1_relu_pack_bwd(const float* d_nodes, const float* nodes, const float* const* level_feats,
 const float* const* level_weights, const int* level_channels, const int* level_side, int n_levels,
 int batch, int64_t n_rows, int64_t row_offset, void* workspace, float* const* d_feats,
 float* const* d_weights, float* const* d_biases, eg_stream_t stream);
"""
NAMES = ["eg_conv1x1_relu_pack_bwd", "eg_conv1x1_relu_pack_bwd_plan", "eg_conv1x1_relu_pack_bwd_workspace_bytes"]

DEFAULT = ((2, 4, 8, 16, 32, 64, 128, 224), (512, 256, 128, 64, 32, 16, 8, 4))
# (sides, chans, batch) of tests/test_gpu_tail_bwd.py
SMALL = [((2, 3, 8), (32, 31, 64), 2), ((1, 4, 17), (1, 33, 5), 1), ((6,), (512,), 2),
         ((2, 40), (64, 4), 3), ((1, 3, 65), (33, 64, 5), 1), ((4, 72), (16, 4), 2), ((2, 4, 8, 16), (512, 256, 31, 1), 5),
         ((3, 12), (40, 256), 7)]
CASES = SMALL + [(*DEFAULT, b) for b in (1, 8, 32, 64)]


def cap(c):
    """The documented cap on the slices of a level with c channels."""
    return max(16, min(1024, 4096 // c))


def tiles(side, batch):
    return batch * -(-side * side // 64)


def _ints(v):
    return (ct.c_int * len(v))(*v)


def plan(sides, chans, batch):
    lib = _lib.load()
    n = len(sides)
    slices, tps = (ct.c_int * n)(), (ct.c_int * n)()
    assert lib.eg_conv1x1_relu_pack_bwd_plan(_ints(chans), _ints(sides), n, batch, slices, tps) == _lib.EG_OK
    return list(slices), list(tps)


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_and_binding_declare_abi_153():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert sorted(want) == NAMES
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name == "eg_conv1x1_relu_pack_bwd")
    assert _lib.ABI_VERSION >= 153
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 153: .*eg_conv1x1_relu_pack_bwd_plan", _flat(text))            # the ABI history line
    assert "clamp(4096 / c, 16, 1024)" in text                                            # the cap this file restates


def test_library_reports_the_abi_and_exports_the_entry_points(built_lib):
    lib = _lib.load()
    assert lib.eg_version() == _lib.ABI_VERSION >= 153
    assert not [n for n in NAMES if not hasattr(lib, n)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c[0])) + f"-b{c[2]}")
def test_plan_covers_the_tiles_under_the_cap_and_sizes_the_workspace(case, built_lib):
    sides, chans, batch = case
    lib = _lib.load()
    slices, tps = plan(sides, chans, batch)
    assert (slices, tps) == plan(sides, chans, batch)                                     # a function of the shapes alone
    floats = 0
    for p, c, s, t in zip(sides, chans, slices, tps):
        n = tiles(p, batch)
        assert s >= 1 and t >= 1 and s * t >= n > (s - 1) * t                            # every tile, no empty slice
        assert s <= cap(c) and t == -(-n // cap(c))
        floats += min(cap(c), n) * 128 * (c + 1)
    assert lib.eg_conv1x1_relu_pack_bwd_workspace_bytes(_ints(chans), _ints(sides), len(sides), batch) == 4 * floats


def test_plan_of_the_default_dims(built_lib):
    """Batch 1: the frame-sized level (784 tiles, 4 channels) gets 784 one-tile workgroups, more than two per CU of 256; from batch
    2 on its slices hold several tiles and its workspace no longer grows."""
    slices, tps = plan(*DEFAULT, 1)
    assert (slices[-1], tps[-1]) == (784, 1) and slices[-1] >= 2 * 256
    assert slices[:4] == [1, 1, 1, 4] and tps[:7] == [1] * 7
    slices8, tps8 = plan(*DEFAULT, 8)
    assert (slices8[-1], tps8[-1]) == (896, 7) and (slices8[-2], tps8[-2]) == (512, 4)
    lib = _lib.load()
    nbytes = lambda sides, chans, b: lib.eg_conv1x1_relu_pack_bwd_workspace_bytes(_ints(chans), _ints(sides), len(sides), b)
    for p, c in zip(*DEFAULT):                                                            # per level: the cap is reached at batch 32 or not
        if tiles(p, 32) >= cap(c):
            assert nbytes([p], [c], 32) == nbytes([p], [c], 64) == 4 * cap(c) * 128 * (c + 1)
        else:
            assert nbytes([p], [c], 32) < nbytes([p], [c], 64)
    assert [tiles(p, 32) >= cap(c) for p, c in zip(*DEFAULT)] == [True] * 8
    total = nbytes(*DEFAULT, 64)
    assert total == nbytes(*DEFAULT, 32) == nbytes(*DEFAULT, 4096) == 19_922_944          # "19.9 MB" of the header
    assert all(4 * cap(c) * 128 * (c + 1) <= 2_621_440 for c in range(1, 257))            # "2.62 MB per level up to 256 channels"


def test_out_of_range_shapes_have_no_plan(built_lib):
    lib = _lib.load()
    one, out = _ints([4]), (ct.c_int * 16)()
    nbytes = lib.eg_conv1x1_relu_pack_bwd_workspace_bytes
    for chans, sides, n, batch in (([4], [8], 1, 0), ([0], [8], 1, 1), ([4], [0], 1, 1), ([4] * 17, [2] * 17, 17, 1), ([4], [8], 0, 1),
                                   ([4], [224], 1, 42800), ([4], [46341], 1, 1)):
        assert nbytes(_ints(chans), _ints(sides), n, batch) == 0, (chans, sides, n, batch)
        assert lib.eg_conv1x1_relu_pack_bwd_plan(_ints(chans), _ints(sides), n, batch, out, out) == _lib.EG_ERR_ARG
    assert nbytes(None, one, 1, 1) == 0 and nbytes(one, None, 1, 1) == 0
    assert lib.eg_conv1x1_relu_pack_bwd_plan(one, one, 1, 1, None, out) == _lib.EG_ERR_ARG
    assert nbytes(_ints([4]), _ints([224]), 1, 42799) > 0                                 # 42799 * 50176 < 2^31 rows


def test_bad_arguments_return_eg_err_arg_with_nothing_launched(built_lib):
    """Without a GPU a launch would come back as EG_ERR_HIP: EG_ERR_ARG shows that the check came first."""
    lib = _lib.load()
    mem = (ct.c_float * 64)()                              # never dereferenced: every call below is refused
    p = [ct.c_void_p(ct.addressof(mem) // 16 * 16 + 16 * (i + 1)) for i in range(8)]
    arr = lambda *v: (ct.c_void_p * len(v))(*v)

    def bwd(d_nodes=p[0], nodes=p[1], feats=arr(p[2]), ws_=arr(p[3]), chans=(8,), sides=(4,), n=1, batch=1, n_rows=16, row_offset=0,
            workspace=p[4], df=arr(p[5]), dw=arr(p[6]), db=arr(p[7])):
        return lib.eg_conv1x1_relu_pack_bwd(d_nodes, nodes, feats, ws_, _ints(chans), _ints(sides), n, batch, n_rows, row_offset, workspace,
                                            df, dw, db, None)

    odd = ct.c_void_p(p[0].value + 4)
    rows = [(dict(d_nodes=None), "NULL"), (dict(nodes=None), "NULL"),
            (dict(n=17, chans=(8,) * 17, sides=(1,) * 17, feats=arr(*[p[2]] * 17), ws_=arr(*[p[3]] * 17), df=None, dw=None, db=None), "bad argument"),
            (dict(n=0), "bad argument"), (dict(batch=0), "bad argument"), (dict(n_rows=0), "bad argument"), (dict(row_offset=-1), "bad argument"),
            (dict(n_rows=15), "do not fit"), (dict(row_offset=1), "do not fit"),
            (dict(batch=1 << 16, n_rows=1 << 15), "exceeds int32"),
            (dict(sides=(0,)), "bad side"), (dict(chans=(0,)), "bad side"),
            (dict(d_nodes=odd), "16-byte"), (dict(nodes=odd), "16-byte"), (dict(feats=arr(odd)), "16-byte"), (dict(df=arr(odd)), "16-byte"),
            (dict(ws_=arr(None)), "needs its weight"), (dict(feats=arr(None)), "needs its features"), (dict(workspace=None), "workspace")]
    for kw, words in rows:
        assert bwd(**kw) == _lib.EG_ERR_ARG, kw
        assert words in _lib.last_error(), (kw, _lib.last_error())
    # nothing wanted: nothing to launch, so EG_OK without a device
    assert bwd(df=None, dw=None, db=None, workspace=None) == _lib.EG_OK
    assert bwd(df=arr(None), dw=arr(None), db=arr(None), workspace=None, feats=None, ws_=None) == _lib.EG_OK


SMALL_MODEL = dict(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=16, num_aux_graphs=3,
                   node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit",
                   use_coordinate_graph=False)


def test_model_switch(monkeypatch):
    import torch
    from echoglad_amd import ops
    m = UNetNodeFeatureModel(**SMALL_MODEL)
    keys = list(m.state_dict())
    assert m.hip_tail is False
    assert m.enable_hip_frontend(True, train=True).hip_tail is False                     # as before this switch existed
    assert m.enable_hip_frontend(True, tail=True) is m and m.hip_tail is True and m.hip_frontend_train is False
    assert m.enable_hip_frontend(True, train=True, tail=True).hip_tail is True and m.hip_frontend_train is True
    assert m.enable_hip_frontend(False, tail=True).hip_tail is False
    assert list(m.state_dict()) == keys
    seen = []
    monkeypatch.setattr(ops, "conv1x1_relu_pack_levels", lambda *a, **k: seen.append(k["backward"]) or torch.zeros(2 * m._row_ranges()[0], 128))
    x = torch.randn(2, 4, 16, 16)
    for flag in (False, True):
        m.enable_hip_frontend(True, tail=flag).create_node_pixels(x, 2)
    assert seen == ["torch", "hip"]
    with pytest.raises(ValueError, match='"torch" or "hip"'):
        monkeypatch.undo()
        ops.conv1x1_relu_pack_levels([x], [torch.zeros(128, 4)], [None], 2, 256, backward="rocm")


def test_tail_with_connection_nodes_is_refused():
    m = UNetNodeFeatureModel(**SMALL_MODEL, use_connection_nodes=True)
    with pytest.raises(ValueError, match="use_connection_nodes"):
        m.enable_hip_frontend(True, train=True, tail=True)
    assert m.hip_frontend is False and m.hip_tail is False
    assert m.enable_hip_frontend(True, train=True).hip_frontend_train is True            # without the tail: as before
