"""CPU: the host side of the connection rows' fixed-order means (csrc/conn_rows.hip) -- the ABI, the chunk plan and the workspace
formula as include/echoglad_hip.h documents them, the refusals that come before any launch, and the model switches.  No GPU needed."""
import ctypes as ct
import re

import pytest

from echoglad_amd import _lib
from echoglad_amd.examples import UNetNodeFeatureModel
from echoglad_amd.nn import HierarchicalPatchModel

DECLS = """
int eg_conn_rows_plan(int64_t rows, int* chunks, int* rows_per_chunk);
size_t eg_conn_rows_workspace_bytes(const int64_t* src_base, const int64_t* src_rows, int n_conn, int batch, int64_t n_rows);
int eg_conn_rows_fwd(float* nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
 void* workspace, eg_stream_t stream);
int eg_conn_rows_bwd(float* d_nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
 eg_stream_t stream);
"""
NAMES = ["eg_conn_rows_bwd", "eg_conn_rows_fwd", "eg_conn_rows_plan", "eg_conn_rows_workspace_bytes"]
ROWS = [1, 4, 63, 64, 65, 256, 400, 4097, 16384, 50176, 200704]


def _i64(v):
    return (ct.c_int64 * len(v))(*v)


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def plan(rows):
    chunks, rpc = ct.c_int(), ct.c_int()
    assert _lib.load().eg_conn_rows_plan(rows, ct.byref(chunks), ct.byref(rpc)) == _lib.EG_OK
    return chunks.value, rpc.value


def test_header_and_binding_declare_abi_157():
    text = open(_lib.HEADER_PATH).read()
    header = _flat(re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    want = _lib.parse_header(DECLS)
    assert sorted(want) == NAMES
    for decl in DECLS.strip().split(";"):
        if decl.strip():
            assert _flat(decl) + ";" in header, decl
    for name, (res, args, takes_stream) in want.items():
        assert _lib.SIGNATURES[name] == (res, args)
        assert (name in _lib.TAKES_STREAM) == takes_stream == (name in ("eg_conn_rows_fwd", "eg_conn_rows_bwd"))
    assert _lib.ABI_VERSION >= 157
    assert f"#define EG_ABI_VERSION {_lib.ABI_VERSION}" in text
    assert re.search(r"\* 157: .*eg_conn_rows_plan", _flat(text))                          # the ABI history line
    assert "rows_per_chunk = max(128, ceil(rows / 512))" in text                           # the plan this file restates
    assert "d(rows) = (ceil(min(rows, rows_per_chunk) / 8) - 1) + 7 + (chunks - 1)" in _flat(text).replace("* ", "")


def test_library_reports_the_abi_and_exports_the_entry_points(built_lib):
    lib = _lib.load()
    assert lib.eg_version() == _lib.ABI_VERSION >= 157
    assert not [n for n in NAMES if not hasattr(lib, n)]


@pytest.mark.parametrize("rows", ROWS)
def test_plan_covers_the_rows_and_is_the_documented_arithmetic(rows, built_lib):
    chunks, rpc = plan(rows)
    assert (chunks, rpc) == plan(rows)
    assert chunks >= 1 and rpc >= 1 and chunks * rpc >= rows > (chunks - 1) * rpc          # every row, no empty chunk
    assert rpc == max(128, -(-rows // 512)) and chunks == -(-rows // rpc) and chunks <= 512
    from echoglad_amd import ops
    assert ops.conn_rows_plan(rows) == (chunks, rpc)
    assert ops.conn_rows_chain(rows) == (-(-min(rows, rpc) // 8) - 1) + 7 + (chunks - 1)


def test_plan_of_the_frame_sized_level_and_bad_rows(built_lib):
    lib = _lib.load()
    assert plan(50176) == (392, 128) and plan(50176)[0] >= 256                             # at least one chunk per CU at batch 1
    assert plan(128) == (1, 128) and plan(129) == (2, 128) and plan(200704) == (512, 392)
    c, r = ct.c_int(), ct.c_int()
    for rows in (0, -1, 1 << 31):
        assert lib.eg_conn_rows_plan(rows, ct.byref(c), ct.byref(r)) == _lib.EG_ERR_ARG
    assert lib.eg_conn_rows_plan(4, None, ct.byref(r)) == _lib.EG_ERR_ARG
    assert lib.eg_conn_rows_plan(4, ct.byref(c), None) == _lib.EG_ERR_ARG


def test_workspace_is_the_header_formula_and_the_plan_ignores_the_batch(built_lib):
    """batch * (sum over the distinct sources of more than one chunk of chunks) * 512 bytes."""
    lib = _lib.load()
    nbytes = lambda base, rows, batch, n_rows: lib.eg_conn_rows_workspace_bytes(_i64(base), _i64(rows), len(base), batch, n_rows)
    rows = [4, 16, 64, 256, 1024, 4096, 16384, 50176]                                      # the default dims, "level"
    base, at = [], len(rows)
    for r in rows:
        base.append(at)
        at += r
    per_frame = sum(plan(r)[0] for r in rows if plan(r)[0] > 1)
    assert per_frame == 2 + 8 + 32 + 128 + 392
    for batch in (1, 3, 32):
        assert nbytes(base, rows, batch, at) == batch * per_frame * 512
        assert nbytes(base, rows, batch, at + 4) == batch * per_frame * 512
    # "frame": eight rows name one source -- summed once
    assert nbytes([base[-1]] * 8, [50176] * 8, 2, at) == 2 * 392 * 512
    # nothing above one chunk: no workspace; a table the forward refuses: 0
    assert nbytes([3, 7, 135], [4, 128, 1], 5, 200) == 0
    assert nbytes([2], [4], 1, 200) == 0 and nbytes([3], [400], 1, 200) == 0
    assert lib.eg_conn_rows_workspace_bytes(None, _i64([4]), 1, 1, 100) == 0


def test_bad_arguments_are_refused_with_nothing_launched(built_lib):
    """Without a GPU a launch would come back as EG_ERR_HIP: EG_ERR_ARG / EG_ERR_UNSUPPORTED show that the check came first."""
    lib = _lib.load()
    mem = (ct.c_float * 64)()                              # never dereferenced: every call below is refused
    p = [ct.c_void_p(ct.addressof(mem) // 16 * 16 + 16 * (i + 1)) for i in range(2)]
    odd = ct.c_void_p(p[0].value + 4)

    def fwd(nodes=p[0], batch=1, n_rows=1000, base=(3, 10, 500), rows=(4, 400, 129), n=None, ws=p[1], null=()):
        b = None if "base" in null else _i64(base)
        r = None if "rows" in null else _i64(rows)
        n = len(base) if n is None else n
        return (lib.eg_conn_rows_fwd(nodes, batch, n_rows, n, b, r, ws, None), lib.eg_conn_rows_bwd(nodes, batch, n_rows, n, b, r, None))

    A, U = _lib.EG_ERR_ARG, _lib.EG_ERR_UNSUPPORTED
    cases = [(dict(nodes=None), A, "NULL"), (dict(null=("base",)), A, "NULL"), (dict(null=("rows",)), A, "NULL"),
             (dict(nodes=odd), A, "16-byte"),
             (dict(n=0), A, "at least 1"), (dict(batch=0), A, "at least 1"), (dict(n_rows=0), A, "at least 1"),
             (dict(rows=(4, 0, 129)), A, "at least one row"), (dict(rows=(4, -1, 129)), A, "at least one row"),
             (dict(base=(2, 10, 500)), A, "touches the connection rows"), (dict(base=(3, 10, 0)), A, "touches the connection rows"),
             (dict(base=(3, 10, 872)), A, "ends past"), (dict(n_rows=628), A, "ends past"),
             (dict(base=(3, 6, 500)), A, "equal or disjoint"), (dict(base=(3, 10, 409)), A, "equal or disjoint"),
             (dict(base=tuple(range(17, 34)), rows=(1,) * 17, n=17), U, "at most 16"),
             (dict(batch=1 << 16, n_rows=1 << 15), U, "exceeds int32")]
    for kw, rc, words in cases:
        for got in fwd(**kw):
            assert got == rc, (kw, got)
            assert words in _lib.last_error(), (kw, _lib.last_error())
    # the workspace is wanted by the forward alone, and only for a source of more than one chunk
    assert lib.eg_conn_rows_fwd(p[0], 1, 1000, 3, _i64((3, 10, 500)), _i64((4, 400, 129)), None, None) == A
    assert "workspace" in _lib.last_error()
    assert lib.eg_conn_rows_fwd(p[0], 1, 1000, 3, _i64((3, 10, 500)), _i64((4, 400, 129)), odd, None) == A
    # (equal sources and ranges that fit exactly are accepted: tests/test_gpu_conn_rows.py runs them, nothing here may launch)


SMALL_UNET = dict(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=16, num_aux_graphs=3,
                  node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, num_gnn_layers=2, output_activation="logit",
                  use_coordinate_graph=False)


def test_switch_semantics():
    m = UNetNodeFeatureModel(**SMALL_UNET, use_connection_nodes=True)
    keys = list(m.state_dict())
    assert m.hip_conn_rows is False
    with pytest.raises(ValueError, match="use_connection_nodes"):
        m.enable_hip_frontend(True, train=True, tail=True)                                  # off: refused as before
    assert m.hip_tail is False
    assert m.enable_hip_conn_rows() is m and m.hip_conn_rows is True
    assert m.enable_hip_frontend(True, train=True, tail=True) is m and m.hip_tail is True    # accepted behind the switch
    with pytest.raises(ValueError, match="enable_hip_conn_rows"):
        m.enable_hip_conn_rows(False)                                                        # not under the tail
    assert m.hip_conn_rows is True
    m.enable_hip_frontend(True, train=True)
    assert m.hip_tail is False and m.enable_hip_conn_rows(False).hip_conn_rows is False
    assert list(m.state_dict()) == keys and "hip_conn_rows" not in dict(m.named_buffers())
    # without connection nodes the switch changes nothing and binds nothing
    plain = UNetNodeFeatureModel(**SMALL_UNET).enable_hip_conn_rows().enable_hip_frontend(True, tail=True)
    assert plain.enable_hip_conn_rows(False).hip_tail is True
    base = HierarchicalPatchModel(frame_size=16, num_aux_graphs=3, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                  use_connection_nodes=True)
    assert base.hip_conn_rows is False and base.enable_hip_conn_rows().hip_conn_rows is True
    assert base.enable_hip_conn_rows(False).hip_conn_rows is False


def test_models_pass_conn_rows_only_behind_the_switch(monkeypatch):
    import torch
    from echoglad_amd import ops
    from echoglad_amd.nn import CNNHierarchicalPatchModel
    seen = []

    def fake(name):
        def f(*a, **k):
            seen.append((name, k.get("conn_rows", "absent")))
            return torch.zeros(1, 128)
        return f
    for name in ("pyramid_pack", "pack_levels", "conv1x1_relu_pack_levels"):
        monkeypatch.setattr(ops, name, fake(name))
    monkeypatch.setattr(ops, "pyramid_supported", lambda x, sides: True)
    kw = dict(frame_size=16, num_aux_graphs=3, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32, use_connection_nodes=True)
    finish = lambda self, feats, B, node_coords, conn: seen.append(("finish", conn is None)) or feats
    monkeypatch.setattr(HierarchicalPatchModel, "_finish_node_features", finish)
    x128, x4 = torch.randn(2, 128, 16, 16), torch.randn(2, 4, 16, 16)
    models = [(HierarchicalPatchModel(**kw), x128, "pyramid_pack", "frame"),
              (CNNHierarchicalPatchModel(cnn_layers_out_width=[8, 4, 2], **kw), x128, "pack_levels", "level"),
              (UNetNodeFeatureModel(**SMALL_UNET, use_connection_nodes=True), x4, "conv1x1_relu_pack_levels", "level")]
    for m, x, name, mode in models:
        m.eval()
        for flag, want in ((False, "absent"), (True, mode)):
            seen.clear()
            with torch.no_grad():
                m.enable_hip_conn_rows(flag).create_node_pixels(x, 2)
            assert seen == [(name, want), ("finish", flag)], (name, flag, seen)
    # the base model's adaptive_avg_pool2d route
    monkeypatch.setattr(ops, "pyramid_supported", lambda x, sides: False)
    seen.clear()
    with torch.no_grad():
        models[0][0].enable_hip_conn_rows(True).create_node_pixels(x128, 2)
    assert seen == [("pack_levels", "frame"), ("finish", True)]


def test_conn_rows_keyword_is_checked_before_anything_runs():
    import torch
    from echoglad_amd import ops
    maps = [torch.zeros(1, 128, 2, 2), torch.zeros(1, 128, 4, 4)]
    with pytest.raises(ValueError, match='"level" or "frame"'):
        ops.pack_levels(maps, 1, 22, 2, conn_rows="mean")
    with pytest.raises(RuntimeError, match="row_offset 1 != 2 levels"):
        ops.pack_levels(maps, 1, 22, 1, conn_rows="level")
    with pytest.raises(RuntimeError, match="row_offset 0 != 2 levels"):
        ops.pyramid_pack(torch.zeros(1, 128, 4, 4), [2], 1, 20, 0, conn_rows="frame")
    with pytest.raises(RuntimeError, match="row_offset 3 != 1 levels"):
        ops.conv1x1_relu_pack_levels([torch.zeros(1, 4, 4, 4)], [torch.zeros(128, 4)], [None], 1, 19, 3, conn_rows="level")
