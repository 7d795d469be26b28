"""The ctypes table that echoglad_amd/_lib.py reads from include/echoglad_hip.h, and the public surface of echoglad_amd.ops.
No GPU and no built library needed: the table comes from the header's text alone."""
import ctypes as ct
import re

import pytest

from echoglad_amd import _lib

_p, _i, _i64, _u64, _f, _sz = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_uint64, ct.c_float, ct.c_size_t

# written out by hand, argument by argument, from the declarations (every pointer but the three typed structs is a void*)
PINNED = {
    "eg_last_error": (ct.c_char_p, []),
    "eg_gcn_layer_train_fwd": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _f, _f, _i, _f, _u64, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "eg_criteria_ex_fwd": (_i, [_p, _p, _p, _i, _i64, _p, _p, _i, _p, _f, _f, _f, _p, _p, _i64, _f, _p, _p, _p,
                                _p, _p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "eg_adam_step": (_i, [_p, _i, _p, _f, _p, _f, _f, _f, _f, _i, _p]),
    "eg_confusion_counts": (_i, [_p, _p, _p, _i64, _i, _p, _sz, _p, _i64, _p, _p]),
    "eg_gcn_layer_bwd_lower": (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _f, _u64, _i, _p, _p, _p, _p, _p, _p, _p,
                                    ct.POINTER(_lib.GivenSums), ct.POINTER(_lib.LowerSums), _p]),
    "eg_classifier_train_fwd": (_i, [_p, _i, _i64, _i64, _i64, ct.POINTER(_lib.ClsTrainParams), _p, _p, _p, _p, _i, _p, _p]),
    "eg_workspace_bytes": (_sz, []),
    "eg_graph_ps_launches": (ct.c_uint, [_p]),
    "eg_graph_num_nodes": (_i64, [_p]),
}


def _declarations():
    """(name, number of parameters) of every function the header declares, by a count of commas that knows nothing of types."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(eg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        found[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return found


def test_every_declaration_has_an_entry_with_as_many_arguments():
    declared = _declarations()
    assert len(declared) >= 80 and "eg_topo_create" in declared and declared["eg_version"] == 0
    assert set(_lib.SIGNATURES) == set(declared)
    assert _lib.header_symbols() == sorted(declared)
    for name, count in declared.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == count, (name, count, argtypes)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    restype, argtypes = _lib.SIGNATURES[name]
    want_res, want_args = PINNED[name]
    assert restype is want_res
    assert len(argtypes) == len(want_args)
    for k, (got, want) in enumerate(zip(argtypes, want_args)):
        if isinstance(want, type) and issubclass(want, ct._Pointer):
            assert issubclass(got, ct._Pointer) and got._type_ is want._type_, (name, k)
        else:
            assert got is want, (name, k, got, want)


def test_stream_argument_is_recognised_only_in_last_place():
    assert "eg_gcn_layer_fwd" in _lib.TAKES_STREAM and "eg_adam_step" in _lib.TAKES_STREAM
    assert "eg_csr_create" not in _lib.TAKES_STREAM          # (its stream sits in front of the handle it returns)
    assert "eg_version" not in _lib.TAKES_STREAM and "eg_heatmap_workspace_bytes" not in _lib.TAKES_STREAM


def test_a_type_without_a_mapping_raises_with_the_entry_points_name():
    good = _lib.parse_header("int eg_fake(const float* x, int64_t rows, eg_stream_t stream);")
    assert good == {"eg_fake": (_i, [_p, _i64, _p], True)}
    for header in ("int eg_fake(const float* x, long double y, eg_stream_t stream);",
                   "int eg_fake(struct foo* x);",
                   "double eg_fake(void);",
                   "int eg_fake(const int side[], int n);",          # an array parameter: its name must not be taken for the type's end
                   "int eg_fake(eg_given_sums given);"):              # a struct by value
        with pytest.raises(RuntimeError, match="eg_fake"):
            _lib.parse_header(header)
    with pytest.raises(RuntimeError, match="eg_fake"):
        _lib.parse_header("int eg_fake(void);\nint eg_fake(int again);")


def test_a_missing_header_names_its_path(monkeypatch, tmp_path):
    gone = tmp_path / "include" / "echoglad_hip.h"
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    with pytest.raises(RuntimeError, match=re.escape(str(gone))):
        _lib._read_header()


PUBLIC_OPS = """C CLS_GRADS_FLOATS CONFUSION_MAX_CHANNELS CONFUSION_WORKSPACE_BYTES COORD_MLP_GRADS_FLOATS Graph LANDMARK_DETAIL_FLOATS
LANDMARK_RECORD_FLOATS LAUNCH_KINDS avg_pool_pyramid bce_logits bce_logits_fwd bce_probs bce_probs_fwd bilinear4 bilinear4_bwd
bilinear4_fwd bn_act_bwd bn_act_fwd bn_act_fwd_tiles bn_stats classifier_bwd classifier_fwd classifier_layer_sums_supported
classifier_recompute_h_supported classifier_train_fwd classifier_train_fwd_act colsum128 confusion_counts conv1x1_relu_pack_levels
coord_mlp_bwd coord_mlp_fwd coord_update_bwd coord_update_fwd dropout_epoch dropout_epoch_add dropout_epoch_set dweight128 edge_hash
elm_reduce gcn_aggregate gcn_layer_bwd gcn_layer_cls_fwd gcn_layer_fwd gcn_layer_train_fwd heatmap_expect heatmap_expect_bwd
heatmap_expect_fwd landmark_criteria landmark_record_coord landmark_record_hm landmark_record_workspace_bytes layer_timing
linear128_fwd lower_sums_supported new_kidsum pack_levels pyramid_pack pyramid_supported scatter_coord_rows""".split()


def test_ops_exports_every_public_name():
    from echoglad_amd import ops
    assert len(PUBLIC_OPS) == len(set(PUBLIC_OPS)) == 60
    assert [n for n in PUBLIC_OPS if not hasattr(ops, n)] == []
    assert not hasattr(ops, "train_chain_supported")
    assert ops.C == 128 and ops.CLS_GRADS_FLOATS == 19076 and ops.COORD_MLP_GRADS_FLOATS == 5042


def test_call_helper_counts_arguments_and_names_the_entry_point(built_lib):
    """The one call path refuses a wrong number of arguments by name before ctypes sees them, and a status other than EG_OK
    raises with the entry point's name (a null graph handle: EG_ERR_ARG, nothing is launched)."""
    from echoglad_amd.ops import _core
    with pytest.raises(RuntimeError, match="eg_graph_num_nodes takes 1 arguments, got 2"):
        _core.raw("eg_graph_num_nodes", None, None)
    assert _core.raw("eg_graph_destroy", None) == _lib.EG_OK
    with pytest.raises(RuntimeError, match="eg_debug_phase_cycles failed"):
        _core.call("eg_debug_phase_cycles", None, None, 0)
    with pytest.raises(RuntimeError, match="eg_debug_layer_timing_begin: argument 1"):          # a float where the header says int
        _core.raw("eg_debug_layer_timing_begin", 1.5)
    with pytest.raises(RuntimeError, match="does not export eg_no_such_entry"):
        _core.raw("eg_no_such_entry")
