"""Thin Python wrappers over the C-ABI (no compute here; pointers + stream only).

Every function enqueues on ``torch.cuda.current_stream()`` and returns torch
tensors that own the output memory.  Inputs must be CUDA fp32 contiguous
``[rows, 128]``.

One module per family of entry points; ``_core`` holds what they share (the call into the library, the argument checker,
the scratch cache).  Everything public is re-exported here: ``from echoglad_amd import ops; ops.gcn_layer_fwd(...)``."""
from ._core import C, _level_arrays, _ptr, _stream                                         # noqa: F401  (_*: tests' raw ABI calls)
from .graph import LAUNCH_KINDS, Graph, dropout_epoch, dropout_epoch_add, dropout_epoch_set, edge_hash, layer_timing   # noqa: F401
from .infer import classifier_fwd, conv1x1_relu_heads, fold_lo_index, fold_lo_table, gcn_aggregate, gcn_layer_cls_fold_fwd, gcn_layer_cls_fwd, gcn_layer_fwd, linear128_fwd, new_kidsum, split3_planes          # noqa: F401
from .train import (CLS_GRADS_FLOATS, bn_act_bwd, bn_act_fwd, bn_act_fwd_tiles, bn_stats, classifier_bwd,             # noqa: F401
                    classifier_layer_sums_supported, classifier_recompute_h_supported, classifier_train_fwd,
                    classifier_train_fwd_act, colsum128, dweight128, gcn_layer_bwd, gcn_layer_train_fwd, lower_sums_supported)
from .coord import (COORD_MLP_GRADS_FLOATS, bilinear4, bilinear4_bwd, bilinear4_fwd, coord_mlp_bwd, coord_mlp_fwd,     # noqa: F401
                    coord_update_bwd, coord_update_fwd, scatter_coord_rows)
from .criteria import (CONFUSION_MAX_CHANNELS, CONFUSION_WORKSPACE_BYTES, HEATMAP_RENDER_OUTPUTS, LANDMARK_DETAIL_FLOATS,   # noqa: F401
                       LANDMARK_RECORD_FLOATS, bce_logits, bce_logits_fwd, bce_probs, bce_probs_fwd, confusion_counts, elm_reduce,
                       heatmap_expect, heatmap_expect_bwd, heatmap_expect_fwd, heatmap_render, landmark_criteria, landmark_record_coord, landmark_record_hm,
                       landmark_record_workspace_bytes)
from .frontend import adaptive_max_pool, adaptive_max_pool_train, conv3x3_relu_bn, conv3x3_relu_bn_train               # noqa: F401
from .embedder import embed_block, embed_block_train, pyramid_block, pyramid_block_train                                        # noqa: F401
from .frame_prep import frame_prep                                                                                     # noqa: F401
from .labels import node_labels                                                                                  # noqa: F401
from .pack import (avg_pool_pyramid, conn_rows_bwd, conn_rows_chain, conn_rows_fwd, conn_rows_plan, conv1x1_relu_pack_levels,   # noqa: F401
                   pack_levels, pyramid_pack, pyramid_supported)
