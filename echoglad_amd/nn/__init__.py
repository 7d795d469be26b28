"""Host-side mirror of the reference's operator surface for the GNN hot path.

Same names, constructor arguments, call shapes and state_dict keys as the
reference (src/core/models.py:262-553 and the torch_geometric classes it
imports at :5), so a loop shaped like src/engine.py:240-262 drives the HIP
kernels unchanged and ``miccai2023.pth``-style checkpoints load ``strict=True``:

    gnn_layers.{i}.module_0.lin.weight / .bias        (GCNConv)
    gnn_layers.{i}.module_1.{weight,bias,running_*}   (BatchNorm1d)
    node_classifiers.{c}.{0,1,4,5,8}.*
    node_coordinate_mlp.{i}.{0,1,4,5,8}.*

Compute goes through the C-ABI library only (echoglad_amd/ops/); torch is
used for parameter storage, autograd bookkeeping, streams and the tiny
per-landmark coordinate MLP (4 rows per frame).  There is no CPU fallback.

By role:
    _resolve   edge_index -> graph handle (GraphResolver, the resolver every stand-alone GCNConv shares)
    _heads     parameter tables of the heads / coordinate MLPs and their stacked layout
    _train     ROUTES, the train-mode blocks (layer, heads, coordinate update) and the autograd nodes over them
    modules    GCNConv, Sequential, JumpingKnowledge, eval-mode folding
    embedder   CNNResBlock, CNN: the reference's CNN embedder, torch modules by default, the HIP embedder after enable_hip
    cnn_pyramid  CNNHierarchicalPatchModel: the reference's CNN-pyramid variant, torch modules by default, ops.pyramid_block after
               enable_hip_pyramid
    frontend   unet_decoder_maps / unet_decoder_maps_train: the UNet variant's encoder / decoder on the HIP front-end operators
    model      HierarchicalPatchModel: forward_nodes and its three routes"""
from ._heads import (_HEAD_SIZES, _MLP_NAMES, _head_param_offsets, _mlp_grads, _move_into, _seq_params, _stack_head_params,
                     _unstack_head_grads, _views_of)
from ._resolve import _SHARED_RESOLVER, GraphResolver
from ._train import ROUTES, Routes
from .embedder import CNN, CNNResBlock
from .frontend import unet_decoder_maps, unet_decoder_maps_train
from .model import HierarchicalPatchModel
from .cnn_pyramid import CNNHierarchicalPatchModel
from .modules import C, GCNConv, JumpingKnowledge, Sequential

__all__ = ["C", "ROUTES", "Routes", "GraphResolver", "HierarchicalPatchModel", "GCNConv", "Sequential", "JumpingKnowledge",
           "unet_decoder_maps", "unet_decoder_maps_train", "CNN", "CNNResBlock", "CNNHierarchicalPatchModel"]
