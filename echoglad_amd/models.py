"""The reference's model registry and builder (src/builders/model_builder.py): the seven names a ``model:`` config section may
hold, mapped to this package's classes, and ``build`` in the reference builder's shape."""
from __future__ import annotations

from copy import deepcopy

import torch.nn as nn

from .examples import UNet, UNetNoGNN, UNetNodeFeatureModel
from .nn import CNN, CNNHierarchicalPatchModel, HierarchicalPatchModel


class IdenticalModel(nn.Module):
    """The reference's ``IdenticalModel`` (src/core/models.py): the embedder of the configurations without one."""

    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, x):
        return x


MODELS = {
    "cnn": CNN,
    "identical": IdenticalModel,
    "hierarchicalpatch": HierarchicalPatchModel,
    "cnn_hierarchical_patch": CNNHierarchicalPatchModel,
    "unet_hierarchical_patch": UNetNodeFeatureModel,
    "unet_noGNN": UNetNoGNN,
    "unet": UNet,
}


def build(model_config, logger=None) -> dict:
    """{key: MODELS[name](**rest)} for every key of ``model_config`` but ``checkpoint_path`` (the engine's business), in the config's
    order: ``{'embedder': ..., 'landmark': ...}`` for configs/default.yml.  The caller's config is not modified.  A name outside
    the registry raises KeyError with the known ones."""
    config = deepcopy(model_config)
    config.pop("checkpoint_path", None)
    model = {}
    for key in config:
        name = config[key].pop("name")
        if name not in MODELS:
            raise KeyError(f"unknown model name {name!r} for {key!r}: the registry holds {', '.join(MODELS)}")
        model[key] = MODELS[name](**config[key])
    if logger is not None and hasattr(logger, "infov"):
        logger.infov("Model is created.")
    return model
