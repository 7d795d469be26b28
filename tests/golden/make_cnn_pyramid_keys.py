#!/usr/bin/env python3
"""Generate tests/golden/cnn_pyramid_state_keys.json: the state_dict keys (in order) and shapes of the reference's
CNNHierarchicalPatchModel (src/core/models.py:556-636), by running the reference's own class the way make_golden.py runs the UNet
variant for unet_state_keys.json.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cnn_pyramid_keys.py

One stand-in: the class wraps its Sequential in torchvision's IntermediateLayerGetter, and torchvision is not installed where
the fixtures are made (make_golden.py stubs the name with `object`, which cannot be constructed with arguments).  `_Getter` below
restates what that class registers, from its documentation: a ModuleDict of the model's children in order, up to and including
the last one named in return_layers.  Everything else that runs is the reference's code; only the key list is written."""
import json
import os
from collections import OrderedDict

import torch.nn as nn

import make_golden as MG            # installs the stubs and imports the reference's modules (nothing is generated on import)

HERE = os.path.dirname(os.path.abspath(__file__))


class _Getter(nn.ModuleDict):
    def __init__(self, model, return_layers):
        wanted = {str(k) for k in return_layers}
        if not wanted.issubset(name for name, _ in model.named_children()):
            raise ValueError("return_layers are not present in model")
        layers = OrderedDict()
        for name, module in model.named_children():
            layers[name] = module
            wanted.discard(name)
            if not wanted:
                break
        super().__init__(layers)


def main():
    MG.RM.IntermediateLayerGetter = _Getter
    m = MG.RM.CNNHierarchicalPatchModel(frame_size=224, gnn_dropout_p=0.5, classifier_dropout_p=0.5, node_embedding_dim=128,
                                        node_hidden_dim=128, num_output_channels=4, num_gnn_layers=3, num_aux_graphs=7,
                                        gnn_jk_mode="last", classifier_hidden_dim=32, residual=True, use_coordinate_graph=True,
                                        output_activation="logit", use_connection_nodes=False, use_main_graph_only=False)
    state = m.state_dict()
    json.dump({"n_parameters": int(sum(p.numel() for p in m.parameters())), "keys": list(state),
               "state_dict": {k: list(v.shape) for k, v in state.items()}},
              open(os.path.join(HERE, "cnn_pyramid_state_keys.json"), "w"), indent=0, sort_keys=True)
    print("cnn pyramid keys", len(state))


if __name__ == "__main__":
    main()
