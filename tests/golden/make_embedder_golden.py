#!/usr/bin/env python3
"""Generate tests/golden/cnn_embedder.npz by RUNNING THE REFERENCE'S OWN ``CNN`` (src/core/models.py:155-260) on the CPU.

    PYTHONDONTWRITEBYTECODE=1 ECHOGLAD_REFERENCE=<the reference tree> python tests/golden/make_embedder_golden.py

The reference tree is imported read-only with its missing third-party modules stubbed.  Only DATA is written: for
each of the two models below, the state_dict's key list, seeded parameters with non-trivial running statistics, a [2, 1, 12, 12]
input, the eval-mode output, and -- with cnn_dropout_p = 0, in training mode -- the output, every parameter's gradient for a seeded
dout and the running statistics afterwards.

    <model>/keys                  the state_dict's keys, in order (one string array)
    <model>/state/<key>           the state_dict that was loaded
    <model>/x, eval_out, train_out, dout
    <model>/grad/<parameter>      d sum(train_out * dout) / d parameter
    <model>/after/<key>           running_mean, running_var, num_batches_tracked after the training-mode forward
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np

# name -> constructor arguments (cnn_dropout_p as the default configuration has it; the training-mode run sets it to 0)
MODELS = {
    "default": dict(out_channels=[4], kernel_sizes=[3], pool_sizes=[1], cnn_dropout_p=0.1),
    "c884": dict(out_channels=[8, 8, 4]),
}
SEED = 20231


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    for name in ("torch_geometric", "torchvision", "torchvision.models", "torchsummary"):
        if name not in sys.modules:
            mod(name)
    mod("torch_geometric.nn", GCNConv=None, Sequential=None, global_add_pool=None, JumpingKnowledge=None)
    mod("torchvision.models._utils", IntermediateLayerGetter=None)
    sys.modules["torchsummary"].summary = None
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        mod("matplotlib")
        mod("matplotlib.pyplot", new_figure_manager=None)


def seeded_state(model, gen):
    """Parameters N(0, 1) scaled by their fan-in, BatchNorm weights of both signs, running statistics away from (0, 1)."""
    import torch
    state = {}
    for key, t in model.state_dict().items():
        if key.endswith("num_batches_tracked"):
            state[key] = torch.tensor(3, dtype=t.dtype)
        elif key.endswith("running_var"):
            state[key] = 0.5 + torch.rand(t.shape, generator=gen)
        elif key.endswith("running_mean"):
            state[key] = 0.3 * torch.randn(t.shape, generator=gen)
        elif key.endswith("bn.weight"):
            sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(t.numel())])
            state[key] = sign * (0.5 + torch.rand(t.shape, generator=gen))
        elif key.endswith("bn.bias"):
            state[key] = 0.3 * torch.randn(t.shape, generator=gen)
        elif key.endswith(".bias"):
            state[key] = 0.05 * torch.randn(t.shape, generator=gen)
        else:
            fan_in = t[0].numel()
            state[key] = torch.randn(t.shape, generator=gen) / fan_in ** 0.5
    return state


def main():
    import torch
    ref = os.environ.get("ECHOGLAD_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set ECHOGLAD_REFERENCE (or pass as the first argument) to the reference tree")
    _install_stubs()
    sys.path.insert(0, ref)
    from src.core.models import CNN          # reference code, executed not copied
    torch.set_num_threads(1)
    out = {}
    for i, (name, kwargs) in enumerate(MODELS.items()):
        gen = torch.Generator().manual_seed(SEED + i)
        model = CNN(**kwargs)
        state = seeded_state(model, gen)
        model.load_state_dict(state, strict=True)
        out[f"{name}/keys"] = np.array(list(model.state_dict().keys()))
        for key, t in state.items():
            out[f"{name}/state/{key}"] = t.numpy().copy()
        x = torch.randn(2, 1, 12, 12, generator=gen)
        out[f"{name}/x"] = x.numpy().copy()
        model.eval()
        with torch.no_grad():
            out[f"{name}/eval_out"] = model(x).numpy().copy()
        train = CNN(**dict(kwargs, cnn_dropout_p=0.0))
        train.load_state_dict(state, strict=True)
        train.train()
        y = train(x)
        dout = torch.randn(y.shape, generator=gen)
        (y * dout).sum().backward()
        out[f"{name}/train_out"] = y.detach().numpy().copy()
        out[f"{name}/dout"] = dout.numpy().copy()
        for key, p in train.named_parameters():
            out[f"{name}/grad/{key}"] = p.grad.numpy().copy()
        for key, t in train.state_dict().items():
            if "running_" in key or key.endswith("num_batches_tracked"):
                out[f"{name}/after/{key}"] = t.numpy().copy()
    path = os.path.join(HERE, "cnn_embedder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
