"""CNN embedder (1 -> 4 channels at 224, the default configuration): torch modules on the device (MIOpen) against the HIP embedder
(nn.CNN.enable_hip), on one device.

    python tools/embedder_time.py [out.txt]          (GPU box; under rocprofv3 --kernel-trace --stats for per-launch times)

Legs, at batch 1 and 8:
    eval    the forward under torch.no_grad()
    train   forward + backward (loss = the sum of the output), parameter gradients only: the frames ask for none
each as three interleaved pairs (torch, hip, torch, hip, torch, hip), every figure a host clock around ITERS calls that ends in a
device synchronise, after a warm-up of both routes.  The baseline is always the torch-module route.
    step    a replayed engine.GraphedTrainStep of a small pairing (frame 16, 3 aux levels, batch 2, UNetNodeFeatureModel on the HIP
            front-end, two criteria, capturable Adam): the torch embedder FROZEN -- its weight gradient adds with atomics, so a
            step that is to repeat bit for bit has to freeze it -- against the HIP embedder TRAINABLE.
Prints one line per pair and a JSON summary line; with a path, appends what it printed to that file.  No gate."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from echoglad_amd import data, engine, losses  # noqa: E402
from echoglad_amd.examples import UNetNodeFeatureModel  # noqa: E402
from echoglad_amd.nn import CNN  # noqa: E402

WARMUP, ITERS, PAIRS = 10, 50, 3
DEV = "cuda:0"
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def timed(fn, iters=ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3          # ms per call


def pairs(name, fns):
    """Three interleaved pairs of fns = {"torch": ..., "hip": ...} -> {route: [ms, ms, ms]}."""
    ms = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    for pair in range(PAIRS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
        say(f"{name}, pair {pair}: torch {ms['torch'][-1]:.4f} ms, hip {ms['hip'][-1]:.4f} ms ({ms['torch'][-1] / ms['hip'][-1]:.2f}x)")
    return ms


def block_legs(result):
    torch.manual_seed(0)
    model = CNN(out_channels=[4], cnn_dropout_p=0.1).to(DEV)
    params = list(model.parameters())
    for B in (1, 8):
        frames = torch.randn(B, 1, 224, 224, device=DEV)

        def forward(hip):
            model.enable_hip(hip)
            with torch.no_grad():
                model(frames)

        def step(hip):
            model.enable_hip(hip, train=hip)
            for p in params:
                p.grad = None
            model(frames).sum().backward()

        model.eval()
        ev = pairs(f"eval, batch {B}", {"torch": lambda: forward(False), "hip": lambda: forward(True)})
        model.train()
        tr = pairs(f"train, batch {B}", {"torch": lambda: step(False), "hip": lambda: step(True)})
        result["batches"][str(B)] = {"eval_ms_torch": ev["torch"], "eval_ms_hip": ev["hip"], "fwd_bwd_ms_torch": tr["torch"],
                                     "fwd_bwd_ms_hip": tr["hip"],
                                     "hip_faster_in_every_pair": {"eval": all(a > b for a, b in zip(ev["torch"], ev["hip"])),
                                                                  "train": all(a > b for a, b in zip(tr["torch"], tr["hip"]))}}


def step_leg(result):
    B, frame, naux = 2, 16, 3
    crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, frame, naux)}
    steps = {}
    for route in ("torch", "hip"):
        np.random.seed(11)
        torch.manual_seed(11)
        ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame)
        batch = data.to_device(data.collate([ds[i] for i in range(B)], ds.topology), DEV)
        landmark = UNetNodeFeatureModel(encoder_embedding_widths=[8, 4, 2], encoder_embedding_dims=[8, 16, 32], frame_size=frame,
                                        num_aux_graphs=naux, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                        num_gnn_layers=2, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                        classifier_dropout_p=0.5).to(DEV).train().enable_hip_frontend(True, train=True)
        embedder = CNN(out_channels=[4], cnn_dropout_p=0.1).to(DEV).train()
        params = list(landmark.parameters())
        if route == "hip":
            embedder.enable_hip(True, train=True)
            params += list(embedder.parameters())
        else:
            for q in embedder.parameters():
                q.requires_grad_(False)
        opt = torch.optim.Adam(params, lr=1e-4, capturable=True)
        model = {"embedder": embedder, "landmark": landmark}

        def loss_fn(model=model, batch=batch):
            preds, cp = engine.forward_batch(model, batch, False)
            return sum(engine.compute_loss(crit, preds, batch.y, cp, None, batch.valid_labels, B).values())

        steps[route] = engine.GraphedTrainStep(loss_fn, opt, warmup=2)
    ms = pairs(f"replayed step {frame}/{naux}, batch {B}", steps)
    result["step"] = {"ms_torch_embedder_frozen": ms["torch"], "ms_hip_embedder_trainable": ms["hip"],
                      "hip_faster_in_every_pair": all(a > b for a, b in zip(ms["torch"], ms["hip"]))}


def main():
    assert torch.cuda.is_available(), "embedder_time.py measures on a GPU"
    result = {"tool": "embedder_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "batches": {}}
    block_legs(result)
    step_leg(result)
    say(json.dumps(result))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write("\n".join(_lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
