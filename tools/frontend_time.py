"""UNet front-end at 224/7, default dims: torch modules (MIOpen) against the HIP front-end (enable_hip_frontend), on one device.

    python tools/frontend_time.py [batch]            (GPU box; under rocprofv3 --kernel-trace --stats for per-launch times)
    python tools/frontend_time.py train              the training leg: forward + backward of `decoder_maps` at batch 1 and 8

Three interleaved pairs (off, on, off, on, off, on) of `decoder_maps` and of frame -> logits (`model(x=..., edge_index=...)`), each
a host clock around ITERS calls that ends in a device synchronise, after a warm-up of every shape.  Prints one line per pair and
a JSON summary line; exits non-zero if the two routes' maps differ by more than 1e-3 of the map's largest value.

The training leg times forward + backward (loss = the sum of every map) of `decoder_maps` in training mode with
enable_hip_frontend(True, train=False) -- torch modules (MIOpen), what the parent of the training route ran -- against train=True
(frontend_train.hip), again in three interleaved pairs per batch size on one device, and prints one JSON line.  No gate."""
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd.examples import UNetNodeFeatureModel  # noqa: E402
from echoglad_amd.topology import HierTopology, TopologySpec  # noqa: E402

WARMUP, ITERS, PAIRS = 10, 50, 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3          # ms per call


def train_leg():
    assert torch.cuda.is_available(), "frontend_time.py measures on a GPU"
    dev = "cuda:0"
    torch.manual_seed(0)
    model = UNetNodeFeatureModel(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                 num_gnn_layers=3, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                 classifier_dropout_p=0.5).to(dev).train()
    params = list(model.down_convs.parameters()) + list(model.up_convs.parameters())
    result = {"tool": "frontend_time", "leg": "train", "device": torch.cuda.get_device_name(0), "iters": ITERS, "batches": {}}
    for B in (1, 8):
        frames = torch.randn(B, 4, 224, 224, device=dev)

        def step():
            for p in params:
                p.grad = None
            sum(m.sum() for m in model.decoder_maps(frames)).backward()

        ms = {"torch": [], "hip": []}
        for name in ms:                                     # warm-up of both routes
            model.enable_hip_frontend(True, train=name == "hip")
            for _ in range(WARMUP):
                step()
        for pair in range(PAIRS):
            for name in ms:
                model.enable_hip_frontend(True, train=name == "hip")
                ms[name].append(timed(step))
            print(f"train, batch {B}, pair {pair}: forward + backward torch {ms['torch'][-1]:.3f} ms, hip {ms['hip'][-1]:.3f} ms "
                  f"({ms['torch'][-1] / ms['hip'][-1]:.2f}x)", flush=True)
        result["batches"][str(B)] = {"fwd_bwd_ms_torch": ms["torch"], "fwd_bwd_ms_hip": ms["hip"],
                                     "hip_faster_in_every_pair": all(a > b for a, b in zip(ms["torch"], ms["hip"]))}
    print(json.dumps(result))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "train":
        return train_leg()
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    assert torch.cuda.is_available(), "frontend_time.py measures on a GPU"
    dev = "cuda:0"
    torch.manual_seed(0)
    model = UNetNodeFeatureModel(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                                 num_gnn_layers=3, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                                 classifier_dropout_p=0.5).to(dev).eval()
    topo = HierTopology(TopologySpec(224, 7, False, False))
    ei = torch.from_numpy(topo.batched_edge_index(B)).to(dev)
    frames = torch.randn(B, 4, 224, 224, device=dev)
    routes = {"off": False, "on": True}
    front = {k: [] for k in routes}
    e2e = {k: [] for k in routes}
    with torch.no_grad():
        maps = {}
        for name, flag in routes.items():                   # warm-up of both routes, and the two routes' outputs side by side
            model.enable_hip_frontend(flag)
            for _ in range(WARMUP):
                model(x=frames, edge_index=ei)
                maps[name] = [m.clone() for m in model.decoder_maps(frames)]
        worst = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(maps["on"], maps["off"]))
        for pair in range(PAIRS):
            for name, flag in routes.items():
                model.enable_hip_frontend(flag)
                front[name].append(timed(lambda: model.decoder_maps(frames)))
                e2e[name].append(timed(lambda: model(x=frames, edge_index=ei)))
            print(f"pair {pair}: front-end off {front['off'][-1]:.3f} ms, on {front['on'][-1]:.3f} ms "
                  f"({front['off'][-1] / front['on'][-1]:.2f}x); frame->logits off {e2e['off'][-1]:.3f} ms, on {e2e['on'][-1]:.3f} ms", flush=True)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(__file__)).stdout.strip()
    except OSError:
        commit = ""
    print(json.dumps({"tool": "frontend_time", "batch": B, "device": torch.cuda.get_device_name(0), "commit": commit or None,
                      "iters": ITERS, "frontend_ms_off": front["off"], "frontend_ms_on": front["on"],
                      "frame_to_logits_ms_off": e2e["off"], "frame_to_logits_ms_on": e2e["on"],
                      "faster_in_every_pair": all(a > b for a, b in zip(front["off"], front["on"])),
                      "max_relative_map_difference": worst}))
    return 0 if worst <= 1e-3 else 1


if __name__ == "__main__":
    sys.exit(main())
