"""Frame preparation on one device: ops.frame_prep (frame_prep.hip, one launch) against the torch-on-device composition of the same
stages (.float() / 255, affine_grid, the two index swaps and bmm, grid_sample, interpolate, flip).

    python tools/frame_prep_time.py [out.txt]        (GPU box)
    python tools/frame_prep_time.py step [out.txt]   the graphed batch-1 training step fed raw batches against prepared ones

Kernel legs: 640 -> 608 -> 224 with C = 3 at batch 1, 8 and 32, and 224 -> 224 resize-only with C = 1 at batch 1 and 32.  Every leg
is timed with a pair of device events around as many calls as fill a window of at least 0.5 s (sized from a probe after the warm-up);
the two routes alternate (hip, torch, hip, torch, hip, torch) and the spread over a route's three windows is printed beside its
median.  The two routes' outputs are compared first: the tool exits non-zero if they differ by more than 1e-3.

Step leg: engine.GraphedTrainStep at 224/7, batch 1, coordinate graph, a 1x1-convolution embedder.  "raw": every step copies a uint8
640 x 640 x 3 frame, eight numbers and two matrices into the static batch and replays a graph whose first two nodes are
data.device_frames_ and data.device_labels_.  "prepared": every step copies a float 224 x 224 frame and the prepared landmark
integers and replays the graph without the preparation node -- the step as it was before raw frames existed.  Host clock around
the copies and replays, ending in a device synchronise; the routes alternate; three windows of at least 0.5 s each.

Prints one line per window and one JSON line; with a file argument the same text is written there as well."""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for sub in ("tests", os.path.join("tests", "golden")):             # gpu_util.model_pair and what it imports
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from echoglad_amd import data, engine, losses, ops  # noqa: E402

WARMUP, PAIRS, WINDOW_S = 20, 3, 0.5
DEV = "cuda:0"
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def torch_route(src, inv, W, F, flip):
    """The stages as torch operators on the device, the way the reference's transform_image drives them."""
    x = src.float() / 255
    B = x.shape[0]
    if W > 0:
        eye = torch.tensor([[[1, 0, 0], [0, 1, 0]]], dtype=torch.float32, device=x.device).expand(B, 2, 3)
        grid = torch.nn.functional.affine_grid(eye, [B, 1, W, W], align_corners=False).reshape(B, W * W, 2)
        grid = grid[..., [1, 0]]
        grid = grid.bmm(inv[:, :, :2].transpose(1, 2)) + inv[:, :, 2].unsqueeze(1)
        grid = grid[..., [1, 0]].reshape(B, W, W, 2)
        x = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    x = torch.nn.functional.interpolate(x, size=(F, F), mode="bilinear", align_corners=False)
    return torch.where(flip.bool().view(B, 1, 1, 1), x.flip(-1), x)


def event_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3                   # microseconds per call


def calls_for(fn):
    for _ in range(WARMUP):
        fn()
    probe = event_window(fn, 20)
    return max(20, int(WINDOW_S * 1e6 / max(probe, 1.0)) + 1)


def kernel_legs():
    result = {"tool": "frame_prep_time", "leg": "kernel", "device": torch.cuda.get_device_name(0), "window_s": WINDOW_S, "shapes": {}}
    worst = 0.0
    for S, W, F, C, B in ((640, 608, 224, 3, 1), (640, 608, 224, 3, 8), (640, 608, 224, 3, 32), (224, 0, 224, 1, 1), (224, 0, 224, 1, 32)):
        g = torch.Generator(device="cpu").manual_seed(S + B)
        src = torch.randint(0, 256, (B, C, S, S), dtype=torch.uint8, generator=g).to(DEV)
        flip = (torch.arange(B) % 2).to(torch.uint8).to(DEV)
        inv = None
        if W > 0:
            pairs = [data.affine_matrix(tx=0.01 * (b % 3), ty=-0.01 * (b % 2), sx=S / W, sy=S / W, rotation_theta=0.05 * (b % 5),
                                        shear_theta=0.02 * (b % 4)) for b in range(B)]
            inv = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
        out = torch.empty(B, C, F, F, device=DEV)
        hip = lambda: ops.frame_prep(src, out, matrix_inv=inv, warp_size=W, flip=flip)
        ref = lambda: torch_route(src, inv, W, F, flip)
        diff = float((hip() - ref()).abs().max())
        worst = max(worst, diff)
        n = {"hip": calls_for(hip), "torch": calls_for(ref)}
        us = {"hip": [], "torch": []}
        name = f"{S}->{W or S}->{F} C={C} B={B}"
        for pair in range(PAIRS):
            for route, fn in (("hip", hip), ("torch", ref)):
                us[route].append(event_window(fn, n[route]))
            say(f"{name}, window {pair}: hip {us['hip'][-1]:.2f} us ({n['hip']} calls), torch {us['torch'][-1]:.2f} us ({n['torch']} calls), "
                f"{us['torch'][-1] / us['hip'][-1]:.2f}x")
        med = {k: sorted(v)[1] for k, v in us.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in us.items()}
        say(f"{name}: hip median {med['hip']:.2f} us (spread {100 * spread['hip']:.1f} %), torch median {med['torch']:.2f} us "
            f"(spread {100 * spread['torch']:.1f} %), max |hip - torch| = {diff:.3g}")
        result["shapes"][name] = {"us_hip": us["hip"], "us_torch": us["torch"], "max_abs_difference": diff}
    say(json.dumps(result))
    return 0 if worst <= 1e-3 else 1


def step_leg():
    from gpu_util import model_pair
    frame, naux, B, n_batches = 224, 7, 1, 8
    result = {"tool": "frame_prep_time", "leg": "step", "device": torch.cuda.get_device_name(0), "window_s": WINDOW_S}
    np.random.seed(3)
    torch.manual_seed(3)
    ds = data.SyntheticEchoDataset(num_aux_graphs=naux, frame_size=frame, use_coordinate_graph=True, labels="coords", frames="raw",
                                   crop_size=640, warp_size=608, flip_p=0.5, make_gray=True,
                                   augment={"rotation": (-0.1, 0.1), "shear": (-0.05, 0.05), "translation": (-0.02, 0.02)})
    raw = [data.collate([ds[i]], ds.topology) for i in range(n_batches)]
    prepared = []
    for hb in raw:                                           # what a host-side preparation would hand over: x, integers
        d = data.device_frames_(data.to_device(copy.copy(hb), DEV))
        p = copy.copy(hb)
        for k in [k for k in vars(p) if k.startswith(("raw_", "prep_"))]:
            delattr(p, k)
        p.x, p.label_coords, p.node_coord_y = d.x.cpu(), d.label_coords.cpu(), d.node_coord_y.cpu()
        prepared.append(p)
    crit = losses.build({"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
                         "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": frame, "num_aux_graphs": naux, "batch_size": B,
                         "use_coordinate_graph": True, "use_main_graph_only": False, "num_output_channels": 4})
    runs = {}
    for route, host in (("raw", raw), ("prepared", prepared)):
        hip, _ = model_pair(frame, naux, 3, coord=True, seed=5)
        hip.train()
        torch.manual_seed(5)
        emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(DEV)
        for q in emb.parameters():
            q.requires_grad_(False)
        model = {"embedder": emb, "landmark": hip}
        opt = torch.optim.Adam(list(hip.parameters()), lr=1e-4, capturable=True)
        static = data.to_device(copy.copy(host[0]), DEV)
        coords0 = static.node_coords.clone()

        def loss_fn(static=static, model=model, coords0=coords0):
            data.device_frames_(static)
            data.device_labels_(static)
            static.node_coords = coords0.clone()
            preds, cp = engine.forward_batch(model, static, True)
            return engine.total_loss(engine.compute_loss(crit, preds, static.y, cp, static.node_coord_y, static.valid_labels, B))

        step = engine.GraphedTrainStep(loss_fn, opt, warmup=2)
        k = [0]

        def one(static=static, host=host, step=step, k=k):
            data.copy_batch_(static, host[k[0] % n_batches])
            k[0] += 1
            step()

        runs[route] = one

    def host_window(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3      # ms per step

    calls = {}
    for route, fn in runs.items():
        for _ in range(WARMUP):
            fn()
        calls[route] = max(20, int(WINDOW_S * 1e3 / host_window(fn, 20)) + 1)
    ms = {k: [] for k in runs}
    for pair in range(PAIRS):
        for route, fn in runs.items():
            ms[route].append(host_window(fn, calls[route]))
        say(f"step, window {pair}: raw {ms['raw'][-1]:.4f} ms, prepared {ms['prepared'][-1]:.4f} ms ({calls['raw']} / {calls['prepared']} steps)")
    med = {k: sorted(v)[1] for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    say(f"step 224/7 batch 1: raw median {med['raw']:.4f} ms (spread {100 * spread['raw']:.1f} %), prepared median "
        f"{med['prepared']:.4f} ms (spread {100 * spread['prepared']:.1f} %)")
    result.update({"ms_raw": ms["raw"], "ms_prepared": ms["prepared"]})
    say(json.dumps(result))
    return 0


def main():
    assert torch.cuda.is_available(), "frame_prep_time.py measures on a GPU"
    args = sys.argv[1:]
    leg = step_leg if args and args[0] == "step" else kernel_legs
    path = next((a for a in args if a != "step"), None)
    rc = leg()
    if path:
        with open(path, "a") as f:
            f.write("\n".join(_lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
