"""The optimizer update on the parameter set of the default landmark model (224 / 7 levels, coordinate graph: 82 tensors, 330 KB):
the one-launch SGD / RMSprop / Adam of echoglad_amd.optim against torch's own classes, and the batch-1 captured training step
(engine.GraphedTrainStep) with each of the three.

    python tools/optim_time.py            (GPU box; under rocprofv3 --kernel-trace --stats for per-launch times)

Per leg: a warm-up, then PAIRS rounds over all legs interleaved inside this one process.  A leg's device figure is the mean over ITERS
steps of the time between a device event recorded in front of ``step()`` and one behind it (for torch's foreach routes that spans
every launch of the chain and the gaps between them -- what the route costs a stream); its host figure is a host clock around ITERS
steps that ends in a device synchronise.  Then the replay time of the whole captured batch-1 step with each one-launch optimizer
(tensor lr).  With ``--launches``: the device kernels of one step of every leg as torch.profiler counts them, after everything else
(None when the profiler is not available).  Prints one line per leg and a JSON summary line whose ``torch_faster_anywhere`` names the
legs where a torch route had the lower device time in every round."""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from echoglad_amd import data, engine, losses, optim  # noqa: E402

WARMUP, ITERS, PAIRS = 10, 50, 3
FRAME, NAUX = 224, 7


def device_ms(fn):
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    torch.cuda.synchronize()
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / ITERS


def host_ms(fn, n=ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def launches_of(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name and "Memset" not in e.name)
    except Exception:                                     # noqa: BLE001  (a diagnostic: the timings do not depend on it)
        return None


def main():
    assert torch.cuda.is_available(), "optim_time.py measures on a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(bench.model_kwargs(FRAME, NAUX, 3, coord=True), dev, train=True)
    shapes = [tuple(p.shape) for p in model.parameters()]

    def fresh():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.1) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-3
        return ps

    legs = {
        "sgd: one launch": lambda ps: optim.SGD(ps, lr=1e-4, momentum=0.9),
        "sgd: torch foreach": lambda ps: torch.optim.SGD(ps, lr=1e-4, momentum=0.9, foreach=True),
        "rmsprop: one launch": lambda ps: optim.RMSprop(ps, lr=1e-4),
        "rmsprop: torch foreach": lambda ps: torch.optim.RMSprop(ps, lr=1e-4, foreach=True),
        "rmsprop: torch foreach capturable": lambda ps: torch.optim.RMSprop(ps, lr=1e-4, foreach=True, capturable=True),
        "adam: one launch": lambda ps: optim.Adam(ps, lr=1e-4),
        "adam: torch fused capturable": lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True, capturable=True),
    }
    opts = {name: make(fresh()) for name, make in legs.items()}
    for o in opts.values():
        for _ in range(WARMUP):
            o.step()
    result = {"tool": "optim_time", "device": torch.cuda.get_device_name(0), "tensors": len(shapes),
              "elements": int(sum(torch.Size(s).numel() for s in shapes)), "iters": ITERS, "pairs": PAIRS, "legs": {}}
    ms = {name: {"device_ms": [], "host_ms": []} for name in opts}
    for _ in range(PAIRS):
        for name, o in opts.items():
            ms[name]["device_ms"].append(device_ms(o.step))
            ms[name]["host_ms"].append(host_ms(o.step))
    for name, o in opts.items():
        result["legs"][name] = dict(ms[name])
        print(f"{name}: device {min(ms[name]['device_ms']):.4f} - {max(ms[name]['device_ms']):.4f} ms, host {min(ms[name]['host_ms']):.4f} - "
              f"{max(ms[name]['host_ms']):.4f} ms per step", flush=True)
    slower = []
    for algo in ("sgd", "rmsprop", "adam"):
        ours = ms[f"{algo}: one launch"]["device_ms"]
        for name in opts:
            if name.startswith(algo + ": torch") and all(t < o for t, o in zip(ms[name]["device_ms"], ours)):
                slower.append(name)
    result["torch_faster_anywhere"] = slower

    # the whole batch-1 training step as one HIP graph, with each one-launch optimizer (fresh model each: the steps train it)
    B = 1
    ds = data.SyntheticEchoDataset(num_aux_graphs=NAUX, frame_size=FRAME, use_coordinate_graph=True)
    host = data.collate([ds[0]], ds.topology)
    crit = {"bce": losses.WeightedBCEWithLogitsLoss("none", 9000, 1), "elm": losses.ExpectedLandmarkMSE(10, B, FRAME, NAUX),
            "coordinate": engine.MSE(1)}
    result["graphed_step_ms"] = {}
    for name, cfg in (("sgd", {"name": "sgd", "lr": 1e-4, "momentum": 0.9}), ("rmsprop", {"name": "rmsprop", "lr": 1e-4}),
                      ("adam", {"name": "adam", "lr": 1e-4})):
        md = {"embedder": torch.nn.Conv2d(1, 128, kernel_size=1).to(dev),
              "landmark": bench.build_model(bench.model_kwargs(FRAME, NAUX, 3, coord=True), dev, train=True)}
        static = data.to_device(copy.copy(host), dev)
        coords0 = static.node_coords.clone()
        opt = optim.build(cfg, md, device_lr=True)

        def loss_fn():
            static.node_coords = coords0.clone()
            preds, cp = engine.forward_batch(md, static, True)
            return engine.total_loss(engine.compute_loss(crit, preds, static.y, cp, static.node_coord_y, static.valid_labels, B))
        step = engine.GraphedTrainStep(loss_fn, opt, warmup=2)
        for _ in range(WARMUP):
            step()
        times = [host_ms(step) for _ in range(PAIRS)]
        result["graphed_step_ms"][name] = times
        print(f"GraphedTrainStep, batch 1, {name}: {min(times):.4f} - {max(times):.4f} ms per replay", flush=True)
    if "--launches" in sys.argv:
        print(json.dumps(result), flush=True)            # (the timings stand whatever the profiler does)
        for name, o in opts.items():
            result["legs"][name]["launches"] = launches_of(o.step)
            print(f"{name}: {result['legs'][name]['launches']} launches per step", flush=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
