"""CNN-pyramid variant (seven CNNResBlock(128 -> 128, kernel 3, adaptive max pool) at 224 / 7 levels): the convolution on the f32-input
matrix instruction (ops.pyramid_block, csrc/pyramid_conv.hip) against the route the parent had for the same bits, the embedder's
vector kernel followed by the pool wrapper (ops.adaptive_max_pool(ops.embed_block(...))), on one device.

    python tools/pyramid_time.py [out.txt]          (GPU box)

Legs:
    block    sides 224, 128, 64, 32, 16, 8, 4 (the inputs of the seven blocks) at batch 1 and 8, `conv` (side_out = side: the convolution launch alone) and `block` (with the
             pool to the next side).  CALLS calls of one route are captured into a HIP graph and the replay is timed with device
             events, so a figure is device time per call without the host between launches; the two routes alternate in PAIRS
             windows of one process.  Reported: the median, the spread (max - min) / median over the windows, and for `conv` the
             rate 2 * 9 * 128 * 128 * batch * side^2 / time against the 157.3 TFLOP/s fp32 roof.  The outputs of the two routes are
             compared with torch.equal before anything is timed.  (eg_pyramid_block_fwd takes the matrix route from side 4 on; the
             threshold in DESIGN 3.6d was set from this leg run on a build with PY_MFMA_MIN_SIDE = 1.)
    pyramid  all seven blocks on frames [B, 128, 224, 224]: eager (a host clock around ITERS calls that ends in a device
             synchronise) and replayed from one captured graph, both routes.
    model    model(x=frames, edge_index=...) of nn.CNNHierarchicalPatchModel at 224 / 7 with enable_hip_graph(): the torch modules
             (MIOpen) against enable_hip_pyramid(), ms per frame.
Prints one line per figure and a JSON summary line; with a path, appends what it printed to that file.  No gate."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd import ops  # noqa: E402
from echoglad_amd.nn import CNNHierarchicalPatchModel  # noqa: E402
from echoglad_amd.synthetic import fill_state_dict  # noqa: E402
from echoglad_amd.topology import HierTopology, TopologySpec  # noqa: E402

WARMUP, ITERS, PAIRS, CALLS = 3, 20, 3, 10
ROOF_TF = 157.3
DEV = "cuda:0"
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def block_params(seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(128, 128, 3, 3, generator=g) / (9 * 128) ** 0.5).to(DEV)
    b = (0.05 * torch.randn(128, generator=g)).to(DEV)
    bn = tuple(t.to(DEV) for t in (0.5 + torch.rand(128, generator=g), 0.3 * torch.randn(128, generator=g),
                                   0.3 * torch.randn(128, generator=g), 0.5 + torch.rand(128, generator=g))) + (1e-5,)
    return w, b, bn


def mfma_route(x, w, b, bn, side_out):
    return ops.pyramid_block(x, w, b, bn, side_out)


def parent_route(x, w, b, bn, side_out):
    y = ops.embed_block(x, w, b, bn)
    return y if side_out == x.shape[2] else ops.adaptive_max_pool(y, side_out)


def graphed(fn, calls):
    """A captured graph of `calls` calls of fn -> a function that replays it and returns device microseconds per call."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    graph.replay()
    torch.cuda.synchronize()

    def run():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        graph.replay()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / calls
    return run


def eager(fn):
    for _ in range(WARMUP):
        fn()

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / ITERS * 1e6
    return run


def windows(name, runs):
    """PAIRS alternating windows of runs = {"mfma": ..., "parent": ...} -> {route: {"us": median, "spread": (max - min) / median}}."""
    us = {k: [] for k in runs}
    for _ in range(PAIRS):
        for k, run in runs.items():
            us[k].append(run())
    out = {k: {"us": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v), "windows": v} for k, v in us.items()}
    keys = list(runs)
    text = ", ".join(f"{k} {out[k]['us']:.1f} us (spread {100 * out[k]['spread']:.1f} %)" for k in keys)
    if len(keys) == 2:
        text += f", {out[keys[1]]['us'] / out[keys[0]]['us']:.2f}x"
    say(f"{name}: {text}")
    return out


def block_legs(result):
    w, b, bn = block_params(1)
    for B in (1, 8):
        for side, nxt in ((224, 128), (128, 64), (64, 32), (32, 16), (16, 8), (8, 4), (4, 2)):
            x = torch.randn(B, 128, side, side, generator=torch.Generator().manual_seed(side)).to(DEV)
            flop = 2.0 * 9 * 128 * 128 * B * side * side
            for leg, side_out in (("conv", side), ("block", nxt)):
                with torch.no_grad():
                    assert torch.equal(mfma_route(x, w, b, bn, side_out), parent_route(x, w, b, bn, side_out)), (B, side, side_out)
                    calls = CALLS if B * side * side > 64 * 64 else 4 * CALLS
                    out = windows(f"{leg} {side} -> {side_out}, batch {B}",
                                  {"mfma": graphed(lambda: mfma_route(x, w, b, bn, side_out), calls),
                                   "parent": graphed(lambda: parent_route(x, w, b, bn, side_out), calls)})
                if leg == "conv":
                    for k in out:
                        out[k]["tflops"] = flop / out[k]["us"] / 1e6
                        out[k]["share_of_fp32_roof"] = out[k]["tflops"] / ROOF_TF
                    say(f"    conv {side}, batch {B}: mfma {out['mfma']['tflops']:.1f} TF/s ({100 * out['mfma']['share_of_fp32_roof']:.0f} % of "
                        f"{ROOF_TF}), parent {out['parent']['tflops']:.1f} TF/s ({100 * out['parent']['share_of_fp32_roof']:.0f} %)")
                a, p = out["mfma"], out["parent"]
                out["mfma_wins_by_more_than_both_spreads"] = p["us"] - a["us"] > a["spread"] * a["us"] + p["spread"] * p["us"]
                result["block"][f"{leg}_{side}_to_{side_out}_b{B}"] = out


def pyramid_legs(result):
    widths = [128, 64, 32, 16, 8, 4, 2]
    blocks = [block_params(10 + i) for i in range(len(widths))]

    def run(route, x):
        for (w, b, bn), width in zip(blocks, widths):
            x = route(x, w, b, bn, width)
        return x

    for B in (1, 8):
        frames = torch.randn(B, 128, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
        with torch.no_grad():
            assert torch.equal(run(mfma_route, frames), run(parent_route, frames))
            e = windows(f"pyramid eager, batch {B}", {"mfma": eager(lambda: run(mfma_route, frames)),
                                                      "parent": eager(lambda: run(parent_route, frames))})
            g = windows(f"pyramid replayed, batch {B}", {"mfma": graphed(lambda: run(mfma_route, frames), 1),
                                                         "parent": graphed(lambda: run(parent_route, frames), 1)})
        result["pyramid"][f"b{B}"] = {"eager": e, "replayed": g}


def model_legs(result):
    frame, naux = 224, 7
    model = CNNHierarchicalPatchModel(frame_size=frame, num_aux_graphs=naux, node_embedding_dim=128, node_hidden_dim=128,
                                      classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit")
    fill_state_dict(model, 5)
    model = model.to(DEV).eval().enable_hip_graph()
    topo = HierTopology(TopologySpec(frame, naux, False, False))
    for B in (1, 8):
        ei = torch.from_numpy(topo.batched_edge_index(B).copy()).to(DEV)
        frames = (0.5 * torch.randn(B, 128, frame, frame, generator=torch.Generator().manual_seed(4))).to(DEV)

        def forward(hip):
            model.enable_hip_pyramid(hip)
            with torch.no_grad():
                return model(x=frames, edge_index=ei)[0]

        out = windows(f"model(x=frames) {frame} / {naux}, batch {B}", {"hip_pyramid": eager(lambda: forward(True)),
                                                                       "torch_pyramid": eager(lambda: forward(False))})
        for k in out:
            out[k]["ms_per_frame"] = out[k]["us"] / B / 1e3
        say(f"    per frame: hip pyramid {out['hip_pyramid']['ms_per_frame']:.3f} ms, torch pyramid {out['torch_pyramid']['ms_per_frame']:.3f} ms")
        result["model"][f"b{B}"] = out


def main():
    assert torch.cuda.is_available(), "pyramid_time.py measures on a GPU"
    result = {"tool": "pyramid_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "calls_per_graph": CALLS, "pairs": PAIRS,
              "block": {}, "pyramid": {}, "model": {}}
    block_legs(result)
    pyramid_legs(result)
    model_legs(result)
    say(json.dumps(result))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write("\n".join(_lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
