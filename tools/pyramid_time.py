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
    train    (only with --train, and then alone)  the training route, per block input side 224, 128, 64, 32, 16, 8, 4: every new
             entry point beside what it replaces -- eg_pyramid_conv_fwd against eg_embed_conv_fwd, eg_pyramid_conv_bwd_data against
             eg_conv3x3_bwd_data + eg_embed_res_bwd_input, eg_pyramid_conv_bwd_weight against eg_conv3x3_bwd_weight (batch 1 only: the
             old entry point's workspace is one slice of the whole gradient per 32 x 8 tile; the new one is also timed alone at batch
             8) -- replayed from captured graphs as in `block`; then the whole block forward + backward and the whole pyramid at batch
             1 and 8, ops.pyramid_block_train against CNNResBlock from torch modules (the route training took before), eager and
             replayed.  The outputs of old and new entry points are compared before anything is timed (torch.equal for the forward and
             the data gradient, 1e-4 of the largest entry for the weight gradient, whose order of summation is its own).
Prints one line per figure and a JSON summary line; with a path, appends what it printed to that file.  No gate."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd import ops  # noqa: E402
from echoglad_amd.nn import CNNHierarchicalPatchModel, CNNResBlock  # noqa: E402
from echoglad_amd.ops import embedder as E  # noqa: E402
from echoglad_amd.synthetic import fill_state_dict  # noqa: E402
from echoglad_amd.topology import HierTopology, TopologySpec  # noqa: E402

WARMUP, ITERS, PAIRS, CALLS = 3, 20, 3, 10
ROOF_TF = 157.3
DEV = "cuda:0"
_out = None             # the text file every printed line is appended to, as it is printed


def say(text):
    print(text, flush=True)
    if _out:
        with open(_out, "a") as f:
            f.write(text + "\n")


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


SIDES = ((224, 128), (128, 64), (64, 32), (32, 16), (16, 8), (8, 4), (4, 2))


def _bytes(name, *args):
    return max(int(E.raw(name, *args)), 256)


def train_entry_legs(result):
    """Every new entry point beside what it replaces, device time per call."""
    w, b, _ = block_params(1)
    C = 128
    for B in (1, 8):
        for side, nxt in SIDES:
            g = torch.Generator().manual_seed(side)
            x, dz, ds = (torch.randn(B, C, side, side, generator=g).to(DEV) for _ in range(3))
            new = lambda: torch.empty(B, C, side, side, device=DEV)
            calls = CALLS if B * side * side > 64 * 64 else 4 * CALLS
            tag = f"side {side}, batch {B}"
            legs = {}
            # forward
            z0, z1 = new(), new()
            old_f = lambda: E.call("eg_embed_conv_fwd", x, B, C, side, w, b, C, z0)
            new_f = lambda: E.call("eg_pyramid_conv_fwd", x, B, side, w, b, z1)
            old_f(), new_f()
            assert torch.equal(z0, z1), tag
            legs["conv_fwd"] = windows(f"conv_fwd {tag}", {"mfma": graphed(new_f, calls), "vector": graphed(old_f, calls)})
            # data gradient
            d0, d1 = new(), new()

            def old_d():
                E.call("eg_conv3x3_bwd_data", dz, w, B, C, side, C, side, 0, d0, None, None)
                E.call("eg_embed_res_bwd_input", ds, None, B, C, C, side, d0)
            new_d = lambda: E.call("eg_pyramid_conv_bwd_data", dz, w, ds, B, side, d1)
            old_d(), new_d()
            assert torch.equal(d0, d1), tag
            legs["conv_bwd_data"] = windows(f"conv_bwd_data {tag}", {"new": graphed(new_d, calls), "old": graphed(old_d, calls)})
            # weight gradient
            g1 = torch.empty(C, C, 3, 3, device=DEV)
            ws1 = torch.empty(_bytes("eg_pyramid_train_workspace_bytes", B, side, side), dtype=torch.uint8, device=DEV)
            new_w = lambda: E.call("eg_pyramid_conv_bwd_weight", x, dz, B, side, ws1, g1)
            if B == 1:
                g0 = torch.empty(C, C, 3, 3, device=DEV)
                ws0 = torch.empty(_bytes("eg_frontend_train_workspace_bytes", B, C, C, side), dtype=torch.uint8, device=DEV)
                old_w = lambda: E.call("eg_conv3x3_bwd_weight", x, C, side, None, 0, B, side, dz, C, ws0, g0)
                old_w(), new_w()
                err = float((g0 - g1).abs().max()) / float(g0.abs().max())
                assert err < 1e-4, (tag, err)
                legs["conv_bwd_weight"] = windows(f"conv_bwd_weight {tag} (workspace {ws1.numel() / 2 ** 20:.1f} MiB against "
                                                  f"{ws0.numel() / 2 ** 20:.1f} MiB)", {"mfma": graphed(new_w, calls), "vector": graphed(old_w, calls)})
            else:
                legs["conv_bwd_weight"] = windows(f"conv_bwd_weight {tag} (workspace {ws1.numel() / 2 ** 20:.1f} MiB; the old entry "
                                                  f"point would take {_bytes('eg_frontend_train_workspace_bytes', B, C, C, side) / 2 ** 20:.1f} MiB)",
                                                  {"mfma": graphed(new_w, calls)})
            flop = 2.0 * 9 * C * C * B * side * side
            say("    " + ", ".join(f"{k} {flop / list(v.values())[0]['us'] / 1e6:.1f} TF/s" for k, v in legs.items()) + f" of {ROOF_TF} (new route)")
            for k, v in legs.items():
                keys = list(v)
                if len(keys) == 2:
                    a, p = v[keys[0]], v[keys[1]]
                    v["new_not_slower_beyond_the_spreads"] = a["us"] - p["us"] <= a["spread"] * a["us"] + p["spread"] * p["us"]
            result["train"][f"entries_{side}_b{B}"] = legs


def _torch_block(width, seed):
    torch.manual_seed(seed)
    return CNNResBlock(in_channels=128, padding=1, out_channels=128, kernel_size=3, out_size=width, cnn_dropout_p=0.1).to(DEV).train()


def _chain(blocks, hip):
    """forward + backward of a chain of CNNResBlocks from `frames` (a leaf that asks for its gradient, as behind a trainable embedder)."""
    def run(frames, dout):
        x = frames
        for i, blk in enumerate(blocks):
            if hip:
                x = ops.pyramid_block_train(x, blk.conv.weight, blk.conv.bias, blk.bn, blk.pool.output_size[0], blk.dropout.p, 1000 + i)
            else:
                x = blk(x)
        x.backward(dout)
    return run


def _safely(make, what):
    try:
        return make()
    except Exception as e:                                # a route that cannot be captured is a finding, not the end of the tool
        say(f"    {what}: not measured ({type(e).__name__}: {str(e).splitlines()[0][:160]})")
        torch.cuda.synchronize()
        return None


def train_block_legs(result):
    """The whole block and the whole pyramid, forward + backward, HIP against the torch modules."""
    cases = [(f"block {side} -> {nxt}", [nxt], side) for side, nxt in SIDES] + [("pyramid 224 / 7", [w for _, w in SIDES], 224)]
    for B in (1, 8):
        for name, widths, side in cases:
            blocks = [_torch_block(w, 20 + i) for i, w in enumerate(widths)]
            params = [q for blk in blocks for q in blk.parameters()]
            frames = torch.randn(B, 128, side, side, generator=torch.Generator().manual_seed(side)).to(DEV).requires_grad_()
            dout = torch.randn(B, 128, widths[-1], widths[-1], generator=torch.Generator().manual_seed(7)).to(DEV)

            def step(hip):
                run = _chain(blocks, hip)

                def fn():
                    for q in params + [frames]:
                        q.grad = None
                    run(frames, dout)
                return fn
            e = windows(f"train {name}, batch {B}, eager", {"hip": eager(step(True)), "torch": eager(step(False))})
            runs = {}
            for key, hip in (("hip", True), ("torch", False)):
                side_stream = torch.cuda.Stream()             # (torch.cuda.graph wants its warm-up on a side stream for autograd)
                side_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side_stream):
                    r = _safely(lambda: graphed(step(hip), 1), f"{key} replayed")
                torch.cuda.current_stream().wait_stream(side_stream)
                if r is not None:
                    runs[key] = r
            g = windows(f"train {name}, batch {B}, replayed", runs) if runs else {}
            result["train"][f"{name.replace(' ', '_')}_b{B}"] = {"eager": e, "replayed": g}
            del blocks, params, frames
            torch.cuda.empty_cache()


def main():
    global _out
    assert torch.cuda.is_available(), "pyramid_time.py measures on a GPU"
    argv = [a for a in sys.argv[1:] if a != "--train"]
    _out = argv[0] if argv else None
    result = {"tool": "pyramid_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "calls_per_graph": CALLS, "pairs": PAIRS,
              "block": {}, "pyramid": {}, "model": {}, "train": {}}
    if "--train" in sys.argv[1:]:
        train_entry_legs(result)
        train_block_legs(result)
    else:
        block_legs(result)
        pyramid_legs(result)
        model_legs(result)
    say(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
