"""Connection-node features of the UNet model behind its decoder, default dims (channels 512 .. 4 on sides 2 .. 128 and 224, 7 aux
levels, 8 connection rows per frame), at batch 1 and 8: the route of `enable_hip_conn_rows()` (means over the packed node rows in
HIP, inside the packing node) against the switch-off route (every level's relu(conv1x1) once more through torch, its mean, an
indexed assignment into the node array -- into a clone of it in training), in one process on one device.

    python tools/conn_rows_time.py            (GPU box)

The decoder's maps are computed once and held fixed (`decoder_maps` returns them), so what is timed is `create_node_pixels` behind the
decoder.  Two measurements per batch size:
  eval    `create_node_pixels` in eval mode under torch.no_grad(): off against on.
  train   training mode, forward + backward: `(create_node_pixels(...) * g).sum().backward()` with the maps and the `linears` as
          leaves -- the multiply gives the packing node a gradient buffer of its own, as the GNN stack's backward does; it costs both
          routes the same two passes.  off (torch tail backward) against on (torch tail backward) against on + the HIP tail backward
          (`enable_hip_frontend(tail=True)`, which the switch-off route cannot have).
Per measurement: WARMUP calls of every route, then PAIRS rounds in which the routes alternate; each figure is device time between two
events around ITERS calls, in ms per call.  Prints every round, then min / median / max per route, the largest difference between the
routes' node rows, and one JSON line.  There is no gate: where the new route is slower the table says so.  Reads nothing outside the
repository."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd.examples import UNetNodeFeatureModel  # noqa: E402

WARMUP, ITERS, PAIRS = 5, 20, 5
FRAME, NAUX = 224, 7


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(ITERS):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / ITERS          # ms per call


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def compare(title, routes):
    """routes: name -> callable.  Alternating rounds after a warm-up of each -> name -> list of ms per call."""
    for fn in routes.values():
        for _ in range(WARMUP):
            fn()
    ms = {name: [] for name in routes}
    for rnd in range(PAIRS):
        for name, fn in routes.items():
            ms[name].append(timed(fn))
        print(f"{title}, round {rnd}: " + ", ".join(f"{name} {v[-1]:.3f} ms" for name, v in ms.items()), flush=True)
    for name, v in ms.items():
        s = spread(v)
        print(f"{title}: {name:14s} min {s['min']:.3f}  median {s['median']:.3f}  max {s['max']:.3f} ms", flush=True)
    return ms


def main():
    assert torch.cuda.is_available(), "conn_rows_time.py measures on a GPU"
    dev = "cuda:0"
    result = {"tool": "conn_rows_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "pairs": PAIRS, "batches": {}}
    for B in (1, 8):
        torch.manual_seed(B)
        model = UNetNodeFeatureModel(frame_size=FRAME, num_aux_graphs=NAUX, node_embedding_dim=128, node_hidden_dim=128,
                                     classifier_hidden_dim=32, num_gnn_layers=3, output_activation="logit",
                                     use_connection_nodes=True).to(dev).eval().enable_hip_frontend(True)
        frames = torch.randn(B, 4, FRAME, FRAME, device=dev)
        with torch.no_grad():
            maps = [m.clone() for m in model.decoder_maps(frames)]
        model.decoder_maps = lambda _frames: maps                      # held fixed: what is timed lies behind the decoder

        def eval_route(flag):
            def run():
                with torch.no_grad():
                    return model.enable_hip_conn_rows(flag).create_node_pixels(frames, B)
            return run
        off, on = eval_route(False)(), eval_route(True)()
        n_conn = NAUX + 1
        rows_equal = bool(torch.equal(off.view(B, -1, 128)[:, n_conn:], on.view(B, -1, 128)[:, n_conn:]))
        conn_diff = float((off - on).view(B, -1, 128)[:, :n_conn].abs().max()) / float(off.view(B, -1, 128)[:, :n_conn].abs().max())
        print(f"batch {B}: rows behind the connection rows bit-equal: {rows_equal}; connection rows differ by {conn_diff:.2e} of the largest", flush=True)
        ms_eval = compare(f"batch {B} eval create_node_pixels", {"off": eval_route(False), "on": eval_route(True)})

        model.train()
        leaves = [m.clone().requires_grad_(True) for m in maps]
        model.decoder_maps = lambda _frames: leaves
        g = torch.randn(off.shape[0], 128, device=dev)
        params = leaves + list(model.linears.parameters())

        def train_route(flag, tail):
            def run():
                for q in params:
                    q.grad = None
                model.enable_hip_frontend(True, train=True, tail=False)
                model.enable_hip_conn_rows(flag).enable_hip_frontend(True, train=True, tail=tail)
                (model.create_node_pixels(frames, B) * g).sum().backward()
            return run
        ms_train = compare(f"batch {B} train forward + backward", {"off": train_route(False, False), "on": train_route(True, False),
                                                                 "on + hip tail": train_route(True, True)})
        result["batches"][str(B)] = {"rows_bit_equal": rows_equal, "connection_rows_relative_difference": conn_diff,
                                     "eval_ms": {k: spread(v) for k, v in ms_eval.items()}, "eval_ms_rounds": ms_eval,
                                     "train_ms": {k: spread(v) for k, v in ms_train.items()}, "train_ms_rounds": ms_train}
        del model, maps, leaves, off, on, g
        torch.cuda.empty_cache()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
