#!/usr/bin/env python3
"""Per-batch time of one evaluation step: eager ``engine.eval_step`` with the host-mode landmark evaluator, eager with
the device-history mode, and ``engine.GraphedEvalStep`` -- configs[1] shape (224 x 224 frames, 7 auxiliary levels, 3 layers) at
batch 1 and 8 and a coordinate-graph model at batch 1, the default config's criteria and both evaluation standards.

    python tools/eval_step_time.py [--steps 50] [--warmup 10] [--repeats 3]

Every variant reads a new batch the same way (``data.copy_batch_`` into one static device batch).  Device events around ``steps``
calls after ``warmup`` calls; the variants are interleaved, ``repeats`` rounds on one device.  One JSON line per (case, variant), then
a markdown table of the medians."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from echoglad_amd import data, engine, evaluators, losses  # noqa: E402
from echoglad_amd import nn as egnn  # noqa: E402

CASES = [("224/7 heat map, batch 1", False, 1), ("224/7 heat map, batch 8", False, 8), ("224/7 coordinate graph, batch 1", True, 1)]
FRAME, NAUX, LAYERS = 224, 7, 3


def setup(coord, B, n_batches, dev):
    torch.manual_seed(0)
    lm = egnn.HierarchicalPatchModel(frame_size=FRAME, gnn_dropout_p=0.5, classifier_dropout_p=0.5, node_embedding_dim=128,
                                     node_hidden_dim=128, num_output_channels=4, num_gnn_layers=LAYERS, num_aux_graphs=NAUX,
                                     classifier_hidden_dim=32, use_coordinate_graph=coord, output_activation="logit").to(dev).eval()
    emb = torch.nn.Conv2d(1, 128, kernel_size=1).to(dev).eval()
    np.random.seed(0)
    ds = data.SyntheticEchoDataset(num_aux_graphs=NAUX, frame_size=FRAME, use_coordinate_graph=coord)
    host = [data.collate([ds[B * i + j] for j in range(B)], ds.topology) for i in range(n_batches)]
    crit = losses.build({"WeightedBceWithLogits": {"loss_weight": 1, "reduction": "none", "ones_weight": 9000},
                         "ExpectedLandmarkMse": {"loss_weight": 10}, "frame_size": FRAME, "num_aux_graphs": NAUX, "batch_size": B,
                         "use_coordinate_graph": coord, "use_main_graph_only": False, "num_output_channels": 4})
    return {"embedder": emb, "landmark": lm}, host, crit


def make_evaluators(B, coord, max_updates):
    return evaluators.build({"standards": ["balancedaccuracy", "landmarkcoorderror"], "batch_size": B, "frame_size": FRAME,
                             "use_coordinate_graph": coord}, max_updates=max_updates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n_batches = 4
    table = []
    for name, coord, B in CASES:
        model, host, crit = setup(coord, B, n_batches, dev)
        static = data.to_device(copy.copy(host[0]), dev)
        cap = args.steps + args.warmup + 8
        ev_host = make_evaluators(B, coord, None)
        ev_dev = make_evaluators(B, coord, cap)
        ev_graph = make_evaluators(B, coord, cap)
        step = engine.GraphedEvalStep(model, static, crit, B, use_coordinate_graph=coord, evaluators=ev_graph)

        def eager(evs):
            def run(i):
                data.copy_batch_(static, host[i % n_batches])
                engine.eval_step(model, static, crit, B, coord, evs)
            return run

        def graphed(i):
            data.copy_batch_(static, host[i % n_batches])
            step()
        variants = [("eager, host evaluator", eager(ev_host), ev_host), ("eager, device evaluator", eager(ev_dev), ev_dev),
                    ("GraphedEvalStep", graphed, ev_graph)]
        times = {v[0]: [] for v in variants}
        for _ in range(args.repeats):
            for vname, run, evs in variants:
                for ev in evs.values():
                    ev.reset()
                for i in range(args.warmup):
                    run(i)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for i in range(args.steps):
                    run(i)
                t1.record()
                t1.synchronize()
                times[vname].append(t0.elapsed_time(t1) * 1000.0 / args.steps)
        assert step.captures == 1, step.captures
        for vname, ts in times.items():
            rec = {"case": name, "variant": vname, "us_per_batch": ts, "median_us": statistics.median(ts)}
            print(json.dumps(rec), flush=True)
            table.append(rec)
    print("\n| case | variant | median us / batch | repeats |\n|---|---|---|---|")
    for r in table:
        print(f"| {r['case']} | {r['variant']} | {r['median_us']:.0f} | {', '.join(f'{t:.0f}' for t in r['us_per_batch'])} |")


if __name__ == "__main__":
    main()
