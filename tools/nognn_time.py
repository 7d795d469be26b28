"""The no-GNN baselines at 224/7, default dims: the fused tail + heads launch (ops.conv1x1_relu_heads) against the two launches it
replaces (ops.conv1x1_relu_pack_levels, ops.classifier_fwd) on the same decoder maps, on one device.

    python tools/nognn_time.py            (GPU box; under rocprofv3 --kernel-trace --stats for per-launch times)

Per batch size (1 and 8): a warm-up of each leg, then PAIRS interleaved pairs (two, fused, two, fused, ...) inside this one process.
A leg's figure is the mean over ITERS calls of the time between a device event recorded in front of the call and one recorded behind
it -- for the two-launch leg that spans both launches and the gap between them, which is what the composed route costs a caller.
Then the whole eager eval forward of examples.UNetNoGNN (frames -> logits, torch decoder) with fuse_tail off and on, a host clock
around ITERS calls that ends in a device synchronise, in the same interleaved pairs.  Prints one line per pair and a JSON summary line
whose `fused_faster_in_every_pair` is what the `fuse_tail` default follows; exits non-zero if the two routes' logits differ in a bit."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd import ops  # noqa: E402
from echoglad_amd.examples import UNetNoGNN  # noqa: E402

WARMUP, ITERS, PAIRS = 10, 50, 3
BATCHES = (1, 8)


def device_ms(fn):
    """Mean device time of one call: an event pair around each of ITERS calls."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    torch.cuda.synchronize()
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / ITERS


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3


def spread(v):
    return max(v) - min(v)


def main():
    assert torch.cuda.is_available(), "nognn_time.py measures on a GPU"
    dev = "cuda:0"
    torch.manual_seed(0)
    model = UNetNoGNN(frame_size=224, num_aux_graphs=7, node_embedding_dim=128, node_hidden_dim=128, classifier_hidden_dim=32,
                      num_gnn_layers=3, output_activation="logit", use_coordinate_graph=False, gnn_dropout_p=0.5,
                      classifier_dropout_p=0.5).to(dev).eval()
    ws, bs = [m.weight.detach() for m in model.linears], [m.bias.detach() for m in model.linears]
    packed = model._packed_classifier()
    n = model._row_ranges()[2]
    result = {"tool": "nognn_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "pairs": PAIRS, "batches": {}}
    same = True
    with torch.no_grad():
        for B in BATCHES:
            frames = torch.randn(B, 4, 224, 224, device=dev)
            maps = [m.contiguous() for m in model.decoder_maps(frames)]
            legs = {"two": lambda: ops.classifier_fwd(ops.conv1x1_relu_pack_levels(maps, ws, bs, B, n), B, n, 0, n, packed),
                    "fused": lambda: ops.conv1x1_relu_heads(maps, ws, bs, B, packed)}
            same = same and torch.equal(legs["two"](), legs["fused"]())
            ms = {k: [] for k in legs}
            e2e = {"off": [], "on": []}
            for fn in legs.values():
                for _ in range(WARMUP):
                    fn()
            for flag in (False, True):
                model.fuse_tail = flag
                for _ in range(WARMUP):
                    model(x=frames)
            for pair in range(PAIRS):
                for name, fn in legs.items():
                    ms[name].append(device_ms(fn))
                for name, flag in (("off", False), ("on", True)):
                    model.fuse_tail = flag
                    e2e[name].append(host_ms(lambda: model(x=frames)))
                print(f"batch {B}, pair {pair}: two launches {ms['two'][-1]:.4f} ms, fused {ms['fused'][-1]:.4f} ms "
                      f"({ms['two'][-1] / ms['fused'][-1]:.2f}x); frames -> logits fuse_tail off {e2e['off'][-1]:.3f} ms, on {e2e['on'][-1]:.3f} ms",
                      flush=True)
            diffs = [a - b for a, b in zip(ms["two"], ms["fused"])]
            result["batches"][str(B)] = {"two_launches_ms": ms["two"], "fused_ms": ms["fused"], "difference_ms": diffs,
                                         "spread_two_ms": spread(ms["two"]), "spread_fused_ms": spread(ms["fused"]),
                                         "frames_to_logits_ms_fuse_tail_off": e2e["off"], "frames_to_logits_ms_fuse_tail_on": e2e["on"],
                                         "fused_faster_in_every_pair": all(d > 0 for d in diffs)}
    result["fused_faster_in_every_pair"] = all(b["fused_faster_in_every_pair"] for b in result["batches"].values())
    result["logits_bit_equal"] = same
    print(json.dumps(result))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
