"""Backward of the UNet tail alone (relu(conv1x1) of every level + node packing), default dims -- channels 512 .. 4 on sides 2 .. 128
and 224 -- at batch 1 and 8: the torch route (eg_unpack_levels + torch's relu / conv2d gradients per level, MIOpen) against the HIP
route (eg_conv1x1_relu_pack_bwd), in one process on one device.

    python tools/tail_time.py            (GPU box; under rocprofv3 --kernel-trace --stats for per-launch times)

Per batch size: the forward is run once per route outside the timed window, then PAIRS interleaved pairs (torch, hip, torch, hip, ..)
of a host clock around ITERS backward calls (torch.autograd.grad with retain_graph) that ends in a device synchronise, after WARMUP
calls of each route.  Prints one line per pair, the largest difference between the two routes' gradients, and one JSON line with the
min and the median per route.  (The HIP route is two launches by construction: products, then the sum over slices.  Launch counts
per route come from the rocprofv3 kernel trace; a node count of a captured backward is not printed.)  Exits non-zero if the gradients differ by more than 1e-4 of their largest entry or if the HIP route
is more than 5 % slower than the torch route (by the medians) at either batch size.  Reads nothing outside the repository."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from echoglad_amd import ops  # noqa: E402

WARMUP, ITERS, PAIRS = 10, 30, 5
SIDES = [2, 4, 8, 16, 32, 64, 128, 224]
CHANS = [512, 256, 128, 64, 32, 16, 8, 4]
C = 128


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e3          # ms per call


def main():
    assert torch.cuda.is_available(), "tail_time.py measures on a GPU"
    dev = "cuda:0"
    result = {"tool": "tail_time", "device": torch.cuda.get_device_name(0), "iters": ITERS, "pairs": PAIRS, "batches": {}}
    ok = True
    for B in (1, 8):
        torch.manual_seed(B)
        n_rows = sum(p * p for p in SIDES)
        feats = [torch.randn(B, c, p, p, device=dev, requires_grad=True) for p, c in zip(SIDES, CHANS)]
        ws = [(torch.randn(C, c, 1, 1, device=dev) / c ** 0.5).requires_grad_(True) for c in CHANS]
        bs = [(0.5 * torch.randn(C, device=dev)).requires_grad_(True) for _ in CHANS]
        g = torch.randn(B * n_rows, C, device=dev)
        ins = feats + ws + bs
        outs = {r: ops.conv1x1_relu_pack_levels(feats, ws, bs, B, n_rows, 0, backward=r) for r in ("torch", "hip")}
        back = {r: (lambda o=o: torch.autograd.grad(o, ins, g, retain_graph=True)) for r, o in outs.items()}
        grads = {r: back[r]() for r in back}
        worst = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(grads["hip"], grads["torch"]))
        for r in back:
            for _ in range(WARMUP):
                back[r]()
        ms = {"torch": [], "hip": []}
        for pair in range(PAIRS):
            for r in ms:
                ms[r].append(timed(back[r]))
            print(f"batch {B}, pair {pair}: backward torch {ms['torch'][-1]:.3f} ms, hip {ms['hip'][-1]:.3f} ms "
                  f"({ms['torch'][-1] / ms['hip'][-1]:.2f}x)", flush=True)
        med = {r: statistics.median(v) for r, v in ms.items()}
        not_slower = med["hip"] <= 1.05 * med["torch"]
        print(f"batch {B}: largest gradient difference {worst:.2e} of the largest entry; median torch {med['torch']:.3f} ms, hip {med['hip']:.3f} ms", flush=True)
        result["batches"][str(B)] = {"bwd_ms_torch": ms["torch"], "bwd_ms_hip": ms["hip"], "min_ms": {r: min(v) for r, v in ms.items()},
                                     "median_ms": med, "torch_over_hip": med["torch"] / med["hip"],
                                     "max_relative_gradient_difference": worst, "hip_not_slower_within_5_percent": not_slower}
        ok = ok and not_slower and worst <= 1e-4
    print(json.dumps(result))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
