"""The landmark evaluator's overlay images on one device: get_overlays (heatmap_render.hip: one decode pass for (max, sum exp) and one
render launch) against the reference's route to the same three images (src/engine.py:563-580, src/core/evaluators.py:497-616): `.cpu()`
of the whole [B * nodes, 4] logits and labels and of the frames, a host softmax over frame 0's main grid, its per-channel
normalisation, and the overlays as torch operators on the host ending in mul(255).byte() in HWC order (what ToPILImage does).

    python tools/heatmap_render_time.py [out.txt]        (GPU box)

F = 224 with the 224 / 7 row layout (72,020 rows per frame), batch 1 and batch 8.  Three legs per batch, each ending on the host
with the images of frame 0 -- what the figure needs:
  hip      get_overlays(count=1) and the read-back of its three 150 KB images
  host     the reference's route
and one that stays on the device:
  hip-all  get_overlays(count=B): every frame's three images, no read-back (device events)
Host clock around calls that end in a device synchronise or a read-back (hip, host), device events (hip-all); warm-up, then three
windows of at least 0.5 s per leg, the legs alternating; the spread over a leg's windows is printed beside its median.  The two
routes' images of frame 0 are compared first: base and gt must be equal, pred may differ by 1 on at most 1 % of the bytes; the tool
exits non-zero otherwise.

Prints one line per window and one JSON line; with a file argument the same text is appended there as well."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from echoglad_amd import evaluators  # noqa: E402

WARMUP, WINDOWS, WINDOW_S = 10, 3, 0.5
FRAME, NAUX = 224, 7
DEV = "cuda:0"
COLOURS = ((0, 1, 1), (1, 0.7, 0.9), (0, 1, 0), (1, 0, 0))
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def n_rows(frame=FRAME, naux=NAUX):
    return sum(4 ** (k + 1) for k in range(naux)) + frame * frame


def host_overlay(x, maps):
    """x [F, F], maps [F, F, 4] on the host -> uint8 [F, F, 3]: 0.8 x grey, the four colours times their maps, max, mul(255).byte()."""
    img = torch.max(torch.zeros(3, *x.shape), torch.tensor((0.8, 0.8, 0.8)).view(3, 1, 1) * x)
    for c, colour in enumerate(COLOURS):
        img = torch.max(img, torch.tensor(colour, dtype=torch.float32).view(3, 1, 1) * maps[:, :, c])
    return img.mul(255).byte().permute(1, 2, 0).contiguous()


def host_route(x, logits, labels, batch, frame=FRAME):
    """The reference's route for frame 0 -> the three images on the host."""
    lg, lb, xh = logits.detach().cpu(), labels.detach().cpu(), x.detach().cpu()[0, 0]
    y0 = lb.view(batch, -1, 4)[0, -frame * frame:, :].view(frame, frame, 4)
    p = torch.softmax(lg.view(batch, -1, 4)[0:1, -frame * frame:, :], dim=1).view(frame, frame, 4)
    p = p / p.max(dim=0, keepdim=True)[0].max(dim=1, keepdim=True)[0]
    return {"pred_img": host_overlay(xh, p), "gt_img": host_overlay(xh, y0), "coord_img": host_overlay(xh, torch.zeros_like(p))}


def inputs(batch, device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + batch)
    rows = n_rows()
    logits = torch.randn(batch * rows, 4, generator=g) * 3
    labels = torch.zeros(batch, rows, 4)
    for b in range(batch):
        for c in range(4):
            labels[b, rows - 1 - int(torch.randint(0, FRAME * FRAME, (1,), generator=g)), c] = 1
    x = torch.rand(batch, 1, FRAME, FRAME, generator=g)
    return x.to(device), logits.to(device), labels.view(-1, 4).to(device)


def host_window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6            # microseconds per call


def event_window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def main():
    assert torch.cuda.is_available(), "heatmap_render_time.py measures on a GPU"
    result = {"tool": "heatmap_render_time", "device": torch.cuda.get_device_name(0), "frame": FRAME, "rows_per_frame": n_rows(),
              "window_s": WINDOW_S, "batches": {}}
    rc = 0
    for batch in (1, 8):
        x, logits, labels = inputs(batch, DEV)
        ev = evaluators.LandmarkExpectedCoordiantesEvaluator(None, batch, FRAME, False)
        legs = {"hip": (host_window, lambda: {k: v.cpu() for k, v in ev.get_overlays(x, logits, labels, 0, 1).items()}),
                "host": (host_window, lambda: host_route(x, logits, labels, batch)),
                "hip-all": (event_window, lambda: ev.get_overlays(x, logits, labels, 0, batch))}
        got, want = legs["hip"][1](), legs["host"][1]()
        differ = {}
        for k in want:
            d = (got[k][0].to(torch.int16) - want[k].to(torch.int16)).abs()
            differ[k] = (int(d.max()), float((d > 0).float().mean()))
        ok = differ["coord_img"][0] == 0 and differ["gt_img"][0] == 0 and differ["pred_img"][0] <= 1 and differ["pred_img"][1] <= 0.01
        rc |= 0 if ok else 1
        say(f"batch {batch}: images of frame 0, hip against host (largest byte difference, share of bytes that differ): {differ}"
            + ("" if ok else "   <-- MISMATCH"))
        calls = {}
        for name, (window, fn) in legs.items():
            for _ in range(WARMUP):
                fn()
            calls[name] = max(5, int(WINDOW_S * 1e6 / max(window(fn, 5), 1.0)) + 1)
        us = {name: [] for name in legs}
        for w in range(WINDOWS):
            for name, (window, fn) in legs.items():
                us[name].append(window(fn, calls[name]))
            say(f"batch {batch}, window {w}: " + ", ".join(f"{name} {us[name][-1]:.1f} us ({calls[name]} calls)" for name in legs))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        say(f"batch {batch}: " + ", ".join(f"{k} median {med[k]:.1f} us (spread {100 * (max(v) - min(v)) / med[k]:.1f} %)" for k, v in us.items())
            + f"; host / hip = {med['host'] / med['hip']:.1f}x")
        result["batches"][str(batch)] = {"us": us, "byte_difference": {k: list(v) for k, v in differ.items()}}
    say(json.dumps(result))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write("\n".join(_lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
