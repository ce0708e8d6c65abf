#!/usr/bin/env python
"""Time the composition of the feature-swapping figure: cvhip.figures.swap_figure (four cv_make_grid launches into one
canvas) against the torch composition the reference gets from torchvision, written out here: make_grid as its
per-image ``narrow().narrow().copy_()`` loop, make_colored_grid's masked assignments and the torch.cat of the parts,
on the same device tensors.  The decode is not part of either side: both get the same X and decoded images.  The two
results are compared bit for bit before anything is timed.  Prints one JSON line.

Shapes: n = 10 images of 28 x 28 x 1 (the notebook's) and n = 32 of 64 x 64 x 3; uniform random images, seeded.
Per shape, after WARMUP calls of each side, ROUNDS rounds alternate torch / device in the same process; a round is
ITERS calls between two HIP events, divided by ITERS (the torch side's boolean-index assignments synchronise inside
every call: that wait is part of what it costs):
  torch_ms, device_ms   median per-call time of the side (min and max over the rounds beside it)
  speedup               torch_ms / device_ms
  not_slower            device_ms (median) <= torch_ms (median)
  bytes                 4 (M C H W + 3 Hg Wg) summed over the figure's four parts: what the device side reads and writes
  hbm_fraction          bytes / device_ms as a fraction of PEAK_BW

Usage: python tools/figure_time.py [--iters 20] [--rounds 7]
"""

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WARMUP = 3
SHAPES = ((10, 1, 28), (32, 3, 64))
PEAK_BW = 8.0e12  # bytes / s: the MI355X HBM3E peak


def torch_make_grid(images, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid's algorithm (no normalize / scale_each) in torch ops on the images' device."""
    if images.size(1) == 1:
        images = torch.cat((images, images, images), 1)
    if images.size(0) == 1:
        return images.squeeze(0)
    m = images.size(0)
    xmaps = min(nrow, m)
    ymaps = int(math.ceil(float(m) / xmaps))
    height, width = int(images.size(2) + padding), int(images.size(3) + padding)
    grid = images.new_full((images.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= m:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(
                2, x * width + padding, width - padding).copy_(images[k])
            k += 1
    return grid


def torch_colored_grid(images, nrow, color):
    grid = torch_make_grid(images, nrow=nrow, pad_value=0.25)
    tested, values = {"red": (0, (1, 0, 0)), "blue": (2, (0, 0, 1))}[color]
    for ch in range(3):
        grid[ch][grid[tested] == 0.25] = values[ch]
    return grid


def torch_swap_figure(X, decoded):
    n, _, h, w = X.shape
    hgrid = torch_colored_grid(X, n, "blue")
    vgrid = torch_colored_grid(X, 1, "red")
    main = torch_make_grid(decoded, nrow=n)
    corner = torch.ones(3, h + 4, w + 4, device=X.device)
    return torch.cat([torch.cat([corner, vgrid], dim=1), torch.cat([hgrid, main], dim=1)], dim=-1)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def figure_bytes(n, c, h, w):
    from cvhip.figures import grid_size

    parts = [(n, c, grid_size(n, h, w, 1)), (n, c, grid_size(n, h, w, n)), (n * n, c, grid_size(n * n, h, w, n)),
             (0, c, (h + 4, w + 4))]
    return sum(4 * (m * cc * h * w + 3 * gh * gw) for m, cc, (gh, gw) in parts)


def measure(n, c, size, iters, rounds):
    from cvhip import figures

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(100 * n + size)
    X = torch.rand(n, c, size, size, generator=g).to(dev)
    decoded = torch.rand(n * n, c, size, size, generator=g).to(dev)
    runs = {"torch": lambda: torch_swap_figure(X, decoded), "device": lambda: figures.swap_figure(X, decoded)}
    same = bool(torch.equal(runs["torch"]().view(torch.int32), runs["device"]().view(torch.int32)))
    for _ in range(WARMUP):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ts[k].append(timed(fn, iters))
    row = {"n": n, "c": c, "size": size, "bit_identical": same}
    for k in runs:
        s = summary(ts[k])
        row[f"{k}_ms"] = s["median"]
        row[f"{k}_ms_min_max"] = [s["min"], s["max"]]
    row["speedup"] = round(row["torch_ms"] / row["device_ms"], 2)
    row["not_slower"] = bool(row["device_ms"] <= row["torch_ms"])
    row["bytes"] = figure_bytes(n, c, size, size)
    row["hbm_fraction"] = round(row["bytes"] / (row["device_ms"] * 1e-3) / PEAK_BW, 5)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("figure_time: needs the ROCm device")
    rows = [measure(n, c, size, a.iters, a.rounds) for n, c, size in SHAPES]
    print(json.dumps({"tool": "figure_time", "device": torch.cuda.get_device_name(0), "iters": a.iters,
                      "rounds": a.rounds, "peak_bw": PEAK_BW, "rows": rows}))
    if not all(r["bit_identical"] and r["not_slower"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
