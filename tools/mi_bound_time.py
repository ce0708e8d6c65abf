#!/usr/bin/env python
"""Time the notebook-size MI-bound sweep (code/mi_experiment.ipynb: 11 cluster widths x 100 repeats of 1500 points,
four temperatures): src.utils.mi_bounds.mi_bound_sweep (one cv_blobs launch, one cv_snn_bounds call, one cv_knn_mi
call) against the same sweep composed per trial from the entry points that existed before it: torch.randn-built
blobs, contrastive_loss x 8 (four temperatures, ps False / True) and knn_mi x 1.  HIP events around each sweep, after
warm runs of both sides; five rounds alternate the two sides in one process; median, min and max per side.  Then the
batched path's three parts on their own, five runs each.  Prints one JSON line.

Usage: python tools/mi_bound_time.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "clear-vae_amd"), ROOT]

import numpy as np
import torch

from cvhip import bounds, rng
from cvhip.metrics import knn_mi
from src.losses import contrastive_loss
from src.utils.mi_bounds import mi_bound_sweep

STDS = np.linspace(1, 4, 11)
R, N, TAUS = 100, 1500, (0.1, 0.3, 0.5, 1.0)
CENTERS = torch.tensor([-1.0, 2.0, 7.0], device="cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def batched():
    return mi_bound_sweep(STDS, repeats=R, n_samples=N, taus=TAUS)


def composed(repeats=R):
    label = torch.arange(N, device="cuda") // (N // 3)
    out = []
    with torch.no_grad():
        for sd in STDS:
            for _ in range(repeats):
                x = CENTERS[label][:, None] + float(sd) * torch.randn(N, 3, device="cuda")
                vals = [contrastive_loss(x, None, label, "cosine", tau, ps=ps) for ps in (False, True) for tau in TAUS]
                out.append((torch.stack(vals), knn_mi(x, label)))
    return out


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": v}


def main():
    torch.manual_seed(0)
    rng.reset_counters()
    res = {}
    for _ in range(2):
        batched()
    composed(repeats=2)
    tb, tc = [], []
    for _ in range(5):
        tb.append(timed(batched)[0])
        tc.append(timed(composed)[0])
    res["batched_sweep"] = stats(tb)
    res["composed_sweep"] = stats(tc)
    # the split of the batched path
    per_trial = [float(s) for s in STDS for _ in range(R)]
    x, label = bounds.gaussian_blobs(per_trial, N)
    B = x.shape[0]
    parts = {"blobs": lambda: bounds.gaussian_blobs(per_trial, N),
             "bounds": lambda: bounds.snn_bounds(x, label, TAUS),
             "knn_mi": lambda: knn_mi(x.permute(1, 0, 2).reshape(N, B * 3), label)}
    for k, fn in parts.items():
        fn()
        res[k] = stats([timed(fn)[0] for _ in range(5)])
    r = batched()
    res["check"] = {"snn_tau0.1_std1": float(r["snn"][:R, 0].mean()), "pssnn_tau0.1_std1": float(r["pssnn"][:R, 0].mean()),
                    "knn_std1": float(r["knn_mi"][:R].mean()), "knn_std4": float(r["knn_mi"][-R:].mean()),
                    "count_min": int(r["count"].min())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
