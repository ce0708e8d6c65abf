#!/usr/bin/env python
"""Time gMIG (src.losses.mutual_info_gap) on synthetic latents: the device backend (cvhip.metrics.gmig) against the
sklearn backend on the same tensors.  Prints one JSON line.

Per size (N, d_c + d_s): the median of 5 timed calls after 2 warm-ups of
  device_ms   mutual_info_gap(..., backend="device"), HIP events around the call (which ends in its one host read)
  kernel_ms   the two cv_knn_mi calls alone (class ids, digamma table and workspace prepared), HIP events
  sklearn_ms  mutual_info_gap(..., backend="sklearn") on the same device tensors, wall clock (it copies them to the
              host and runs one KD-tree per latent dimension there)
and from kernel_ms the kernel's compare-steps per second (2 passes x N^2 x d: one fp64 subtract-and-compare per
neighbour candidate per pass) and that rate as a fraction of the fp64 vector peak, counting 2 fp64 operations per
compare-step against 78.6 TFLOP/s (AMD's MI355X figure, which counts an FMA as 2).

Usage: python tools/gmig_time.py [--sizes 10000x32,20000x128] [--classes 10] [--skip-sklearn]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
WARMUP, TIMED = 2, 5


def latents(n, d, classes, seed=0):
    """Labels, and latents whose first half (the content columns) carries the label while the second half (style)
    does not (continuous fp32: no ties to speak of)."""
    g = np.random.default_rng(seed)
    y = g.integers(0, classes, n)
    x = g.standard_normal((n, d)) + 0.5 * y[:, None] * (np.arange(d) < d // 2)
    return torch.tensor(y, device="cuda"), torch.tensor(x, dtype=torch.float32, device="cuda")


def median_events(fn):
    ts = []
    for it in range(WARMUP + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def median_wall(fn):
    ts = []
    for it in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_only(label, z, zd):
    from cvhip import _lib, metrics

    n = z.shape[0]
    cls, kept, _ = metrics._classes(label)
    assert bool(kept.all()), "synthetic labels all occur at least twice"
    psi = metrics.digamma_table(n, z.device)
    out = torch.empty(zd, dtype=torch.float64, device=z.device)
    work = metrics._workspace(n, zd, z.device)
    views = (z[:, :zd], z[:, zd:])

    def run():
        for v in views:
            _lib.call("cv_knn_mi", v.data_ptr(), v.stride(0), n, zd, cls.data_ptr(), 3, psi.data_ptr(), None,
                      out.data_ptr(), work.data_ptr(), _lib.stream_handle())

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000x32,20000x128")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--skip-sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gmig_time: needs the ROCm device")
    from src.losses import mutual_info_gap

    res = {"metric": "gmig_ms", "warmup": WARMUP, "timed": TIMED, "sizes": []}
    for spec in args.sizes.split(","):
        n, d = (int(v) for v in spec.split("x"))
        zd = d // 2
        label, z = latents(n, d, args.classes)
        c, s = z[:, :zd], z[:, zd:]
        row = {"n": n, "d": d}
        dev = mutual_info_gap(label, c, s, backend="device")
        row["device_ms"] = round(median_events(lambda: mutual_info_gap(label, c, s, backend="device")), 3)
        row["kernel_ms"] = round(median_events(kernel_only(label, z, zd)), 3)
        steps = 2.0 * n * n * d
        row["compare_steps_per_s"] = round(steps / (row["kernel_ms"] * 1e-3), 1)
        row["fp64_vector_peak_fraction"] = round(2.0 * row["compare_steps_per_s"] / FP64_VECTOR_PEAK, 4)
        row["gmig_device"] = dev
        if not args.skip_sklearn:
            row["gmig_sklearn"] = float(mutual_info_gap(label, c, s, backend="sklearn"))
            row["sklearn_ms"] = round(median_wall(lambda: mutual_info_gap(label, c, s, backend="sklearn")), 1)
            row["speedup"] = round(row["sklearn_ms"] / row["device_ms"], 1)
        res["sizes"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
