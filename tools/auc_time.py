#!/usr/bin/env python
"""Time the metric tail of the classifier evaluate() paths (src.losses.auc) on synthetic logits: the device backend
(cvhip.metrics.auc) against the sklearn backend on the same device tensors.  Prints one JSON line.

Per size (n, c): 5 timed calls after 2 warm-ups, reported as the median and the min-max range, of
  device_ms   auc(..., backend="device"), HIP events around the call (softmax, label sort, cv_rank_auc, and its two
              small host reads: the input checks and the per-class results)
  kernel_ms   the cv_rank_auc call alone (softmax, order, start and workspace prepared), HIP events
  sklearn_ms  auc(..., backend="sklearn") on the same device tensors, wall clock (it copies the softmax to the host
              and runs 2 c sklearn calls there)
and not_slower = device_ms <= sklearn_ms + (sklearn max - sklearn min), the convention of tools/probe_time.py.

Usage: python tools/auc_time.py [--sizes 10000x10,34000x2] [--skip-sklearn]
"""

import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, TIMED = 2, 5


def logits(n, c, seed=0):
    """Labels with every class present, and fp32 logits that carry the label (continuous: no ties to speak of)."""
    g = np.random.default_rng(seed)
    y = g.integers(0, c, n)
    y[:c] = np.arange(c)
    x = g.standard_normal((n, c))
    x[np.arange(n), y] += 1.5
    return torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(y, device="cuda")


def timed_events(fn):
    ts = []
    for it in range(WARMUP + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= WARMUP:
            ts.append(a.elapsed_time(b))
    return ts


def timed_wall(fn):
    ts = []
    for it in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def kernel_only(logit, y):
    from cvhip import _lib, metrics

    n, c = logit.shape
    ph = logit.softmax(dim=1)
    lab32 = y.to(torch.int32)
    sorted_lab, order = torch.sort(y, stable=True)
    start = torch.searchsorted(sorted_lab, torch.arange(c + 1, device=y.device)).to(torch.int32)
    order = order.to(torch.int32)
    ap_sum = torch.empty(c, dtype=torch.float64, device=y.device)
    u2 = torch.empty(c, dtype=torch.int64, device=y.device)
    work = metrics._rank_workspace(n, c, logit.device)
    keep = (ph, lab32, order, start, ap_sum, u2, work)

    def run(_keep=keep):
        _lib.call("cv_rank_auc", ph.data_ptr(), ph.stride(0), n, c, lab32.data_ptr(), order.data_ptr(),
                  start.data_ptr(), None, ap_sum.data_ptr(), u2.data_ptr(), work.data_ptr(), _lib.stream_handle())

    return run


def put(row, key, ts, digits=3):
    row[key] = round(statistics.median(ts), digits)
    row[key + "_range"] = [round(min(ts), digits), round(max(ts), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000x10,34000x2")
    ap.add_argument("--skip-sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("auc_time: needs the ROCm device")
    from src.losses import auc

    warnings.simplefilter("ignore")
    res = {"metric": "auc_ms", "warmup": WARMUP, "timed": TIMED, "sizes": []}
    for spec in args.sizes.split(","):
        n, c = (int(v) for v in spec.split("x"))
        logit, y = logits(n, c)
        row = {"n": n, "c": c}
        dev = auc(logit, y, backend="device")
        put(row, "device_ms", timed_events(lambda: auc(logit, y, backend="device")))
        put(row, "kernel_ms", timed_events(kernel_only(logit, y)))
        row["pair_tests_per_s"] = round(float(n) * n / (row["kernel_ms"] * 1e-3), 1)
        if not args.skip_sklearn:
            ref = auc(logit, y, backend="sklearn")
            row["dicts_equal"] = all(float(d[k]) == float(s[k]) for d, s in zip(dev, ref) for k in range(c))
            put(row, "sklearn_ms", timed_wall(lambda: auc(logit, y, backend="sklearn")), 2)
            lo, hi = row["sklearn_ms_range"]
            row["not_slower"] = row["device_ms"] <= row["sklearn_ms"] + (hi - lo)
            row["speedup"] = round(row["sklearn_ms"] / row["device_ms"], 1)
        res["sizes"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
