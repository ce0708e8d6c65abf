#!/usr/bin/env python
"""Time one CLEAR-MIM training step (src.trainer.ClearMIMVAETrainer._train) with InfoNCE and CLUBMean as the estimator:
backend="device" (HIP kernels, the one-graph fused step) against backend="torch" (the plain-PyTorch estimator, which
keeps the trainer on the module path) on the same device-resident batches.  Prints one JSON line.

Shapes are the reference's: VAE z_dim 16 on 28x28x1 at batch 128 and 512, VAE64 z_dim 64 on 64x64x3 at batch 128
(get_clearmimvae_trainer's estimator: x_dim = y_dim = z_dim / 2, hidden_size = z_dim).  Per shape and estimator,
after WARMUP epochs of each backend, ROUNDS rounds alternate torch / device in the same process; a round is one
_train epoch over BATCHES batches between two HIP events, divided by the number of batches:
  torch_ms, device_ms   median per-step time of the backend (min and max over the rounds beside it)
  speedup               torch_ms / device_ms
  faster                device_ms (max over its rounds) < torch_ms (min over its rounds)
Then the memory of one InfoNCE evaluation at n = 4096 (z_dim 64): the device workspace in bytes against the peak
allocation of the torch forward + backward (the [N, N, dx+dy] and [N, N, H] tensors).

Usage: python tools/mim_est_time.py [--batches 10] [--rounds 5] [--no-memory]
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WARMUP = 2
SHAPES = (("VAE", 16, 1, 28, 128), ("VAE", 16, 1, 28, 512), ("VAE64", 64, 3, 64, 128))
KINDS = ("InfoNCE", "CLUBMean")


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def measure(kind, arch, z, ch, hw, bs, nbatch, rounds):
    from src.utils.trainer_utils import get_clearmimvae_trainer

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    batches = [(torch.rand(bs, ch, hw, hw, generator=g).to(dev), torch.randint(0, 10, (bs,), generator=g).to(dev))
               for _ in range(nbatch)]
    trainers = {}
    for backend in ("torch", "device"):
        torch.manual_seed(0)
        trainers[backend] = get_clearmimvae_trainer(
            beta=1 / 8, mi_estimator=kind, la=3.0, vae_lr=5e-4, mi_estimator_lr=2e-3, z_dim=z, alpha=100.0,
            temperature=0.1, device=dev, vae_arch=arch, in_channel=ch, backend=backend)
    runs = {b: (lambda t=t: t._train(batches, False, 0, [], [])) for b, t in trainers.items()}
    for _ in range(WARMUP):
        for fn in runs.values():
            fn()
    if trainers["device"]._engine is None or trainers["torch"]._engine is not None:
        sys.exit("mim_est_time: the device backend must run the fused step and the torch backend the module path")
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ts[k].append(timed(fn, nbatch))
    row = {"estimator": kind, "arch": arch, "z": z, "batch": bs}
    for k in runs:
        s = summary(ts[k])
        row[f"{k}_ms"] = s["median"]
        row[f"{k}_ms_min_max"] = [s["min"], s["max"]]
    row["speedup"] = round(row["torch_ms"] / row["device_ms"], 2)
    row["faster"] = bool(row["device_ms_min_max"][1] < row["torch_ms_min_max"][0])
    return row


def memory(n=4096, z=64):
    """Bytes of one InfoNCE forward + backward at batch n: the device workspace (cv_infonce_workspace_bytes) and the
    torch path's peak allocation above what was allocated before the call."""
    from cvhip import _lib
    from src.models.mi_estimator import InfoNCE

    dev = torch.device("cuda", 0)
    d = z // 2
    est = InfoNCE(d, d, z, backend="torch").to(dev)
    x = torch.randn(n, d, device=dev, requires_grad=True)
    y = torch.randn(n, d, device=dev, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        est(x, y).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    except torch.cuda.OutOfMemoryError:
        peak = None
    return {"n": n, "z": z, "device_workspace_bytes": int(_lib.lib().cv_infonce_workspace_bytes(n, z)),
            "torch_peak_bytes": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-memory", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mim_est_time: needs the ROCm device")
    rows = [measure(k, *s, args.batches, args.rounds) for k in KINDS for s in SHAPES]
    res = {"metric": "mim_step_ms", "warmup_epochs": WARMUP, "rounds": args.rounds, "batches": args.batches,
           "shapes": rows, "all_faster": all(r["faster"] for r in rows)}
    if not args.no_memory:
        res["memory"] = memory()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
