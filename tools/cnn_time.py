#!/usr/bin/env python
"""Time the CNN baseline's training step (src.trainer.SimpleCNNTrainer._train) for the two script shapes: the "device"
backend (cvhip.cnn.CnnStep: one HIP graph per step) against the "torch" backend on the same resident batches.  Prints
one JSON line.

Shapes: SimpleCNNClassifier on 28x28x1 and SimpleCNN64Classifier on 64x64x3, 10 classes, batch 128, Adam lr 1e-4
(get_cnn_trainer).  Per shape, after WARMUP epochs of each backend, ROUNDS rounds alternate torch / device in the same
process; a round is one _train epoch over BATCHES device-resident batches between two HIP events, divided by the
number of batches:
  torch_ms, device_ms   median per-step time of the backend (min and max over the rounds beside it)
  speedup               torch_ms / device_ms
  launches              the C-ABI calls of one device step's graph, in order (plus the batch copy before it)
  not_slower            device_ms <= torch_ms + (torch max - torch min): the device step is not slower than the torch
                        step beyond the spread of the torch measurements of this run

Usage: python tools/cnn_time.py [--batch 128] [--batches 20] [--rounds 7]
"""

import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from torch import nn  # noqa: E402

WARMUP = 2
SHAPES = (("SimpleCNNClassifier", 1, 28), ("SimpleCNN64Classifier", 3, 64))
N_CLASS = 10


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def measure(arch, ch, hw, bs, nbatch, rounds):
    import src.models.cnn as M
    from src.trainer import SimpleCNNTrainer

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model0 = getattr(M, arch)(n_class=N_CLASS, in_channel=ch)
    batches = [(torch.rand(bs, ch, hw, hw, device=dev), torch.randint(0, N_CLASS, (bs, 1), device=dev))
               for _ in range(nbatch)]
    trainers = {}
    for backend in ("torch", "device"):
        model = copy.deepcopy(model0).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        trainers[backend] = SimpleCNNTrainer(model, opt, nn.CrossEntropyLoss(), 10, dev, backend=backend)
    runs = {k: (lambda t=t: t._train(batches, False, 0)) for k, t in trainers.items()}
    for _ in range(WARMUP):
        for fn in runs.values():
            fn()
    eng = trainers["device"]._engine
    if eng is None or eng.steps_taken != WARMUP * nbatch:
        sys.exit("cnn_time: the device backend did not take the steps")
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ts[k].append(timed(fn, nbatch))
    row = {"arch": arch, "batch": bs, "image": [ch, hw, hw], "n_class": N_CLASS}
    for k in runs:
        s = summary(ts[k])
        row[f"{k}_ms"] = s["median"]
        row[f"{k}_ms_min_max"] = [s["min"], s["max"]]
    spread = row["torch_ms_min_max"][1] - row["torch_ms_min_max"][0]
    row["speedup"] = round(row["torch_ms"] / row["device_ms"], 2)
    row["not_slower"] = bool(row["device_ms"] <= row["torch_ms"] + spread)
    row["launches"] = ["cv_copy_many"] + [c[0] for c in eng.sizes[bs]["prog"].calls]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cnn_time: needs the ROCm device")
    res = {"metric": "cnn_step_ms", "warmup_epochs": WARMUP, "rounds": args.rounds, "batches": args.batches,
           "shapes": [measure(*s, args.batch, args.batches, args.rounds) for s in SHAPES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
