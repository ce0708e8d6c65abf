#!/usr/bin/env python
"""Time the LAM baseline's training step (src.trainer.LAMCNNTrainer._train) for the two script shapes: the "device"
backend (cvhip.lam.LamStep: one HIP graph per step) against the "torch" backend (the reference's loop: three trunk
forwards, ss_pairing on the host, lam_loss) on the same resident batches.  The method of tools/cnn_time.py.  Prints one
JSON line.

Shapes: LAMCNNClassifier on 28x28x1 and LAMCNN64Classifier on 64x64x3, 10 classes, batch 128, Adam lr 1e-4,
lam_coef 0.1 (get_lamcnn_trainer).  Per shape, after WARMUP epochs of each backend, ROUNDS rounds alternate torch /
device in the same process; a round is one _train epoch over BATCHES device-resident batches between two HIP events,
divided by the number of batches:
  torch_ms, device_ms   median per-step time of the backend (min and max over the rounds beside it)
  cnn_device_ms         for orientation: the device CNN baseline (cvhip.cnn.CnnStep on the Simple model with the same
                        trunk) in the same rounds
  speedup               torch_ms / device_ms
  launches              the C-ABI calls of one device step's graph, in order (plus the batch copy before it)
  not_slower            device_ms <= torch_ms + (torch max - torch min): the device step is not slower than the torch
                        step beyond the spread of the torch measurements of this run

Usage: python tools/lam_time.py [--batch 128] [--batches 20] [--rounds 7]
"""

import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from torch import nn  # noqa: E402

from cnn_time import WARMUP, summary, timed  # noqa: E402

SHAPES = (("LAMCNNClassifier", "SimpleCNNClassifier", 1, 28), ("LAMCNN64Classifier", "SimpleCNN64Classifier", 3, 64))
N_CLASS = 10
LAM_COEF = 0.1


def measure(arch, simple, ch, hw, bs, nbatch, rounds):
    import src.models.cnn as M
    from src.trainer import LAMCNNTrainer, SimpleCNNTrainer

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model0 = getattr(M, arch)(n_class=N_CLASS, in_channel=ch)
    batches = [(torch.rand(bs, ch, hw, hw, device=dev), torch.randint(0, N_CLASS, (bs, 1), device=dev))
               for _ in range(nbatch)]
    trainers = {}
    for backend in ("torch", "device"):
        model = copy.deepcopy(model0).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        trainers[backend] = LAMCNNTrainer(model, opt, nn.CrossEntropyLoss(), {"lam_coef": LAM_COEF}, 10, dev,
                                          backend=backend)
    model = getattr(M, simple)(n_class=N_CLASS, in_channel=ch).to(dev)
    trainers["cnn_device"] = SimpleCNNTrainer(model, torch.optim.Adam(model.parameters(), lr=1e-4),
                                              nn.CrossEntropyLoss(), 10, dev, backend="device")
    runs = {k: (lambda t=t: t._train(batches, False, 0)) for k, t in trainers.items()}
    for _ in range(WARMUP):
        for fn in runs.values():
            fn()
    for k in ("device", "cnn_device"):
        eng = trainers[k]._engine
        if eng is None or eng.steps_taken != WARMUP * nbatch:
            sys.exit(f"lam_time: the {k} backend did not take the steps")
    eng = trainers["device"]._engine
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ts[k].append(timed(fn, nbatch))
    row = {"arch": arch, "batch": bs, "image": [ch, hw, hw], "n_class": N_CLASS, "lam_coef": LAM_COEF}
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
        sys.exit("lam_time: needs the ROCm device")
    res = {"metric": "lam_step_ms", "warmup_epochs": WARMUP, "rounds": args.rounds, "batches": args.batches,
           "shapes": [measure(*s, args.batch, args.batches, args.rounds) for s in SHAPES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
