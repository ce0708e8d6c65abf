#!/usr/bin/env python
"""Time the downstream probe's training step (src.trainer.DownstreamMLPTrainer._train) for the two script shapes: the
"device" backend (cvhip.probe.ProbeStep: one HIP graph per step) against the "torch" backend on the same resident
batches, and the frozen encoder alone, so the probe's share of a step is visible.  Prints one JSON line.

Shapes: VAE z=16 on 28x28x1 and VAE64 z=64 on 64x64x3, batch 128, probe Linear(z/2, 256)-BN-ReLU-Linear(256, 10), Adam
lr 3e-4 (run_styledmnist_downstream_expr.py:110-117).  Per shape, after WARMUP epochs of each backend, ROUNDS rounds
alternate torch / device / encoder-only in the same process; a round is one _train epoch over BATCHES device-resident
batches between two HIP events, divided by the number of batches:
  torch_ms, device_ms   median per-step time of the backend (min and max over the rounds beside it)
  encode_ms             vae.encode(X)[0] alone under no_grad (what the torch backend spends before its probe)
  encode_graph_ms       the batch copy and the eval-mode encoder program replayed as a graph of its own (what the
                        device step spends before cv_probe_step)
  not_slower            device_ms <= torch_ms + (torch max - torch min): the device step is not slower than the torch
                        step beyond the spread of the torch measurements of this run

Usage: python tools/probe_time.py [--batch 128] [--batches 20] [--rounds 7]
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
SHAPES = (("VAE", 16, 1, 28), ("VAE64", 64, 3, 64))


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def measure(arch, z, ch, hw, bs, nbatch, rounds):
    import src.models.vae as V
    from src.trainer import DownstreamMLPTrainer

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = getattr(V, arch)(z, ch).to(dev).eval()
    for p in vae.parameters():
        p.requires_grad = False
    batches = [(torch.rand(bs, ch, hw, hw, device=dev), torch.randint(0, 10, (bs, 1), device=dev))
               for _ in range(nbatch)]
    probe0 = nn.Sequential(nn.Linear(z // 2, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, 10))
    trainers = {}
    for backend in ("torch", "device"):
        mlp = copy.deepcopy(probe0).to(dev)
        opt = torch.optim.Adam(mlp.parameters(), lr=3e-4)
        trainers[backend] = DownstreamMLPTrainer(vae, mlp, opt, nn.CrossEntropyLoss(), 10, dev, backend=backend)

    def encode_only():
        with torch.no_grad():
            for X, _ in batches:
                vae.encode(X)[0]

    runs = {"torch": lambda: trainers["torch"]._train(batches, False, 0),
            "device": lambda: trainers["device"]._train(batches, False, 0), "encode": encode_only}
    for _ in range(WARMUP):
        for fn in runs.values():
            fn()
    eng = trainers["device"]._engine
    if eng is None or eng.steps_taken != WARMUP * nbatch:
        sys.exit("probe_time: the device backend did not take the steps")
    # the encoder part of the device step alone: the same program, workspace and batch copy, as its own graph
    from cvhip import _lib
    from cvhip.plan import Program

    G = eng.sizes[bs]
    enc = Program()
    G["ws"].encoder_program(enc, G["X"], train=False)
    enc.run()
    enc_graph = _lib.StepGraph(lambda s: enc.run(s))

    def encode_graph():
        for X, y in batches:
            eng._load_batch(G, X, y)
            enc_graph.replay()

    runs["encode_graph"] = encode_graph
    encode_graph()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ts[k].append(timed(fn, nbatch))
    row = {"arch": arch, "z": z, "batch": bs, "image": [ch, hw, hw]}
    for k in runs:
        s = summary(ts[k])
        row[f"{k}_ms"] = s["median"]
        row[f"{k}_ms_min_max"] = [s["min"], s["max"]]
    spread = row["torch_ms_min_max"][1] - row["torch_ms_min_max"][0]
    row["speedup"] = round(row["torch_ms"] / row["device_ms"], 2)
    row["probe_share_torch"] = round(1.0 - row["encode_ms"] / row["torch_ms"], 3)
    row["probe_share_device"] = round(1.0 - row["encode_graph_ms"] / row["device_ms"], 3)
    row["not_slower"] = bool(row["device_ms"] <= row["torch_ms"] + spread)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_time: needs the ROCm device")
    res = {"metric": "probe_step_ms", "warmup_epochs": WARMUP, "rounds": args.rounds, "batches": args.batches,
           "shapes": [measure(*s, args.batch, args.batches, args.rounds) for s in SHAPES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
