#!/usr/bin/env python
"""Time a whole CLEARVAETrainer training step with a supcon loss name on its two step forms: the module path
(hyperparameter["loss_step"] = "module": per-layer autograd, two SupConFn calls, torch Adam — what these loss names
trained with before the fused step existed) against the fused step ("fused": cvhip.engine.ClearStep with
cv_supcon_step, one replayed HIP graph), and, for context, the snn_loss fused step at the same shape.  Prints one JSON
line.

Shapes: VAE z = 16 on 28x28x1 at batch 512 (the benchmark's headline shape) and VAE64 z = 64 on 64x64x3 at batch
256; both supcon losses, cosine, temperature 0.1, alpha 100, ps = True; images ~ U[0, 1), labels uniform in 0..9,
seeded, ITERS batches resident on the device.  Per shape and loss every leg has its own trainer from the same seed;
after WARMUP passes of each leg over the batches (the fused legs' eager and capturing steps among them), ROUNDS
rounds alternate the legs in the same process; a round is one _train() pass over the ITERS batches between two HIP
events, divided by ITERS:
  <leg>_ms           median per-step time of the leg, <leg>_ms_min_max the extremes over its rounds
  speedup            module_ms / fused_ms
  not_slower         fused_ms (median) <= the module path's fastest round

Usage: python tools/supcon_step_time.py [--iters 10] [--rounds 5] [--legs module,fused,snn]
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

WARMUP = 3
SHAPES = (("VAE", 16, 1, 28, 512), ("VAE64", 64, 3, 64, 256))
LOSSES = ("supcon_in_loss", "supcon_out_loss")
LEGS = ("module", "fused", "snn")


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def make_trainer(arch, zt, C, leg, loss_name):
    from src.models.vae import VAE, VAE64
    from src.trainer import CLEARVAETrainer

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = (VAE if arch == "VAE" else VAE64)(total_z_dim=zt, in_channel=C).to(dev)
    opt = torch.optim.Adam(vae.parameters(), lr=5e-4)
    hp = {"temperature": 0.1, "alpha": 100, "beta": 1 / 8, "ps": True, "loc": 0, "scale": 1}
    if leg != "snn":
        hp.update(loss_name=loss_name, loss_step=leg)
    return CLEARVAETrainer(vae, opt, "cosine", hp, 1, dev)


def measure(arch, zt, C, hw, n, loss_name, legs, iters, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1000 * n + zt)
    batches = [(torch.rand(n, C, hw, hw, generator=g).to(dev), torch.randint(0, 10, (n,), generator=g).to(dev))
               for _ in range(iters)]
    trainers = {leg: make_trainer(arch, zt, C, leg, loss_name) for leg in legs}

    def run(leg):
        trainers[leg]._train(batches, False, 0)

    for _ in range(WARMUP):
        for leg in legs:
            run(leg)
    torch.cuda.synchronize()
    row = {"arch": arch, "z": zt, "image": [C, hw, hw], "n": n, "loss": loss_name}
    for leg in legs:  # (what each leg really ran on)
        eng = trainers[leg]._engine
        row[f"{leg}_engine"] = eng is not None
        if leg != "module" and (eng is None or "graphs" not in eng.graphs.get(n, {})):
            sys.exit(f"supcon_step_time: the {leg} leg did not reach its step graph")
    if "module" in legs and trainers["module"]._engine is not None:
        sys.exit("supcon_step_time: the module leg built an engine")
    ts = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(leg)
            b.record()
            b.synchronize()
            ts[leg].append(a.elapsed_time(b) / iters)
    for leg in legs:
        s = summary(ts[leg])
        row[f"{leg}_ms"] = s["median"]
        row[f"{leg}_ms_min_max"] = [s["min"], s["max"]]
    if "module" in legs and "fused" in legs:
        row["speedup"] = round(row["module_ms"] / row["fused_ms"], 2)
        row["not_slower"] = bool(row["fused_ms"] <= row["module_ms_min_max"][0])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    legs = tuple(a.legs.split(","))
    if not legs or any(leg not in LEGS for leg in legs):
        sys.exit(f"supcon_step_time: --legs takes a comma-separated subset of {LEGS}")
    if not torch.cuda.is_available():
        sys.exit("supcon_step_time: needs the ROCm device")
    rows = [measure(*shape, ln, legs, a.iters, a.rounds) for shape in SHAPES for ln in LOSSES]
    print(json.dumps({"tool": "supcon_step_time", "device": torch.cuda.get_device_name(0), "iters": a.iters,
                      "rounds": a.rounds, "legs": list(legs), "rows": rows}))


if __name__ == "__main__":
    main()
