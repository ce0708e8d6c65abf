#!/usr/bin/env python
"""Time a whole evaluate() epoch of the CLEAR trainers on its two backends: the module path (backend="module":
EncodeFn / DecodeFn / two SampleFn calls, cv_output_forward + cv_mse_sum, two cv_kl and the contrastive / MI calls per
batch, Python-side sums and three torch.cat at the end) against the fused pass (backend="fused":
cvhip.evaluate.EvalPass, one replayed HIP graph per batch, the sums and latents on the device).  Prints one JSON line.

Shapes: VAE z = 16 on 28x28x1 at batch 128 over 7,500 images (the Styled-MNIST scripts' validation split: 58 batches
of 128 and one of 76) and at batch 512 over 7,680; VAE64 z = 64 on 64x64x3 at batch 128 over 4,096.  Per shape CLEAR
(cosine, ps = True) and CLEAR-MIM (CLUBSample); images ~ U[0, 1), labels uniform in 0..9, seeded, every batch resident
on the device.  Both backends run on ONE trainer (evaluation changes no weights), with CVHIP_GMIG=device on both sides.
After WARMUP rounds of each backend (the fused pass's eager and capturing batches among them), ROUNDS rounds alternate
the backends in the same process; a round is one evaluate() call between two reads of the host clock, the second after
a device synchronise (evaluate() itself ends with host reads on both backends):
  <backend>_ms         median round of the backend, <backend>_ms_min_max the extremes over its rounds
  gmig_ms              median of the metric call alone (mutual_info_gap, backend "device", on the epoch's latents) with
                       its own synchronise: part of every round of both backends
  ratio                module_ms / fused_ms
  not_slower           fused_ms (median) <= the module path's fastest round

Usage: python tools/eval_time.py [--rounds 7] [--warmup 2] [--shapes 0,1,2]
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

import torch  # noqa: E402

SHAPES = (("VAE", 16, 1, 28, 128, 7500), ("VAE", 16, 1, 28, 512, 7680), ("VAE64", 64, 3, 64, 128, 4096))
TRAINERS = ("clear", "mim")
BACKENDS = ("module", "fused")


class Loader:
    """Resident batches with the two things evaluate() asks a DataLoader for."""

    def __init__(self, batches):
        self.batches = batches
        self.dataset = range(sum(int(b[1].numel()) for b in batches))

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def make_trainer(kind, arch, zt, C):
    from src.utils import trainer_utils as U

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if kind == "clear":
        return U.get_clearvae_trainer(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=zt, alpha=100, temperature=0.1, device=dev,
                                      vae_arch=arch, in_channel=C)
    return U.get_clearmimvae_trainer(beta=1 / 8, mi_estimator="CLUBSample", la=2.0, vae_lr=5e-4, mi_estimator_lr=2e-3,
                                     z_dim=zt, alpha=100, temperature=0.1, device=dev, vae_arch=arch, in_channel=C)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(kind, arch, zt, C, hw, n, total, rounds, warmup):
    from src.losses import mutual_info_gap

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1000 * n + zt)
    batches = []
    left = total
    while left > 0:
        m = min(n, left)
        batches.append((torch.rand(m, C, hw, hw, generator=g).to(dev), torch.randint(0, 10, (m,), generator=g).to(dev)))
        left -= m
    loader = Loader(batches)
    tr = make_trainer(kind, arch, zt, C)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*runs as 'module'.*")  # (a refusal of the fused backend would warn: nothing to compare then)
        for _ in range(warmup):
            for b in BACKENDS:
                tr.evaluate(loader, False, 0, backend=b)
    ep = tr._eval_pass
    if ep is None or any(G["graph"] is None for G in ep.sizes.values() if G["count"] > 1):
        sys.exit("eval_time: the fused backend did not reach its graphs")
    ts = {b: [] for b in BACKENDS}
    gm = []
    for _ in range(rounds):
        for b in BACKENDS:
            ms, _ = clock(lambda: tr.evaluate(loader, False, 0, backend=b))
            ts[b].append(ms)
        _, _, label, lat_c, lat_s = ep.finish()
        ms, _ = clock(lambda: mutual_info_gap(label, lat_c, lat_s, backend="device"))
        gm.append(ms)
    row = {"trainer": kind, "arch": arch, "z": zt, "image": [C, hw, hw], "batch": n, "images": total,
           "batches": len(batches)}
    for b in BACKENDS:
        row[f"{b}_ms"] = round(statistics.median(ts[b]), 3)
        row[f"{b}_ms_min_max"] = [round(min(ts[b]), 3), round(max(ts[b]), 3)]
    row["gmig_ms"] = round(statistics.median(gm), 3)
    row["ratio"] = round(row["module_ms"] / row["fused_ms"], 2)
    row["not_slower"] = bool(row["fused_ms"] <= row["module_ms_min_max"][0])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1,2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_time: needs the ROCm device")
    os.environ["CVHIP_GMIG"] = "device"
    rows = []
    for i in (int(v) for v in a.shapes.split(",")):
        for kind in TRAINERS:
            rows.append(measure(kind, *SHAPES[i], a.rounds, a.warmup))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "eval_time", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
                      "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
