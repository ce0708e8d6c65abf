"""Generate the InfoNCE / CLUBMean golden fixtures tests/golden/mim_{infonce,clubmean}_*.npz from the REAL reference
(development container only): one real `ClearMIMVAETrainer._train` step in float64 with the reference's `InfoNCE`
(mi_estimator.py:245-273) or `CLUBMean` (mi_estimator.py:65-105) as the estimator, driven by gen_golden.run_case.

run_case loads the estimator from `cpu_ref.det_mlp(d, z)`, whose keys are the p_mu / p_logvar pair's; for the time of
a case this generator points that one name at the deterministic weights of the estimator at hand
(tests/nce_ref.py:det_weights) and restores it.  Nothing in gen_golden.py or oracle/ is edited.  The estimator's
initial state_dict is stored in the fixture (est_init__*, the fp32 values), so the tests need no weight rule.

The file names do not start with "vae" (tests/golden_cases.py:names() globs vae*.npz).
tests/test_gpu_mim_nce_step.py reads the files written here.

Usage (where the reference checkout exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mi2.py
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import gen_golden as GG  # noqa: E402
import nce_ref as NR  # noqa: E402

# name, arch, z, C, n, n_labels, mode, sim_fn, ps, estimator, store_xhat
CASES = [
    ("mim_infonce_vae_n64", "VAE", 16, 1, 64, 10, "mim", "cosine", None, "InfoNCE", False),
    ("mim_clubmean_vae_n64", "VAE", 16, 1, 64, 10, "mim", "cosine", None, "CLUBMean", False),
    ("mim_infonce_vae64_n16", "VAE64", 64, 3, 16, 4, "mim", "cosine", None, "InfoNCE", False),
]


def main():
    if not os.path.isdir(GG.REF):
        raise SystemExit(f"{GG.REF} not found: the golden fixtures are generated in the development container only")
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case[0] not in only:
            continue
        kind = case[9]
        init = {}

        def det_weights(d, z, kind=kind, init=init):
            init.update({k: v.numpy() for k, v in NR.det_weights(kind, d, z).items()})
            return {k: v.astype(np.float64) for k, v in init.items()}

        orig = GG.R.det_mlp
        GG.R.det_mlp = det_weights
        try:
            name, out = GG.run_case(case)
        finally:
            GG.R.det_mlp = orig
        for k, v in init.items():
            out["est_init__" + k] = v.astype(np.float32)
        # the five updates' noise as the fp32 values the tests inject (they cast it to fp32 whatever its type); with
        # it the files stay within the size of the existing mim_*.npz
        out["extra_noise"] = out["extra_noise"].astype(np.float32)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  mi={float(out['mi']):.9g} "
              f"mi_learning={out['mi_learning']}")


if __name__ == "__main__":
    main()
