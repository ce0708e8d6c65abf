"""Generate the CLUB / VarUB golden fixtures tests/golden/mim_*.npz from the REAL reference (development
container only), with gen_golden.run_case as it stands: one real `ClearMIMVAETrainer._train` step in float64
with the reference's `CLUB` (mi_estimator.py:9-62) or `VarUB` (mi_estimator.py:201-231) as the estimator.

The file names do not start with "vae": tests/golden_cases.py:names() globs vae*.npz into the golden and oracle
tests of the two older estimators, whose helpers know nothing of these kinds.  tests/test_mi_golden_club_varub.py
reads the files written here.

Usage (where the reference checkout exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mi.py
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as GG  # noqa: E402

# name, arch, z, C, n, n_labels, mode, sim_fn, ps, estimator, store_xhat
CASES = [
    ("mim_club_vae_n64", "VAE", 16, 1, 64, 10, "mim", "cosine", None, "CLUB", False),
    ("mim_varub_vae_n64", "VAE", 16, 1, 64, 10, "mim", "cosine", None, "VarUB", False),
    ("mim_club_vae64_n16", "VAE64", 64, 3, 16, 4, "mim", "cosine", None, "CLUB", False),
]


def main():
    if not os.path.isdir(GG.REF):
        raise SystemExit(f"{GG.REF} not found: the golden fixtures are generated in the development container only")
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case[0] not in only:
            continue
        name, out = GG.run_case(case)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  mi={float(out['mi']):.9g} "
              f"mi_learning[0]={float(out['mi_learning'][0]):.9g}")


if __name__ == "__main__":
    main()
