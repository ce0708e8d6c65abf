"""Golden vectors of the reference notebook's SNN / PSSNN modules and blob layout (development container only).

Reads the REAL notebook (read-only, /root/reference/code/mi_experiment.ipynb, never copied) at run time, writes its
code cells 0-3 (imports, logsumexp, PSSNN / SNN, generate_gaussian_blobs) to a module file in a temporary directory
outside the repository and imports that file (the cell's @jit.script needs source it can look up, so exec alone
fails).  Evaluates the notebook's own classes in fp64 on the CPU on seeded fp32 inputs and writes
tests/golden/mi_bounds.npz: per case the input, the labels, and per temperature the (SNN, PS-SNN) values and the number
of finite rows behind each (read off the notebook's own torch.isfinite call); plus the label vector and row count its
generate_gaussian_blobs returns for (n_samples, n_blobs) = (100, 3) and (96, 4).  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mi_bounds.py
"""

import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NOTEBOOK = "/root/reference/code/mi_experiment.ipynb"
TAUS = (0.01, 0.1, 0.3, 1.0)
sys.dont_write_bytecode = True


def load_notebook_module(tmp):
    cells = [c for c in json.load(open(NOTEBOOK))["cells"] if c["cell_type"] == "code"][:4]
    path = os.path.join(tmp, "mi_experiment_cells.py")
    with open(path, "w") as f:
        f.write("\n\n".join("".join(c["source"]) for c in cells) + "\n")
    spec = importlib.util.spec_from_file_location("mi_experiment_cells", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(23)
    out = {}
    # three blobs, the notebook's setting in small
    lab = np.repeat(np.arange(3), 32)
    out["blobs"] = (np.array([-1.0, 2.0, 7.0])[lab][:, None] + 2.0 * rng.standard_normal((96, 3)), lab)
    # antipodal: two classes at +- one direction, radius in [1, 2], noise 0.01; every negative similarity is about -1
    v = rng.standard_normal(5)
    v /= np.linalg.norm(v)
    sign = np.repeat([1.0, -1.0], 35)
    x = (sign * rng.uniform(1.0, 2.0, 70))[:, None] * v[None, :] + 0.01 * rng.standard_normal((70, 5))
    lab = np.repeat([0, 1], 35)
    out["antipodal"] = (x, lab)
    lab2 = lab.copy()
    lab2[3] = 11  # two labels that occur once: their rows have no positive
    lab2[50] = 12
    out["antipodal_singletons"] = (x, lab2)
    out["d1"] = (rng.standard_normal((9, 1)) + 0.3, np.array([0, 1, 0, 1, 1, 0, 0, 1, 0]))
    out["one_label"] = (rng.standard_normal((33, 4)), np.full(33, 4))
    # labels that alias when truncated to 32 bits
    out["wide_labels"] = (rng.standard_normal((40, 8)), np.array([5, 5 + 2 ** 32, 7], dtype=np.int64)[rng.integers(0, 3, 40)])
    x = rng.standard_normal((24, 3))
    x[7] = 0.0
    out["zero_row"] = (x, rng.integers(0, 3, 24))
    return {k: (np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.int64)) for k, (a, b) in out.items()}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mod = load_notebook_module(tmp)
        seen = []
        orig = torch.isfinite

        def recording(t):
            m = orig(t)
            seen.append(int(m.sum()))
            return m

        out = {"taus": np.array(TAUS)}
        torch.isfinite = recording
        try:
            for name, (x, lab) in cases().items():
                val = np.zeros((len(TAUS), 2))
                cnt = np.zeros((len(TAUS), 2), dtype=np.int64)
                xt, lt = torch.tensor(x).double(), torch.tensor(lab)
                for t, tau in enumerate(TAUS):
                    for c, cls in enumerate((mod.SNN, mod.PSSNN)):
                        del seen[:]
                        val[t, c] = float(cls(tau)(xt, lt))
                        cnt[t, c] = seen[-1]
                out[f"{name}__x"], out[f"{name}__label"] = x, lab
                out[f"{name}__value"], out[f"{name}__count"] = val, cnt
        finally:
            torch.isfinite = orig
        for n_samples, n_blobs in ((100, 3), (96, 4)):
            centers = [-1.0, 2.0, 7.0, 11.0][:n_blobs]
            s, lab = mod.generate_gaussian_blobs(n_blobs=n_blobs, n_samples=n_samples, centers=centers)
            out[f"blob_label_{n_samples}_{n_blobs}"] = lab.numpy().astype(np.int64)
            out[f"blob_rows_{n_samples}_{n_blobs}"] = np.array(s.shape[0])
    np.savez_compressed(os.path.join(HERE, "mi_bounds.npz"), **out)
    print("wrote", sum(k.endswith("__x") for k in out), "cases")


if __name__ == "__main__":
    main()
