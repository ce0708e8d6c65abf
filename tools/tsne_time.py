#!/usr/bin/env python
"""Time one full t-SNE fit of cvhip.tsne.TSNE (the notebooks' arguments: perplexity 30, learning rate 200, PCA init,
1000 iterations) on N synthetic latents in ten Gaussian clusters, D = 8 and D = 32, against sklearn on the host.
Every figure is one run, wall clock.  Prints one JSON line.

  device        TSNE(...).fit(X) on a numpy array: upload, affinities, PCA init, 1000 iterations, the final KL pass and
                the copy back; affinities_s is cvhip.tsne.affinities alone (synchronised), per_iter_ms the rest / 1000
  sklearn_bh    sklearn's default method (barnes_hut, n_jobs=16), one full fit
  sklearn_exact sklearn's method="exact".  One iteration of it takes about 2 s at N = 10000 (an N x N fp64 pdist,
                several passes over it), a full fit about 35 minutes, so what is run is its two parts once each:
                _joint_probabilities on the N x N distances, and _kl_divergence three times (the minimum is kept);
                est_fit_s = joint_P_s + 1000 * kl_divergence_s.  --full-exact runs the full fit instead.

Usage: python tools/tsne_time.py [--n 10000] [--dims 8,32] [--skip-sklearn] [--full-exact]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ARGS = dict(perplexity=30, learning_rate=200, init="pca")


def latents(n, d, seed=0):
    g = np.random.default_rng(seed + d)
    centres = g.normal(size=(10, d)) * 3.0
    return (centres[g.integers(0, 10, n)] + g.normal(size=(n, d))).astype(np.float32)


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def device(X):
    from cvhip import tsne

    x = torch.as_tensor(X).cuda()
    torch.cuda.synchronize()
    _, ta = clock(lambda: (tsne.affinities(x, 30.0), torch.cuda.synchronize()))
    m, tf = clock(lambda: tsne.TSNE(**ARGS).fit(X))
    per_iter_ms = (tf - ta) / m.n_iter_ * 1e3
    return dict(fit_s=round(tf, 4), affinities_s=round(ta, 4), per_iter_ms=round(per_iter_ms, 4), kl=m.kl_divergence_)


def sklearn_bh(X):
    from sklearn.manifold import TSNE

    m, tf = clock(lambda: TSNE(random_state=0, n_jobs=16, **ARGS).fit(X))
    return dict(fit_s=round(tf, 2), kl=float(m.kl_divergence_), n_iter=int(m.n_iter_))


def sklearn_exact(X, full):
    from sklearn.manifold import TSNE, _t_sne as sk
    from sklearn.metrics import pairwise_distances

    if full:
        # verbose: a progress line every 50 iterations (the fit is silent for a quarter of an hour otherwise)
        m, tf = clock(lambda: TSNE(random_state=0, method="exact", verbose=2, **ARGS).fit(X))
        return dict(fit_s=round(tf, 1), kl=float(m.kl_divergence_), n_iter=int(m.n_iter_))
    n = len(X)
    P, tp = clock(lambda: sk._joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), 30.0, 0))
    Y = (np.random.default_rng(1).normal(size=(n, 2)) * 1e-4).astype(np.float32).ravel()
    tk = min(clock(lambda: sk._kl_divergence(Y, P, 1.0, n, 2))[1] for _ in range(3))
    return dict(joint_P_s=round(tp, 2), kl_divergence_s=round(tk, 3), est_fit_s=round(tp + 1000 * tk, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dims", default="8,32")
    ap.add_argument("--skip-sklearn", action="store_true")
    ap.add_argument("--full-exact", action="store_true")
    a = ap.parse_args()
    from cvhip import tsne

    tsne.TSNE(perplexity=30, max_iter=5).fit(latents(500, 8))  # library load and first launches
    torch.cuda.synchronize()
    out = {"metric": "tsne_fit_s", "n": a.n, "runs": 1, "sizes": []}
    for d in (int(s) for s in a.dims.split(",")):
        X = latents(a.n, d)
        row = {"d": d, "device": device(X)}
        if not a.skip_sklearn:
            row["sklearn_bh"] = sklearn_bh(X)
            row["sklearn_exact"] = sklearn_exact(X, a.full_exact)
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
