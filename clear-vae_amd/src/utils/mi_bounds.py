"""The numerical study behind the claim that SNN and PS-SNN bound the mutual information
(``code/mi_experiment.ipynb``), on the device.

The notebook's cells 1-3 (``logsumexp``, ``PSSNN`` / ``SNN``, ``generate_gaussian_blobs``) are replaced by

    from src.utils.mi_bounds import PSSNN, SNN, generate_gaussian_blobs

and its loop cells run unchanged: the blobs come from one ``cv_blobs`` launch and already live on the device
(``.cuda()`` on them is a no-op, the CPU ``randperm`` indexes them as it is), a 2-D input goes through
``contrastive_loss`` (``cv_ntxent``) and stays differentiable.  :func:`mi_bound_sweep` is the whole experiment as one
call: every trial of every cluster width is drawn at once, ``cv_snn_bounds`` evaluates both bounds at every
temperature in one pass over the pairs and ``cv_knn_mi`` gives the kNN estimate of all trials in one call.
matplotlib is imported only by :func:`plot_mi_bounds`, when it draws.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from cvhip import bounds as _bounds
from cvhip.metrics import knn_mi
from src.losses import contrastive_loss

_CURVES = ("lightskyblue", "skyblue", "deepskyblue", "dodgerblue")


class _Bound(nn.Module):
    _ps = False

    def __init__(self, tau):
        super().__init__()
        self.tau = tau

    def forward(self, x, label):
        """``[n, d]``: the notebook's scalar, differentiable (``contrastive_loss``).  ``[B, n, d]``: one fp64 value
        per trial from ``cvhip.bounds.snn_bounds``, forward only."""
        if x.dim() == 3:
            if x.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError(f"{type(self).__name__}: the batched [B, n, d] path has no backward; "
                                          "detach the input or call it per trial with [n, d]")
            snn, pssnn, _ = _bounds.snn_bounds(x, label, [self.tau])
            return (pssnn if self._ps else snn)[:, 0]
        return contrastive_loss(x, None, label, "cosine", self.tau, ps=self._ps)


class SNN(_Bound):
    """The notebook's ``SNN(tau)``: the mean over the finite rows of ``lse_all - lse_pos``."""


class PSSNN(_Bound):
    """The notebook's ``PSSNN(tau)``: the mean over the finite rows of ``lse_all - lse_neg``."""

    _ps = True


def generate_gaussian_blobs(n_blobs: int = 3, n_samples: int = 100, dim: int = 3, centers=[-1.0, 2.0, 7.0],
                            cluster_std=1.0, device="cuda"):
    """The notebook's generator with its names and defaults, drawn on ``device``: a scalar ``cluster_std`` returns
    ``(samples [n, dim], labels [n])``, a sequence or tensor of B widths ``(samples [B, n, dim], labels [n])``, with
    ``n = (n_samples // n_blobs) * n_blobs``."""
    scalar = not isinstance(cluster_std, torch.Tensor) and not hasattr(cluster_std, "__len__")
    stds = [cluster_std] if scalar else cluster_std
    x, label = _bounds.gaussian_blobs(stds, n_samples, dim=dim, centers=centers, n_blobs=n_blobs, device=device)
    return (x[0] if scalar else x), label


def mi_bound_sweep(stds, repeats: int = 100, n_samples: int = 1500, n_blobs: int = 3, dim: int = 3,
                   centers=(-1.0, 2.0, 7.0), taus=(0.1, 0.3, 0.5, 1.0), n_neighbors: int = 3) -> dict:
    """The notebook's loop cells 4 and 6 as one call: ``len(stds) * repeats`` trials in the notebook's order (the std
    outer, the repeat inner), as a dict of device tensors

        "std"     fp32 [S R]        the cluster width of every trial
        "knn_mi"  fp64 [S R, dim]   the kNN estimate per input dimension (sklearn's mutual_info_classif)
        "snn"     fp64 [S R, T]     "pssnn"  fp64 [S R, T]     the bounds at every temperature
        "count"   int32 [S R, T, 2] the finite rows behind (snn, pssnn)

    plus ``"taus"``, the temperatures as a tuple of floats (the curve labels of :func:`plot_mi_bounds`).  One ``cv_blobs`` launch, one ``cv_snn_bounds`` call and one ``cv_knn_mi`` call on the ``[n, S R dim]`` view of the
    blobs (the trials share one label vector).  No result is read back to the host (``stds`` given as a sequence is
    checked on the host; ``knn_mi``'s label bookkeeping, ``torch.unique``, is the one place that waits for the device).

    The notebook's ``randperm`` shuffle is omitted: every statistic here is invariant under a permutation of the
    rows, up to the index tie-breaks of the kNN count, which continuous data does not meet."""
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError("mi_bound_sweep: repeats must be positive")
    tau_list = _bounds.check_taus(taus)
    if isinstance(stds, torch.Tensor) and stds.device.type == "cuda":
        per_trial = stds.to(torch.float32).reshape(-1).repeat_interleave(repeats)
    else:
        if isinstance(stds, torch.Tensor):
            stds = stds.reshape(-1).tolist()
        per_trial = [float(s) for s in stds for _ in range(repeats)]
    x, label = _bounds.gaussian_blobs(per_trial, n_samples, dim=dim, centers=centers, n_blobs=n_blobs)
    B, n, _ = x.shape
    snn, pssnn, count = _bounds.snn_bounds(x, label, tau_list)
    mi = knn_mi(x.permute(1, 0, 2).reshape(n, B * dim), label, n_neighbors).reshape(B, dim)
    std = per_trial if isinstance(per_trial, torch.Tensor) else torch.tensor(per_trial, dtype=torch.float32).to(x.device)
    return {"std": std, "knn_mi": mi, "snn": snn, "pssnn": pssnn, "count": count, "taus": tuple(tau_list)}


def plot_mi_bounds(result: dict, which: str = "pssnn", ax=None):
    """The notebook's figure (cells 5 and 7) from a :func:`mi_bound_sweep` result: the kNN estimate in black (negated
    for ``"snn"``, as cell 6 does) and one curve per temperature over the trials.  Returns the axes."""
    if which not in ("pssnn", "snn"):
        raise ValueError("plot_mi_bounds: which must be 'pssnn' or 'snn'")
    import matplotlib.pyplot as plt

    if ax is None:
        _, ax = plt.subplots(figsize=(5, 3))
    mi = result["knn_mi"].detach().cpu().numpy()
    vals = result[which].detach().cpu().numpy()
    name = "PS-SNN" if which == "pssnn" else "SNN"
    lines = ax.plot(-mi if which == "snn" else mi, color="black")
    lines[0].set_label("KNN estimate")
    taus = result.get("taus") or tuple(range(vals.shape[1]))
    for t in range(vals.shape[1]):
        ax.plot(vals[:, t], color=_CURVES[t % len(_CURVES)], label=f"{name} $(\\tau = {taus[t]})$")
    ax.set_xlabel("steps")
    ax.set_ylabel("MI" if which == "pssnn" else "-MI")
    ax.legend()
    return ax
