"""Evaluation metrics on the device: the kNN mutual information behind gMIG (losses.py:10-16).

The reference's ``mutual_info_gap`` runs sklearn's ``mutual_info_classif`` (Ross 2014: continuous feature against
a discrete label, k = 3) on host copies of every validation latent.  :func:`knn_mi` computes the same statistic
with ``cv_knn_mi`` (csrc/cv_metric.hip): per feature and per point whose label occurs at least twice, the
neighbours are ordered by the key ``(|x_j - x_i| in fp64, j)``; the radius neighbour is the
``k_i = min(k, cnt_i - 1)``-th smallest key of the point's own class and ``m_i`` is one plus the number of keys
below it among all kept points.  Then

    mi = max(0, psi(n) + mean psi(k_i) - mean psi(cnt_i) - mean psi(m_i))

This is sklearn's ``_compute_mi_cd`` without its 1e-10 noise and its ``scale()`` (the statistic is rank based):
where no two distances tie at a radius the integers are sklearn's, where they tie the index breaks the tie, so the
value is deterministic.  The label-only terms are torch ops on the device, the digamma table is built on the host
once per size and uploaded; the O(n^2 d) search is the kernel.  Nothing is copied to the host except :func:`gmig`'s
one final scalar.
"""

from __future__ import annotations

import torch

from . import _lib

_EULER_GAMMA = 0.5772156649015328606
_WORK: dict = {}
_PSI: dict = {}


def _require_gpu(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError("clear-vae_amd: HIP kernels need tensors on the ROCm device ('cuda')")


def digamma_table(n: int, device) -> torch.Tensor:
    """fp64 ``[n + 1]`` with ``t[m] = psi(m) = -gamma + sum_{j<m} 1/j`` for ``m = 1..n`` (``t[0]`` is unused).

    The cumulative sum runs on the host, sequentially, so the table has the same bits on every call (a device scan
    may combine its partial sums in an order that depends on timing); the last table of each device is kept."""
    device = torch.device(device)
    hit = _PSI.get(device)
    if hit is not None and hit[0] == n:
        return hit[1]
    t = torch.zeros(n + 1, dtype=torch.float64)
    if n > 1:
        t[2:] = torch.cumsum(1.0 / torch.arange(1, n, dtype=torch.float64), 0)
    t = (t - _EULER_GAMMA).to(device)
    _PSI[device] = (n, t)
    return t


def _workspace(n: int, d: int, device) -> torch.Tensor:
    key = (n, d, device)
    w = _WORK.get(key)
    if w is None:
        nbytes = int(_lib.lib().cv_knn_mi_workspace_bytes(n, d))
        w = _WORK[key] = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)
    return w


def _classes(label: torch.Tensor):
    """(cls int32 [n] with -1 where the label occurs once, kept mask [n], class sizes of the kept labels)."""
    _, inv, counts = torch.unique(label.reshape(-1), return_inverse=True, return_counts=True)
    cnt = counts[inv]
    kept = cnt >= 2
    cls = torch.where(kept, inv, torch.full_like(inv, -1)).to(torch.int32).contiguous()
    return cls, kept, cnt[kept]


def knn_mi(latent: torch.Tensor, label: torch.Tensor, n_neighbors: int = 3, return_counts: bool = False):
    """kNN mutual information (nats) between each column of ``latent`` [n, d] (fp32, on the device) and the integer
    ``label`` [n]: an fp64 ``[d]`` tensor on the device.  With ``return_counts`` also the int32 ``[d, n_kept]``
    neighbour counts ``m_i`` and the boolean ``[n]`` mask of kept points (labels that occur at least twice).

    Rows may be strided (a ``z[:, :z_dim]`` view) as long as the column stride is 1.  Raises ``ValueError`` when
    fewer than two points are kept (every label unique): sklearn returns nan there."""
    _require_gpu(latent, label)
    if latent.dim() != 2 or latent.dtype != torch.float32:
        raise ValueError("knn_mi: latent must be a 2-D float32 tensor")
    if label.is_floating_point() or label.is_complex() or label.dtype == torch.bool:
        raise ValueError("knn_mi: label must be an integer tensor")
    n, d = latent.shape
    if label.numel() != n:
        raise ValueError(f"knn_mi: {label.numel()} labels for {n} rows")
    if d < 1:
        raise ValueError("knn_mi: latent has no columns")
    if not 1 <= int(n_neighbors) <= 8:
        raise ValueError("knn_mi: n_neighbors must be in 1..8")
    k = int(n_neighbors)
    if n < 2:
        raise ValueError("knn_mi: fewer than two points share a label (sklearn returns nan here)")
    if latent.stride(1) != 1 or latent.stride(0) < d:
        latent = latent.contiguous()
    cls, kept, cnt = _classes(label.to(latent.device))
    n_kept = int(cnt.numel())  # the shape of a device tensor: no copy
    if n_kept < 2:
        raise ValueError("knn_mi: fewer than two points share a label (sklearn returns nan here)")
    psi = digamma_table(n, latent.device)
    m = torch.empty((d, n), dtype=torch.int32, device=latent.device) if return_counts else None
    psi_sum = torch.empty(d, dtype=torch.float64, device=latent.device)
    work = _workspace(n, d, latent.device)
    _lib.call("cv_knn_mi", latent.data_ptr(), latent.stride(0), n, d, cls.data_ptr(), k, psi.data_ptr(),
              _lib.ptr(m), psi_sum.data_ptr(), work.data_ptr(), _lib.stream_handle())
    k_i = torch.clamp(cnt - 1, max=k)
    const = psi[n_kept] + psi[k_i].mean() - psi[cnt].mean()
    mi = torch.clamp(const - psi_sum / n_kept, min=0.0)
    if return_counts:
        return mi, m[:, kept], kept
    return mi


def gmig(label: torch.Tensor, latent_c: torch.Tensor, latent_s: torch.Tensor, n_neighbors: int = 3) -> float:
    """gMIG (losses.py:10-16) on the device: (mean MI of the content latents - mean MI of the style latents) / H(label),
    with the label entropy in fp64 from the class counts; one host read at the end."""
    _require_gpu(label, latent_c, latent_s)
    mi_c = knn_mi(latent_c, label, n_neighbors)
    mi_s = knn_mi(latent_s, label, n_neighbors)
    counts = torch.unique(label.reshape(-1), return_counts=True)[1].to(torch.float64)
    p = counts / counts.sum()
    H = -(p * torch.log(p)).sum()
    return float((mi_c.mean() - mi_s.mean()) / H)
