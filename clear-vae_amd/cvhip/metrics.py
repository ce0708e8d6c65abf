"""Evaluation metrics on the device: the kNN mutual information behind gMIG (losses.py:10-16) and the rank counts
behind average precision and AUROC (losses.py:24-33).

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

The reference's ``auc`` runs sklearn's ``average_precision_score`` and ``roc_auc_score`` once per class on host
copies of the softmax.  Both are rank statistics: for class k with scores ``s_j = softmax(logit)[j, k]``, P positives
(``y == k``) and N = n - P negatives, every positive i gets the exact integers

    ge_pos_i = #{j positive : s_j >= s_i}     (itself included)
    ge_neg_i = #{j negative : s_j >= s_i}
    gt_neg_i = #{j negative : s_j >  s_i}

and then ``AP_k = (1/P) sum_i ge_pos_i / (ge_pos_i + ge_neg_i)`` (positives tied at a threshold share one precision,
and the recall step there is their count over P: sklearn's step-wise sum) and ``AUROC_k = U2_k / (2 P N)`` with the
integer ``U2_k = sum_i [2 (N - ge_neg_i) + (ge_neg_i - gt_neg_i)]`` (Mann-Whitney, ties one half).
:func:`rank_counts` computes the counts and the two sums with ``cv_rank_auc``; :func:`auc` is ``losses.auc`` on top
of it.
"""

from __future__ import annotations

import torch

from . import _lib

_EULER_GAMMA = 0.5772156649015328606
_WORK: dict = {}
_PSI: dict = {}
_RANK_WORK: dict = {}
RANK_MAX_N = 1 << 22


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


def _rank_workspace(n: int, c: int, device) -> torch.Tensor:
    key = (n, c, device)
    w = _RANK_WORK.get(key)
    if w is None:
        nbytes = int(_lib.lib().cv_rank_auc_workspace_bytes(n, c))
        w = _RANK_WORK[key] = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)
    return w


def _check_rank_inputs(name: str, score: torch.Tensor, label: torch.Tensor):
    _require_gpu(score)
    if not isinstance(label, torch.Tensor):
        raise ValueError(f"{name}: the labels must be a tensor")
    if score.dim() != 2 or score.dtype != torch.float32:
        raise ValueError(f"{name}: the scores must be a 2-D float32 tensor")
    if label.is_floating_point() or label.is_complex() or label.dtype == torch.bool:
        raise ValueError(f"{name}: the labels must be an integer tensor")
    n, c = score.shape
    if label.numel() != n:
        raise ValueError(f"{name}: {label.numel()} labels for {n} rows")
    if not 1 <= n <= RANK_MAX_N:
        raise ValueError(f"{name}: the number of rows must be in 1..{RANK_MAX_N} (n={n})")
    if not 1 <= c <= RANK_MAX_N:
        raise ValueError(f"{name}: the number of columns must be in 1..{RANK_MAX_N} (c={c})")


def rank_counts(score: torch.Tensor, label: torch.Tensor, return_counts: bool = False):
    """The rank statistics of every column of ``score`` [n, c] (fp32, on the device) against the integer ``label`` [n]
    with values in ``[0, c)``, one class against the rest: device tensors ``(P int64 [c], ap_sum fp64 [c],
    u2 int64 [c])`` as in the module docstring.  With ``return_counts`` also the int32 ``[n, 3]`` counts
    ``(ge_pos, ge_neg, gt_neg)`` of every sample for its own class.

    Rows may be strided (a ``z[:, :c]`` view) as long as the column stride is 1.  The scores must be finite and the
    labels in range; this function reads nothing back to check that (:func:`auc` does).  A sample whose label is out
    of range belongs to no class and counts as a negative of every class.  ``order`` and ``start`` are label-only
    torch ops on the device: a stable sort, and a binary search of the sorted labels for each class's first
    position, which is the cumulative sum of the class sizes without the host read ``torch.bincount`` makes."""
    _check_rank_inputs("rank_counts", score, label)
    n, c = score.shape
    dev = score.device
    if score.stride(1) != 1 or score.stride(0) < c:
        score = score.contiguous()
    label = label.reshape(-1).to(dev)
    lab32 = label.to(torch.int32).contiguous()
    sorted_lab, order = torch.sort(label, stable=True)
    start = torch.searchsorted(sorted_lab, torch.arange(c + 1, device=dev, dtype=sorted_lab.dtype))
    order32, start32 = order.to(torch.int32), start.to(torch.int32)
    counts = torch.zeros((n, 3), dtype=torch.int32, device=dev) if return_counts else None
    ap_sum = torch.empty(c, dtype=torch.float64, device=dev)
    u2 = torch.empty(c, dtype=torch.int64, device=dev)
    work = _rank_workspace(n, c, dev)
    _lib.call("cv_rank_auc", score.data_ptr(), score.stride(0), n, c, lab32.data_ptr(), order32.data_ptr(),
              start32.data_ptr(), _lib.ptr(counts), ap_sum.data_ptr(), u2.data_ptr(), work.data_ptr(),
              _lib.stream_handle())
    P = start[1:] - start[:-1]
    if return_counts:
        return P, ap_sum, u2, counts
    return P, ap_sum, u2


def auc_values(logit: torch.Tensor, y: torch.Tensor):
    """The unrounded ``(aupr, auroc)`` lists of :func:`auc` (Python floats, one per class ``0..c-1``)."""
    import warnings

    from sklearn.exceptions import UndefinedMetricWarning

    _check_rank_inputs("auc", logit, y)
    y = y.reshape(-1).to(logit.device)
    ph = logit.detach().softmax(dim=1)
    # what must hold before anything is launched, in one small copy: the label range (which also is the number of
    # classes, as in the reference) and the finiteness of the scores
    lo, hi, bad = torch.stack([y.min(), y.max(), (~torch.isfinite(ph)).any().to(y.dtype)]).tolist()
    if lo < 0:
        raise ValueError("auc: negative label")
    if bad:
        raise ValueError("auc: the scores contain NaN or infinity")
    c = hi + 1
    if c > ph.shape[1]:
        raise ValueError(f"auc: label {hi} has no column in the {ph.shape[1]} logits")
    P, ap_sum, u2 = rank_counts(ph[:, :c], y)
    # the one copy of the results: (P, the bits of ap_sum, u2) as int64
    host = torch.stack([P, ap_sum.view(torch.int64), u2]).cpu()
    Ps, aps, u2s = host[0].tolist(), host[1].view(torch.float64).tolist(), host[2].tolist()
    n = ph.shape[0]
    aupr, auroc = [], []
    for k in range(c):
        p, neg = Ps[k], n - Ps[k]
        if p == 0:
            warnings.warn("No positive class found in y_true, recall is set to one for all thresholds.",
                          UserWarning, stacklevel=2)
        if p == 0 or neg == 0:
            warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.",
                          UndefinedMetricWarning, stacklevel=2)
            aupr.append(0.0 if p == 0 else 1.0)
            auroc.append(float("nan"))
        else:
            aupr.append(aps[k] / p)
            auroc.append(u2s[k] / (2 * p * neg))
    return aupr, auroc


def auc(logit: torch.Tensor, y: torch.Tensor):
    """``losses.auc`` (losses.py:24-33) on the device: the dicts ``(aupr, auroc)`` with keys ``0..c-1``,
    ``c = int(y.max() + 1)``, and values ``round(float, 3)``.  The softmax is torch's on the logits' device (the bits
    the sklearn backend sees), the counts are ``cv_rank_auc``'s.  A class without positives has ``aupr`` 0.0, one
    without negatives 1.0; ``auroc`` is nan for both, with sklearn's ``UndefinedMetricWarning``.

    Raises ``ValueError`` for logits that are not on the device or not fp32, a floating-point or negative label, a
    row-count mismatch and a non-finite score, before anything is launched.  Two small copies to the host: the
    checks, then the per-class results."""
    aupr, auroc = auc_values(logit, y)
    return ({k: round(v, 3) for k, v in enumerate(aupr)}, {k: round(v, 3) for k, v in enumerate(auroc)})
