"""Exact t-SNE on the device for the notebooks' latent plots: a drop-in for the one line
``from sklearn.manifold import TSNE`` of the demo notebooks and ``expr/visual_utils.py`` (``tsne_plot``), which call
``TSNE(n_components=2, perplexity=30, learning_rate=200, init='pca').fit_transform(mu.cpu().numpy())``.

The algorithm is sklearn's ``method="exact"`` (not its default Barnes-Hut approximation), computed matrix-free by
csrc/cv_tsne.hip: memory is O(N D), no N x N array of distances, P or Q is built.

    affinities   cv_tsne_affinity: per row the precision beta_i of the conditional Gaussian whose entropy is
                 ln(perplexity) (sklearn's bisection, tolerance 1e-5, at most 100 steps) and logz_i = ln S_i
    kl_grad      cv_tsne_pair + cv_tsne_update: KL(P || Q) and its gradient at an embedding, with
                 p_ij = max((c_ij + c_ji) / 2N, 2.2e-16), c_ij = exp(-beta_i d_ij - logz_i), rebuilt per pair
    descend      cv_tsne_run: sklearn's schedule (early exaggeration and momentum 0.5 for ``exploration_iter``
                 iterations, then 1 and 0.8, update and gains reset at the switch), every launch on the current stream
    TSNE         the class: ``fit`` / ``fit_transform``, ``embedding_``, ``kl_divergence_``, ``n_iter_``,
                 ``learning_rate_``

Differences from sklearn: the method is always exact; there is no early stopping (``min_grad_norm``,
``n_iter_without_progress``): every one of ``max_iter`` iterations runs; ``kl_divergence_`` is the KL divergence *at
the returned embedding* (sklearn reports the value from before its last update); the result is bit-reproducible (no
atomics, fixed summation order) and with ``init="pca"`` needs no ``random_state``.  Only ``n_components=2`` and the
Euclidean metric; 1 <= D <= 64 and perplexity < N <= 65536."""

from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_N = 65536
MAX_D = 64
_WORK: dict = {}


def _require_gpu(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError("clear-vae_amd: HIP kernels need tensors on the ROCm device ('cuda')")


def _check_x(name: str, x: torch.Tensor):
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be a 2-D float32 tensor")
    n, d = x.shape
    if not 1 <= d <= MAX_D:
        raise ValueError(f"{name}: the number of columns must be in 1..{MAX_D} (D={d})")
    if not 2 <= n <= MAX_N:
        raise ValueError(f"{name}: the number of rows must be in 2..{MAX_N} (N={n})")


def _check_perplexity(name: str, perplexity, n: int):
    p = float(perplexity)
    if not 0.0 < p < n:
        raise ValueError(f"{name}: perplexity must be positive and less than the number of rows ({p}, N={n})")
    return p


def _check_rows(name: str, n: int, **vecs):
    for k, v in vecs.items():
        if v.dtype != torch.float32 or v.numel() != n:
            raise ValueError(f"{name}: {k} must be float32 with one entry per row of x")


def _check_y(name: str, y: torch.Tensor, n: int):
    if y.dim() != 2 or tuple(y.shape) != (n, 2) or y.dtype != torch.float32:
        raise ValueError(f"{name}: the embedding must be a float32 [{n}, 2] tensor (got {tuple(y.shape)})")


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x with unit column stride and a row stride >= D (a ``z[:, :d]`` view passes as it is)."""
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _workspace(n: int, device) -> torch.Tensor:
    key = (n, device)
    w = _WORK.get(key)
    if w is None:
        _WORK.clear()  # one size at a time: the partials of N = 65536 take 16 MiB
        nbytes = int(_lib.lib().cv_tsne_workspace_bytes(n))
        w = _WORK[key] = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)
    return w


def affinities(x: torch.Tensor, perplexity: float):
    """``(beta, logz)``, fp32 ``[N]`` device tensors: the precision of every row's conditional Gaussian at the given
    perplexity and the logarithm of its normaliser (module docstring).  ``x``: fp32 ``[N, D]`` on the device; rows may
    be strided.  The input must be finite; this function reads nothing back to check that (:class:`TSNE` does)."""
    _require_gpu(x)
    _check_x("affinities", x)
    n, d = x.shape
    p = _check_perplexity("affinities", perplexity, n)
    x = _rows(x)
    beta = torch.empty(n, dtype=torch.float32, device=x.device)
    logz = torch.empty(n, dtype=torch.float32, device=x.device)
    _lib.call("cv_tsne_affinity", x.data_ptr(), x.stride(0), n, d, p, beta.data_ptr(), logz.data_ptr(),
              _lib.stream_handle())
    return beta, logz


def kl_grad(x: torch.Tensor, beta: torch.Tensor, logz: torch.Tensor, y: torch.Tensor, exaggeration: float = 1.0):
    """``(kl, grad)`` at the embedding ``y`` (fp32 ``[N, 2]``): the KL divergence of sklearn's ``_kl_divergence`` for
    the joint P multiplied by ``exaggeration`` (an fp64 0-d device tensor) and its gradient (fp32 ``[N, 2]``)."""
    _require_gpu(x, beta, logz, y)
    _check_x("kl_grad", x)
    n, d = x.shape
    _check_rows("kl_grad", n, beta=beta, logz=logz)
    _check_y("kl_grad", y, n)
    if not float(exaggeration) > 0.0:
        raise ValueError("kl_grad: the exaggeration must be positive")
    x, beta, logz, y = _rows(x), beta.contiguous(), logz.contiguous(), y.contiguous()
    work = _workspace(n, x.device)
    kl = torch.empty((), dtype=torch.float64, device=x.device)
    grad = torch.empty((n, 2), dtype=torch.float32, device=x.device)
    s = _lib.stream_handle()
    _lib.call("cv_tsne_pair", x.data_ptr(), x.stride(0), n, d, beta.data_ptr(), logz.data_ptr(), y.data_ptr(),
              float(exaggeration), 1, work.data_ptr(), s)
    _lib.call("cv_tsne_update", n, work.data_ptr(), None, None, None, 0.0, 0.0, 0, grad.data_ptr(), kl.data_ptr(), s)
    return kl, grad


def _run(x, beta, logz, y0, n_iter, exploration_iter, early_exaggeration, learning_rate, want_kl):
    n, d = x.shape
    y = y0.clone().contiguous()
    update, gains = torch.empty_like(y), torch.empty_like(y)
    kl = torch.empty((), dtype=torch.float64, device=x.device) if want_kl else None
    work = _workspace(n, x.device)
    _lib.call("cv_tsne_run", x.data_ptr(), x.stride(0), n, d, beta.data_ptr(), logz.data_ptr(), y.data_ptr(),
              update.data_ptr(), gains.data_ptr(), int(n_iter), int(exploration_iter), float(early_exaggeration),
              float(learning_rate), work.data_ptr(), _lib.ptr(kl), _lib.stream_handle())
    return y, kl


def descend(x: torch.Tensor, beta: torch.Tensor, logz: torch.Tensor, y0: torch.Tensor, n_iter: int,
            exploration_iter: int = 250, early_exaggeration: float = 12.0, learning_rate: float = 200.0):
    """``n_iter`` iterations of sklearn's gradient descent from ``y0`` (not written to): the new fp32 ``[N, 2]``
    embedding.  The first ``exploration_iter`` iterations use ``early_exaggeration`` and momentum 0.5, the rest 1 and
    0.8; update and gains start afresh at the switch.  Every iteration runs (no early stopping)."""
    _require_gpu(x, beta, logz, y0)
    _check_x("descend", x)
    n = x.shape[0]
    _check_rows("descend", n, beta=beta, logz=logz)
    _check_y("descend", y0, n)
    if int(n_iter) < 0 or int(exploration_iter) < 0:
        raise ValueError("descend: n_iter and exploration_iter must not be negative")
    if not float(early_exaggeration) > 0.0:
        raise ValueError("descend: early_exaggeration must be positive")
    return _run(_rows(x), beta.contiguous(), logz.contiguous(), y0, n_iter, exploration_iter, early_exaggeration,
                learning_rate, False)[0]


def auto_learning_rate(n: int, early_exaggeration: float = 12.0) -> float:
    """sklearn's ``learning_rate="auto"``: ``max(N / early_exaggeration / 4, 50)``."""
    return max(n / float(early_exaggeration) / 4.0, 50.0)


def pca_init(x: torch.Tensor) -> torch.Tensor:
    """sklearn's ``init="pca"`` with torch in fp64 on ``x``'s device: the projections on the top two eigenvectors of
    the D x D covariance, each with the sign that makes its largest-magnitude loading positive, scaled to standard
    deviation 1e-4 on the first axis; fp32 ``[N, 2]``.  With D = 1 the second axis is zero."""
    xd = x.to(torch.float64)
    xc = xd - xd.mean(dim=0, keepdim=True)
    _, vec = torch.linalg.eigh(xc.t() @ xc)
    k = min(2, vec.shape[1])
    v = vec.flip(1)[:, :k]
    top = v.gather(0, v.abs().argmax(dim=0, keepdim=True))
    v = v * torch.where(top < 0, -1.0, 1.0)
    y = torch.zeros((x.shape[0], 2), dtype=torch.float64, device=x.device)
    y[:, :k] = xc @ v
    return (y / y[:, 0].std(unbiased=False) * 1e-4).to(torch.float32)


class TSNE:
    """``sklearn.manifold.TSNE`` for the notebooks' call, on the device (module docstring for the differences).

    ``fit_transform(X)``: a numpy array in (any float dtype; it is uploaded as fp32) gives a float32 numpy array
    ``[N, 2]`` out, copied back once; a device tensor in (fp32) gives a device tensor out.  ``learning_rate="auto"`` is
    sklearn's ``max(N / early_exaggeration / 4, 50)``.  ``init``: ``"pca"`` (:func:`pca_init`), ``"random"``
    (1e-4 N(0, 1) from a torch generator seeded with ``random_state``) or an ``[N, 2]`` array or tensor.

    Attributes after ``fit``: ``embedding_``; ``kl_divergence_``, the KL divergence **at the returned embedding**
    (sklearn stores the value computed before its last update); ``n_iter_`` = ``max_iter`` (no early stopping);
    ``learning_rate_``."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto",
                 max_iter=1000, init="pca", random_state=None, exploration_iter=250):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.init = init
        self.random_state = random_state
        self.exploration_iter = exploration_iter

    def _check_params(self, n: int, d: int):
        if self.n_components != 2:
            raise ValueError(f"TSNE: only n_components=2 is implemented (got {self.n_components})")
        if not 1 <= d <= MAX_D:
            raise ValueError(f"TSNE: the number of columns must be in 1..{MAX_D} (D={d})")
        if not 2 <= n <= MAX_N:
            raise ValueError(f"TSNE: the number of rows must be in 2..{MAX_N} (N={n})")
        _check_perplexity("TSNE", self.perplexity, n)
        if not float(self.early_exaggeration) > 0.0:
            raise ValueError("TSNE: early_exaggeration must be positive")
        if int(self.max_iter) < 0 or int(self.exploration_iter) < 0:
            raise ValueError("TSNE: max_iter and exploration_iter must not be negative")
        if isinstance(self.learning_rate, str):
            if self.learning_rate != "auto":
                raise ValueError("TSNE: learning_rate must be a number or 'auto'")
            lr = auto_learning_rate(n, self.early_exaggeration)
        else:
            lr = float(self.learning_rate)
            if not lr > 0.0:
                raise ValueError("TSNE: learning_rate must be positive")
        if isinstance(self.init, str):
            if self.init not in ("pca", "random"):
                raise ValueError("TSNE: init must be 'pca', 'random' or an [N, 2] array")
        elif tuple(np.shape(self.init)) != (n, 2):
            raise ValueError(f"TSNE: init must have shape ({n}, 2), got {tuple(np.shape(self.init))}")
        return lr

    def _init(self, x: torch.Tensor) -> torch.Tensor:
        n = x.shape[0]
        if isinstance(self.init, str) and self.init == "pca":
            return pca_init(x)
        if isinstance(self.init, str):
            g = torch.Generator()
            g.manual_seed(0 if self.random_state is None else int(self.random_state))
            return (1e-4 * torch.randn((n, 2), generator=g, dtype=torch.float32)).to(x.device)
        return torch.as_tensor(self.init).to(device=x.device, dtype=torch.float32)

    def fit(self, X, y=None):
        as_numpy = not isinstance(X, torch.Tensor)
        if as_numpy:
            X = np.asarray(X)
            if X.ndim != 2 or X.dtype.kind != "f":
                raise ValueError("TSNE: X must be a 2-D floating-point array")
        elif X.dim() != 2 or X.dtype != torch.float32:
            raise ValueError("TSNE: X must be a 2-D float32 tensor")
        n, d = X.shape
        lr = self._check_params(n, d)
        if as_numpy:
            x = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float32)).to("cuda")
        else:
            _require_gpu(X)
            x = _rows(X.detach())
        # what must hold before anything is launched, in one small copy
        if bool((~torch.isfinite(x)).any()):
            raise ValueError("TSNE: X contains NaN or infinity")
        beta, logz = affinities(x, self.perplexity)
        emb, kl = _run(x, beta, logz, self._init(x), self.max_iter, self.exploration_iter, self.early_exaggeration,
                       lr, True)
        if as_numpy:
            # the one copy of the results: the embedding (exact in fp64) and the KL divergence
            host = torch.cat([emb.reshape(-1).to(torch.float64), kl.reshape(1)]).cpu().numpy()
            self.embedding_ = host[:-1].astype(np.float32).reshape(n, 2)
            self.kl_divergence_ = float(host[-1])
        else:
            self.embedding_ = emb
            self.kl_divergence_ = float(kl)
        self.n_iter_ = int(self.max_iter)
        self.learning_rate_ = lr
        return self

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_
