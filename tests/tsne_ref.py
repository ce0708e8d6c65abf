"""fp64 NumPy restatement of exact t-SNE (sklearn's method="exact"), dense N x N, for tests only.

The four pieces cvhip.tsne computes matrix-free on the device:
  search_beta   sklearn's _binary_search_perplexity: per row the precision beta_i with H_i = ln(perplexity)
  joint_P       the symmetrised, normalised, clamped joint P rebuilt from (beta, logz)
  kl_grad       sklearn's _kl_divergence (KL and gradient) for a P multiplied by an exaggeration factor
  descend       sklearn's two _gradient_descent phases, update and gains reset at the switch, no early stopping
plus the PCA initialisation and the seeded inputs of the device tests.  tests/test_tsne_ref.py holds this file
against sklearn's own private functions.

Two deliberate differences from sklearn, both invisible at the inputs tested: the exponent of the search is shifted by
the row's smallest distance (sklearn replaces a sum that underflowed to zero by 1e-8 instead), and Q is not clamped at
2.2e-16 (q_ij / Z gets that small only for embeddings wider than about 1e4)."""

import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)  # sklearn's MACHINE_EPSILON
PERPLEXITY_TOL = 1e-5
N_STEPS = 100


def sqdist(X):
    """Dense squared Euclidean distances in fp64, by differences (no |a|^2 + |b|^2 - 2ab cancellation)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    D = np.zeros((n, n))
    for c in range(d):
        t = X[:, c][:, None] - X[None, :, c]
        t *= t
        D += t
    return D


def _min_offdiag(D):
    M = D.copy()
    np.fill_diagonal(M, np.inf)
    return M.min(axis=1)


def row_entropy(D, beta, rows=None):
    """(H_i, ln S_i) of the conditional Gaussians with precisions beta over the rows `rows` of D (default: all)."""
    rows = np.arange(len(D)) if rows is None else rows
    Dr = D[rows]
    Dr[np.arange(len(rows)), rows] = np.inf
    m = Dr.min(axis=1)
    R = Dr - m[:, None]
    R[np.arange(len(rows)), rows] = 0.0
    E = np.exp(-beta[:, None] * R)
    E[np.arange(len(rows)), rows] = 0.0
    S = E.sum(axis=1)
    T = (R * E).sum(axis=1)
    return np.log(S) + beta * T / S, np.log(S) - beta * m


def search_beta(X, perplexity, D=None):
    """sklearn's bisection per row: (beta, logz = ln S_i, H, converged)."""
    D = sqdist(X) if D is None else D
    n = len(D)
    target = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    H, logz = np.zeros(n), np.zeros(n)
    conv = np.zeros(n, dtype=bool)
    rows = np.arange(n)
    for step in range(N_STEPS):
        H[rows], logz[rows] = row_entropy(D, beta[rows], rows)
        diff = H[rows] - target
        ok = np.abs(diff) <= PERPLEXITY_TOL
        conv[rows[ok]] = True
        rows, diff = rows[~ok], diff[~ok]
        if len(rows) == 0 or step + 1 == N_STEPS:  # the beta evaluated last is the one kept, as in sklearn
            break
        up = diff > 0
        r = rows[up]
        lo[r] = beta[r]
        beta[r] = np.where(np.isinf(hi[r]), beta[r] * 2.0, 0.5 * (beta[r] + hi[r]))
        r = rows[~up]
        hi[r] = beta[r]
        beta[r] = np.where(np.isinf(lo[r]), beta[r] * 0.5, 0.5 * (beta[r] + lo[r]))
    return beta, logz, H, conv


def joint_P(X, beta, logz, D=None):
    """p_ij = max((c_ij + c_ji) / 2N, eps), c_ij = exp(-beta_i d_ij - logz_i); zero diagonal."""
    D = sqdist(X) if D is None else D
    n = len(D)
    beta, logz = np.asarray(beta, np.float64), np.asarray(logz, np.float64)
    with np.errstate(over="ignore"):
        C = np.exp(-beta[:, None] * D - logz[:, None])
    np.fill_diagonal(C, 0.0)
    P = np.maximum((C + C.T) / (2.0 * n), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def kl_grad(P, Y, exaggeration=1.0, with_kl=True):
    """(KL, grad [N, 2]) of sklearn's _kl_divergence for the joint P multiplied by `exaggeration` (KL None without
    `with_kl`)."""
    Y = np.asarray(Y, dtype=np.float64)
    n = len(Y)
    d2 = np.zeros((n, n))
    for c in range(Y.shape[1]):
        t = Y[:, c][:, None] - Y[None, :, c]
        d2 += t * t
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    eP = exaggeration * P
    kl = None
    if with_kl:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = eP * (np.log(eP) - np.log(q) + np.log(Z))
        np.fill_diagonal(t, 0.0)
        kl = t.sum()
    W = (eP - q / Z) * q
    grad = np.empty_like(Y)
    for c in range(Y.shape[1]):
        grad[:, c] = 4.0 * (W * (Y[:, c][:, None] - Y[None, :, c])).sum(axis=1)
    return kl, grad


def descend(P, Y0, n_iter, exploration_iter=250, early_exaggeration=12.0, learning_rate=200.0):
    """sklearn's schedule: exaggeration and momentum 0.5 for the first exploration_iter iterations, then 1 and 0.8;
    update and gains start afresh at the switch (sklearn's second _gradient_descent call).  Every iteration runs."""
    Y = np.array(Y0, dtype=np.float64)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iter):
        early = it < exploration_iter
        if it == exploration_iter:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        _, grad = kl_grad(P, Y, early_exaggeration if early else 1.0, with_kl=False)
        inc = update * grad < 0.0
        gains[inc] += 0.2
        gains[~inc] *= 0.8
        np.clip(gains, 0.01, np.inf, out=gains)
        update = (0.5 if early else 0.8) * update - learning_rate * (grad * gains)
        Y += update
    return Y


def pca_init(X):
    """The first two principal components (signs: the largest-magnitude loading positive; a missing second axis is
    zero), scaled to standard deviation 1e-4 on the first axis."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2]
    for c in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    Y = np.zeros((len(X), 2))
    Y[:, : V.shape[1]] = Xc @ V
    return Y / np.std(Y[:, 0]) * 1e-4


# ---------------------------------------------------------------- seeded inputs


def three_clusters(n=192, d=8, seed=0):
    """(X fp32 [n, d], labels): three Gaussian clusters."""
    g = np.random.default_rng(seed)
    lab = np.arange(n) % 3
    centres = g.normal(size=(3, d)) * 4.0
    return (centres[lab] + g.normal(size=(n, d))).astype(np.float32), lab


def _blobs(g, n, d, k=4):
    return (g.normal(size=(k, d))[g.integers(0, k, n)] * 3.0 + g.normal(size=(n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X fp32 [N, D], perplexity) of a device-test case; the same array on every call (do not write to it)."""
    g = np.random.default_rng(abs(hash_name(name)))
    if name == "min":
        return g.normal(size=(4, 1)).astype(np.float32), 2.0
    if name in ("n257", "n257_p5"):
        return case_n257(), 30.0 if name == "n257" else 5.0
    if name == "d64":
        return _blobs(g, 300, 64), 30.0
    if name == "d20":  # the 32-column build of the kernels (the other cases cover 4, 8, 16 and 64)
        return _blobs(g, 130, 20), 15.0
    if name == "n1000":
        return _blobs(g, 1000, 3), 30.0
    if name == "n4096":
        return _blobs(g, 4096, 16, k=8), 30.0
    if name == "dups":
        X = _blobs(g, 128, 6)
        X[112:] = X[:16]
        X[:, 3] = 0.75
        return X, 20.0
    if name == "scaled_up":
        return (case_n257() * np.float32(1e3)), 30.0
    if name == "scaled_down":
        return (case_n257() * np.float32(1e-3)), 30.0
    if name == "clusters":
        return three_clusters()[0], 30.0
    raise KeyError(name)


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) + 12345


@functools.lru_cache(maxsize=None)
def case_n257():
    return _blobs(np.random.default_rng(257), 257, 5)


@functools.lru_cache(maxsize=None)
def view_case():
    """[257, 9] fp32 whose left 5 columns are the n257 case."""
    g = np.random.default_rng(9)
    wide = g.normal(size=(257, 9)).astype(np.float32)
    wide[:, :5] = case_n257()
    return wide
