"""NumPy fp64 restatement of the kNN mutual-information statistic of cv_knn_mi (a helper, not a test).

Per feature column x and label y (sklearn's _compute_mi_cd without its 1e-10 noise and its scale(); ties broken
by index):
  kept points       the label occurs at least twice; n = their number, cnt_i the class size, k_i = min(k, cnt_i - 1)
  key               (D_ij, j), D_ij = |(double)x_j - (double)x_i|, ordered by distance, then index
  radius neighbour  j* = the k_i-th smallest key among kept j != i with y_j == y_i
  count             m_i = 1 + #{kept j != i : (D_ij, j) < (D_ij*, j*)}
  mi                max(0, psi(n) + mean psi(k_i) - mean psi(cnt_i) - mean psi(m_i))
"""

import numpy as np
from scipy.special import digamma


def make_inputs(N, d, C, seed):
    """Labels first, then features: every value a multiple of 2^-20 (every distance exact in fp64 and far above
    sklearn's 1e-10 noise); odd columns carry the label, even ones do not."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, N)
    X = rng.standard_normal((N, d)) + 0.5 * y[:, None] * (np.arange(d) % 2)
    X = (np.clip(np.round(X * 2**20), -2**23 + 1, 2**23 - 1) / 2**20).astype(np.float32)
    return X, y


def kept_mask(y):
    y = np.asarray(y).reshape(-1)
    _, inv, counts = np.unique(y, return_inverse=True, return_counts=True)
    return counts[inv] >= 2


def knn_mi_oracle(X, y, k=3):
    """(mi [d] fp64, m [d, n_kept] int64, radius_tie): radius_tie is true if any point of any feature has a second
    kept j != i at exactly the radius distance D_ij* (where sklearn's noise, not the index, would decide)."""
    X = np.asarray(X)
    y = np.asarray(y).reshape(-1)
    keep = kept_mask(y)
    Xk = X[keep].astype(np.float64)
    yk = y[keep]
    n, d = Xk.shape
    _, inv, counts = np.unique(yk, return_inverse=True, return_counts=True)
    cnt = counts[inv]
    ki = np.minimum(k, cnt - 1)
    same = inv[:, None] == inv[None, :]
    idx = np.arange(n)
    jj = np.broadcast_to(idx[None, :], (n, n))
    notself = ~np.eye(n, dtype=bool)
    mi = np.empty(d)
    m = np.empty((d, n), dtype=np.int64)
    tie = False
    for f in range(d):
        D = np.abs(Xk[None, :, f] - Xk[:, None, f])  # D[i, j]
        order = np.lexsort((jj, D), axis=1)  # per row: by D, then by j
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, jj, axis=1)  # rank[i, j] = position of key (D_ij, j) in row i
        # the k_i-th same-class non-self key in sorted order
        elig = np.take_along_axis(same & notself, order, axis=1)
        pos = np.argmax(np.cumsum(elig, axis=1) == ki[:, None], axis=1)  # sorted position of j*
        jstar = order[idx, pos]
        Dstar = D[idx, jstar]
        below = (rank < pos[:, None]) & notself
        m[f] = 1 + below.sum(axis=1)
        at_radius = (D == Dstar[:, None]) & notself
        tie = tie or bool((at_radius.sum(axis=1) > 1).any())
        mi[f] = max(0.0, digamma(n) + digamma(ki).mean() - digamma(cnt).mean() - digamma(m[f]).mean())
    return mi, m, tie
