"""An independent fp64 statement of the SNN / PS-SNN bounds (include/clearvae.h, cv_snn_bounds), written from the
semantics and not from the reference notebook: masked log-sum-exps per row over an explicit [n, n] similarity matrix.
The golden file (tests/golden/mi_bounds.npz) ties it to the notebook's own classes."""

import numpy as np


def _masked_lse(a, mask):
    """Row-wise log sum exp of a[i, j] over mask[i, j]; -inf for an empty row.  NaN propagates."""
    out = np.full(a.shape[0], -np.inf)
    for i in range(a.shape[0]):
        v = a[i, mask[i]]
        if v.size == 0:
            continue
        if np.isnan(v).any():
            out[i] = np.nan
            continue
        m = v.max()
        out[i] = m + np.log(np.exp(v - m).sum())
    return out


def bounds(x, label, taus):
    """x [n, d] (any float dtype, evaluated in fp64), label [n] integers, taus a sequence.

    Returns (bound [T, 2], count [T, 2], rows [T, 3, n]) with bound[t] = (SNN, PS-SNN) = the mean over the rows whose
    term is finite (NaN when there is none), count = how many rows that is, rows = lse_all, lse_pos, lse_neg."""
    x = np.asarray(x, dtype=np.float64)
    label = np.asarray(label).astype(np.int64)
    n = x.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        norm = np.sqrt((x * x).sum(axis=1))
        u = x / np.maximum(norm, 1e-8)[:, None]
        s = u @ u.T
        off = ~np.eye(n, dtype=bool)
        same = label[:, None] == label[None, :]
        T = len(taus)
        bound = np.full((T, 2), np.nan)
        count = np.zeros((T, 2), dtype=np.int64)
        rows = np.zeros((T, 3, n))
        for t, tau in enumerate(taus):
            a = s / float(tau)
            rows[t, 0] = _masked_lse(a, off)
            rows[t, 1] = _masked_lse(a, off & same)
            rows[t, 2] = _masked_lse(a, ~same)
            for c in range(2):
                term = rows[t, 0] - rows[t, 1 + c]
                fin = np.isfinite(term)
                count[t, c] = int(fin.sum())
                if count[t, c]:
                    bound[t, c] = term[fin].mean()
    return bound, count, rows
