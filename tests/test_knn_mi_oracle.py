"""The kNN mutual-information statistic without a GPU: the NumPy oracle (tests/knn_mi_oracle.py) against sklearn on
tie-free inputs, the `backend` keyword of src.losses.mutual_info_gap, and the host validation of cv_knn_mi."""

import ctypes

import numpy as np
import pytest
import torch
from sklearn.feature_selection import mutual_info_classif

from knn_mi_oracle import knn_mi_oracle, make_inputs

TIE_FREE = [(512, 4, 4, 0), (777, 6, 10, 5)]


@pytest.mark.parametrize("N,d,C,seed", TIE_FREE)
def test_oracle_equals_sklearn_on_tie_free_inputs(N, d, C, seed):
    X, y = make_inputs(N, d, C, seed)
    mi, m, tie = knn_mi_oracle(X, y, 3)
    assert not tie
    # below 8 members sklearn's NearestNeighbors switches to brute force, whose rounded radii disagree with its own
    # KD-tree count
    assert np.bincount(y, minlength=C).min() >= 8
    assert m.shape == (d, N) and m.min() >= 3
    for s in (0, 1, 2):
        ref = mutual_info_classif(X, y, discrete_features=False, random_state=s)
        assert np.abs(mi - ref).max() <= 1e-9, (s, mi, ref)


def test_oracle_excludes_singleton_labels():
    X, y = make_inputs(40, 2, 3, 1)
    y = y.copy()
    y[5], y[17] = 100, 101  # two labels that occur once
    mi, m, _ = knn_mi_oracle(X, y, 3)
    keep = np.ones(40, dtype=bool)
    keep[[5, 17]] = False
    mi2, m2, _ = knn_mi_oracle(X[keep], y[keep], 3)
    assert m.shape == (2, 38)
    assert np.array_equal(m, m2) and np.array_equal(mi, mi2)


def _gap_inputs():
    X, y = make_inputs(777, 6, 10, 5)
    return torch.tensor(y), torch.tensor(X[:, :3]), torch.tensor(X[:, 3:])


def test_gap_backend_sklearn_is_the_default(monkeypatch):
    from src.losses import mutual_info_gap

    monkeypatch.delenv("CVHIP_GMIG", raising=False)
    label, c, s = _gap_inputs()
    # tie-free input: sklearn's noise cannot change an integer, so two unseeded calls agree exactly
    assert mutual_info_gap(label, c, s, backend="sklearn") == mutual_info_gap(label, c, s)
    monkeypatch.setenv("CVHIP_GMIG", "sklearn")
    assert mutual_info_gap(label, c, s) == mutual_info_gap(label, c, s, backend="sklearn")


def test_gap_backend_bad_name_raises(monkeypatch):
    from src.losses import mutual_info_gap

    label, c, s = _gap_inputs()
    with pytest.raises(ValueError):
        mutual_info_gap(label, c, s, backend="kdtree")
    monkeypatch.setenv("CVHIP_GMIG", "gpu")
    with pytest.raises(ValueError):
        mutual_info_gap(label, c, s)


def test_gap_backend_device_rejects_cpu_tensors(monkeypatch):
    from src.losses import mutual_info_gap

    label, c, s = _gap_inputs()
    with pytest.raises(ValueError, match="ROCm device"):
        mutual_info_gap(label, c, s, backend="device")
    monkeypatch.setenv("CVHIP_GMIG", "device")
    with pytest.raises(ValueError, match="ROCm device"):
        mutual_info_gap(label, c, s)


def test_digamma_table_on_the_host():
    from scipy.special import digamma

    from cvhip.metrics import digamma_table

    t = digamma_table(10000, "cpu").numpy()
    assert np.abs(t[1:] - digamma(np.arange(1, 10001))).max() <= 1e-10


def test_knn_mi_host_validation():
    """cv_knn_mi rejects bad arguments before anything is enqueued (no GPU needed)."""
    from cvhip import _lib

    L = _lib.lib()
    assert L.cv_knn_mi_workspace_bytes(2, 1) >= 8
    assert L.cv_knn_mi_workspace_bytes(20000, 128) >= 128 * 8
    x = (ctypes.c_float * 8)()
    cls = (ctypes.c_int32 * 4)()
    psi = (ctypes.c_double * 5)()
    out = (ctypes.c_double * 2)()
    work = (ctypes.c_double * 2)()
    a = ctypes.addressof
    good = dict(x=a(x), ldx=2, n=4, d=2, cls=a(cls), k=3, psi=a(psi), m_out=None, out=a(out), work=a(work))

    def rc(**kw):
        v = dict(good, **kw)
        r = L.cv_knn_mi(v["x"], v["ldx"], v["n"], v["d"], v["cls"], v["k"], v["psi"], v["m_out"], v["out"],
                        v["work"], None)
        if r != 0:
            assert b"knn_mi" in L.cv_last_error()
        return r

    for bad in (dict(k=0), dict(k=9), dict(n=1), dict(d=0), dict(ldx=1), dict(x=None), dict(cls=None),
                dict(psi=None), dict(out=None)):
        assert rc(**bad) != 0, bad
