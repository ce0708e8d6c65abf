"""tests/tsne_ref.py (the fp64 restatement the device t-SNE is tested against) held against sklearn's own private
functions: _joint_probabilities, _kl_divergence and _gradient_descent of sklearn.manifold._t_sne.

Bars (the agreement measured with sklearn 1.7.2 in brackets):
  P          1e-6 of max P   [6e-8: sklearn rounds the distances to fp32]
  KL         1e-12           [1e-15]
  descent    1e-10 of max|Y| after 5 iterations [1e-13] and over the two-phase schedule, 2 + 4 and 3 + 5 [2e-14]
  5 points, two of them identical, perplexity 2: P to 1e-12 [1e-15]"""

import numpy as np
import pytest

import tsne_ref as R

sk = pytest.importorskip("sklearn.manifold._t_sne")
if not all(hasattr(sk, f) for f in ("_joint_probabilities", "_kl_divergence", "_gradient_descent")):
    pytest.skip("this sklearn has no _t_sne._joint_probabilities / _kl_divergence / _gradient_descent",
                allow_module_level=True)


def _condensed(M):
    return M[np.triu_indices(len(M), 1)]


def _case():
    X, _ = R.three_clusters()
    D = R.sqdist(X)
    beta, logz, H, conv = R.search_beta(X, 30.0, D)
    assert conv.all()
    return X, D, R.joint_P(X, beta, logz, D)


CASE = None


def case():
    global CASE
    if CASE is None:
        CASE = _case()
    return CASE


def test_joint_P_matches_sklearn():
    X, D, P = case()
    sk_P = sk._joint_probabilities(D.astype(np.float32), 30.0, 0)
    err = np.abs(_condensed(P) - sk_P).max() / sk_P.max()
    print("P: max error / max P =", err)
    assert err <= 1e-6
    assert abs(P.sum() - 1.0) <= 1e-4 and np.array_equal(P, P.T)


def test_joint_P_with_identical_rows():
    X = np.random.default_rng(3).normal(size=(5, 3)).astype(np.float32)
    X[4] = X[1]
    D32 = R.sqdist(X).astype(np.float32)  # both sides see the rounded distances here: what is left is the algorithm
    D = D32.astype(np.float64)
    assert D[1, 4] == 0.0
    beta, logz, H, conv = R.search_beta(X, 2.0, D)
    P = R.joint_P(X, beta, logz, D)
    sk_P = sk._joint_probabilities(D32, 2.0, 0)
    err = np.abs(_condensed(P) - sk_P).max()
    print("5 points: max P error =", err, "converged rows", int(conv.sum()))
    assert err <= 1e-12


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_kl_and_gradient_match_sklearn(exaggeration):
    X, D, P = case()
    Y = np.random.default_rng(5).normal(size=(len(X), 2)) * 3.0
    kl, grad = R.kl_grad(P, Y, exaggeration)
    sk_kl, sk_grad = sk._kl_divergence(Y.ravel().copy(), exaggeration * _condensed(P), 1.0, len(X), 2)
    print("KL", kl, sk_kl, "grad error", np.abs(grad.ravel() - sk_grad).max() / np.abs(sk_grad).max())
    assert abs(kl - sk_kl) <= 1e-12 * max(1.0, abs(sk_kl))
    assert np.abs(grad.ravel() - sk_grad).max() <= 1e-12 * np.abs(sk_grad).max()
    assert R.kl_grad(P, Y, exaggeration, with_kl=False)[0] is None


def _sk_descent(P, Y0, it, max_iter, momentum, exaggeration):
    n = len(Y0)
    p, _, last = sk._gradient_descent(sk._kl_divergence, Y0.ravel().copy(), it, max_iter, n_iter_check=10 ** 6,
                                      n_iter_without_progress=10 ** 6, momentum=momentum, learning_rate=200.0,
                                      min_grad_norm=0.0, args=[exaggeration * _condensed(P), 1.0, n, 2], kwargs={})
    assert last == max_iter - 1
    return p.reshape(n, 2)


def test_descent_matches_sklearn():
    X, D, P = case()
    Y0 = R.pca_init(X)
    got = R.descend(P, Y0, 5)
    ref = _sk_descent(P, Y0, 0, 5, 0.5, 12.0)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("5 iterations: error / max|Y| =", err)
    assert err <= 1e-10


@pytest.mark.parametrize("first,second", [(2, 4), (3, 5)])
def test_two_phase_schedule_matches_sklearn(first, second):
    """sklearn starts a second _gradient_descent at the switch: update and gains start afresh there."""
    X, D, P = case()
    Y0 = R.pca_init(X)
    got = R.descend(P, Y0, first + second, exploration_iter=first)
    mid = _sk_descent(P, Y0, 0, first, 0.5, 12.0)
    ref = _sk_descent(P, mid, first, first + second, 0.8, 1.0)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(first, "+", second, "iterations: error / max|Y| =", err)
    assert err <= 1e-10


def test_pca_init_matches_sklearn():
    from sklearn.decomposition import PCA

    X, _, _ = case()
    ref = PCA(n_components=2, svd_solver="full").fit_transform(X.astype(np.float64))
    ref = ref / np.std(ref[:, 0]) * 1e-4
    got = R.pca_init(X)
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
    assert abs(np.std(got[:, 0]) - 1e-4) <= 1e-15
    assert np.array_equal(R.pca_init(X[:, :1])[:, 1], np.zeros(len(X)))


@pytest.mark.parametrize("name", ["min", "n257", "n257_p5", "d64", "d20", "n1000", "dups", "scaled_up", "scaled_down",
                                  "clusters"])
def test_the_search_converges_on_every_row_of_the_device_cases(name):
    X, perplexity = R.case(name)
    beta, logz, H, conv = R.search_beta(X, perplexity)
    assert conv.all(), np.flatnonzero(~conv)
    assert np.abs(H - np.log(perplexity)).max() <= 1e-5
