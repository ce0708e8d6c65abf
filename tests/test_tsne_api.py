"""cvhip.tsne without a device: every ValueError that is raised before anything is uploaded or launched, and the
"auto" learning rate."""

import numpy as np
import pytest
import torch


def _x(n=40, d=5):
    return np.random.default_rng(0).normal(size=(n, d)).astype(np.float32)


def test_functional_entries_reject_cpu_tensors():
    from cvhip import tsne

    x = torch.as_tensor(_x())
    v, y = torch.ones(40), torch.zeros(40, 2)
    with pytest.raises(ValueError, match="ROCm device"):
        tsne.affinities(x, 10.0)
    with pytest.raises(ValueError, match="ROCm device"):
        tsne.kl_grad(x, v, v, y)
    with pytest.raises(ValueError, match="ROCm device"):
        tsne.descend(x, v, v, y, 3)
    with pytest.raises(ValueError, match="ROCm device"):
        tsne.TSNE(perplexity=10).fit(x)
    with pytest.raises(ValueError, match="ROCm device"):
        tsne.affinities(_x(), 10.0)  # not a tensor at all


@pytest.mark.parametrize("kw,X,match", [
    (dict(n_components=3), _x(), "n_components"),
    (dict(), _x(40, 65), r"1\.\.64"),
    (dict(), np.zeros((40, 0), np.float32), r"1\.\.64"),
    (dict(perplexity=1.0), _x(1, 5), r"2\.\.65536"),
    (dict(perplexity=40), _x(), "perplexity"),
    (dict(perplexity=41.5), _x(), "perplexity"),
    (dict(perplexity=0), _x(), "perplexity"),
    (dict(perplexity=-3), _x(), "perplexity"),
    (dict(perplexity=10), _x().astype(np.int32), "floating-point"),
    (dict(perplexity=10), _x()[0], "2-D"),
    (dict(perplexity=10), torch.as_tensor(_x()).double(), "float32"),
    (dict(perplexity=10, init=np.zeros((40, 3))), _x(), r"shape \(40, 2\)"),
    (dict(perplexity=10, init=np.zeros((39, 2))), _x(), r"shape \(40, 2\)"),
    (dict(perplexity=10, init="spectral"), _x(), "init"),
    (dict(perplexity=10, learning_rate="fast"), _x(), "learning_rate"),
    (dict(perplexity=10, learning_rate=0.0), _x(), "learning_rate"),
    (dict(perplexity=10, early_exaggeration=0.0), _x(), "early_exaggeration"),
    (dict(perplexity=10, max_iter=-1), _x(), "max_iter"),
])
def test_tsne_rejects_before_any_upload(kw, X, match, monkeypatch):
    from cvhip import _lib, tsne

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match=match):
        tsne.TSNE(**kw).fit(X)


def test_row_count_limit():
    from cvhip import tsne

    class Big:  # 65537 rows without the memory
        shape, ndim, dtype = (65537, 4), 2, np.dtype(np.float32)

    with pytest.raises(ValueError, match=r"2\.\.65536"):
        tsne.TSNE()._check_params(*Big.shape)
    assert tsne.MAX_N == 65536 and tsne.MAX_D == 64


def test_auto_learning_rate():
    from cvhip import tsne

    assert tsne.auto_learning_rate(10000) == max(10000 / 12.0 / 4.0, 50.0) == pytest.approx(208.3333333333)
    assert tsne.auto_learning_rate(192) == 50.0
    assert tsne.auto_learning_rate(65536, 4.0) == 4096.0
    t = tsne.TSNE(perplexity=10)
    assert t.learning_rate == "auto" and t._check_params(40, 5) == 50.0
    assert tsne.TSNE(perplexity=10, early_exaggeration=2.0)._check_params(4000, 5) == 500.0
    assert tsne.TSNE(perplexity=10, learning_rate=200)._check_params(40, 5) == 200.0


def test_c_entry_points_refuse_bad_sizes_without_a_launch():
    """Host-side validation of the four cv_tsne_* calls: every one is rejected before anything is enqueued, so the
    (never dereferenced) pointers may be anything non-null."""
    from cvhip import _lib

    L = _lib.lib()
    p = 4096  # stands for any non-null pointer
    for n, d, ldx, perplexity, word in [(1, 4, 4, 0.5, b"n must be"), (65537, 4, 4, 30.0, b"n must be"),
                                        (100, 0, 4, 30.0, b"1..64"), (100, 65, 65, 30.0, b"1..64"),
                                        (100, 8, 7, 30.0, b"row stride"), (100, 8, 8, 100.0, b"perplexity"),
                                        (100, 8, 8, 0.0, b"perplexity"), (100, 8, 8, float("nan"), b"perplexity")]:
        assert L.cv_tsne_affinity(p, ldx, n, d, perplexity, p, p, None) != 0
        assert word in L.cv_last_error(), (n, d, ldx, perplexity, L.cv_last_error())
    assert L.cv_tsne_affinity(None, 8, 100, 8, 30.0, p, p, None) != 0 and b"must be given" in L.cv_last_error()
    assert L.cv_tsne_pair(p, 8, 100, 65, p, p, p, 1.0, 0, p, None) != 0 and b"1..64" in L.cv_last_error()
    assert L.cv_tsne_pair(p, 8, 100, 8, p, p, p, 0.0, 0, p, None) != 0 and b"exaggeration" in L.cv_last_error()
    assert L.cv_tsne_pair(p, 8, 100, 8, p, p, p, 1.0, 0, None, None) != 0 and b"must be given" in L.cv_last_error()
    assert L.cv_tsne_update(1, p, p, p, p, 0.5, 200.0, 0, None, None, None) != 0 and b"n must be" in L.cv_last_error()
    assert L.cv_tsne_update(100, p, p, None, p, 0.5, 200.0, 0, None, None, None) != 0
    assert b"update and gains" in L.cv_last_error()
    assert L.cv_tsne_update(100, p, None, None, None, 0.5, 200.0, 0, None, None, None) != 0
    assert b"nothing to do" in L.cv_last_error()
    assert L.cv_tsne_run(p, 8, 100, 8, p, p, p, p, p, -1, 250, 12.0, 200.0, p, None, None) != 0
    assert b"negative" in L.cv_last_error()
    assert L.cv_tsne_run(p, 8, 100, 8, p, p, p, None, p, 10, 250, 12.0, 200.0, p, None, None) != 0
    assert b"must be given" in L.cv_last_error()
    # the workspace: 7 fp64 partials per (slab, row) and 3 per tile of 256 rows; the slab count depends on n alone
    assert L.cv_tsne_workspace_bytes(1) == 0 and L.cv_tsne_workspace_bytes(65537) == 0
    assert L.cv_tsne_workspace_bytes(4) == (7 * 1 * 4 + 3) * 8
    assert L.cv_tsne_workspace_bytes(257) == (7 * 5 * 257 + 2 * 3) * 8
    assert L.cv_tsne_workspace_bytes(10000) == (7 * 25 * 10000 + 40 * 3) * 8
    assert L.cv_tsne_workspace_bytes(65536) == (7 * 4 * 65536 + 256 * 3) * 8


def test_defaults_are_the_notebooks_call():
    from cvhip import tsne

    t = tsne.TSNE(n_components=2, perplexity=30, learning_rate=200, init="pca")
    assert (t.n_components, t.perplexity, t.learning_rate, t.init) == (2, 30, 200, "pca")
    assert (t.early_exaggeration, t.max_iter, t.exploration_iter, t.random_state) == (12.0, 1000, 250, None)
    with pytest.raises(TypeError):
        tsne.TSNE(2, 30.0)  # keyword-only after n_components, as in sklearn
