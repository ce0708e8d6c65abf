"""cv_knn_mi / cvhip.metrics on the device against the NumPy oracle (tests/knn_mi_oracle.py).

The bars are the same for every case: the int32 neighbour counts m equal the oracle's exactly, and mi is within 1e-9
absolute (fp64 sums of at most 1e4 terms of magnitude at most 12, plus the cumulative-sum digamma table, itself
compared with scipy at 1e-10)."""

import functools

import numpy as np
import pytest
import torch

from knn_mi_oracle import kept_mask, knn_mi_oracle, make_inputs

pytestmark = pytest.mark.gpu

MI_TOL = 1e-9


def _quarters():
    """n=300, d=3: column 0 in multiples of 1/4, column 1 of 1/64, column 2 constant (heavy value and distance ties)."""
    X, y = make_inputs(300, 3, 5, 11)
    X = X.copy()
    X[:, 0] = np.round(X[:, 0] * 4) / 4
    X[:, 1] = np.round(X[:, 1] * 64) / 64
    X[:, 2] = 0.75
    return X, y


def _singletons():
    """n=64, d=4: three labels that occur once and one label of size 2 among four larger classes."""
    X, y = make_inputs(64, 4, 4, 3)
    y = y.copy()
    y[[7, 30, 63]] = [50, 51, 52]
    y[[0, 41]] = 60
    return X, y


def _wide():
    """n=300 (two tiles of points) x 2100 features (more than one resident round of workgroups): four distinct
    columns repeated, so both the tile and the feature loops of a workgroup take more than one trip."""
    X, y = make_inputs(300, 4, 6, 13)
    return np.tile(X, (1, 525)), y


@functools.lru_cache(maxsize=None)
def case(name):
    """(X fp32 [n, d], y, k, oracle mi, oracle m, radius_tie), computed once per case and shared."""
    k = 3
    if name == "min":
        X, y = np.array([[0.5], [-1.25]], dtype=np.float32), np.array([3, 3])
    elif name == "five":
        X, y = make_inputs(5, 3, 2, 2)
        y = np.array([0, 1, 1, 0, 1])
    elif name == "singletons":
        X, y = _singletons()
    elif name == "n257":
        X, y = make_inputs(257, 5, 10, 4)
    elif name == "n257_k1":
        X, y = make_inputs(257, 5, 10, 4)
        k = 1
    elif name == "n257_k5":
        X, y = make_inputs(257, 5, 10, 4)
        k = 5
    elif name == "ties":
        X, y = _quarters()
    elif name == "n512":
        X, y = make_inputs(512, 4, 4, 0)
    elif name == "n777":
        X, y = make_inputs(777, 6, 10, 5)
    elif name == "n4096":
        X, y = make_inputs(4096, 2, 7, 6)
    elif name == "wide":
        X, y = _wide()
        mi, m, tie = knn_mi_oracle(X[:, :4], y, k)
        return X, y, k, np.tile(mi, 525), np.tile(m, (525, 1)), tie
    else:
        raise KeyError(name)
    mi, m, tie = knn_mi_oracle(X, y, k)
    return X, y, k, mi, m, tie


def device_mi(X, y, k, **kw):
    from cvhip import metrics

    return metrics.knn_mi(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), n_neighbors=k, **kw)


def test_digamma_table_matches_scipy():
    from scipy.special import digamma

    from cvhip.metrics import digamma_table

    t = digamma_table(10000, "cuda").cpu().numpy()
    assert np.abs(t[1:] - digamma(np.arange(1, 10001))).max() <= 1e-10


@pytest.mark.parametrize("name", ["min", "five", "singletons", "n257", "n257_k1", "n257_k5", "ties", "n512", "n777",
                                  "n4096", "wide"])
def test_counts_and_mi_match_the_oracle(name):
    X, y, k, mi_ref, m_ref, _ = case(name)
    mi, m, kept = device_mi(X, y, k, return_counts=True)
    assert mi.dtype == torch.float64 and mi.shape == (X.shape[1],) and mi.is_cuda
    assert m.dtype == torch.int32
    assert np.array_equal(kept.cpu().numpy(), kept_mask(y))
    m = m.cpu().numpy()
    assert m.shape == m_ref.shape
    bad = np.argwhere(m != m_ref)
    assert bad.size == 0, (len(bad), bad[:5], m[tuple(bad[0])], m_ref[tuple(bad[0])])
    mi = mi.cpu().numpy()
    assert np.isfinite(mi).all()
    err = np.abs(mi - mi_ref).max()
    print(name, "max |mi - oracle| =", err)
    assert err <= MI_TOL
    # without the counts the same launch, the same value
    assert torch.equal(device_mi(X, y, k).cpu(), torch.as_tensor(mi))


def test_case_shapes_are_what_they_claim():
    assert case("min")[4].tolist() == [[1, 1]]  # k_i = 1, the one neighbour is the radius: nothing below it
    y = case("five")[1]
    assert sorted(np.bincount(y).tolist()) == [2, 3]
    y = case("singletons")[1]
    assert (np.bincount(y) == 1).sum() == 3 and (np.bincount(y) == 2).sum() == 1
    assert case("singletons")[4].shape == (4, 61)
    assert case("ties")[5] and not case("n512")[5] and not case("n777")[5]


@pytest.mark.parametrize("name", ["n512", "n777"])
def test_tie_free_inputs_match_sklearn(name):
    from sklearn.feature_selection import mutual_info_classif

    X, y, k, _, _, tie = case(name)
    assert not tie
    ref = mutual_info_classif(X, y, discrete_features=False, random_state=0)
    mi = device_mi(X, y, k).cpu().numpy()
    assert np.abs(mi - ref).max() <= MI_TOL


def test_strided_views_are_bit_identical_to_contiguous_copies():
    from cvhip import metrics

    X, y, k, mi_ref, _, _ = case("n777")
    zd = 3
    z = torch.as_tensor(X).cuda()
    assert z.shape[1] == 2 * zd
    lab = torch.as_tensor(y).cuda()
    for view, ref in ((z[:, :zd], mi_ref[:zd]), (z[:, zd:], mi_ref[zd:])):
        assert not view.is_contiguous()
        a, ma, _ = metrics.knn_mi(view, lab, k, return_counts=True)
        b, mb, _ = metrics.knn_mi(view.contiguous(), lab, k, return_counts=True)
        assert torch.equal(a, b) and torch.equal(ma, mb)
        assert np.abs(a.cpu().numpy() - ref).max() <= MI_TOL
    # a column stride other than 1 is made contiguous by the wrapper
    t = z.t().contiguous().t()
    assert t.stride(1) != 1
    assert torch.equal(metrics.knn_mi(t, lab, k), metrics.knn_mi(z, lab, k))


def test_two_calls_are_bit_identical():
    X, y, k, _, _, _ = case("n4096")
    a, ma, _ = device_mi(X, y, k, return_counts=True)
    b, mb, _ = device_mi(X, y, k, return_counts=True)
    assert torch.equal(a, b) and torch.equal(ma, mb)


def test_all_labels_unique_raises():
    from cvhip import metrics

    x = torch.randn(16, 2, device="cuda")
    with pytest.raises(ValueError, match="fewer than two"):
        metrics.knn_mi(x, torch.arange(16, device="cuda"))
    with pytest.raises(ValueError, match="ROCm device"):
        metrics.knn_mi(x.cpu(), torch.zeros(16, dtype=torch.long))
    with pytest.raises(ValueError):
        metrics.knn_mi(x, torch.zeros(16, dtype=torch.long, device="cuda"), n_neighbors=9)


def _gap_tensors():
    X, y = case("n777")[:2]
    z = torch.as_tensor(X).cuda()
    return torch.as_tensor(y).cuda(), z[:, :3], z[:, 3:]


def test_gap_device_backend_matches_sklearn_backend(monkeypatch):
    from src.losses import mutual_info_gap

    monkeypatch.delenv("CVHIP_GMIG", raising=False)
    label, c, s = _gap_tensors()
    ref = float(mutual_info_gap(label, c, s, backend="sklearn"))
    dev = mutual_info_gap(label, c, s, backend="device")
    assert isinstance(dev, float)
    # the only difference is the reference's fp32 label entropy
    print("gMIG sklearn", ref, "device", dev)
    assert abs(dev - ref) <= 1e-5 * max(1.0, abs(ref))
    monkeypatch.setenv("CVHIP_GMIG", "device")
    assert mutual_info_gap(label, c, s) == dev


def test_evaluate_follows_the_environment_switch(monkeypatch):
    """CLEARVAETrainer.evaluate with CVHIP_GMIG=device returns cvhip.metrics.gmig of the latents its own eval
    forward produced (the reparameterisation noise injected, so the forward can be repeated here)."""
    from cvhip import metrics, rng
    from oracle import cpu_ref as R
    from src.utils.trainer_utils import get_clearvae_trainer

    torch.manual_seed(0)
    tr = get_clearvae_trainer(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=8, alpha=100, temperature=0.1, device="cuda")
    zd = tr.model.z_dim
    x, label, _, _, _ = R.det_inputs(256, 1, 28, 8, 10)
    ds = torch.utils.data.TensorDataset(torch.tensor(x, dtype=torch.float32), torch.tensor(label))
    dl = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    g = np.random.default_rng(21)
    noise = [torch.tensor(g.standard_normal((128, zd)), dtype=torch.float32) for _ in range(4)]

    monkeypatch.setenv("CVHIP_GMIG", "device")
    rng.clear_injections()
    rng.inject_noise([t.clone() for t in noise])
    mig, _ = tr.evaluate(dl, False, 0)
    assert rng.pending_noise() == 0
    assert isinstance(mig, float) and np.isfinite(mig)

    rng.inject_noise([t.clone() for t in noise])
    tr.model.eval()
    zs, labs = [], []
    with torch.no_grad():
        for X, lab in dl:
            zs.append(tr.model(X.cuda(), explicit=True)[2])
            labs.append(lab.cuda())
    rng.clear_injections()
    z, lab = torch.cat(zs), torch.cat(labs)
    assert mig == metrics.gmig(lab, z[:, :zd], z[:, zd:])
