"""cv_rank_auc / cvhip.metrics.rank_counts / cvhip.metrics.auc on the device against the NumPy oracle (tests/auc_ref.py)
and against the sklearn backend of src.losses.auc.

The bars, the same for every case:
  counts, P, U2   exact integers
  AP              |ap_sum / P - oracle AP| <= n * 2^-52.  Per side: P correctly rounded fp64 quotients <= 1 (at most
                  2^-53 each) and fewer than P additions of partial sums <= P (at most P * 2^-53 each), so the sum
                  is off by at most (P + P * P) * 2^-53 and the mean by (1 + P) * 2^-53 <= n * 2^-53 (with N = 0
                  every term is exactly 1 and the sum exact); two sides: n * 2^-52
  AUROC           bit-equal to U2 / (2 P N) evaluated in fp64 (both operands are exact integers below 2^53)
  sklearn         1e-12 on the unrounded values (tests/test_auc_oracle.py); the rounded dicts entry by entry
The scores every side sees are torch's fp32 softmax computed on the device (copied to the host for the oracle)."""

import functools
import math
import warnings

import numpy as np
import pytest
import torch
from sklearn.exceptions import UndefinedMetricWarning
from sklearn.metrics import average_precision_score, roc_auc_score

from auc_ref import cases, midpoint_distance, rank_oracle, rare_case

pytestmark = pytest.mark.gpu

NAMES = ["n2_c2", "n5_c1", "n257_c3", "n1025_c2", "n777_c32", "n512_c4_tied", "n600_c10_saturated",
         "n1000_c10_halves", "n500_c2_halves", "rare"]
DEGENERATE = {"n5_c1", "n777_c32"}  # a class without negatives; a class without positives
SK_TOL = 1e-12
MIDPOINT_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits fp32 [n, c] on the device, labels int64 on the device, softmax on the host, labels on the host, oracle),
    computed once per case and shared; nothing here is written to afterwards."""
    x, y = rare_case() if name == "rare" else cases()[name]
    logit, lab = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    ph = logit.softmax(dim=1)
    ph_h = ph.cpu().numpy()
    return logit, lab, ph, ph_h, y, rank_oracle(ph_h, y)


def _same(a, b, tol=0.0):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_counts_and_sums_match_the_oracle(name):
    from cvhip import metrics

    _, lab, ph, _, y, ref = case(name)
    n, c = ph.shape
    P, ap_sum, u2, counts = metrics.rank_counts(ph, lab, return_counts=True)
    assert P.dtype == torch.int64 and u2.dtype == torch.int64 and ap_sum.dtype == torch.float64
    assert P.shape == u2.shape == ap_sum.shape == (c,) and counts.shape == (n, 3)
    assert P.is_cuda and ap_sum.is_cuda and u2.is_cuda and counts.is_cuda
    counts = counts.cpu().numpy().astype(np.int64)
    bad = np.argwhere(counts != ref["counts"])
    assert bad.size == 0, (len(bad), bad[:5], counts[bad[0][0]], ref["counts"][bad[0][0]])
    assert P.cpu().tolist() == ref["P"].tolist()
    assert u2.cpu().tolist() == ref["u2"].tolist()
    ap_sum = ap_sum.cpu().numpy()
    worst = 0.0
    for k in range(c):
        p, neg = int(ref["P"][k]), n - int(ref["P"][k])
        if p == 0:
            assert ap_sum[k] == 0.0
            continue
        err = abs(ap_sum[k] / p - (ref["ap_sum"][k] / p))
        worst = max(worst, err)
        assert err <= n * 2.0 ** -52, (k, err)
        if neg:
            got = float(np.float64(int(u2[k])) / np.float64(2 * p * neg))
            assert got == ref["auroc"][k]
    print(name, "max |ap - oracle| =", worst, "bound", n * 2.0 ** -52)
    # without the counts the same launch, the same values
    P2, ap2, u22 = metrics.rank_counts(ph, lab)
    assert torch.equal(P2, P) and torch.equal(u22, u2) and np.array_equal(ap2.cpu().numpy(), ap_sum)


@pytest.mark.parametrize("name", NAMES)
def test_values_and_dicts_match_sklearn(name):
    """Unrounded: 1e-12 against sklearn's two functions on the same scores.  Rounded: every entry of both dicts equals
    the "sklearn" backend's; the inputs are chosen so that no fp64 reference value lies within 1e-9 of a 3-decimal
    rounding midpoint (asserted here, on the reference side), so 1e-12 cannot change a rounded digit."""
    from cvhip import metrics
    from src import losses

    logit, lab, _, ph_h, y, ref = case(name)
    c = int(y.max()) + 1
    aupr, auroc = _quiet(metrics.auc_values, logit, lab)
    assert len(aupr) == len(auroc) == c
    for k in range(c):
        pos = (y == k).astype(np.float32)
        sk_ap = float(_quiet(average_precision_score, pos, ph_h[:, k]))
        sk_roc = float(_quiet(roc_auc_score, pos, ph_h[:, k]))
        for v in (sk_ap, sk_roc):
            assert math.isnan(v) or midpoint_distance(v) > MIDPOINT_MARGIN, (name, k, v)
        assert _same(aupr[k], sk_ap, SK_TOL), (k, aupr[k], sk_ap)
        assert _same(auroc[k], sk_roc, SK_TOL), (k, auroc[k], sk_roc)
        assert _same(auroc[k], float(ref["auroc"][k])), (k, auroc[k], ref["auroc"][k])
    dev = _quiet(losses.auc, logit, lab, backend="device")
    sk = _quiet(losses.auc, logit, lab, backend="sklearn")
    for d, s in zip(dev, sk):
        assert list(d) == list(s) == list(range(c))
        for k in range(c):
            assert isinstance(d[k], float)
            assert _same(d[k], float(s[k])), (name, k, d[k], s[k])
            assert math.isnan(d[k]) or d[k] == round(d[k], 3)


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_classes_warn_and_match_sklearn(name):
    from src import losses

    logit, lab, _, _, y, ref = case(name)
    with pytest.warns(UndefinedMetricWarning):
        aupr, auroc = losses.auc(logit, lab, backend="device")
    with pytest.warns(UndefinedMetricWarning):
        sk_aupr, sk_auroc = losses.auc(logit, lab, backend="sklearn")
    P = np.bincount(y, minlength=len(aupr))
    hit = 0
    for k in range(len(aupr)):
        if P[k] == 0 or P[k] == len(y):
            hit += 1
            assert aupr[k] == (0.0 if P[k] == 0 else 1.0) == sk_aupr[k]
            assert math.isnan(auroc[k]) and math.isnan(sk_auroc[k])
        else:
            assert not math.isnan(auroc[k])
    assert hit == 1


def test_a_clean_input_does_not_warn():
    from src import losses

    logit, lab = case("n257_c3")[:2]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        losses.auc(logit, lab, backend="device")


def test_strided_view_is_bit_identical_to_its_contiguous_copy():
    from cvhip import metrics

    _, lab, ph, _, _, _ = case("n777_c32")
    wide = torch.cat([ph, torch.full_like(ph[:, :5], 2.0)], dim=1)
    view = wide[:, :32]
    assert not view.is_contiguous() and view.stride(0) == 37
    a = metrics.rank_counts(view, lab, return_counts=True)
    b = metrics.rank_counts(view.contiguous(), lab, return_counts=True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    # a column stride other than 1 is made contiguous by the wrapper
    t = ph.t().contiguous().t()
    assert t.stride(1) != 1
    for s, u in zip(metrics.rank_counts(t, lab), b[:3]):
        assert torch.equal(s, u)
    # logits wider than the labels' range: auc scores the first y.max() + 1 columns of the full softmax
    logit, lab3 = case("n257_c3")[:2]
    wide_logit = torch.cat([logit, logit[:, :2] - 3.0], dim=1)
    got = metrics.auc_values(wide_logit, lab3)
    ph5 = wide_logit.softmax(dim=1)
    P, ap_sum, u2 = metrics.rank_counts(ph5[:, :3].contiguous(), lab3)
    assert len(got[0]) == 3
    assert got[0] == [a / p for a, p in zip(ap_sum.tolist(), P.tolist())]


@pytest.mark.parametrize("name", ["n1025_c2", "n777_c32"])
def test_two_calls_are_bit_identical(name):
    from cvhip import metrics

    _, lab, ph, _, _, _ = case(name)
    a = metrics.rank_counts(ph, lab, return_counts=True)
    b = metrics.rank_counts(ph, lab, return_counts=True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    logit = case(name)[0]
    assert repr(_quiet(metrics.auc, logit, lab)) == repr(_quiet(metrics.auc, logit, lab))


def test_bad_inputs_raise_before_any_launch(monkeypatch):
    from cvhip import _lib, metrics

    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    logit, lab = case("n257_c3")[:2]
    nan_logit = logit.clone()
    nan_logit[100, 1] = float("nan")
    neg = lab.clone()
    neg[5] = -1
    with pytest.raises(ValueError, match="NaN or infinity"):
        metrics.auc(nan_logit, lab)
    with pytest.raises(ValueError, match="negative label"):
        metrics.auc(logit, neg)
    with pytest.raises(ValueError, match="256 labels for 257 rows"):
        metrics.auc(logit, lab[:256])
    with pytest.raises(ValueError, match="float32"):
        metrics.auc(logit.double(), lab)
    with pytest.raises(ValueError, match="integer tensor"):
        metrics.auc(logit, lab.float())
    with pytest.raises(ValueError, match="ROCm device"):
        metrics.auc(logit.cpu(), lab)
    with pytest.raises(ValueError, match="no column"):
        metrics.auc(logit[:, :2], lab)
    assert launched == []
    metrics.auc(logit, lab.cpu())  # labels on the host are moved
    assert launched == ["cv_rank_auc"]


def _loader(n_cls, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(2):
        X = torch.rand(16, 1, 28, 28, generator=g).cuda()
        y = ((torch.arange(16) + b) % n_cls).reshape(-1, 1)
        out.append((X, y))
    return out


def _mlp_trainer():
    from src.models.vae import VAE
    from src.trainer import DownstreamMLPTrainer

    torch.manual_seed(3)
    vae = VAE(16, 1).cuda().eval()
    mlp = torch.nn.Sequential(torch.nn.Linear(8, 32), torch.nn.BatchNorm1d(32), torch.nn.ReLU(),
                              torch.nn.Linear(32, 4)).cuda()
    opt = torch.optim.Adam(mlp.parameters(), lr=1e-3)
    tr = DownstreamMLPTrainer(vae, mlp, opt, torch.nn.CrossEntropyLoss(), 10, torch.device("cuda"), backend="torch")
    return tr, lambda X: tr.model(tr.vae.encode(X)[0])


def _cnn_trainer():
    from src.models.cnn import SimpleCNNClassifier
    from src.trainer import SimpleCNNTrainer

    torch.manual_seed(4)
    model = SimpleCNNClassifier(n_class=4, in_channel=1).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    tr = SimpleCNNTrainer(model, opt, torch.nn.CrossEntropyLoss(), 10, torch.device("cuda"), backend="torch")
    return tr, lambda X: tr.model(X)


@pytest.mark.parametrize("make", [_mlp_trainer, _cnn_trainer], ids=["DownstreamMLPTrainer", "SimpleCNNTrainer"])
def test_evaluate_follows_the_environment_switch(make, monkeypatch):
    """With CVHIP_AUC=device a trainer's evaluate() returns exactly cvhip.metrics.auc of its own concatenated logits
    and labels; with the variable unset, the sklearn dicts of them.  The logits are observed where the trainer hands
    them to auc (the PyTorch convolutions may pick another algorithm on a repeated forward, so a forward repeated
    here is compared to rounding, not to the bit)."""
    from cvhip import metrics
    from src import losses
    from src import trainer as trainer_mod

    tr, forward = make()
    dl = _loader(4, 5)
    handed, device_calls = [], []
    real = metrics.auc
    assert trainer_mod.auc is losses.auc
    monkeypatch.setattr(trainer_mod, "auc", lambda logit, y: (handed.append((logit, y)), losses.auc(logit, y))[1])
    monkeypatch.setattr(metrics, "auc", lambda logit, y: (device_calls.append((logit, y)), real(logit, y))[1])

    monkeypatch.setenv("CVHIP_AUC", "device")
    (aupr, auroc), acc = tr.evaluate(dl, False, 0)
    assert len(handed) == 1 and len(device_calls) == 1
    logits, ys = handed[0]
    assert device_calls[0][0] is logits and device_calls[0][1] is ys
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.shape == (32, 4) and ys.shape == (32,)
    tr.model.eval()
    with torch.no_grad():
        again = torch.cat([forward(X) for X, _ in dl])
    assert torch.allclose(again, logits, rtol=1e-4, atol=1e-5)
    assert torch.equal(ys.cpu(), torch.cat([y.reshape(-1) for _, y in dl]))
    assert (aupr, auroc) == real(logits, ys)
    assert list(aupr) == list(auroc) == [0, 1, 2, 3]
    assert all(isinstance(v, float) and not math.isnan(v) for v in list(aupr.values()) + list(auroc.values()))
    assert float(acc) == float(losses.accurary(logits, ys))

    monkeypatch.delenv("CVHIP_AUC")
    (aupr_s, auroc_s), _ = tr.evaluate(dl, False, 0)
    assert len(handed) == 2 and len(device_calls) == 1  # the device backend was not called
    assert (aupr_s, auroc_s) == losses.auc(*handed[1], backend="sklearn")
