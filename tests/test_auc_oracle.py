"""The rank-count oracle (tests/auc_ref.py) against sklearn's average_precision_score / roc_auc_score, and the
backend switch of src.losses.auc, without a GPU.

The bar against sklearn is 1e-12 absolute: both sides are fp64 evaluations of the same step-wise sum of at most 2000
quotients in [0, 1] (rounding differences of a few 1e-16 per term at worst), far from any modelling difference."""

import math
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, roc_auc_score

from auc_ref import cases, class_stats, make_logits, midpoint_distance, rank_oracle, rare_case, softmax32

TOL = 1e-12
NAMES = ["n2_c2", "n257_c3", "n1025_c2", "n777_c32", "n512_c4_tied", "n600_c10_saturated", "n1000_c10_halves",
         "n500_c2_halves", "rare"]


def _case(name):
    return rare_case() if name == "rare" else cases()[name]


def _sklearn(pos, s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(average_precision_score(pos, s)), float(roc_auc_score(pos, s))


def _same(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_sklearn(name):
    x, y = _case(name)
    ph = softmax32(x)
    ref = rank_oracle(ph, y)
    worst = 0.0
    for k in range(int(y.max()) + 1):
        ap, roc = _sklearn((y == k).astype(np.float32), ph[:, k])
        assert _same(ref["ap"][k], ap, TOL), (k, ref["ap"][k], ap)
        assert _same(ref["auroc"][k], roc, TOL), (k, ref["auroc"][k], roc)
        if not math.isnan(roc):
            worst = max(worst, abs(ref["ap"][k] - ap), abs(ref["auroc"][k] - roc))
    print(name, "max |oracle - sklearn| =", worst)


def test_cases_are_what_they_claim():
    cs = cases()
    P = np.bincount(cs["n777_c32"][1], minlength=32)
    assert P[7] == 0 and P[19] == 1 and (np.delete(P, [7, 19]) > 1).all()
    ph = softmax32(cs["n600_c10_saturated"][0])
    assert (ph == 0.0).any() and (ph == 1.0).any()
    ph = softmax32(cs["n512_c4_tied"][0])
    assert len(np.unique(ph)) == 1
    ph = softmax32(cs["n1000_c10_halves"][0])
    assert len(np.unique(ph[:, 0])) < 1000  # ties within a column
    ph = softmax32(cs["n500_c2_halves"][0])
    assert len(np.unique(ph[:, 0])) < 50  # heavy ties
    y = rare_case()[1]
    assert 10 <= y.sum() <= 30
    assert cs["n5_c1"][1].tolist() == [0] * 5


def test_counts_by_brute_force():
    """The sorted-array oracle equals the definition evaluated pair by pair (small n, heavy ties)."""
    x, y = make_logits(97, 3, 11)
    ph = softmax32(np.round(x * 2) / 2)
    ref = rank_oracle(ph, y)
    for i in range(len(y)):
        k = y[i]
        s, pos = ph[:, k], y == k
        want = [int((s[pos] >= s[i]).sum()), int((s[~pos] >= s[i]).sum()), int((s[~pos] > s[i]).sum())]
        assert ref["counts"][i].tolist() == want


def test_degenerate_classes_follow_the_installed_sklearn():
    s = np.array([0.1, 0.7, 0.7, 0.2, 0.9], dtype=np.float32)
    for pos in (np.zeros(5, dtype=bool), np.ones(5, dtype=bool)):
        ap, roc = _sklearn(pos.astype(np.float32), s)
        st = class_stats(s, pos)
        assert st["ap"] == ap and math.isnan(st["auroc"]) and math.isnan(roc)
    assert class_stats(s, np.zeros(5, dtype=bool))["ap"] == 0.0
    assert class_stats(s, np.ones(5, dtype=bool))["ap"] == 1.0


def test_midpoint_distance():
    assert midpoint_distance(0.9125) < 1e-12 and abs(midpoint_distance(0.912) - 5e-4) < 1e-12
    assert abs(midpoint_distance(0.91249) - 1e-5) < 1e-12


def _dicts_equal(a, b):
    assert len(a) == 2 and len(b) == 2
    for da, db in zip(a, b):
        assert list(da) == list(db)
        for k in da:
            assert _same(float(da[k]), float(db[k]), 0.0), (k, da[k], db[k])


def test_sklearn_backend_is_the_default(monkeypatch):
    from src import losses

    assert losses.AUC_BACKENDS == ("sklearn", "device")
    x, y = cases()["n257_c3"]
    logit, lab = torch.as_tensor(x), torch.as_tensor(y)
    monkeypatch.delenv("CVHIP_AUC", raising=False)
    base = losses.auc(logit, lab)
    assert list(base[0]) == [0, 1, 2]
    # the reference's computation, written out
    ph = softmax32(x)
    for k in range(3):
        ap, roc = _sklearn((y == k).astype(np.float32), ph[:, k])
        assert base[0][k] == round(ap, 3) and base[1][k] == round(roc, 3)
    _dicts_equal(losses.auc(logit, lab, backend="sklearn"), base)
    monkeypatch.setenv("CVHIP_AUC", "sklearn")
    _dicts_equal(losses.auc(logit, lab), base)
    monkeypatch.setenv("CVHIP_AUC", "")
    _dicts_equal(losses.auc(logit, lab), base)


def test_unknown_backend_raises(monkeypatch):
    from src import losses

    x, y = cases()["n257_c3"]
    logit, lab = torch.as_tensor(x), torch.as_tensor(y)
    monkeypatch.setenv("CVHIP_AUC", "gpu")
    with pytest.raises(ValueError, match="unknown backend 'gpu'"):
        losses.auc(logit, lab)
    monkeypatch.delenv("CVHIP_AUC")
    with pytest.raises(ValueError, match="unknown backend"):
        losses.auc(logit, lab, backend="cuda")


def test_device_backend_refuses_cpu_tensors(monkeypatch):
    from src import losses

    x, y = cases()["n257_c3"]
    logit, lab = torch.as_tensor(x), torch.as_tensor(y)
    monkeypatch.delenv("CVHIP_AUC", raising=False)
    with pytest.raises(ValueError, match="ROCm device"):
        losses.auc(logit, lab, backend="device")
    monkeypatch.setenv("CVHIP_AUC", "device")
    with pytest.raises(ValueError, match="ROCm device"):
        losses.auc(logit, lab)
