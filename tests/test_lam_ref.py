"""The LAM references against each other on the CPU (tests/lam_ref.py): the numpy tail against torch fp64 autograd of
the one-forward form, the one-forward form of a whole step against the literal three-forward step of
LAMCNNTrainer._train, and the seed rule at the model seeds the GPU tests use."""

import copy

import numpy as np
import pytest
import torch

import cnn_ref as CR
import lam_ref as LR

TAILS = [((5, 8, 9, 3), "fixed"), ((37, 12, 16, 7), "absent"), ((6, 4, 1, 2), "cross"), ((16, 16, 4, 5), "shuffle")]
CASES = list(LR.MODEL_SEEDS)
IDS = [f"{c[0]}-c{c[1]}-ch{c[2]}-n{c[3]}" for c in CASES]


@pytest.mark.parametrize("shape,kind", TAILS, ids=[f"{LR.shape_id(s)}-{k}" for s, k in TAILS])
@pytest.mark.parametrize("lam", [0.1, 8.0])
def test_numpy_tail_matches_torch_autograd(shape, kind, lam):
    inp = LR.tail_case(shape, kind)
    ref, tt = LR.tail_step(inp, lam), LR.tail_torch(inp, lam)
    for k in ("ce", "lam", "gw", "gb", "gin", "gs1", "gs2", "logits"):
        assert LR.rel_l2(ref[k], tt[k]) <= 1e-12, (k, LR.rel_l2(ref[k], tt[k]))
    label, pair = inp["label"], inp["pair"]
    assert sorted(pair.tolist()) == list(range(shape[0]))
    if kind == "cross":
        assert (label[pair] != label).any()
    else:
        assert (label[pair] == label).all()
    if kind == "fixed":
        assert (pair == np.arange(shape[0])).any() and (pair != np.arange(shape[0])).any()
    if kind == "absent":
        assert shape[3] - 1 not in label


def test_identity_pair_has_no_lam_term():
    inp = LR.tail_case((5, 8, 9, 3), "fixed")
    ident = np.arange(5)
    a, b = LR.tail_step(inp, 0.7, pair=ident), LR.tail_step(inp, 0.0)
    assert a["lam"] == 0.0
    for k in ("ce", "gw", "gb", "gin", "gs1", "gs2"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_forward_form_is_the_literal_step(case):
    arch, n_class, in_ch, n = case
    seed = LR.MODEL_SEEDS[case]
    model0, (X, y), pair, margin, r64, _ = LR.model_case(arch, n_class, in_ch, n, seed)
    assert margin >= LR.MASK_MARGIN, margin  # the seed rule
    assert sorted(pair.tolist()) == list(range(n)) and bool((y[pair] == y).all())
    m3, _, l3, g3 = r64
    m1, l1, g1 = LR.one_forward_step(model0, X, y, pair, 1.0)
    assert abs(l1[0] - l3[0][0]) <= 1e-12 * abs(l3[0][0]) and abs(l1[1] - l3[0][1]) <= 1e-12 * abs(l3[0][1])
    zero = LR.ZERO_GRAD_BIASES[arch]
    for k, g in g3.items():
        if k in zero:  # (mathematically zero: rounding noise on both sides)
            assert float(g.abs().max()) <= 1e-12 and float(g1[k].abs().max()) <= 1e-12, k
        else:
            assert LR.rel_l2(g1[k], g) <= 1e-12, (k, LR.rel_l2(g1[k], g))
    sd1, sd3, sd0 = m1.state_dict(), m3.state_dict(), model0.state_dict()
    for k, v in sd3.items():
        if "num_batches" in k:
            assert int(v) == int(sd1[k]) == int(sd0[k]) + 3, k
        elif "running_" in k:
            assert LR.rel_l2(sd1[k], v) <= 1e-12, (k, LR.rel_l2(sd1[k], v))
    print(f"LAMREF {IDS[CASES.index(case)]} seed {seed}: margin {margin:.3g}, "
          f"{int((pair == torch.arange(n)).sum())} fixed points")


def test_permuted_batch_gives_permuted_features():
    """The identity the one-forward form rests on: net(X[pair]) = net(X)[pair] in train mode."""
    case = CASES[0]
    model0, (X, y), pair, *_ = LR.model_case(*case, LR.MODEL_SEEDS[case])
    m = copy.deepcopy(model0).double().train()
    with torch.no_grad():
        a, b = m.net(X.double())[pair], m.net(X.double()[pair])
    assert CR.rel_l2(b, a) <= 1e-12
