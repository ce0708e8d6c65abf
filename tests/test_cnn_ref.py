"""tests/cnn_ref.py against PyTorch on the CPU: the numpy fp64 restatement of the classifier tail against fp64 modules
and autograd (1e-12 relative: fp64 against fp64, the same formulae), and the seed rule on the seeds the GPU tests
use."""

import numpy as np
import pytest

import cnn_ref as CR

SHAPES = [(5, 20, 3), (2, 16, 2), (37, 130, 7)]

# (arch, n_class, in_channel, n) -> the seeds tests/test_gpu_cnn_trainer.py uses (re-scanned with
# cnn_ref.qualifying_seeds over 0..23: [2, 3, 4, 7, 11], [12], [18])
MODEL_SEEDS = {
    ("SimpleCNNClassifier", 10, 1, 16): 2,
    ("SimpleCNNClassifier", 7, 3, 50): 12,
    ("SimpleCNN64Classifier", 4, 3, 8): 18,
}


@pytest.mark.parametrize("shape", SHAPES, ids=[CR.shape_id(s) for s in SHAPES])
def test_tail_restatement_matches_autograd(shape):
    inp, ref = CR.tail_case(shape)
    assert ref["margin"] >= CR.MASK_MARGIN
    tor = CR.tail_torch(inp)
    for k in ("loss", "logits", "w2", "b2", "gamma", "beta", "da", "rm", "rv"):
        err = CR.rel_l2(ref[k], tor[k])
        assert err <= 1e-12, (k, err)
    assert tor["nbt"] == CR.NBT0 + 1
    assert CR.rel_l2(CR.tail_eval(inp), tor["eval"]) <= 1e-12


def test_fp32_restatement_is_close_but_not_equal():
    """The fp32 restatement (which sizes the n = 2 bound of the GPU test) is the same formulae in fp32."""
    inp, ref = CR.tail_case((37, 130, 7))
    r32 = CR.tail_step(inp, dtype=np.float32)
    assert r32["da"].dtype == np.float32
    for k in ("loss", "w2", "b2", "gamma", "beta", "da", "rm", "rv"):
        err = CR.rel_l2(r32[k], ref[k])
        assert 0 < err < 1e-5, (k, err)


@pytest.mark.parametrize("case", list(MODEL_SEEDS), ids=[f"{c[0]}-c{c[1]}-ch{c[2]}-n{c[3]}" for c in MODEL_SEEDS])
def test_seed_rule_on_the_model_seeds(case):
    seed = MODEL_SEEDS[case]
    arch, n_class, in_ch, n = case
    _, _, margin, r64, _ = CR.model_case(arch, n_class, in_ch, n, seed)
    assert margin >= CR.MASK_MARGIN, (case, seed, margin)
    assert set(CR.ZERO_GRAD_BIASES[arch]) <= set(r64[3])
    # the biases feeding a train-mode BatchNorm: their fp64 gradient is rounding noise around zero
    for k in CR.ZERO_GRAD_BIASES[arch]:
        assert float(r64[3][k].abs().max()) < 1e-12, k


def test_seed_rule_rejects_a_seed():
    """The rule is a real condition: among seeds 0..5 of the n = 50 case none qualifies."""
    assert CR.qualifying_seeds("SimpleCNNClassifier", 7, 3, 50, seeds=range(6)) == []
