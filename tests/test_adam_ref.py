"""The Adam reference of the kernel tests (tests/adam_ref.py) against torch.optim.Adam itself, and the tolerance
rule of tests/test_gpu_adam.py pinned on the reference alone: every wrong restatement of the update (MUTANTS) must
miss the rule by a wide margin, so a kernel that carried one of them could not pass.  CPU only.

Figures (N = 4099, after 12 steps; e32 = error of the fp32 restatement of p against fp64; the tolerance is 8 x e32):
  set A, t0 = 0:      e32 1.3e-4 lr, smallest mutant error 0.84 lr (bc_one_step_behind)
  set A, t0 = 7:      e32 1.2e-4 lr, smallest mutant error 0.10 lr (bc_one_step_behind)
  set A, t0 = 100000: e32 1.5e-4 lr, smallest mutant error 15 lr (beta1_in_v_decay)
  set B, t0 = 0:      e32 3.2e-5 lr, smallest mutant error 0.18 lr (eps_before_bc2)
  set B, t0 = 7:      e32 2.7e-5 lr, smallest mutant error 0.054 lr (eps_before_bc2)
  set B, t0 = 100000: e32 3.5e-5 lr, smallest mutant error 6.3 lr (beta1_in_v_decay)
The bias corrections tend to 1, so a mutant that only moves them fades with t: at t0 = 100000 (beta^t underflows)
those are the reference itself and only the other mutants are checked there."""

import numpy as np
import pytest
import torch

import adam_ref as AR

N = 4099


def _torch_adam(case, hyper_set):
    """torch.optim.Adam on fp64 CPU tensors from the case's (widened) fp32 inputs; state after every step."""
    hyper, scale = AR.SETS[hyper_set]
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in hyper)
    p = torch.tensor(case.p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    if case.t0:
        opt.state[p] = {"step": torch.tensor(float(case.t0)), "exp_avg": torch.tensor(case.m0.astype(np.float64)),
                        "exp_avg_sq": torch.tensor(case.v0.astype(np.float64))}
    out = []
    for k in range(case.steps):
        p.grad = torch.tensor(case.g[k].astype(np.float64) * float(np.float32(scale)))
        opt.step()
        st = opt.state[p]
        assert float(st["step"]) == case.t0 + k + 1
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


@pytest.mark.parametrize("hyper_set", ["A", "B"])
@pytest.mark.parametrize("t0", [0, 7])
def test_reference_is_torch_adam(hyper_set, t0):
    case = AR.make_case(N, hyper_set, t0)
    assert (t0 == 0) == (not case.m0.any() and not case.v0.any())
    got = _torch_adam(case, hyper_set)
    gm = case.gmag
    for k, (p, m, v) in enumerate(got):
        assert np.abs(p - case.P[k]).max() <= 1e-12 * np.abs(case.P[k]).max(), k
        assert (np.abs(m - case.M[k]) <= 1e-12 * gm).all(), k
        assert (np.abs(v - case.V[k]) <= 1e-12 * gm * gm).all(), k


def _mutants_of(hyper_set, t0):
    # without weight decay / with grad_scale = 1 the two mutants that drop them are the reference itself; with the
    # bias corrections at 1 (t0 = 100000: beta^t underflows) so are the mutants that only move those
    ms = [m for m in AR.MUTANTS if hyper_set == "B" or m not in ("weight_decay_ignored", "grad_scale_ignored")]
    if t0 >= 100000:
        ms = [m for m in ms if m not in ("bc_one_step_behind", "no_bc2", "eps_before_bc2")]
    return ms


@pytest.mark.parametrize("hyper_set", ["A", "B"])
@pytest.mark.parametrize("t0", [0, 7, 100000])
def test_tolerance_rule_rejects_every_mutant(hyper_set, t0):
    case = AR.make_case(N, hyper_set, t0)
    hyper, scale = AR.SETS[hyper_set]
    last = case.steps - 1
    lr = case.lr[last]
    # the condition of the rule: 8 x e32 of p stays below 0.02 lr at every step
    print(f"set {hyper_set} t0 {t0}: e32 p {case.e32_p.max():.3g} m {case.e32_m.max():.3g} v {case.e32_v.max():.3g}")
    assert (AR.TOL_FACTOR * case.e32_p < 0.02).all(), case.e32_p
    tol = AR.TOL_FACTOR * case.e32_p[last] * lr
    for mutant in _mutants_of(hyper_set, t0):
        Pm, Mm, Vm = AR.adam_ref(case.p0, case.m0, case.v0, case.g, hyper, t0, scale, mutant=mutant)
        err = np.abs(Pm[last] - case.P[last]).max()
        print(f"  {mutant}: {err / lr:.3g} lr, tolerance {tol / lr:.3g} lr")
        assert err >= 10 * tol, (mutant, err / lr, tol / lr)
        # ... and an element outside its own tolerance (ulp floor included) fails the kernel check
        assert not case.errors(last, Pm[last], case.M[last], case.V[last])[1], mutant


@pytest.mark.parametrize("numel", [4, 1027, 3077])
@pytest.mark.parametrize("hyper_set", ["A", "B"])
@pytest.mark.parametrize("t0", [0, 7, 100000])
def test_tolerance_condition_at_the_kernel_test_shapes(numel, hyper_set, t0):
    """The cv_adam_step cases of tests/test_gpu_adam.py: 8 x e32 of p below 0.02 lr at every step there too, and the
    fp32 restatement inside its own rule."""
    case = AR.make_case(numel, hyper_set, t0)
    assert (AR.TOL_FACTOR * case.e32_p < 0.02).all(), case.e32_p
    hyper, scale = AR.SETS[hyper_set]
    r32 = AR.adam_ref(case.p0, case.m0, case.v0, case.g, hyper, t0, scale, dtype=np.float32)
    assert all(case.errors(k, r32[0][k], r32[1][k], r32[2][k])[1] for k in range(case.steps))


@pytest.mark.parametrize("hyper_set", ["A", "B"])
def test_first_step_cannot_see_a_late_bias_correction(hyper_set):
    """At t = 1 the one-step-behind mutant is the reference bit for bit (its correction is taken from step 1 in both),
    and with zero moments the update is lr g / (|g| + eps) whatever the betas are: why the first-step parity tests
    pass for an optimizer that is wrong from step 2 on."""
    case = AR.make_case(N, hyper_set, 0)
    hyper, scale = AR.SETS[hyper_set]
    Pm, Mm, Vm = AR.adam_ref(case.p0, case.m0, case.v0, case.g, hyper, 0, scale, mutant="bc_one_step_behind")
    assert np.array_equal(Pm[0], case.P[0]) and np.array_equal(Mm[0], case.M[0]) and np.array_equal(Vm[0], case.V[0])
    assert not np.array_equal(Pm[1], case.P[1])
    other = (hyper[0], 0.5, 0.7) + tuple(hyper[3:])
    Po, _, _ = AR.adam_ref(case.p0, case.m0, case.v0, case.g[:1], other, 0, scale)
    assert np.abs(Po[0] - case.P[0]).max() <= 1e-9 * case.lr[0]


def test_fp32_restatement_and_inputs():
    """The inputs are what the kernel tests promise: an exactly-zero block, elements of ~1e15, no square that
    overflows fp32; the reference keeps the zero block's parameters (no weight decay) and moments untouched."""
    case = AR.make_case(N, "A", 0)
    z0, z1 = AR.zero_block(N)
    assert not case.g[:, z0:z1].any() and z1 - z0 >= 8
    big = np.abs(case.g[:, AR.huge_elements(N)])
    assert big.min() > 1e14 and np.isfinite(big.astype(np.float32) ** 2).all()
    mag = np.abs(case.g[:, [i for i in range(N) if not z0 <= i < z1]])
    assert mag.min() >= 1e-9 * 0.999 and (mag == mag[0]).all()
    assert (case.P[:, z0:z1] == case.p0[z0:z1]).all() and not case.M[:, z0:z1].any() and not case.V[:, z0:z1].any()
    # the per-step learning rate of a changed schedule is taken row by row
    rows = np.array([AR.HYPER_A] * 3 + [(1e-3,) + AR.HYPER_A[1:]] * 2)
    a = AR.adam_ref(case.p0, case.m0, case.v0, case.g[:5], rows, 0)[0]
    b = AR.adam_ref(case.p0, case.m0, case.v0, case.g[:3], AR.HYPER_A, 0)
    c = AR.adam_ref(b[0][-1], b[1][-1], b[2][-1], case.g[3:5], rows[4], 3)[0]
    assert np.array_equal(a[:3], b[0])
    # (b's state passes through fp32 on the way into c: equal to fp32 rounding of the parameters)
    assert np.abs(a[4] - c[1]).max() <= 1e-6


def test_adam_state_supported():
    """_AdamState.supported: what the fused step's Adam kernels implement, and nothing else."""
    from cvhip.engine import _AdamState

    ps = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]
    Adam, sup = torch.optim.Adam, _AdamState.supported
    assert sup(Adam(ps, lr=1e-3), ps)
    assert sup(Adam(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01), ps)
    assert not sup(Adam(ps, amsgrad=True), ps)
    assert not sup(Adam(ps, maximize=True), ps)
    assert not sup(Adam([{"params": ps[:1]}, {"params": ps[1:]}]), ps)
    assert not sup(Adam(ps, lr=torch.tensor(1e-3)), ps)
    assert not sup(torch.optim.AdamW(ps), ps)
    assert not sup(Adam(ps[:1]), ps)
    assert not sup(Adam(ps), ps[:1])
    assert not sup(Adam(ps), [ps[0], torch.nn.Parameter(torch.zeros(5))])
