"""CLUB and VarUB as the CLEAR-MIM estimator against golden fixtures of the real reference
(tests/golden/mim_*.npz, made by tests/golden/gen_golden_mi.py: one real ClearMIMVAETrainer._train step each, fp64):
the module path for the MI value on the reference's own latents, and the fused step (cvhip.engine.ClearStep) for
everything the trainer produces.

The checks and bars are those of tests/test_gpu_golden.py (test_module_outputs_vs_golden, test_fused_step_vs_golden)
for its CLEAR-MIM cases: outputs 1e-4 relative (the MI value with an absolute floor of 1), the five learning losses
at 1e-3, gradients median per-tensor < 5e-4 / worst < 2e-2 on the stored samples, parameters after Adam median
< 1e-5 / worst < 5e-3, BN running statistics 1e-3; the estimator's parameters after its five updates at rel-L2 <
1e-3, the bar the TC discriminator gets there.  The fixtures live outside the vae*.npz glob of
tests/golden_cases.py:names(), whose tests build only the two older estimators."""

import numpy as np
import pytest
import torch

import golden_cases as G
from test_gpu_golden import TOL, _bias_before_bn, _close, _model

pytestmark = pytest.mark.gpu

NAMES = ["mim_club_vae_n64", "mim_varub_vae_n64", "mim_club_vae64_n16"]


def _estimator(fx):
    from oracle import cpu_ref as R
    from src.models import mi_estimator as MI

    m = fx["meta"]
    d = m["z"] // 2
    est = getattr(MI, m["estimator"])(d, d, m["z"]).cuda()
    est.load_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in R.det_mlp(d, m["z"]).items()})
    return est


def test_fixtures_are_the_new_estimators():
    kinds = [G.load(n)["meta"]["estimator"] for n in NAMES]
    assert kinds == ["CLUB", "VarUB", "CLUB"]
    assert not set(NAMES) & set(G.names())


@pytest.mark.parametrize("name", NAMES)
def test_module_mi_vs_golden(name):
    """est(z_c, z_s) on the latents of test_module_outputs_vs_golden (the VAE's train-mode forward with the
    fixture's noise) against the reference's MI value."""
    from cvhip import rng

    fx = G.load(name)
    m = fx["meta"]
    x, label, ec, es, perm = G.inputs(fx)
    vae = _model(fx)
    vae.train()
    X = torch.tensor(x, dtype=torch.float32, device="cuda")
    rng.clear_injections()
    rng.inject_noise([torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)])
    with torch.no_grad():
        xhat, lp, z = vae(X, explicit=True)
    assert G.rel(z.cpu().numpy(), fx["z"]) < TOL
    est = _estimator(fx)
    d = m["z"] // 2
    with torch.no_grad():
        mi = est(z[:, :d], z[:, d:])
    assert abs(float(mi) - float(fx["mi"])) <= TOL * max(abs(float(fx["mi"])), 1.0), (float(mi), float(fx["mi"]))


def _build_fused(fx):
    """The fixture's trainer and fused engine with the case's noise queued (and a permutation: the engine's
    injected programs take one whatever the estimator, as for L1OutUB)."""
    from cvhip import rng
    from cvhip.engine import ClearStep
    from src.trainer import ClearMIMVAETrainer

    m = fx["meta"]
    x, label, ec, es, perm = G.inputs(fx)
    hp = G.hyper(fx)
    vae = _model(fx)
    opt = torch.optim.Adam(vae.parameters(), lr=hp["lr"])
    est = _estimator(fx)
    eopt = torch.optim.Adam(est.parameters(), lr=hp["est_lr"])
    tr = ClearMIMVAETrainer(vae, est, {"vae_optim": opt, "mi_estimator_optim": eopt}, m["sim_fn"], hp, 1,
                            torch.device("cuda"))
    eng = ClearStep.build(tr, "mim")
    assert eng is not None, "ClearStep.build refused " + m["estimator"]
    rng.clear_injections()
    noise = [torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)]
    for a, b in fx["extra_noise"]:
        noise += [torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)]
    rng.inject_perm([torch.tensor(perm)])
    rng.inject_noise(noise)
    return tr, eng, est


@pytest.mark.parametrize("name", NAMES)
def test_fused_mim_step_vs_golden(name):
    fx = G.load(name)
    m = fx["meta"]
    arch = m["arch"]
    x, label, ec, es, perm = G.inputs(fx)
    hp = G.hyper(fx)
    tr, eng, est = _build_fused(fx)
    X = torch.tensor(x, dtype=torch.float32, device="cuda")
    losses, learn = eng.step(X, torch.tensor(label, device="cuda"))
    losses = losses.clone().cpu()
    torch.cuda.synchronize()
    for i, k in ((0, "rec"), (1, "kl_c"), (2, "kl_s"), (3, "c_loss")):
        assert _close(losses[i], fx[k]), (k, float(losses[i]), float(fx[k]))
    assert abs(float(losses[5]) - float(fx["mi"])) <= TOL * max(abs(float(fx["mi"])), 1.0), (float(losses[5]),
                                                                                             float(fx["mi"]))
    ll = learn.cpu().numpy()
    assert np.allclose(ll, fx["mi_learning"], rtol=1e-3, atol=1e-3), (ll, fx["mi_learning"])
    # gradients (the arena the Adam kernel consumed) on the stored samples
    rels = []
    lr = hp["lr"]
    for k, p in tr.model.named_parameters():
        g = p.grad.detach().double().cpu().numpy()
        ours, ref = G.pick(fx, "grad__", k, g)
        if _bias_before_bn(k, arch):
            assert np.abs(ours).max() == 0.0, k
            continue
        rels.append((G.rel(ours, ref), k))
    rels.sort()
    print(name, "grad median", rels[len(rels) // 2], "worst", rels[-1])
    assert rels[len(rels) // 2][0] < 5e-4, rels[-3:]
    assert rels[-1][0] < 2e-2, rels[-3:]
    # parameters after the trainer's Adam step
    prels = []
    for k, p in tr.model.named_parameters():
        ours, ref = G.pick(fx, "after__", k, p.detach().double().cpu().numpy())
        if _bias_before_bn(k, arch):
            assert np.abs(ours - ref).max() <= 2.5 * lr, k
            continue
        prels.append((G.rel(ours, ref), k))
    prels.sort()
    assert prels[len(prels) // 2][0] < 1e-5, prels[-3:]
    assert prels[-1][0] < 5e-3, prels[-3:]
    # BatchNorm running statistics after the step's six train-mode forwards
    for k, v in tr.model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert G.rel(v.double().cpu().numpy(), fx["buf__" + k]) < 1e-3, k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(fx["buf__" + k]), k
    # the estimator after its five learning steps
    erels = [(G.rel(p.detach().double().cpu().numpy(), fx["est_after__" + k]), k) for k, p in est.named_parameters()]
    print(name, "estimator after", max(erels))
    assert max(erels)[0] < 1e-3, sorted(erels)[-3:]
