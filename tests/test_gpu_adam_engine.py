"""The optimizer inside the fused step (cvhip/engine.py _AdamState, ClearStep) against the fp64 reference of
tests/adam_ref.py: torch.optim.Adam with non-default betas, eps and weight decay (hyper set B) that has already
taken steps when the engine adopts it, six engine steps (the first eager, the rest replayed from the step graph) and
a learning rate changed between two replays.  Smallest fused configuration: VAE, z = 16, 28 x 28, n = 32, CLEAR-VAE.

The check is independent of whether the step's gradients are right (tests/test_gpu_parity.py and others check
those): after every step arena.grad still holds what the Adam launch consumed, and the reference applies
torch.optim.Adam's update to exactly those gradients, from the state the engine adopted, at t = 4, 5, ...  Tolerance:
the rule of tests/test_gpu_adam.py (adam_ref.Case: 8 x the error of the fp32 restatement, one ulp at least).

Measured on an MI355X, largest over the 6 steps (p in units of the step's lr, m in |g|, v in g^2; the kernel may use
8 x e32): e32 p 5.1e-4, m 1.1e-7, v 2.9e-7; the engine, with ADAM_PACK on and off alike, p 5.1e-4, m 1.1e-7, v 2.9e-7
(p: 9.6e-5 before the learning rate drops by 4 x at step 5, which re-expresses the accumulated error in the smaller
unit)."""

import numpy as np
import pytest
import torch

import adam_ref as AR

pytestmark = pytest.mark.gpu

N, WARM_STEPS, STEPS, NEW_LR = 32, 3, 6, 5e-4


def _run(adam_pack):
    from oracle import cpu_ref as R
    from cvhip import engine, rng
    from cvhip.engine import ClearStep
    from test_gpu_parity import _fused_trainer

    prev = engine.ADAM_PACK
    engine.ADAM_PACK = adam_pack
    try:
        torch.manual_seed(977)
        rng.clear_injections()
        rng.reset_counters()
        sd = R.det_state("VAE", 16, 1)
        x, label, _, _, _ = R.det_inputs(N, 1, 28, 16, 4)
        hp = {"temperature": 0.1, "beta": 1 / 32, "loc": 0, "scale": 1, "alpha": 100.0, "ps": True}
        lr, b1, b2, eps, wd = AR.HYPER_B
        tr = _fused_trainer("VAE", 16, 1, sd, hp, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        opt, params = tr.optimizer, list(tr.model.parameters())
        # warm start: torch.optim.Adam itself, three steps on random gradients, before the engine exists
        gen = torch.Generator(device="cuda").manual_seed(5)
        for _ in range(WARM_STEPS):
            for p in params:
                p.grad = 0.01 * torch.randn(p.shape, device="cuda", generator=gen)
            opt.step()
        torch.cuda.synchronize()
        adopted = {id(p): (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                   for p in params}
        assert all(float(opt.state[p]["step"]) == WARM_STEPS and bool(opt.state[p]["exp_avg_sq"].any())
                   for p in params)
        eng = ClearStep.build(tr, "clear")
        assert eng is not None and eng.adam_pack == adam_pack
        A, ad = eng.arena, eng.adam
        for p in params:
            o, n = A.offset[id(p)]
            w, m, v = adopted[id(p)]
            assert torch.equal(A.flat[o:o + n], w.reshape(-1)) and torch.equal(ad.m[o:o + n], m.reshape(-1))
            assert torch.equal(ad.v[o:o + n], v.reshape(-1))
            st = opt.state[p]  # (bound to the flat state: what a checkpoint of the optimizer would save)
            assert st["exp_avg"].data_ptr() == ad.m.data_ptr() + 4 * o and float(st["step"]) == WARM_STEPS
        assert ad.step.tolist() == [WARM_STEPS, 0]

        X = torch.tensor(x, dtype=torch.float32, device="cuda")
        L = torch.tensor(label, device="cuda")
        host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        before, after, grads, rows = [], [], [], []
        for k in range(STEPS):
            if k == 4:  # between steps 4 and 5: a scheduler's write, picked up by refresh_hyper before the replay
                opt.param_groups[0]["lr"] = NEW_LR
            rows.append((opt.param_groups[0]["lr"], b1, b2, eps, wd))
            torch.cuda.synchronize()
            before.append((host(A.flat), host(ad.m), host(ad.v)))
            eng.step(X, L)
            torch.cuda.synchronize()
            grads.append(host(A.grad))
            after.append((host(A.flat), host(ad.m), host(ad.v)))
            assert ad.step.tolist() == [WARM_STEPS + k + 1, 0], (k, ad.step.tolist())
        assert "graphs" in eng.graphs[N]  # (steps 2 .. 6 were replays)
        eng.sync_host_state()
        assert all(float(opt.state[p]["step"]) == WARM_STEPS + STEPS for p in params)
        return dict(before=before, after=after, grads=grads, rows=rows)
    finally:
        engine.ADAM_PACK = prev


@pytest.mark.parametrize("adam_pack", [True, False], ids=["pack", "plain"])
def test_engine_adam_trajectory(adam_pack):
    r = _run(adam_pack)
    assert [row[0] for row in r["rows"]] == [AR.HYPER_B[0]] * 4 + [NEW_LR] * 2
    for k in range(1, STEPS):  # nothing but the step's own Adam launch moves the state
        for a, b in zip(r["before"][k], r["after"][k - 1]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), k
    grads = np.stack(r["grads"])
    assert np.isfinite(grads).all() and all(np.abs(g).max() > 0 for g in grads)
    case = AR.Case(*r["before"][0], grads, np.array(r["rows"]), WARM_STEPS)
    for k in range(STEPS):
        err, ok = case.errors(k, *r["after"][k])
        print(f"ADAMERR engine[{'pack' if adam_pack else 'plain'}] step {k}: kernel p {err[0]:.3g} m {err[1]:.3g}"
              f" v {err[2]:.3g} | e32 p {case.e32_p[k]:.3g} m {case.e32_m[k]:.3g} v {case.e32_v[k]:.3g}")
        assert ok, (k, err, (case.e32_p[k], case.e32_m[k], case.e32_v[k]))
    # the changed learning rate is visible at this tolerance: the old one misses step 5
    stale = AR.Case(*r["before"][0], grads, AR.HYPER_B, WARM_STEPS)
    assert stale.errors(3, *r["after"][3])[1] and not stale.errors(4, *r["after"][4])[1]
