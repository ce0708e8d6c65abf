"""The fused one-graph training step of CLEARVAETrainer with a SupCon loss_name (hyperparameter["loss_step"] =
"fused": cvhip.engine.ClearStep with cv_supcon_step in its latent program) against an fp64 oracle step on the
deterministic state, inputs and noise of oracle.cpu_ref.

The oracle step is oracle.cpu_ref.clear_step (reference trainer.py:452-482) restated with its two contrastive terms
taken from the torch composition of src/losses.py in fp64 on the CPU (contrastive_loss(..., backend="torch"), the
reference of tests/test_gpu_supcon.py).  Bars: tests/test_gpu_parity.py's — LOSS_TOL on the five losses, _check_grads
on the pre-Adam gradients, parameters after Adam against torch Adam on the oracle gradients (median < 1e-5, worst
< 5e-3).  Bit-identity checks follow tests/test_gpu_determinism.py."""

import pytest
import torch

from test_gpu_parity import LOSS_TOL, _bias_before_bn, _check_grads, _model, _rel

pytestmark = pytest.mark.gpu

LOSSES = ("supcon_in_loss", "supcon_out_loss")
NAMES = ("rec", "kl_c", "kl_s", "c_loss", "s_loss")


def _hp(ps, loss_name=None, loss_step=None, **kw):
    hp = {"temperature": 0.1, "alpha": 100.0, "beta": 0.125, "ps": ps, "loc": 0, "scale": 1}
    if loss_name is not None:
        hp["loss_name"] = loss_name
    if loss_step is not None:
        hp["loss_step"] = loss_step
    hp.update(kw)
    return hp


def _trainer(arch, zt, C, sd, hp, sim="cosine", lr=5e-4):
    from src.trainer import CLEARVAETrainer

    vae = _model(arch, zt, C, sd)
    opt = torch.optim.Adam(vae.parameters(), lr=lr)
    return CLEARVAETrainer(vae, opt, sim, hp, 1, torch.device("cuda"))


def _oracle_step(sd, x, label, ec, es, arch, hp, sim, loss_name):
    """cpu_ref.clear_step with the SupCon composition for its two contrastive terms, fp64."""
    from oracle import cpu_ref as R
    from src.losses import contrastive_loss

    P = R.to_torch(sd)
    x, label, ec, es = torch.tensor(x), torch.tensor(label), torch.tensor(ec), torch.tensor(es)
    xhat, lp, z = R.vae_forward(P, x, ec, es, arch, True)
    rec, kl_c, kl_s = R.vae_loss(xhat, x, lp["mu_c"], lp["mu_s"], lp["logvar_c"], lp["logvar_s"])
    c = contrastive_loss(lp["mu_c"], lp["logvar_c"], label, sim, hp["temperature"], loss_name=loss_name,
                         backend="torch")
    s = contrastive_loss(lp["mu_s"], lp["logvar_s"], label, sim, hp["temperature"], loss_name=loss_name, ps=hp["ps"],
                         backend="torch")
    if not hp["ps"]:
        s = -s
    w = R.anneal_weight(0, hp["beta"], hp.get("loc", 0), hp.get("scale", 1))
    loss = rec + w * kl_c + w * kl_s + hp["alpha"] * c + hp["alpha"] * s
    params = {k: v for k, v in P.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    return {"rec": rec, "kl_c": kl_c, "kl_s": kl_s, "c_loss": c, "s_loss": s, "grads": dict(zip(params, grads))}


_ORACLE = {}


def _oracle(arch, zt, n, sim, ps, loss_name):
    """The oracle step of a case, computed once and shared by the fused and the module-path test."""
    from oracle import cpu_ref as R

    key = (arch, zt, n, sim, ps, loss_name)
    if key not in _ORACLE:
        C = 1 if arch == "VAE" else 3
        sd = R.det_state(arch, zt, C)
        x, label, ec, es, _ = R.det_inputs(n, C, R.IMAGE[arch], zt, 10)
        _ORACLE[key] = (sd, x, label, ec, es, _oracle_step(sd, x, label, ec, es, arch, _hp(ps), sim, loss_name))
    return _ORACLE[key]


def _check_losses(got, o, ps):
    """got: rec, kl_c, kl_s, c and the style term before its sign (the oracle's s_loss is negated when not ps)."""
    vals = dict(zip(NAMES, got))
    vals["s_loss"] = vals["s_loss"] if ps else -vals["s_loss"]
    for k, v in vals.items():
        ref = float(o[k])
        print(f"SUPCON_FUSED {k} dev={v:.7g} ref={ref:.7g} e={abs(v - ref) / max(abs(ref), 1e-3):.3g}")
        assert abs(v - ref) <= LOSS_TOL * max(abs(ref), 1e-3), (k, v, ref)


CASES = [("VAE", 16, 64, "cosine", True), ("VAE", 16, 50, "cosine", False), ("VAE", 16, 48, "jeffrey", True),
         ("VAE64", 64, 16, "cosine", True)]
IDS = [f"{c[0]}-n{c[2]}-{c[3]}-ps{int(c[4])}" for c in CASES]


# ----------------------------------------------------------------------------- 1. one fused step vs the oracle step


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("arch,zt,n,sim,ps", CASES, ids=IDS)
def test_fused_supcon_step(arch, zt, n, sim, ps, loss_name):
    from oracle import cpu_ref as R
    from cvhip import rng
    from cvhip.engine import ClearStep

    sd, x, label, ec, es, o = _oracle(arch, zt, n, sim, ps, loss_name)
    C = 1 if arch == "VAE" else 3
    tr = _trainer(arch, zt, C, sd, _hp(ps, loss_name, "fused"), sim)
    eng = tr._fused()
    assert isinstance(eng, ClearStep) and eng.supcon is not None
    rng.clear_injections()
    rng.inject_noise([torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)])
    losses = eng.step(torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda"))
    losses = losses.clone().cpu()
    torch.cuda.synchronize()
    _check_losses([float(v) for v in losses[:5]], o, ps)  # (losses[4] is the style term before its sign)
    _check_grads({k: p.grad for k, p in tr.model.named_parameters()}, o["grads"], arch)
    P0 = R.to_torch(sd, requires_grad=False)
    names = list(o["grads"])
    ref_params = [P0[k].clone().requires_grad_(True) for k in names]
    for p_, k in zip(ref_params, names):
        g = o["grads"][k]
        p_.grad = torch.zeros_like(g) if _bias_before_bn(k, arch) else g.clone()
    torch.optim.Adam(ref_params, lr=5e-4).step()
    cur = dict(tr.model.named_parameters())
    prel = sorted((_rel(cur[k], p_), k) for p_, k in zip(ref_params, names))
    assert prel[len(prel) // 2][0] < 1e-5, prel[-3:]
    assert prel[-1][0] < 5e-3, prel[-3:]
    eng.sync_host_state()
    st = tr.optimizer.state[cur["encoder.0.weight"]]
    assert int(float(st["step"])) == 1 and st["exp_avg"].data_ptr() >= eng.adam.m.data_ptr()


# ----------------------------------------------------------------------------- 2. the module path is the default


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("arch,zt,n,sim,ps", CASES[:2], ids=IDS[:2])
def test_module_path_is_still_the_default(arch, zt, n, sim, ps, loss_name, monkeypatch):
    """No loss_step: no engine is built, and one module-path step's losses meet the same oracle bars."""
    from cvhip import rng

    monkeypatch.delenv("CVHIP_SUPCON_STEP", raising=False)
    sd, x, label, ec, es, o = _oracle(arch, zt, n, sim, ps, loss_name)
    tr = _trainer(arch, zt, 1, sd, _hp(ps, loss_name), sim)
    assert tr._fused() is None and tr._engine is None
    rng.clear_injections()
    rng.inject_noise([torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)])
    from src import trainer as T

    seen = []  # what _train's vae_loss and two contrastive_loss calls returned, in call order

    def recording(fn):
        def call(*a, **k):
            seen.append(fn(*a, **k))
            return seen[-1]
        return call

    monkeypatch.setattr(T, "contrastive_loss", recording(T.contrastive_loss))
    monkeypatch.setattr(T, "vae_loss", recording(T.vae_loss))
    ds = torch.utils.data.TensorDataset(torch.tensor(x, dtype=torch.float32), torch.tensor(label))
    tr._train(torch.utils.data.DataLoader(ds, batch_size=n, shuffle=False), False, 0)
    assert tr._engine is None
    (rec, kl_c, kl_s), c, s = seen
    _check_losses([float(rec), float(kl_c), float(kl_s), float(c), float(s)], o, ps)


# ----------------------------------------------------------------------------- 3. replays are bit-identical


def _replays(arch, zt, C, hw, n, hp, reps=4):
    """tests/test_gpu_determinism.py::_replays for a CLEARVAETrainer built from `hp`."""
    from oracle import cpu_ref as R
    from cvhip import rng

    rng.clear_injections()
    sd = R.det_state(arch, zt, C)
    x, label, _, _, _ = R.det_inputs(n, C, hw, zt, 4)
    tr = _trainer(arch, zt, C, sd, hp, lr=3e-5)
    eng = tr._fused()
    assert eng is not None
    X = torch.tensor(x, dtype=torch.float32, device="cuda")
    L = torch.tensor(label, device="cuda")
    for _ in range(3):  # (eager, capture, replay)
        eng.step(X, L)
    torch.cuda.synchronize()

    def state():
        return ([eng.arena.flat, eng.adam.m, eng.adam.v, eng.adam.step, eng.anneal, eng.offset]
                + [b for _, b in tr.model.named_buffers()])

    snap = [t.clone() for t in state()]
    outs = []
    for _ in range(reps):
        for t, s in zip(state(), snap):
            t.copy_(s)
        torch.cuda.synchronize()
        lo = eng.step(X, L)
        torch.cuda.synchronize()
        ws = eng.graphs[n]["ws"]
        outs.append(dict(losses=lo.clone(), flat=eng.arena.flat.clone(), grad=eng.arena.grad.clone(),
                         dheads=ws.dheads.clone(), dz=ws.dz.clone(),
                         bufs=torch.cat([b.double().reshape(-1) for _, b in tr.model.named_buffers()])))
    assert "graphs" in eng.graphs[n]
    return outs


def _same_bits(a, b):
    # (losses may hold NaN-free floats only here; compared as bits all the same)
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


@pytest.mark.parametrize("arch,zt,C,hw,n", [("VAE", 16, 1, 28, 64), ("VAE64", 64, 3, 64, 16)])
def test_step_replays_are_bit_identical(arch, zt, C, hw, n):
    """The snn_loss step first, as the control: if it fails too, the cause is not the SupCon step."""
    for loss_name in (None,) + LOSSES:
        outs = _replays(arch, zt, C, hw, n, _hp(True, loss_name, "fused" if loss_name else None))
        for k in outs[0]:
            for o in outs[1:]:
                assert _same_bits(outs[0][k], o[k]), (loss_name or "snn_loss", k,
                                                      float((outs[0][k].double() - o[k].double()).abs().max()))


# ----------------------------------------------------------------------------- 4. graph replay == eager


@pytest.mark.parametrize("loss_name", LOSSES)
def test_graph_replay_is_the_eager_step(loss_name):
    """Steps 1-3 of one engine (eager, capture, replay) and three eager steps of a second engine from the same state
    and the same Philox counters: the same losses and parameters, bit for bit."""
    from oracle import cpu_ref as R
    from cvhip import rng

    arch, zt, C, n = "VAE", 16, 1, 64
    sd = R.det_state(arch, zt, C)
    outs = []
    for graphs in (True, False):
        rng.clear_injections()
        rng.reset_counters()
        tr = _trainer(arch, zt, C, sd, _hp(True, loss_name, "fused"))
        eng = tr._fused()
        eng.graphs_enabled = graphs
        traj = []
        for step in range(3):
            x, label, _, _, _ = R.det_inputs(n, C, 28, zt, 10, seed=100 + step)
            traj.append(eng.step(torch.tensor(x, dtype=torch.float32, device="cuda"),
                                 torch.tensor(label, device="cuda")).clone())
        torch.cuda.synchronize()
        assert ("graphs" in eng.graphs[n]) == graphs
        outs.append((torch.stack(traj), eng.arena.flat.clone()))
    assert _same_bits(outs[0][0], outs[1][0]), (outs[0][0], outs[1][0])
    assert _same_bits(outs[0][1], outs[1][1]), float((outs[0][1] - outs[1][1]).abs().max())


# ----------------------------------------------------------------------------- 5. a refused batch


@pytest.mark.parametrize("loss_name", LOSSES)
def test_a_refused_batch_takes_the_module_path(loss_name):
    """Batches of 32, 32, 1, 32 (the engine refuses a batch of one sample): the third takes the module-path step with
    the device SupCon loss and torch Adam, the engine adopts the host counters and goes on."""
    from oracle import cpu_ref as R

    arch, zt, C = "VAE", 16, 1
    sd = R.det_state(arch, zt, C)
    x, label, _, _, _ = R.det_inputs(97, C, 28, zt, 10)
    X, L = torch.tensor(x, dtype=torch.float32), torch.tensor(label)
    batches = [(X[0:32], L[0:32]), (X[32:64], L[32:64]), (X[64:65], L[64:65]), (X[65:97], L[65:97])]
    tr = _trainer(arch, zt, C, sd, _hp(True, loss_name, "fused"))
    tr.model.train()
    eng = tr._fused()
    assert eng is not None and not eng.accepts(batches[2][0].cuda()) and eng.accepts(batches[0][0].cuda())
    before = eng.arena.flat.clone()
    tr._train(batches, False, 0)
    torch.cuda.synchronize()
    assert tr._engine is eng
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    assert not torch.equal(before, eng.arena.flat)
    p0 = next(iter(tr.model.parameters()))
    assert int(float(tr.optimizer.state[p0]["step"])) == len(batches)
    assert int(eng.adam.step[0]) == len(batches)


# ----------------------------------------------------------------------------- 6. no kept content row


def test_a_batch_with_no_kept_content_row():
    """All labels distinct, supcon_in_loss: the content branch (ps = 0) keeps no row, so its loss is NaN and it adds
    exactly zero to d(heads); the style branch (ps = 1) keeps every row.  Every parameter stays finite."""
    from oracle import cpu_ref as R

    arch, zt, C, n = "VAE", 16, 1, 32
    sd = R.det_state(arch, zt, C)
    x, _, _, _, _ = R.det_inputs(n, C, 28, zt, 10)
    tr = _trainer(arch, zt, C, sd, _hp(True, "supcon_in_loss", "fused"))
    eng = tr._fused()
    losses = eng.step(torch.tensor(x, dtype=torch.float32, device="cuda"), torch.arange(n, device="cuda")).clone()
    torch.cuda.synchronize()
    assert bool(torch.isnan(losses[3])) and bool(torch.isfinite(losses[[0, 1, 2, 4]]).all()), losses
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    assert bool(torch.isfinite(eng.arena.grad).all())


# ----------------------------------------------------------------------------- 7. the engine's programs

PROGRAMS = ("fwd", "dec", "lat", "enc", "upd")

# the call names of an snn_loss engine's programs (VAE z = 16, n = 64, default schedule switches), taken from the
# parent commit of the SupCon step
SNN_CALLS = {
    "fwd": ["cv_pack_conv_weights_zero", "cv_conv_forward_kpack", "cv_conv_forward_kpack", "cv_conv_forward_kpack",
            "cv_heads_forward", "cv_decoder_input_forward", "cv_ntxent_aux", "cv_conv_forward_kpack",
            "cv_ntxent_aux_flush", "cv_ntxent_aux", "cv_conv_forward_kpack", "cv_ntxent_aux_flush",
            "cv_convt_output_loss"],
    "dec": ["cv_conv_backward_deferred_kpack", "cv_conv_backward_deferred_kpack_side",
            "cv_conv_backward_deferred_kpack_side", "cv_decoder_input_backward"],
    "lat": ["cv_latent_combine_dz"],
    "enc": ["cv_heads_backward", "cv_conv_backward_deferred_kpack_side", "cv_conv_backward_deferred_kpack_side",
            "cv_conv_backward_weight_deferred", "join", "cv_step_reduce"],
    "upd": ["cv_adam_step"],
}


def _call_names(eng, n):
    G = eng.graphs[n]
    return {k: [str(c[0]) for c in G[k].calls] for k in PROGRAMS}


@pytest.mark.parametrize("loss_name", LOSSES)
def test_supcon_programs_hold_no_ntxent_call(loss_name):
    from oracle import cpu_ref as R

    arch, zt, C, n = "VAE", 16, 1, 64
    sd = R.det_state(arch, zt, C)
    x, label, _, _, _ = R.det_inputs(n, C, 28, zt, 10)
    tr = _trainer(arch, zt, C, sd, _hp(True, loss_name, "fused"))
    eng = tr._fused()
    eng.step(torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda"))
    torch.cuda.synchronize()
    G = eng.graphs[n]
    for key, prog in G.items():
        calls = getattr(prog, "calls", None)
        if calls is None:
            continue
        for c in calls:
            name = str(c[0])
            assert not name.startswith("cv_ntxent") and name != "cv_latent_step", (key, name)
    lat = [str(c[0]) for c in G["lat"].calls]
    assert lat[0] in ("cv_latent_combine_dz", "cv_latent_combine") and lat[1:] == ["cv_supcon_step"] * 2, lat
    assert G["lat_inj"] is G["lat"]


def test_snn_programs_are_unchanged():
    from oracle import cpu_ref as R

    arch, zt, C, n = "VAE", 16, 1, 64
    sd = R.det_state(arch, zt, C)
    x, label, _, _, _ = R.det_inputs(n, C, 28, zt, 10)
    tr = _trainer(arch, zt, C, sd, _hp(True, None, "fused"))  # (snn_loss ignores the key)
    eng = tr._fused()
    assert eng.supcon is None
    eng.step(torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda"))
    torch.cuda.synchronize()
    assert _call_names(eng, n) == SNN_CALLS
