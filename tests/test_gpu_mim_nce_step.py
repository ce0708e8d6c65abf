"""InfoNCE and CLUBMean with backend="device" as the CLEAR-MIM estimator: the fused step (cvhip.engine.ClearStep) and
the module path against golden fixtures of the real reference (tests/golden/mim_infonce_*.npz, mim_clubmean_*.npz,
made by tests/golden/gen_golden_mi2.py: one real ClearMIMVAETrainer._train step each, fp64, the estimator's initial
state_dict stored in the file).

The checks and bars are those of tests/test_mi_golden_club_varub.py, run by its own test bodies with the estimator
builder swapped for one that reads the fixture: outputs 1e-4 relative (the MI value with an absolute floor of 1), the
five learning losses at 1e-3, VAE gradients median per-tensor < 5e-4 / worst < 2e-2, parameters after Adam median
< 1e-5 / worst < 5e-3, BN running statistics 1e-3, the estimator's parameters after its five updates rel-L2 < 1e-3.
The module path (use_fused = False) runs the same trainer step through autograd and torch.optim.Adam and is held to
the same MI, learning-loss and estimator bars.

Then the step's schedules: MIM_BRANCHES against the sequential form at n = 32, bit for bit (as
tests/test_gpu_mim_branches.py), and three replayed steps twice from the same seed."""

import numpy as np
import pytest
import torch

import golden_cases as G
import test_mi_golden_club_varub as TG
from test_gpu_golden import TOL

pytestmark = pytest.mark.gpu

NAMES = ["mim_infonce_vae_n64", "mim_clubmean_vae_n64", "mim_infonce_vae64_n16"]
KINDS = {"InfoNCE": 6, "CLUBMean": 5}


def _estimator(fx):
    from src.models import mi_estimator as MI

    m = fx["meta"]
    d = m["z"] // 2
    est = getattr(MI, m["estimator"])(d, d, m["z"], backend="device").cuda()
    est.load_state_dict({k: torch.tensor(fx["est_init__" + k], dtype=torch.float32) for k in est.state_dict()})
    return est


@pytest.fixture
def golden_estimator(monkeypatch):
    monkeypatch.setattr(TG, "_estimator", _estimator)


def test_fixtures_are_the_new_estimators():
    kinds = [G.load(n)["meta"]["estimator"] for n in NAMES]
    assert kinds == ["InfoNCE", "CLUBMean", "InfoNCE"]
    assert not set(NAMES) & set(G.names())


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("arch,z,C", [("VAE", 16, 1), ("VAE64", 64, 3)])
def test_factory_device_backend_is_fused(kind, arch, z, C):
    from cvhip.engine import ClearStep
    from src.utils.trainer_utils import get_clearmimvae_trainer

    tr = get_clearmimvae_trainer(beta=1 / 8, mi_estimator=kind, la=3.0, vae_lr=5e-4, mi_estimator_lr=2e-3, z_dim=z,
                                 alpha=100.0, temperature=0.1, device=torch.device("cuda"), vae_arch=arch,
                                 in_channel=C, backend="device")
    assert tr.mi_estimator.backend == "device"
    eng = tr._fused()
    assert isinstance(eng, ClearStep) and eng.kind == KINDS[kind]


@pytest.mark.parametrize("name", NAMES)
def test_module_mi_vs_golden(name, golden_estimator):
    TG.test_module_mi_vs_golden(name)


@pytest.mark.parametrize("name", NAMES)
def test_fused_mim_step_vs_golden(name, golden_estimator):
    TG.test_fused_mim_step_vs_golden(name)


@pytest.mark.parametrize("name", NAMES)
def test_module_path_step_vs_golden(name, golden_estimator):
    """The same trainer step with use_fused = False: autograd through the device estimator functions and
    torch.optim.Adam."""
    fx = G.load(name)
    x, label, ec, es, perm = G.inputs(fx)
    tr, eng, est = TG._build_fused(fx)  # (queues the case's noise)
    tr.use_fused = False
    tr._engine = None
    X = torch.tensor(x, dtype=torch.float32, device="cuda")
    mi_l, ll_l = [], []
    tr._train([(X, torch.tensor(label, device="cuda"))], False, 0, mi_l, ll_l)
    torch.cuda.synchronize()
    assert abs(mi_l[0] - float(fx["mi"])) <= TOL * max(abs(float(fx["mi"])), 1.0), (mi_l, float(fx["mi"]))
    assert np.allclose(np.array(ll_l), fx["mi_learning"], rtol=1e-3, atol=1e-3), (ll_l, fx["mi_learning"])
    erels = [(G.rel(p.detach().double().cpu().numpy(), fx["est_after__" + k]), k) for k, p in est.named_parameters()]
    print(name, "module path: estimator after", max(erels))
    assert max(erels)[0] < 1e-3, sorted(erels)[-3:]


def _trainer(kind, arch="VAE", zt=16, C=1):
    from oracle import cpu_ref as R
    from src.models import mi_estimator as MI
    from src.trainer import ClearMIMVAETrainer
    from test_gpu_parity import _model as parity_model

    torch.manual_seed(4321)
    vae = parity_model(arch, zt, C, R.det_state(arch, zt, C))
    est = getattr(MI, kind)(zt // 2, zt // 2, zt, backend="device").cuda()  # (seeded default init)
    hp = {"temperature": 0.1, "beta": 1 / 32, "loc": 0, "scale": 1, "alpha": 100.0, "lambda": 3.0}
    opt = torch.optim.Adam(vae.parameters(), lr=3e-5)
    eopt = torch.optim.Adam(est.parameters(), lr=2e-3)
    return ClearMIMVAETrainer(vae, est, {"vae_optim": opt, "mi_estimator_optim": eopt}, "cosine", hp, 1,
                              torch.device("cuda"))


def _run(kind, branches, steps, n=32):
    from oracle import cpu_ref as R
    from cvhip import engine, rng
    from cvhip.engine import ClearStep

    prev = engine.MIM_BRANCHES
    engine.MIM_BRANCHES = branches
    try:
        rng.clear_injections()
        rng.reset_counters()
        tr = _trainer(kind)
        eng = ClearStep.build(tr, "mim")
        assert eng is not None and eng.kind == KINDS[kind]
        x, label, _, _, _ = R.det_inputs(n, 1, 28, 16, 4)
        X, L = torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda")
        res = []
        for _ in range(steps):
            lo, learn = eng.step(X, L)
            torch.cuda.synchronize()
            res.append(dict(loss=lo[:6].cpu().numpy().copy(), learn=learn.cpu().numpy().copy(),
                            flat=eng.arena.flat.cpu().numpy().copy(), est=eng.est_arena.flat.cpu().numpy().copy()))
        G_ = eng.graphs[n]
        return dict(res=res, lanes={c[3] for c in G_["learn"].calls}, replayed="graphs" in G_)
    finally:
        engine.MIM_BRANCHES = prev


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_branched_schedule_matches_sequential(kind):
    a, b = _run(kind, 2, 2), _run(kind, 0, 2)
    assert any(isinstance(v, int) and v >= 1 for v in a["lanes"]), a["lanes"]
    assert not any(isinstance(v, int) and v >= 1 for v in b["lanes"]), b["lanes"]
    assert a["replayed"] and b["replayed"]
    for step, (ra, rb) in enumerate(zip(a["res"], b["res"])):
        for k in ("loss", "learn", "flat", "est"):
            assert _same_bits(ra[k], rb[k]), (step, k)
        assert np.isfinite(ra["learn"]).all() and np.abs(ra["learn"]).max() > 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_three_replayed_steps_repeat(kind):
    from cvhip import engine

    a, b = _run(kind, engine.MIM_BRANCHES, 3), _run(kind, engine.MIM_BRANCHES, 3)
    assert a["replayed"]
    for step, (ra, rb) in enumerate(zip(a["res"], b["res"])):
        for k in ("loss", "learn", "flat", "est"):
            assert _same_bits(ra[k], rb[k]), (step, k)
    assert not _same_bits(a["res"][0]["est"], a["res"][2]["est"])  # (the estimator did train)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_outside_the_envelope_warns_once_and_runs_the_torch_paths(kind):
    """hidden_size = 128 is outside the kernels' widths: the module call warns once and returns what backend="torch"
    returns on the same weights; ClearStep.build warns once, declines, and the trainer trains on the module path."""
    import warnings

    from src.models import mi_estimator as MI
    from src.trainer import ClearMIMVAETrainer

    torch.manual_seed(3)
    est = getattr(MI, kind)(8, 8, 128, backend="device").cuda()
    twin = getattr(MI, kind)(8, 8, 128, backend="torch").cuda()
    twin.load_state_dict(est.state_dict())
    x, y = torch.randn(32, 8, device="cuda"), torch.randn(32, 8, device="cuda")
    with pytest.warns(RuntimeWarning, match="outside the device envelope"):
        a = est(x, y)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b, la, lb = est(x, y), est.learning_loss(x, y), twin.learning_loss(x, y)
    assert torch.equal(a, twin(x, y)) and torch.equal(a, b) and torch.equal(la, lb)

    tr = _trainer(kind)
    tr.mi_estimator = est
    tr.mi_estimator_optimizer = torch.optim.Adam(est.parameters(), lr=2e-3)
    with pytest.warns(RuntimeWarning, match="outside the fused step's envelope"):
        assert tr._fused() is None
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert tr._fused() is None
    from oracle import cpu_ref as R

    xb, label, _, _, _ = R.det_inputs(32, 1, 28, 16, 4)
    mi_l, ll_l = [], []
    tr._train([(torch.tensor(xb, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda"))], False, 0,
              mi_l, ll_l)
    assert len(mi_l) == 1 and len(ll_l) == 5 and np.isfinite(mi_l + ll_l).all()
