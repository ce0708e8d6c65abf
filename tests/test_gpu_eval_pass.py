"""cvhip.evaluate.EvalPass and evaluate(backend="fused") of the VAE trainers.

Weights and inputs come from oracle.cpu_ref.det_state / det_inputs (one det_inputs draw per batch), noise and the CLUB-S
permutation are injected through cvhip.rng.  The bar everywhere is the project's LOSS_TOL (tests/test_gpu_parity.py):
|value - ref| <= 1e-4 * max(|ref|, 1e-3) for the per-epoch means, rel-L2 < 1e-4 for the latents.  The terms the fp64
oracle restates are compared with it; the others with the module path's evaluate() on the same weights, batches and
noise (their kernels have their own fp64 tests: what is checked here is the pass's pointers, strides, signs and
scaling, where an error is of order one)."""

import functools
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
DEV = torch.device("cuda", 0)


def close(v, ref):
    if math.isnan(ref) or math.isnan(v):
        return math.isnan(ref) and math.isnan(v)
    return abs(v - ref) <= LOSS_TOL * max(abs(ref), 1e-3)


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Loader:
    """A list of (X, label) batches with the two things evaluate() asks a DataLoader for."""

    def __init__(self, batches):
        self.batches = batches
        self.dataset = range(sum(int(b[1].numel()) for b in batches))

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


@functools.lru_cache(maxsize=None)
def epoch(arch, zt, C, total, bs):
    """The epoch's batches as det_inputs draws (numpy, never written to): [(x, label, eps_c, eps_s, perm)]."""
    from oracle import cpu_ref as R

    out, b = [], 0
    while total > 0:
        n = min(bs, total)
        out.append(R.det_inputs(n, C, R.IMAGE[arch], zt, 10, seed=11 + b))
        total -= n
        b += 1
    return out


def loader_of(ep):
    return Loader([(torch.tensor(x, dtype=torch.float32, device=DEV), torch.tensor(lab, device=DEV))
                   for x, lab, *_ in ep])


def inject(ep, perms=False):
    from cvhip import rng

    rng.clear_injections()
    for _, _, ec, es, pm in ep:
        rng.inject_noise([torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)])
        if perms:
            rng.inject_perm([torch.tensor(pm)])


def load_det(module, sd):
    module.load_state_dict({k: torch.as_tensor(np.asarray(v)).float() if np.asarray(v).dtype != np.int64
                            else torch.as_tensor(np.asarray(v)) for k, v in sd.items()})


def make_trainer(kind, arch="VAE", zt=16, C=1, ps=True, sim="cosine", est="CLUBSample", loss_name="snn_loss",
                 backend=None, group_mode="GVAE"):
    from oracle import cpu_ref as R
    from src.utils import trainer_utils as U

    if kind == "clear":
        tr = U.get_clearvae_trainer(beta=1 / 8, ps=ps, vae_lr=5e-4, z_dim=zt, alpha=100, temperature=0.1, device=DEV,
                                    vae_arch=arch, in_channel=C, loss_name=loss_name)
        tr.sim_fn = sim
    elif kind == "mim":
        tr = U.get_clearmimvae_trainer(beta=1 / 8, mi_estimator=est, la=2.0, vae_lr=5e-4, mi_estimator_lr=2e-3,
                                       z_dim=zt, alpha=100, temperature=0.1, device=DEV, vae_arch=arch, in_channel=C,
                                       backend=backend)
        if est in ("CLUBSample", "L1OutUB", "CLUB", "VarUB"):
            load_det(tr.mi_estimator, R.det_mlp(zt // 2, zt))
    elif kind == "tc":
        tr = U.get_cleartcvae_trainer(beta=1 / 8, la=2.0, vae_lr=5e-4, factor_cls_lr=1e-3, z_dim=zt, alpha=100,
                                      temperature=0.1, device=DEV, vae_arch=arch, in_channel=C)
        load_det(tr.factor_cls, R.det_disc(zt))
    else:
        tr = U.get_hierarchical_vae_trainer(beta=1 / 8, vae_lr=5e-4, z_dim=zt, group_mode=group_mode, device=DEV,
                                            vae_arch=arch, in_channel=C)
    load_det(tr.model, R.det_state(arch, zt, C))
    return tr


def run_pass(tr, mode, ep, perms=False, graphs=True, injected=True):
    """One epoch through EvalPass directly: (means [5], label, lat_c, lat_s, pass)."""
    from cvhip import rng
    from cvhip.evaluate import EvalPass

    P = EvalPass.build(tr, mode)
    assert P is not None, EvalPass.unsupported_reason(tr, mode)
    P.graphs_enabled = graphs
    tr.model.eval()
    if injected:
        inject(ep, perms)
    else:
        rng.clear_injections()
    L = loader_of(ep)
    P.begin(len(L.dataset))
    for X, lab in L:
        assert P.accepts(X)
        P.batch(X, lab)
    totals, nb, label, lat_c, lat_s = P.finish()
    assert nb == len(L)
    return [t / nb for t in totals], label, lat_c, lat_s, P


@functools.lru_cache(maxsize=None)
def oracle_epoch(arch, zt, C, total, bs, sim, ps, est):
    """fp64 per-epoch means (rec, kl_c, kl_s, c_loss, last) and latents of the epoch, computed once."""
    from oracle import cpu_ref as R

    P = R.to_torch(R.det_state(arch, zt, C), requires_grad=False)
    M = R.to_torch(R.det_mlp(zt // 2, zt), requires_grad=False) if est else None
    d = zt // 2
    tot, zs = np.zeros(5), []
    ep = epoch(arch, zt, C, total, bs)
    with torch.no_grad():
        for x, lab, ec, es, pm in ep:
            X, lab = torch.tensor(x, dtype=torch.float64), torch.tensor(lab)
            xhat, lp, z = R.vae_forward(P, X, torch.tensor(ec), torch.tensor(es), arch, train=False)
            rec, kc, ks = R.vae_loss(xhat, X, **lp)
            c = R.contrastive_loss(lp["mu_c"], lp["logvar_c"], lab, sim, 0.1, ps=False)
            if est == "CLUBSample":
                last = R.club_sample(M, z[:, :d], z[:, d:], torch.tensor(pm))
            elif est == "L1OutUB":
                last = R.l1out(M, z[:, :d], z[:, d:])
            else:
                s = R.contrastive_loss(lp["mu_s"], lp["logvar_s"], lab, sim, 0.1, ps=ps)
                last = s if ps else -s
            tot += np.array([float(v) for v in (rec, kc, ks, c, last)])
            zs.append(z)
    return tot / len(ep), torch.cat(zs)


ORACLE_CASES = [
    ("VAE", 16, 1, 150, 64, "cosine", True, None),
    ("VAE", 16, 1, 150, 64, "cosine", False, None),
    ("VAE", 16, 1, 150, 64, "jeffrey", True, None),
    ("VAE64", 64, 3, 40, 16, "cosine", True, None),
    ("VAE", 16, 1, 150, 64, "cosine", True, "CLUBSample"),
    ("VAE", 16, 1, 150, 64, "cosine", True, "L1OutUB"),
]


@pytest.mark.parametrize("cfg", ORACLE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pass_matches_the_fp64_oracle(cfg):
    arch, zt, C, total, bs, sim, ps, est = cfg
    ref, zref = oracle_epoch(*cfg)
    if est:
        tr, mode = make_trainer("mim", arch, zt, C, est=est), "mim"
        tr.sim_fn = sim
    else:
        tr, mode = make_trainer("clear", arch, zt, C, ps=ps, sim=sim), "clear"
    ep = epoch(arch, zt, C, total, bs)
    means, label, lat_c, lat_s, P = run_pass(tr, mode, ep, perms=est == "CLUBSample")
    names = ("rec", "kl_c", "kl_s", "c_loss", "last")
    for nm, v, r in zip(names, means, ref):
        print(nm, v, r)
    for nm, v, r in zip(names, means, ref):
        assert close(v, float(r)), (nm, v, float(r))
    d = zt // 2
    assert lat_c.shape == (total, d) and lat_s.shape == (total, d)
    assert rel(lat_c, zref[:, :d]) < LOSS_TOL and rel(lat_s, zref[:, d:]) < LOSS_TOL
    assert torch.equal(label.cpu(), torch.cat([torch.tensor(b[1]) for b in ep]))
    assert len(P.sizes) == len({len(b[1]) for b in ep})  # one workspace / graph per batch size


def evaluate_spy(tr, loader, backend, monkeypatch, **kw):
    """trainer.evaluate with mutual_info_gap replaced by a recorder: (mse, label, lat_c, lat_s, per-epoch means).  The
    module path's means are collected from _module_batch's return values (the GVAE trainer's from vae_loss)."""
    import src.trainer as T

    got, rows = {}, []

    def fake_gmig(label, lat_c, lat_s, backend=None):
        got.update(label=label.clone(), lat_c=lat_c.clone(), lat_s=lat_s.clone())
        return 0.25

    monkeypatch.setattr(T, "mutual_info_gap", fake_gmig)
    if backend == "module" and hasattr(tr, "_module_batch"):
        orig = tr._module_batch

        def spy(X, label, last_fn):
            vals, z = orig(X, label, last_fn)
            rows.append([float(v) for v in vals])
            return vals, z

        monkeypatch.setattr(tr, "_module_batch", spy)
    elif backend == "module":
        orig_loss = T.vae_loss

        def spy_loss(*a, **k):
            vals = orig_loss(*a, **k)
            rows.append([float(v) for v in vals])
            return vals

        monkeypatch.setattr(T, "vae_loss", spy_loss)
    mig, mse = tr.evaluate(loader, False, 0, backend=backend, **kw)
    monkeypatch.undo()
    assert mig == 0.25
    if backend == "module":
        means = list(np.sum(np.array(rows, dtype=np.float64), axis=0) / len(loader))
    else:
        means = (tr._eval_pass.totals[:5].cpu() / len(loader)).tolist()
    return mse, got["label"], got["lat_c"], got["lat_s"], means


MODULE_CASES = [
    ("clear", dict(loss_name="supcon_in_loss")), ("clear", dict(loss_name="supcon_out_loss")),
    ("mim", dict(est="CLUB")), ("mim", dict(est="VarUB")), ("mim", dict(est="CLUBMean", backend="device")),
    ("mim", dict(est="InfoNCE", backend="device")), ("tc", {}), ("group", {}),
]


@pytest.mark.parametrize("kind,kw", MODULE_CASES, ids=lambda v: "-".join(map(str, v.values())) if isinstance(v, dict) else v)
def test_pass_matches_the_module_path(kind, kw, monkeypatch):
    ep = epoch("VAE", 16, 1, 150, 64)
    tr = make_trainer(kind, **kw)
    L = loader_of(ep)
    inject(ep)
    mse_m, lab_m, zc_m, zs_m, means_m = evaluate_spy(tr, L, "module", monkeypatch)
    inject(ep)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*runs as 'module'.*")  # a refusal would warn: the fused path itself must have run
        mse_f, lab_f, zc_f, zs_f, means_f = evaluate_spy(tr, L, "fused", monkeypatch)
    n = len(means_m)
    for i in range(n):
        print(i, means_f[i], means_m[i])
    for i in range(n):
        assert close(means_f[i], means_m[i]), (i, means_f[i], means_m[i])
    assert close(mse_f, mse_m)
    assert torch.equal(lab_f, lab_m) and zc_f.shape == zc_m.shape
    assert rel(zc_f, zc_m.cpu()) < LOSS_TOL and rel(zs_f, zs_m.cpu()) < LOSS_TOL


def test_mig_and_mse(monkeypatch):
    from src.losses import mutual_info_gap

    monkeypatch.setenv("CVHIP_GMIG", "device")
    ep = epoch("VAE", 16, 1, 150, 64)
    tr = make_trainer("clear")
    L = loader_of(ep)
    inject(ep)
    _, mse_m = tr.evaluate(L, False, 0, backend="module")
    inject(ep)
    monkeypatch.setenv("CVHIP_EVAL", "fused")  # (the environment switch, as _valid and the scripts use it)
    mig_f, mse_f = tr.evaluate(L, False, 0)
    assert close(mse_f, mse_m), (mse_f, mse_m)
    _, _, label, lat_c, lat_s = tr._eval_pass.finish()
    assert label.shape[0] == 150
    assert mig_f == mutual_info_gap(label, lat_c, lat_s, backend="device")


def test_a_batch_of_one_goes_through_the_module_path(monkeypatch):
    ep = epoch("VAE", 16, 1, 65, 64)
    assert [len(b[1]) for b in ep] == [64, 1]
    tr = make_trainer("clear")
    L = loader_of(ep)
    inject(ep)
    mse_m, lab_m, zc_m, zs_m, means_m = evaluate_spy(tr, L, "module", monkeypatch)
    inject(ep)
    mse_f, lab_f, zc_f, zs_f, means_f = evaluate_spy(tr, L, "fused", monkeypatch)
    assert lab_f.shape[0] == 65 and torch.equal(lab_f, lab_m)
    for i in range(5):
        assert close(means_f[i], means_m[i]), (i, means_f[i], means_m[i])
    assert close(mse_f, mse_m)
    assert rel(zc_f, zc_m.cpu()) < LOSS_TOL and rel(zs_f, zs_m.cpu()) < LOSS_TOL
    assert int(tr._eval_pass.totals[7]) == 2


def test_eager_equals_replayed():
    from cvhip import rng

    ep = epoch("VAE", 16, 1, 214, 64)  # 64, 64, 64, 22: the third batch of 64 replays the graph captured at the second
    tr = make_trainer("mim", est="CLUBSample")
    out = []
    for graphs in (False, True):
        torch.manual_seed(5)
        rng.reset_counters()
        means, label, lat_c, lat_s, P = run_pass(tr, "mim", ep, graphs=graphs, injected=False)
        assert (P.sizes[64]["graph"] is not None) == graphs
        out.append((P.totals.clone(), label.clone(), lat_c.clone(), lat_s.clone()))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)


def _snapshot(tr):
    sd = {k: v.clone() for k, v in tr.model.state_dict().items()}
    opt = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
           for i, st in enumerate(tr.optimizer.state.values())}
    return sd, opt, tr.annealer.current_step


def _same_snapshot(a, b):
    assert a[2] == b[2]
    assert a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert a[1].keys() == b[1].keys()
    for i in a[1]:
        for k, v in a[1][i].items():
            assert torch.equal(v, b[1][i][k]) if torch.is_tensor(v) else v == b[1][i][k], (i, k)


def test_nothing_else_moves(monkeypatch):
    from cvhip import rng

    ep = epoch("VAE", 16, 1, 150, 64)
    x, lab, ec, es, _ = ep[0]
    X, Y = torch.tensor(x, dtype=torch.float32, device=DEV), torch.tensor(lab, device=DEV)
    L = loader_of(ep)
    finals = []
    for backend in ("module", "fused"):
        tr = make_trainer("clear")
        tr.model.train()
        eng = tr._fused()
        assert eng is not None

        def step():
            rng.clear_injections()
            rng.inject_noise([torch.tensor(ec, dtype=torch.float32), torch.tensor(es, dtype=torch.float32)])
            tr.model.train()
            eng.step(X, Y)
            tr.annealer.step()
            eng.sync_host_state()

        step()
        before = _snapshot(tr)
        inject(ep)
        evaluate_spy(tr, L, backend, monkeypatch)
        torch.cuda.synchronize()
        _same_snapshot(before, _snapshot(tr))
        assert tr._engine is eng and eng.compatible()
        step()
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in tr.model.state_dict().items()})
    assert all(torch.equal(finals[0][k], finals[1][k]) for k in finals[0])


def _refused(tr, L, ep, monkeypatch, match, **kw):
    """evaluate(backend="fused") warns once with the reason and returns the module path's result."""
    inject(ep)
    ref = evaluate_spy(tr, L, "module", monkeypatch, **kw)
    inject(ep)
    with pytest.warns(UserWarning, match=match):
        got = evaluate_spy_refused(tr, L, monkeypatch, **kw)
    assert got == ref[0]
    inject(ep)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*runs as 'module'.*")  # once: no second warning
        assert evaluate_spy_refused(tr, L, monkeypatch, **kw) == ref[0]


def evaluate_spy_refused(tr, L, monkeypatch, **kw):
    import src.trainer as T

    monkeypatch.setattr(T, "mutual_info_gap", lambda *a, **k: 0.25)
    mig, mse = tr.evaluate(L, False, 0, backend="fused", **kw)
    monkeypatch.undo()
    assert mig == 0.25 and tr._eval_pass is None
    return mse


def test_refusals_warn_once_and_run_the_module_path(monkeypatch):
    ep = epoch("VAE", 16, 1, 150, 64)
    L = loader_of(ep)
    tr = make_trainer("clear")
    tr.transform = lambda x: x
    _refused(tr, L, ep, monkeypatch, "transform")
    tr = make_trainer("mim", est="CLUBMean", backend="torch")
    _refused(tr, L, ep, monkeypatch, "torch backend")
    tr = make_trainer("group")
    _refused(tr, L, ep, monkeypatch, "with_evidence_acc", with_evidence_acc=True)
