"""CLUB and VarUB through the public layers: the trainer factory, the CPU fallback of the two classes, and the
estimator kinds cv_mi_forward / cv_mi_backward accept.  Only the factory test needs the GPU."""

import ctypes

import pytest
import torch


def _mlp(d=4, h=4):
    """A cv_mlp over host memory: the validation under test returns before anything could read it."""
    from cvhip import _lib

    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    return _lib.cv_mlp(p, p, p, p, p, p, p, p, d, h, d), buf


def test_constants_follow_the_header():
    import os
    import re

    from cvhip import _lib

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clearvae.h")).read()
    for name in ("CLUBSAMPLE", "L1OUT", "CLUB", "VARUB"):
        m = re.search(r"CV_MI_%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "MI_" + name), name
    assert (_lib.MI_CLUB, _lib.MI_VARUB) == (3, 4)


@pytest.mark.parametrize("fn", ["cv_mi_forward", "cv_mi_backward"])
def test_unknown_kind_is_still_refused(fn):
    from cvhip import _lib

    L = _lib.lib()
    mlp, buf = _mlp()
    p = ctypes.addressof(buf)
    for kind in (0, 5, 7):
        if fn == "cv_mi_forward":
            rc = L.cv_mi_forward(kind, ctypes.byref(mlp), p, 4, p, 4, 8, None, 0, None, p, p, None)
        else:
            rc = L.cv_mi_backward(kind, ctypes.byref(mlp), p, 4, p, 4, 8, p, None, 1.0, p, p, 4, 0, None, None, None,
                                  None, 0, None)
        assert rc != 0
        assert b"unknown estimator %d" % kind in L.cv_last_error(), L.cv_last_error()


@pytest.mark.parametrize("kind", [3, 4])
def test_new_kinds_pass_the_kind_check(kind):
    """With n = 1 a known kind gets as far as the argument check (no launch); neither needs perm or offset."""
    from cvhip import _lib

    L = _lib.lib()
    mlp, buf = _mlp()
    p = ctypes.addressof(buf)
    rc = L.cv_mi_forward(kind, ctypes.byref(mlp), p, 4, p, 4, 1, None, 0, None, p, p, None)
    assert rc != 0
    assert b"mi_forward: bad args" in L.cv_last_error(), L.cv_last_error()
    rc = L.cv_mi_backward(kind, ctypes.byref(mlp), p, 4, p, 4, 1, p, None, 1.0, p, p, 4, 0, None, None, None, None,
                          0, None)
    assert rc != 0
    assert b"mi_backward: bad args" in L.cv_last_error(), L.cv_last_error()


@pytest.mark.parametrize("n,d,hidden", [(5, 3, 8), (64, 8, 16)])
def test_cpu_forward_keeps_the_reference_formulas(n, d, hidden):
    """On CPU tensors CLUB.forward / VarUB.forward are the reference's plain-PyTorch formulas
    (mi_estimator.py:43-55, 222-224), differentiable, in whatever dtype the module has."""
    from src.models.mi_estimator import CLUB, VarUB

    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, d, generator=g, dtype=torch.float64, requires_grad=True)
    y = (1.5 * torch.randn(n, d, generator=g, dtype=torch.float64) + 0.7).requires_grad_(True)
    for cls in (CLUB, VarUB):
        torch.manual_seed(3)
        est = cls(d, d, hidden).double()
        out = est(x, y)
        mu, logvar = est.p_mu(x), est.p_logvar(x)
        if cls is CLUB:
            pos = (-((mu - y) ** 2) / 2.0 / logvar.exp()).sum(dim=-1)
            neg = torch.stack([(-((y - mu[i]) ** 2).mean(dim=0) / 2.0 / logvar[i].exp()).sum() for i in range(n)])
            ref = (pos - neg).mean()
        else:
            ref = 0.5 * (mu ** 2 + logvar.exp() - 1.0 - logvar).sum() / (n * d)
        assert out.dtype == torch.float64 and out.device.type == "cpu"
        o, r = float(out.detach()), float(ref.detach())
        assert abs(o - r) <= 1e-12 * max(abs(r), 1.0), (cls.__name__, o, r)
        (gx,) = torch.autograd.grad(out, x, retain_graph=True)
        (rx,) = torch.autograd.grad(ref, x)
        assert float((gx - rx).abs().max()) <= 1e-12


def test_factory_resolves_all_six_names():
    from src.utils.trainer_utils import get_clearmimvae_trainer

    for name in ("CLUBSample", "L1OutUB", "CLUB", "VarUB", "CLUBMean", "InfoNCE"):
        tr = get_clearmimvae_trainer(beta=1 / 8, mi_estimator=name, la=3.0, vae_lr=5e-4, mi_estimator_lr=2e-3,
                                     z_dim=16, alpha=100, temperature=0.1, device="cpu")
        assert type(tr.mi_estimator).__name__ == name


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("CLUB", True), ("VarUB", True), ("CLUBMean", False), ("InfoNCE", False)])
def test_factory_trainer_is_fused(name, fused):
    """get_clearmimvae_trainer(mi_estimator="CLUB" / "VarUB") on the GPU trains through the one-graph step;
    CLUBMean and InfoNCE stay on the module path."""
    from cvhip import _lib
    from cvhip.engine import ClearStep
    from src.utils.trainer_utils import get_clearmimvae_trainer

    torch.manual_seed(0)
    tr = get_clearmimvae_trainer(beta=1 / 8, mi_estimator=name, la=3.0, vae_lr=5e-4, mi_estimator_lr=2e-3,
                                 z_dim=16, alpha=100, temperature=0.1, device="cuda")
    eng = tr._fused()
    if not fused:
        assert eng is None
        return
    assert isinstance(eng, ClearStep)
    assert eng.kind == {"CLUB": _lib.MI_CLUB, "VarUB": _lib.MI_VARUB}[name]
    g = torch.Generator().manual_seed(5)
    X = torch.rand(32, 1, 28, 28, generator=g).cuda()
    L = torch.randint(0, 10, (32,), generator=g).cuda()
    losses, learn = eng.step(X, L)
    torch.cuda.synchronize()
    assert torch.isfinite(losses[:6]).all() and torch.isfinite(learn).all()
