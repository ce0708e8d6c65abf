"""CLUBMean and InfoNCE through the public layers without a GPU: the backend switch of the two classes and of the
trainer factory, the CPU formulas under backend="device", the cv_critic structs against the header, and the
host-side validation of the cv_infonce_* entry points and of CV_MI_CLUBMEAN (every call is rejected before a
launch)."""

import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _classes():
    from src.models.mi_estimator import CLUBMean, InfoNCE

    return CLUBMean, InfoNCE


def test_default_backend_is_torch_and_env_switches(monkeypatch):
    monkeypatch.delenv("CVHIP_MI_EST", raising=False)
    for cls in _classes():
        assert cls(4, 4, 8).backend == "torch"
        assert cls(4, 4, 8, backend="device").backend == "device"
    monkeypatch.setenv("CVHIP_MI_EST", "device")
    for cls in _classes():
        assert cls(4, 4, 8).backend == "device"
        assert cls(4, 4, 8, backend="torch").backend == "torch"  # (the argument wins)
    monkeypatch.setenv("CVHIP_MI_EST", "torch")
    for cls in _classes():
        assert cls(4, 4, 8).backend == "torch"


def test_bad_backend_raises(monkeypatch):
    monkeypatch.delenv("CVHIP_MI_EST", raising=False)
    for cls in _classes():
        with pytest.raises(ValueError, match="torch.*device"):
            cls(4, 4, 8, backend="hip")
    monkeypatch.setenv("CVHIP_MI_EST", "gpu")
    for cls in _classes():
        with pytest.raises(ValueError, match="torch.*device"):
            cls(4, 4, 8)


def test_state_dict_keys_do_not_depend_on_the_backend():
    for cls in _classes():
        assert list(cls(4, 4, 8, backend="device").state_dict()) == list(cls(4, 4, 8, backend="torch").state_dict())
    assert list(_classes()[0](4, 4, None, backend="device").state_dict()) == ["p_mu.weight", "p_mu.bias"]


@pytest.mark.parametrize("n,d,hidden", [(5, 3, 8), (64, 8, 16)])
def test_device_backend_on_cpu_keeps_the_reference_formulas(n, d, hidden):
    """backend="device" on CPU fp64 tensors: the reference's literal formulas (mi_estimator.py:84-105, 259-273),
    differentiable, equal to backend="torch" on the same weights."""
    import nce_ref as NR

    CLUBMean, InfoNCE = _classes()
    x32, y32 = NR.inputs(n, d)
    for cls in (CLUBMean, InfoNCE):
        W = {k: v.double() for k, v in NR.det_weights(cls.__name__, d, hidden).items()}
        est, twin = cls(d, d, hidden, backend="device").double(), cls(d, d, hidden, backend="torch").double()
        est.load_state_dict(W)
        twin.load_state_dict(W)
        x, y = x32.double().requires_grad_(True), y32.double().requires_grad_(True)
        out = est(x, y)
        if cls is InfoNCE:
            ref, ll_ref = NR.infonce_literal(W, x, y), -NR.infonce_literal(W, x, y)
        else:
            ref, ll_ref = NR.clubmean_literal(NR.p_mu(W, x), y), -NR.clubmean_loglikeli(W, x, y)
        assert out.dtype == torch.float64 and out.device.type == "cpu"
        o, r = float(out.detach()), float(ref.detach())
        assert abs(o - r) <= 1e-12 * max(abs(r), 1.0), (cls.__name__, o, r)
        assert float(twin(x, y).detach()) == o
        (gx,) = torch.autograd.grad(out, x, retain_graph=True)
        (rx,) = torch.autograd.grad(ref, x)
        assert float((gx - rx).abs().max()) <= 1e-12
        ll = float(est.learning_loss(x, y).detach())
        assert abs(ll - float(ll_ref.detach())) <= 1e-12 * max(abs(ll), 1.0)
        assert float(twin.learning_loss(x, y).detach()) == ll


def test_factory_keyword_reaches_the_two_classes_only(monkeypatch):
    from src.utils.trainer_utils import get_clearmimvae_trainer

    monkeypatch.delenv("CVHIP_MI_EST", raising=False)
    kw = dict(beta=1 / 8, la=3.0, vae_lr=5e-4, mi_estimator_lr=2e-3, z_dim=16, alpha=100, temperature=0.1,
              device="cpu")
    for name in ("CLUBMean", "InfoNCE"):
        assert get_clearmimvae_trainer(mi_estimator=name, **kw).mi_estimator.backend == "torch"
        assert get_clearmimvae_trainer(mi_estimator=name, backend="device", **kw).mi_estimator.backend == "device"
        with pytest.raises(ValueError):
            get_clearmimvae_trainer(mi_estimator=name, backend="hip", **kw)
    est = get_clearmimvae_trainer(mi_estimator="CLUBMean", backend="device", **kw).mi_estimator
    assert est.p_mu[0].out_features == 16  # (hidden_size = z_dim, not z_dim // 2: mi_estimator.py:70-76)
    for name in ("CLUBSample", "L1OutUB", "CLUB", "VarUB"):
        a = get_clearmimvae_trainer(mi_estimator=name, backend="device", **kw).mi_estimator
        b = get_clearmimvae_trainer(mi_estimator=name, **kw).mi_estimator
        assert not hasattr(a, "backend") and not hasattr(b, "backend")
        assert list(a.state_dict()) == list(b.state_dict())


def test_constants_follow_the_header():
    import re

    from cvhip import _lib

    hdr = open(os.path.join(ROOT, "include", "clearvae.h")).read()
    for name, want in (("CLUBMEAN", 5), ("INFONCE", 6)):
        m = re.search(r"CV_MI_%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "MI_" + name) == want, name
    from cvhip.engine import MI_KINDS

    assert MI_KINDS["CLUBMean"] == 5 and MI_KINDS["InfoNCE"] == 6


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "clearvae.h"
#define S(T) printf(#T " size %zu\n", sizeof(T));
#define O(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  S(cv_critic) O(cv_critic, w1) O(cv_critic, b1) O(cv_critic, w2) O(cv_critic, b2) O(cv_critic, dx) O(cv_critic, dy)
  O(cv_critic, h)
  S(cv_critic_grad) O(cv_critic_grad, w1) O(cv_critic_grad, b1) O(cv_critic_grad, w2) O(cv_critic_grad, b2)
  return 0;
}
"""


def test_critic_struct_layouts_match_header(tmp_path):
    from cvhip import _lib

    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        parts = line.split()
        T = getattr(_lib, parts[0])
        if parts[1] == "size":
            assert ctypes.sizeof(T) == int(parts[2]), line
        else:
            assert getattr(T, parts[1]).offset == int(parts[2]), line
        seen += 1
    assert seen == 13


def _critic(dx=4, dy=4, h=8, null=None):
    """A cv_critic over host memory: the validation under test returns before anything could read it."""
    from cvhip import _lib

    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ptr = {k: p for k in ("w1", "b1", "w2", "b2")}
    if null:
        ptr[null] = None
    return _lib.cv_critic(ptr["w1"], ptr["b1"], ptr["w2"], ptr["b2"], dx, dy, h), buf


def _infonce_calls(L, cr, p, n):
    from cvhip import _lib

    g = _lib.cv_critic_grad(p, p, p, p)
    return {
        "cv_infonce_forward": lambda: L.cv_infonce_forward(ctypes.byref(cr), p, 4, p, 4, n, p, p, None),
        "cv_infonce_backward": lambda: L.cv_infonce_backward(ctypes.byref(cr), p, 4, p, 4, n, p, None, 1.0, p, p, 4, 0,
                                                             None, None, None, None, 0, None),
        "cv_infonce_learning_step": lambda: L.cv_infonce_learning_step(ctypes.byref(cr), p, 4, p, 4, n, p, p,
                                                                       ctypes.byref(g), None, None, None, None, 0,
                                                                       None, None, None),
    }


@pytest.mark.parametrize("fn", ["cv_infonce_forward", "cv_infonce_backward", "cv_infonce_learning_step"])
def test_infonce_entry_points_reject_before_any_launch(fn):
    from cvhip import _lib

    L = _lib.lib()
    for what, kw, n, msg in (("a NULL weight", dict(null="w2"), 8, b"critic weights missing"),
                             ("a NULL bias", dict(null="b1"), 8, b"critic weights missing"),
                             ("h = 65", dict(h=65), 8, b"widths must be in 1..64"),
                             ("dx = 65", dict(dx=65), 8, b"widths must be in 1..64"),
                             ("n = 1", dict(), 1, b"batch must be in 2..")):
        cr, buf = _critic(**kw)
        rc = _infonce_calls(L, cr, ctypes.addressof(buf), n)[fn]()
        assert rc != 0, what
        assert msg in L.cv_last_error(), (what, L.cv_last_error())
        assert fn[3:].encode() in L.cv_last_error(), L.cv_last_error()


def test_infonce_supported_is_the_envelope():
    from cvhip import _lib

    L = _lib.lib()
    assert L.cv_infonce_supported(2, 1, 1, 1) == 1 and L.cv_infonce_supported(4096, 64, 64, 64) == 1
    assert L.cv_infonce_supported(64, 8, 8, 16) == 1 and L.cv_infonce_supported(16, 32, 32, 64) == 1
    for bad in ((1, 8, 8, 16), (64, 65, 8, 16), (64, 8, 65, 16), (64, 8, 8, 65), (64, 0, 8, 16), (1 << 20, 8, 8, 16)):
        assert L.cv_infonce_supported(*bad) == 0, bad


@pytest.mark.parametrize("h", [16, 64])
def test_infonce_workspace_has_no_n_squared_term(h):
    from cvhip import _lib

    L = _lib.lib()
    for n in (1024, 2048, 4096):
        a, b = L.cv_infonce_workspace_bytes(n, h), L.cv_infonce_workspace_bytes(2 * n, h)
        assert 0 < a < b <= 2.5 * a, (n, a, b)
    # against the reference's [N, N, dx+dy] and [N, N, H] fp32 tensors at n = 4096 (mi_estimator.py:262-268)
    assert L.cv_infonce_workspace_bytes(4096, 64) * 50 < 4096 * 4096 * (128 + 64) * 4


def _mlp(d=4, h=4, mean_only=False):
    from cvhip import _lib

    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    q = None if mean_only else p
    return _lib.cv_mlp(p, p, p, p, q, q, q, q, d, h, d), buf


def test_null_logvar_weights_belong_to_clubmean_only():
    """cv_mi_forward(CV_MI_CLUB, ...) with a NULL w3 is still rejected; CV_MI_CLUBMEAN takes exactly that MLP (n = 1
    gets it as far as the argument check, no launch) and refuses a p_logvar network."""
    from cvhip import _lib

    L = _lib.lib()
    mlp, buf = _mlp(mean_only=True)
    p = ctypes.addressof(buf)
    for kind in (_lib.MI_CLUBSAMPLE, _lib.MI_L1OUT, _lib.MI_CLUB, _lib.MI_VARUB):
        assert L.cv_mi_forward(kind, ctypes.byref(mlp), p, 4, p, 4, 8, None, 0, p, p, p, None) != 0
        assert b"MLP weights missing" in L.cv_last_error(), (kind, L.cv_last_error())
        assert L.cv_mi_backward(kind, ctypes.byref(mlp), p, 4, p, 4, 8, p, None, 1.0, p, p, 4, 0, None, None, None,
                                None, 0, None) != 0
        assert b"MLP weights missing" in L.cv_last_error(), (kind, L.cv_last_error())
    assert L.cv_mi_forward(_lib.MI_CLUBMEAN, ctypes.byref(mlp), p, 4, p, 4, 1, None, 0, None, p, p, None) != 0
    assert b"mi_forward: bad args" in L.cv_last_error(), L.cv_last_error()
    assert L.cv_mi_backward(_lib.MI_CLUBMEAN, ctypes.byref(mlp), p, 4, p, 4, 1, p, None, 1.0, p, p, 4, 0, None, None,
                            None, None, 0, None) != 0
    assert b"mi_backward: bad args" in L.cv_last_error(), L.cv_last_error()
    full, buf2 = _mlp()
    assert L.cv_mi_forward(_lib.MI_CLUBMEAN, ctypes.byref(full), p, 4, p, 4, 8, None, 0, None, p, p, None) != 0
    assert b"CV_MI_CLUBMEAN" in L.cv_last_error(), L.cv_last_error()
    # the learning step has no kind argument: the gradient struct must follow the MLP's shape
    g_full = _lib.cv_mlp_grad(p, p, p, p, p, p, p, p)
    assert L.cv_mi_learning_step(ctypes.byref(mlp), p, 4, p, 4, 8, p, p, ctypes.byref(g_full), None, None, None, None,
                                 0, None, None, None) != 0
    assert b"p_logvar gradients follow" in L.cv_last_error(), L.cv_last_error()
    for partial in ("w3", "b4"):  # some but not all of the p_logvar pointers: nobody's MLP
        m2, _ = _mlp()
        setattr(m2, partial, None)
        assert L.cv_mi_learning_step(ctypes.byref(m2), p, 4, p, 4, 8, p, p, ctypes.byref(g_full), None, None, None,
                                     None, 0, None, None, None) != 0
        assert b"MLP weights missing" in L.cv_last_error(), L.cv_last_error()


def test_device_envelope_of_the_two_classes():
    CLUBMean, InfoNCE = _classes()
    assert CLUBMean(8, 8, 16, backend="device").device_supported(64)
    assert not CLUBMean(8, 8, None, backend="device").device_supported(64)  # a single Linear: the torch path
    assert not CLUBMean(8, 8, 65, backend="device").device_supported(64)
    assert not CLUBMean(8, 8, 16, backend="device").device_supported(1)
    assert InfoNCE(8, 8, 16, backend="device").device_supported(64)
    assert InfoNCE(32, 32, 64, backend="device").device_supported(4096)
    assert not InfoNCE(8, 8, 65, backend="device").device_supported(64)
    assert not InfoNCE(65, 8, 16, backend="device").device_supported(64)
    assert not InfoNCE(8, 8, 16, backend="device").device_supported(1)
