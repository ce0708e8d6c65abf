"""The device SupCon losses through the public layers without a GPU: the backend switch of
src.losses.contrastive_loss for the two supcon names, the CV_SUPCON_* constants and the cv_supcon_args layout against
the header (a compiled C probe), every host-side rejection of cv_supcon (observed before any launch: the pointers are
host memory or NULL), the envelope query, the linear stats workspace, and loss_name through CLEARVAETrainer and its
factory."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SUPCON = ("supcon_in_loss", "supcon_out_loss")


def _fx():
    with np.load(os.path.join(HERE, "golden", "supcon.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _call(fx, loss, **kw):
    from src.losses import contrastive_loss

    return contrastive_loss(torch.tensor(fx["mu"]), torch.tensor(fx["logvar"]), torch.tensor(fx["label"]), "jeffrey",
                            float(fx["tau"]), loss_name=loss, **kw)


# ----------------------------------------------------------------------------- contrastive_loss(backend=)


@pytest.mark.parametrize("loss", SUPCON)
def test_backend_default_is_torch_and_env_switches(loss, monkeypatch):
    """No backend and no environment variable: the torch composition (the recorded reference value on CPU tensors).
    CVHIP_SUPCON=device, like backend="device", reaches the device path, which refuses CPU tensors with
    _require_gpu's error; an explicit backend="torch" wins over the environment."""
    fx = _fx()
    ref = float(fx[f"{loss}__jeffrey__ps0"])
    monkeypatch.delenv("CVHIP_SUPCON", raising=False)
    assert abs(float(_call(fx, loss)) - ref) <= 1e-12 * max(abs(ref), 1.0)
    assert abs(float(_call(fx, loss, backend="torch")) - ref) <= 1e-12 * max(abs(ref), 1.0)
    with pytest.raises(RuntimeError, match="HIP kernels need tensors on the ROCm device"):
        _call(fx, loss, backend="device")
    monkeypatch.setenv("CVHIP_SUPCON", "device")
    with pytest.raises(RuntimeError, match="HIP kernels need tensors on the ROCm device"):
        _call(fx, loss)
    assert abs(float(_call(fx, loss, backend="torch")) - ref) <= 1e-12 * max(abs(ref), 1.0)
    monkeypatch.setenv("CVHIP_SUPCON", "torch")
    assert abs(float(_call(fx, loss)) - ref) <= 1e-12 * max(abs(ref), 1.0)


@pytest.mark.parametrize("loss", SUPCON)
def test_bad_backend_raises(loss, monkeypatch):
    fx = _fx()
    monkeypatch.delenv("CVHIP_SUPCON", raising=False)
    with pytest.raises(ValueError, match="unknown backend 'hip'.*torch, device"):
        _call(fx, loss, backend="hip")
    monkeypatch.setenv("CVHIP_SUPCON", "gpu")
    with pytest.raises(ValueError, match="unknown backend 'gpu'.*torch, device"):
        _call(fx, loss)


def test_snn_loss_has_no_torch_backend(monkeypatch):
    """snn_loss + backend="torch" raises; the environment variable is not consulted for that name (CPU tensors get
    as far as _require_gpu, the error snn_loss has always raised for them)."""
    fx = _fx()
    monkeypatch.delenv("CVHIP_SUPCON", raising=False)
    with pytest.raises(ValueError, match="no torch backend"):
        _call(fx, "snn_loss", backend="torch")
    with pytest.raises(ValueError, match="unknown backend"):
        _call(fx, "snn_loss", backend="hip")
    for env in ("torch", "gpu"):
        monkeypatch.setenv("CVHIP_SUPCON", env)
        with pytest.raises(RuntimeError, match="HIP kernels need tensors on the ROCm device"):
            _call(fx, "snn_loss")
    with pytest.raises(RuntimeError, match="HIP kernels need tensors on the ROCm device"):
        _call(fx, "snn_loss", backend="device")


# ----------------------------------------------------------------------------- C-ABI


def test_constants_follow_the_header():
    from cvhip import _lib

    hdr = open(os.path.join(ROOT, "include", "clearvae.h")).read()
    for name, want in (("IN", 0), ("OUT", 1)):
        m = re.search(r"CV_SUPCON_%s = (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, "SUPCON_" + name) == want, name
    assert _lib.SUPCON == {"supcon_in_loss": _lib.SUPCON_IN, "supcon_out_loss": _lib.SUPCON_OUT}


FIELDS = ("mu", "logvar", "ld", "label", "n", "d", "sim", "ps", "kind", "temperature", "stats", "loss_out", "dmu",
          "dlogvar", "gld", "gscale")
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "clearvae.h"
#define S(T) printf(#T " size %zu\n", sizeof(T));
#define O(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  S(cv_supcon_args)
""" + "\n".join("  O(cv_supcon_args, %s)" % f for f in FIELDS) + r"""
  printf("enum %d %d\n", (int)CV_SUPCON_IN, (int)CV_SUPCON_OUT);
  return 0;
}
"""


def test_args_struct_layout_matches_header(tmp_path):
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
        if parts[0] == "enum":
            assert (int(parts[1]), int(parts[2])) == (_lib.SUPCON_IN, _lib.SUPCON_OUT)
            continue
        T = getattr(_lib, parts[0])
        if parts[1] == "size":
            assert ctypes.sizeof(T) == int(parts[2]), line
        else:
            assert getattr(T, parts[1]).offset == int(parts[2]), line
        seen += 1
    assert seen == 1 + len(FIELDS)
    assert [f[0] for f in _lib.cv_supcon_args._fields_] == list(FIELDS)


def _args(**kw):
    """A valid cv_supcon_args over host memory (nothing may read it: every case below is rejected first)."""
    from cvhip import _lib

    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    v = dict(mu=p, logvar=p, ld=4, label=p, n=8, d=4, sim=_lib.SIM["jeffrey"], ps=0, kind=_lib.SUPCON_IN,
             temperature=0.1, stats=p, loss_out=p, dmu=p, dlogvar=p, gld=4, gscale=p)
    v.update(kw)
    return _lib.cv_supcon_args(*[v[f] for f in FIELDS]), buf


REJECTIONS = [
    ("n = 0", dict(n=0), 0, b"batch must be in 1..131072"),
    ("n above the cap", dict(n=131073), 0, b"batch must be in 1..131072"),
    ("d = 0", dict(d=0), 1, b"width must be in 1..64"),
    ("d = 65", dict(d=65, ld=65, gld=65), 0, b"width must be in 1..64"),
    ("sim = 5", dict(sim=5), 0, b"unknown similarity"),
    ("sim = -1", dict(sim=-1), 1, b"unknown similarity"),
    ("kind = 2", dict(kind=2), 0, b"unknown kind"),
    ("kind = -1", dict(kind=-1), 1, b"unknown kind"),
    ("phase = 2", dict(), 2, b"phase must be 0 or 1"),
    ("phase = -1", dict(), -1, b"phase must be 0 or 1"),
    ("NULL mu", dict(mu=None), 0, b"mu, label and stats are required"),
    ("NULL label", dict(label=None), 1, b"mu, label and stats are required"),
    ("NULL stats", dict(stats=None), 0, b"mu, label and stats are required"),
    ("NULL logvar, jeffrey", dict(logvar=None), 0, b"reads logvar"),
    ("NULL logvar, mahalanobis", dict(logvar=None, sim=4), 1, b"reads logvar"),
    ("NULL logvar, modified_l2", dict(logvar=None, sim=2), 0, b"reads logvar"),
    ("temperature = 0", dict(temperature=0.0), 0, b"temperature must be positive"),
    ("temperature < 0", dict(temperature=-0.5), 1, b"temperature must be positive"),
    ("phase 0 without loss_out", dict(loss_out=None), 0, b"phase 0 needs loss_out"),
    ("phase 1 without dmu", dict(dmu=None), 1, b"phase 1 needs dmu and gscale"),
    ("phase 1 without gscale", dict(gscale=None), 1, b"phase 1 needs dmu and gscale"),
    ("ld < d", dict(ld=3), 0, b"row stride"),
]


@pytest.mark.parametrize("what,kw,phase,msg", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_supcon_rejects_before_any_launch(what, kw, phase, msg):
    from cvhip import _lib

    L = _lib.lib()
    a, buf = _args(**kw)
    rc = L.cv_supcon(ctypes.byref(a), phase, None)
    assert rc != 0, what
    err = L.cv_last_error()
    assert msg in err and err.startswith(b"supcon:"), (what, err)


def test_null_args_pointer_is_rejected():
    from cvhip import _lib

    L = _lib.lib()
    assert L.cv_supcon(None, 0, None) != 0
    assert b"supcon: null args" in L.cv_last_error()


def test_supported_is_exactly_the_envelope():
    from cvhip import _lib

    L = _lib.lib()
    for sim in range(5):
        for n, d in ((1, 1), (1, 64), (131072, 1), (131072, 64), (70, 10), (4096, 32)):
            assert L.cv_supcon_supported(n, d, sim) == 1, (n, d, sim)
    for bad in ((0, 8, 0), (-1, 8, 0), (131073, 8, 0), (64, 0, 0), (64, 65, 0), (64, -3, 0), (64, 8, -1), (64, 8, 5)):
        assert L.cv_supcon_supported(*bad) == 0, bad


def test_stats_workspace_is_linear_in_n():
    from cvhip import _lib

    L = _lib.lib()
    f = L.cv_supcon_stats_floats
    per_row = f(2) - f(1)
    assert per_row > 0
    for n in (1, 2, 70, 4096, 4097, 131072):
        assert f(n) == f(1) + (n - 1) * per_row, n
    # one n x n fp32 matrix at n = 4096 is 64 MiB; the statistics are a few floats per row
    assert f(4096) * 4 * 100 < 4096 * 4096 * 4


# ----------------------------------------------------------------------------- trainer / factory

KW = dict(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=16, alpha=100, temperature=0.1, device="cpu")
DEFAULT_HP = {"temperature": 0.1, "alpha": 100, "beta": 1 / 8, "ps": True, "loc": 0, "scale": 1}


def test_factory_default_dict_is_unchanged():
    from src.utils.trainer_utils import get_clearvae_trainer

    for tr in (get_clearvae_trainer(**KW), get_clearvae_trainer(loss_name="snn_loss", **KW)):
        assert tr.hyperparameter == DEFAULT_HP
        assert list(tr.hyperparameter) == list(DEFAULT_HP)
        assert tr.loss_name == "snn_loss" and tr._loss_kw == {}


@pytest.mark.parametrize("loss", SUPCON)
def test_factory_puts_a_supcon_name_into_the_dict(loss):
    from src.utils.trainer_utils import get_clearvae_trainer

    tr = get_clearvae_trainer(loss_name=loss, **KW)
    assert tr.hyperparameter == dict(DEFAULT_HP, loss_name=loss)
    assert tr.loss_name == loss
    assert tr._loss_kw == {"loss_name": loss, "backend": "device"}
    assert tr._fused() is None and tr._engine is None
    tr.use_fused = True
    assert tr._fused() is None


def test_unknown_loss_name_raises_at_construction():
    from src.utils.trainer_utils import get_clearvae_trainer

    with pytest.raises(NameError, match="name 'no_such_loss' is not defined"):
        get_clearvae_trainer(loss_name="no_such_loss", **KW)


def test_trainer_reads_the_key_from_a_hand_built_dict():
    from src.models.vae import VAE
    from src.trainer import CLEARVAETrainer

    vae = VAE(total_z_dim=16, in_channel=1)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    tr = CLEARVAETrainer(vae, opt, "cosine", dict(DEFAULT_HP, loss_name="supcon_out_loss"), 1, torch.device("cpu"))
    assert tr._fused() is None and tr._loss_kw["loss_name"] == "supcon_out_loss"
    with pytest.raises(NameError):
        CLEARVAETrainer(vae, opt, "cosine", dict(DEFAULT_HP, loss_name="supcon"), 1, torch.device("cpu"))
