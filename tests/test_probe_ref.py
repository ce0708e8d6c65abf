"""Without a GPU: the probe reference of tests/probe_ref.py against PyTorch itself, the seed rule, the backend switch
of DownstreamMLPTrainer, and the host-side validation of cv_probe_step / cv_probe_forward (every rejected call
returns before a launch, so the library needs no device)."""

import ctypes

import pytest
import torch
from torch import nn

import probe_ref as PR


def _module(inp):
    n, d, h, c, _ = inp["shape"]
    m = nn.Sequential(nn.Linear(d, h), nn.BatchNorm1d(h, eps=PR.EPS, momentum=PR.MOMENTUM), nn.ReLU(),
                      nn.Linear(h, c)).double()
    T = PR._t(inp, torch.float64)
    with torch.no_grad():
        for p, k in zip(m.parameters(), PR.NAMES):
            p.copy_(T[k])
        m[1].running_mean.copy_(T["rm"])
        m[1].running_var.copy_(T["rv"])
    return m, T


@pytest.mark.parametrize("shape", PR.SHAPES[:5] + PR.SHAPES[6:7], ids=PR.shape_id)
def test_reference_matches_torch(shape):
    """step_ref / eval_ref == nn.Sequential + nn.CrossEntropyLoss() + autograd in fp64, to 1e-12."""
    inp = PR.make_inputs(shape, 0)
    ref = PR.step_ref(inp)
    m, T = _module(inp)
    m.train()
    loss = nn.CrossEntropyLoss()(m(T["x"]), T["label"])
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 * abs(float(loss.detach()))
    for p, k in zip(m.parameters(), PR.NAMES):
        if k == "b1":  # mathematically zero: rounding noise on both sides
            assert float(p.grad.abs().max()) <= 1e-12 and float(ref[k].abs().max()) <= 1e-12
        else:
            assert PR.rel_l2(ref[k], p.grad) <= 1e-12, k
    assert PR.rel_l2(ref["rm"], m[1].running_mean) <= 1e-12
    assert PR.rel_l2(ref["rv"], m[1].running_var) <= 1e-12
    m2, T = _module(inp)
    m2.eval()
    with torch.no_grad():
        assert PR.rel_l2(PR.eval_ref(inp), m2(T["x"])) <= 1e-12


def test_seed_rule_finds_a_seed_for_every_shape():
    for shape in PR.SHAPES:
        seed = PR.find_seed(shape)
        assert seed is not None, shape
        assert PR.step_ref(PR.make_inputs(shape, seed))["margin"] >= PR.MASK_MARGIN


# ------------------------------------------------------------------------------------------------ trainer switch
def _trainer(**kw):
    from src.models.vae import VAE
    from src.trainer import DownstreamMLPTrainer

    mlp = nn.Sequential(nn.Linear(8, 16), nn.BatchNorm1d(16), nn.ReLU(), nn.Linear(16, 3))
    opt = torch.optim.Adam(mlp.parameters(), lr=3e-4)
    return DownstreamMLPTrainer(VAE(16, 1), mlp, opt, nn.CrossEntropyLoss(), 10, torch.device("cpu"), **kw)


def test_backend_switch(monkeypatch):
    monkeypatch.delenv("CVHIP_PROBE", raising=False)
    assert _trainer().backend == "torch"
    assert _trainer(backend="device").backend == "device"
    with pytest.raises(ValueError):
        _trainer(backend="bogus")
    monkeypatch.setenv("CVHIP_PROBE", "device")
    assert _trainer().backend == "device"
    assert _trainer(backend="torch").backend == "torch"  # (an explicit argument wins)
    monkeypatch.setenv("CVHIP_PROBE", "bogus")
    with pytest.raises(ValueError):
        _trainer()


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_probe_supported_contract():
    from cvhip import _lib

    ok = _lib.lib().cv_probe_supported
    for n in (2, 1024):
        for d in (1, 64):
            for h in (1, 512):
                for c in (2, 32):
                    assert ok(n, d, h, c) == 1, (n, d, h, c)
    assert ok(128, 8, 256, 10) == 1 and ok(32, 32, 256, 10) == 1
    assert ok(1, 8, 256, 10) == 0 and ok(0, 8, 256, 10) == 0
    assert ok(128, 0, 256, 10) == 0 and ok(128, 8, 0, 10) == 0 and ok(128, 8, 256, 0) == 0
    wb = _lib.lib().cv_probe_workspace_bytes
    assert wb(128, 256, 10) > 0 and wb(128, 256, 10) % 16 == 0 and wb(1024, 512, 32) >= wb(128, 256, 10)


A = 0x10000  # a fake, 16-byte aligned device address: validation never dereferences it


def _structs(d=8, h=16, c=3, **over):
    from cvhip import _lib

    o = {k: A + 0x1000 * (i + 1) for i, k in enumerate(("w1", "b1", "gamma", "beta", "w2", "b2"))}
    P = dict(o, running_mean=A + 0x8000, running_var=A + 0x9000, nbt=None)
    P.update({k[2:]: v for k, v in over.items() if k.startswith("P_")})
    G = {k: A + 0x100000 + 0x1000 * (i + 1) for i, k in enumerate(("w1", "b1", "gamma", "beta", "w2", "b2"))}
    G.update({k[2:]: v for k, v in over.items() if k.startswith("G_")})
    probe = _lib.cv_probe(P["w1"], P["b1"], P["gamma"], P["beta"], P["w2"], P["b2"], P["running_mean"],
                          P["running_var"], P["nbt"], d, h, c, 1e-5, 0.1)
    grad = _lib.cv_probe_grad(G["w1"], G["b1"], G["gamma"], G["beta"], G["w2"], G["b2"])
    return probe, grad


def _step(probe, grad, x=A + 0x200000, ldx=8, label=A + 0x210000, n=4, work=A + 0x220000, loss=A + 0x230000,
          adam=(None, None, None, None, 0, None, None)):
    from cvhip import _lib

    L = _lib.lib()
    rc = L.cv_probe_step(ctypes.byref(probe), x, ldx, label, n, work, loss, ctypes.byref(grad) if grad else None,
                         *adam, None)
    return rc, L.cv_last_error().decode()


def _arena(params=A, grads=A + 0x100000, numel=0x4000, m=A + 0x300000, v=A + 0x400000, hyper=A + 0x500000,
           step=A + 0x500100):
    return (params, grads, m, v, numel, hyper, step)


@pytest.mark.parametrize("what,kw,word", [
    ("n below 2", dict(n=1), "unsupported shape"),
    ("n above the contract", dict(n=1025), "unsupported shape"),
    ("x missing", dict(x=None), "missing"),
    ("label missing", dict(label=None), "missing"),
    ("work missing", dict(work=None), "missing"),
    ("loss_out missing", dict(loss=None), "missing"),
    ("work unaligned", dict(work=A + 4), "aligned"),
    ("ldx below d", dict(ldx=7), "ldx"),
    ("arena without grads", dict(adam=_arena(grads=None)), "incomplete"),
    ("arena without moments", dict(adam=_arena(m=None)), "incomplete"),
    ("arena without step", dict(adam=_arena(step=None)), "incomplete"),
    ("arena of no elements", dict(adam=_arena(numel=0)), "incomplete"),
    ("gradients before the arena", dict(adam=_arena(grads=A + 0x102000)), "grads arena"),
    ("gradients past the arena", dict(adam=_arena(numel=0x400)), "grads arena"),
    ("parameters at another offset", dict(adam=_arena(params=A + 0x10)), "sits in params"),
])
def test_step_validation_rejects(what, kw, word):
    probe, grad = _structs()
    rc, msg = _step(probe, grad, **kw)
    assert rc != 0, what
    assert "probe_step" in msg and word in msg, (what, msg)


@pytest.mark.parametrize("over,word", [
    (dict(P_w1=None), "missing"), (dict(P_b2=None), "missing"), (dict(P_running_var=None), "missing"),
    (dict(G_gamma=None), "gradient buffers"), (dict(G_b2=None), "gradient buffers"),
])
def test_step_validation_rejects_null_fields(over, word):
    probe, grad = _structs(**over)
    rc, msg = _step(probe, grad)
    assert rc != 0 and word in msg, (over, msg)
    probe, grad = _structs()
    rc, msg = _step(probe, None)
    assert rc != 0 and "gradient buffers" in msg


def test_step_validation_rejects_shapes():
    for d, h, c in ((65, 16, 3), (8, 513, 3), (8, 16, 33), (8, 16, 1)):
        probe, grad = _structs(d, h, c)
        rc, msg = _step(probe, grad, ldx=128)
        assert rc != 0 and "unsupported shape" in msg, (d, h, c, msg)


def test_forward_validation_rejects():
    from cvhip import _lib

    L = _lib.lib()
    probe, _ = _structs()
    x, out = A + 0x200000, A + 0x240000
    for args, word in (((None, 8, 4, out), "missing"), ((x, 8, 4, None), "missing"), ((x, 7, 4, out), "ldx"),
                       ((x, 8, 0, out), "unsupported"), ((x, 8, 1025, out), "unsupported")):
        rc = L.cv_probe_forward(ctypes.byref(probe), *args, None)
        assert rc != 0 and word in L.cv_last_error().decode(), (args, L.cv_last_error())
    bad, _ = _structs(P_gamma=None)
    assert L.cv_probe_forward(ctypes.byref(bad), x, 8, 4, out, None) != 0


LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "clearvae.h"
#define S(T) printf(#T " size %zu\n", sizeof(T));
#define O(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  S(cv_probe) O(cv_probe, w1) O(cv_probe, b2) O(cv_probe, running_mean) O(cv_probe, running_var) O(cv_probe, nbt)
  O(cv_probe, d) O(cv_probe, h) O(cv_probe, c) O(cv_probe, eps) O(cv_probe, momentum)
  S(cv_probe_grad) O(cv_probe_grad, w1) O(cv_probe_grad, gamma) O(cv_probe_grad, b2)
  return 0;
}
"""


def test_probe_struct_layouts_match_header(tmp_path):
    """cv_probe / cv_probe_grad in cvhip/_lib.py against include/clearvae.h (as tests/test_abi.py does for the
    structs it lists): sizes and field offsets from a gcc-compiled program."""
    import os
    import subprocess

    from cvhip import _lib

    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT)
    r = subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    for line in filter(None, out.split("\n")):
        name, field, val = line.split()
        T = getattr(_lib, name)
        if field == "size":
            assert ctypes.sizeof(T) == int(val), line
        else:
            assert getattr(T, field).offset == int(val), line
