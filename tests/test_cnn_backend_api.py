"""The public switch of the device CNN baseline and the host side of its C-ABI, without a GPU:
SimpleCNNTrainer(backend=...) / CVHIP_CNN / get_cnn_trainer(backend=...), cv_cls_supported at its corners,
cv_cls_workspace_bytes, and the host validation of cv_cls_step / cv_cls_forward (nothing is launched)."""

import ctypes

import pytest
import torch
from torch import nn


def _trainer(cls=None, **kw):
    from src.models.cnn import SimpleCNNClassifier
    from src.trainer import SimpleCNNTrainer

    model = SimpleCNNClassifier(10, 1)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    return (cls or SimpleCNNTrainer)(model, opt, nn.CrossEntropyLoss(), 5, torch.device("cpu"), **kw)


def test_backend_names(monkeypatch):
    from src.trainer import SimpleCNNTrainer

    monkeypatch.delenv("CVHIP_CNN", raising=False)
    assert SimpleCNNTrainer.BACKENDS == ("torch", "device")
    assert _trainer().backend == "torch"
    assert _trainer(backend="torch").backend == "torch"
    assert _trainer(backend="device").backend == "device"
    with pytest.raises(ValueError):
        _trainer(backend="hip")
    assert _trainer(backend="torch")._engine is None


def test_environment_variable(monkeypatch):
    monkeypatch.setenv("CVHIP_CNN", "device")
    assert _trainer().backend == "device"
    assert _trainer(backend="torch").backend == "torch"  # (the keyword wins)
    monkeypatch.setenv("CVHIP_CNN", "bogus")
    with pytest.raises(ValueError):
        _trainer()
    monkeypatch.setenv("CVHIP_CNN", "")
    assert _trainer().backend == "torch"


def test_get_cnn_trainer_and_lam_pass_the_backend_through(monkeypatch):
    from src.models.cnn import LAMCNNClassifier
    from src.trainer import LAMCNNTrainer
    from src.utils.trainer_utils import get_cnn_trainer

    monkeypatch.delenv("CVHIP_CNN", raising=False)
    assert get_cnn_trainer(10, torch.device("cpu"), backend="device").backend == "device"
    assert get_cnn_trainer(10, torch.device("cpu")).backend == "torch"
    assert get_cnn_trainer(4, torch.device("cpu"), "SimpleCNN64Classifier", 3, 5).backend == "torch"
    model = LAMCNNClassifier(10, 1)
    tr = LAMCNNTrainer(model, torch.optim.Adam(model.parameters()), nn.CrossEntropyLoss(), {"lam_coef": 0.1}, 5,
                       torch.device("cpu"), backend="device")
    assert tr.backend == "device" and tr.hyperparameter == {"lam_coef": 0.1}


def test_contract_refuses_on_the_cpu_and_the_lam_models():
    from cvhip.cnn import CnnStep, cnn_spec
    from src.models.cnn import LAMCNNClassifier, SimpleCNN64Classifier

    assert "ROCm device" in CnnStep.unsupported_reason(_trainer(backend="device"))
    assert isinstance(cnn_spec(LAMCNNClassifier(10, 1)), str)
    sp = cnn_spec(SimpleCNN64Classifier(4, 3))
    assert (sp.in_ch, sp.H, sp.W, sp.feat, len(sp.enc)) == (3, 64, 64, (512, 2, 2), 5)
    sp = cnn_spec(_trainer().model)
    assert (sp.in_ch, sp.H, sp.W, sp.feat, len(sp.enc)) == (1, 28, 28, (128, 4, 4), 3)


def test_cls_supported_corners_and_workspace():
    from cvhip import _lib

    L = _lib.lib()
    for n, want in ((1, 0), (2, 1), (1024, 1), (1025, 0)):
        assert bool(L.cv_cls_supported(n, 256, 10)) == bool(want), n
    for h, want in ((0, 0), (1, 1), (512, 1), (513, 0)):
        assert bool(L.cv_cls_supported(128, h, 10)) == bool(want), h
    for c, want in ((1, 0), (2, 1), (32, 1), (33, 0)):
        assert bool(L.cv_cls_supported(128, 256, c)) == bool(want), c
    for shape in ((128, 256, 10), (2, 16, 2), (37, 130, 7), (1024, 512, 32)):
        nb = int(L.cv_cls_workspace_bytes(*shape))
        assert nb > 0 and nb % 16 == 0, (shape, nb)


def test_cls_host_validation_launches_nothing():
    """NULL pointers, a misaligned workspace or an unsupported shape are rejected on the host, with the entry's name
    in cv_last_error() (fake non-NULL addresses are never dereferenced: no launch happens)."""
    from cvhip import _lib

    L = _lib.lib()
    ok = _lib.cv_cls(16, 16, 16, 16, 16, 16, None, 256, 10, 1e-5, 0.1)
    G = _lib.cv_cls_grad(16, 16, 16, 16)
    ref = ctypes.byref

    def step(P, a=16, label=16, n=128, work=16, loss=16, da=16, g=G):
        rc = L.cv_cls_step(ref(P) if P is not None else None, a, label, n, work, loss, da,
                           ref(g) if g is not None else None, None)
        return rc, L.cv_last_error()

    bad = [
        step(None),
        step(_lib.cv_cls(None, 16, 16, 16, 16, 16, None, 256, 10, 1e-5, 0.1)),
        step(_lib.cv_cls(16, 16, 16, 16, None, 16, None, 256, 10, 1e-5, 0.1)),
        step(ok, a=None), step(ok, label=None), step(ok, work=None), step(ok, loss=None), step(ok, da=None),
        step(ok, g=None), step(ok, g=_lib.cv_cls_grad(16, None, 16, 16)),
        step(ok, work=24),  # not 16-byte aligned
        step(ok, n=1), step(ok, n=1025),
        step(_lib.cv_cls(16, 16, 16, 16, 16, 16, None, 513, 10, 1e-5, 0.1)),
        step(_lib.cv_cls(16, 16, 16, 16, 16, 16, None, 256, 33, 1e-5, 0.1)),
        step(_lib.cv_cls(16, 16, 16, 16, 16, 16, None, 256, 1, 1e-5, 0.1)),
    ]
    for rc, msg in bad:
        assert rc != 0 and b"cls_step" in msg, (rc, msg)

    def fwd(P, a=16, n=5, logits=16):
        rc = L.cv_cls_forward(ref(P) if P is not None else None, a, n, logits, None)
        return rc, L.cv_last_error()

    bad = [
        fwd(None), fwd(_lib.cv_cls(16, 16, None, 16, 16, 16, None, 256, 10, 1e-5, 0.1)),
        fwd(ok, a=None), fwd(ok, logits=None), fwd(ok, n=0), fwd(ok, n=-3),
        fwd(_lib.cv_cls(16, 16, 16, 16, 16, 16, None, 513, 10, 1e-5, 0.1)),
    ]
    for rc, msg in bad:
        assert rc != 0 and b"cls_forward" in msg, (rc, msg)


def test_struct_sizes():
    from cvhip import _lib

    assert ctypes.sizeof(_lib.cv_cls) == 7 * 8 + 4 * 4
    assert ctypes.sizeof(_lib.cv_cls_grad) == 4 * 8
    assert _lib.cv_cls.h.offset == 56 and _lib.cv_cls.momentum.offset == 68
