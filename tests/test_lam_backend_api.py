"""The public switch of the device LAM baseline and the host side of its C-ABI, without a GPU:
LAMCNNTrainer(backend=...) / CVHIP_CNN / get_lamcnn_trainer(backend=...), lam_spec, LamStep.unsupported_reason on the
CPU, cv_lam_supported at the corners of its contract, cv_lam_workspace_bytes, and the host validation of cv_lam_step /
cv_lam_forward / cv_lam_pair (nothing is launched)."""

import ctypes

import pytest
import torch
from torch import nn


def _trainer(model=None, hyper=None, **kw):
    from src.models.cnn import LAMCNNClassifier
    from src.trainer import LAMCNNTrainer

    model = model or LAMCNNClassifier(10, 1)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    return LAMCNNTrainer(model, opt, nn.CrossEntropyLoss(), hyper or {"lam_coef": 0.1}, 5, torch.device("cpu"), **kw)


def test_backend_keyword_and_environment(monkeypatch):
    monkeypatch.delenv("CVHIP_CNN", raising=False)
    assert _trainer().backend == "torch"
    assert _trainer(backend="device").backend == "device"
    with pytest.raises(ValueError):
        _trainer(backend="hip")
    monkeypatch.setenv("CVHIP_CNN", "device")
    assert _trainer().backend == "device"
    assert _trainer(backend="torch").backend == "torch"  # (the keyword wins)


def test_get_lamcnn_trainer_passes_the_backend_through(monkeypatch):
    from src.trainer import LAMCNNTrainer
    from src.utils.trainer_utils import get_lamcnn_trainer

    monkeypatch.delenv("CVHIP_CNN", raising=False)
    tr = get_lamcnn_trainer(10, torch.device("cpu"), 0.1, backend="device")
    assert type(tr) is LAMCNNTrainer and tr.backend == "device" and tr.hyperparameter == {"lam_coef": 0.1}
    assert get_lamcnn_trainer(10, torch.device("cpu"), 0.1).backend == "torch"
    assert get_lamcnn_trainer(4, torch.device("cpu"), 0.5, "LAMCNN64Classifier", 3, 5).backend == "torch"


def test_lam_spec_accepts_the_lam_models_only():
    from cvhip.lam import lam_params, lam_spec
    from src.models.cnn import LAMCNN64Classifier, LAMCNNClassifier, SimpleCNN64Classifier, SimpleCNNClassifier

    sp = lam_spec(LAMCNNClassifier(10, 1))
    assert (sp.in_ch, sp.H, sp.W, sp.feat, len(sp.enc), sp.F) == (1, 28, 28, (128, 4, 4), 3, 2048)
    assert type(sp.head[0]) is nn.Linear and sp.head[0].out_features == 10 and len(lam_params(sp)) == 14
    sp = lam_spec(LAMCNN64Classifier(4, 3))
    assert (sp.in_ch, sp.H, sp.W, sp.feat, len(sp.enc), sp.F) == (3, 64, 64, (512, 2, 2), 5, 2048)
    assert isinstance(lam_spec(SimpleCNNClassifier(10, 1)), str)
    assert isinstance(lam_spec(SimpleCNN64Classifier(4, 3)), str)
    m = LAMCNNClassifier(10, 1)
    m.cls_head = nn.Linear(2048, 10, bias=False)
    assert "bias" in lam_spec(m)
    m.cls_head = nn.Linear(1024, 10)
    assert "1024" in lam_spec(m)


def test_unsupported_reason_on_the_cpu():
    from cvhip.lam import LamStep
    from src.models.cnn import SimpleCNNClassifier

    assert "ROCm device" in LamStep.unsupported_reason(_trainer(backend="device"))
    assert "SimpleCNNClassifier" in LamStep.unsupported_reason(_trainer(SimpleCNNClassifier(10, 1), backend="device"))
    assert LamStep.build(_trainer(backend="device")) is None


def test_lam_coef_must_be_a_finite_float():
    from cvhip.lam import _lam_coef

    for hyper, want in (({"lam_coef": 0.1}, 0.1), ({"lam_coef": 2}, 2.0), ({"lam_coef": float("nan")}, None),
                        ({"lam_coef": float("inf")}, None), ({"lam_coef": "0.1"}, None), ({"lam_coef": True}, None),
                        ({"other": 1.0}, None)):
        assert _lam_coef(_trainer(hyper=hyper)) == want, hyper


def test_lam_supported_corners_and_workspace():
    from cvhip import _lib

    L = _lib.lib()
    assert L.cv_lam_supported(128, 128, 16, 10) and L.cv_lam_supported(128, 512, 4, 4)  # the two reference trunks
    for n, want in ((1, 0), (2, 1), (1024, 1), (1025, 0)):
        assert bool(L.cv_lam_supported(n, 128, 16, 10)) == bool(want), n
        assert bool(L.cv_lam_supported(n, 512, 4, 32)) == bool(want), n
    for c, want in ((1, 0), (2, 1), (32, 1), (33, 0)):
        assert bool(L.cv_lam_supported(128, 128, 16, c)) == bool(want), c
    for pix, want in ((0, 0), (1, 1), (16, 1), (17, 0)):
        assert bool(L.cv_lam_supported(128, 8, pix, 10)) == bool(want), pix
    for ch, pix, want in ((0, 4, 0), (1, 1, 1), (2048, 1, 1), (2049, 1, 0), (128, 16, 1), (129, 16, 0), (227, 9, 1),
                          (228, 9, 0)):
        assert bool(L.cv_lam_supported(128, ch, pix, 10)) == bool(want), (ch, pix)
    for shape in ((128, 128, 16, 10), (128, 512, 4, 4), (2, 4, 1, 2), (5, 8, 9, 3), (37, 12, 16, 7), (1024, 16, 4, 32),
                  (1024, 128, 16, 32)):
        nb = int(L.cv_lam_workspace_bytes(*shape))
        assert nb > 0 and nb % 16 == 0, (shape, nb)
    assert int(L.cv_lam_workspace_bytes(1, 128, 16, 10)) == 0
    assert int(L.cv_lam_workspace_bytes(128, 128, 17, 10)) == 0


def test_lam_host_validation_launches_nothing():
    """NULL pointers, a misaligned workspace, an unsupported shape or n = 1 are rejected on the host, with the entry's
    name in cv_last_error() (fake non-NULL addresses are never dereferenced: no launch happens)."""
    from cvhip import _lib

    L = _lib.lib()
    ref = ctypes.byref
    n = 128

    def P(w=16, b=16, lam=16, c=10, ch=128, pix=16):
        return _lib.cv_lam(w, b, lam, c, ch, pix)

    def BN(C=128, count=n * 16, train=1, stat=16, rm=16, rv=16):
        return _lib.cv_bn(16, 16, stat, 16, rm, rv, C, count, train, 1e-5, None, None, None)

    G = _lib.cv_lam_grad(16, 16)

    def step(p=P(), y=16, bn=BN(), label=16, pair=16, n=n, work=16, loss=16, gin=16, gstat=16, g=G):
        rc = L.cv_lam_step(ref(p) if p is not None else None, y, ref(bn) if bn is not None else None, label, pair, n,
                           work, loss, gin, gstat, ref(g) if g is not None else None, None)
        return rc, L.cv_last_error()

    bad = [
        step(p=None), step(p=P(w=None)), step(p=P(b=None)), step(p=P(lam=None)),
        step(bn=None), step(bn=BN(C=64)), step(bn=BN(stat=None)), step(bn=BN(train=0)), step(bn=BN(count=n * 16 + 1)),
        step(y=None), step(label=None), step(pair=None), step(work=None), step(loss=None), step(gin=None),
        step(gstat=None), step(g=None), step(g=_lib.cv_lam_grad(16, None)), step(g=_lib.cv_lam_grad(None, 16)),
        step(work=24),  # not 16-byte aligned
        step(n=1, bn=BN(count=16)), step(n=1025, bn=BN(count=1025 * 16)),
        step(p=P(c=33)), step(p=P(c=1)), step(p=P(pix=17), bn=BN(count=n * 17)),
        step(p=P(ch=129), bn=BN(C=129)),
    ]
    for rc, msg in bad:
        assert rc != 0 and b"lam_step" in msg, (rc, msg)

    def fwd(p=P(), y=16, bn=BN(train=0), n=5, logits=16):
        rc = L.cv_lam_forward(ref(p) if p is not None else None, y, ref(bn) if bn is not None else None, n, logits,
                              None)
        return rc, L.cv_last_error()

    bad = [
        fwd(p=None), fwd(p=P(w=None)), fwd(p=P(b=None)), fwd(bn=None), fwd(bn=BN(C=64, train=0)),
        fwd(bn=BN(train=0, rm=None)), fwd(bn=BN(train=0, rv=None)),
        fwd(y=None), fwd(logits=None), fwd(n=0), fwd(n=-3), fwd(p=P(c=33)), fwd(p=P(pix=17)),
        fwd(p=P(ch=129), bn=BN(C=129, train=0)),
    ]
    for rc, msg in bad:
        assert rc != 0 and b"lam_forward" in msg, (rc, msg)

    def pair(label=16, n=64, out=16):
        rc = L.cv_lam_pair(label, n, 7, None, out, None)
        return rc, L.cv_last_error()

    for rc, msg in [pair(label=None), pair(out=None), pair(n=0), pair(n=1025), pair(n=-1)]:
        assert rc != 0 and b"lam_pair" in msg, (rc, msg)


def test_struct_sizes():
    from cvhip import _lib

    assert ctypes.sizeof(_lib.cv_lam) == 3 * 8 + 3 * 4 + 4  # (padded to the pointers' alignment)
    assert ctypes.sizeof(_lib.cv_lam_grad) == 2 * 8
    assert (_lib.cv_lam.w.offset, _lib.cv_lam.b.offset, _lib.cv_lam.lam.offset) == (0, 8, 16)
    assert (_lib.cv_lam.c.offset, _lib.cv_lam.in_ch.offset, _lib.cv_lam.in_pix.offset) == (24, 28, 32)
    assert (_lib.cv_lam_grad.w.offset, _lib.cv_lam_grad.b.offset) == (0, 8)
