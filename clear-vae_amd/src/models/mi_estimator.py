"""MI estimators with the reference's modules and method names (code/src/models/mi_estimator.py).  The four
estimators over the q(y|x) network pair (p_mu, p_logvar) — CLUBSample and L1OutUB, which the CLEAR-MIM scripts
instantiate, and CLUB and VarUB, which `get_clearmimvae_trainer(mi_estimator=...)` resolves as
well — run on libclearvae_hip.so: forward / learning_loss / their gradients are HIP kernels
(cvhip.autograd.MIUpperBoundFn / LearningLossFn), and ClearStep fuses all four.  CLUB and VarUB keep their
plain-PyTorch forward on CPU tensors (they never raised there); CLUBSample and L1OutUB require the GPU.

CLUBMean (a different network: no p_logvar) and InfoNCE (a lower bound with a critic network), the other two names
the factory resolves, take a `backend` switch: "torch" (the default) is plain PyTorch tensor code; "device" runs
CUDA tensors on libclearvae_hip.so (CLUBMean through the CLUB kernels with logvar == 0, InfoNCE through
cv_infonce_* in O(N h) memory instead of the reference's [N, N, dx+dy] tiling) and lets ClearStep fuse them.  The
device envelope is 2 <= n (InfoNCE: n <= 16384), x_dim, y_dim, hidden_size <= 64 and, for CLUBMean, a hidden layer;
a call outside it warns once and runs the torch formulas.  `backend=None` reads CVHIP_MI_EST=torch|device.
"""

from __future__ import annotations

import os
import warnings

import torch
import torch.nn as nn
from torch import Tensor

from cvhip import autograd as _ag
from cvhip import _lib
from cvhip._lib import MI_CLUB, MI_CLUBMEAN, MI_CLUBSAMPLE, MI_L1OUT, MI_VARUB


def _q_nets(x_dim, y_dim, hidden_size):
    """p_mu and p_logvar MLPs of q(y|x) (mi_estimator.py:111-122)."""
    h = hidden_size // 2
    p_mu = nn.Sequential(nn.Linear(x_dim, h), nn.ReLU(), nn.Linear(h, y_dim))
    p_logvar = nn.Sequential(nn.Linear(x_dim, h), nn.ReLU(), nn.Linear(h, y_dim), nn.Tanh())
    return p_mu, p_logvar


class _QEstimator(nn.Module):
    def __init__(self, x_dim, y_dim, hidden_size):
        super().__init__()
        self.p_mu, self.p_logvar = _q_nets(x_dim, y_dim, hidden_size)

    def get_mu_logvar(self, x_samples):
        return self.p_mu(x_samples), self.p_logvar(x_samples)

    def loglikeli(self, x_samples, y_samples):
        if x_samples.device.type == "cuda":
            return -self.learning_loss(x_samples, y_samples)
        mu, logvar = self.get_mu_logvar(x_samples)
        return (-((mu - y_samples) ** 2) / logvar.exp() - logvar).sum(dim=1).mean(dim=0)

    def learning_loss(self, x_samples, y_samples):
        _ag._require_gpu(x_samples, y_samples)
        return _ag.LearningLossFn.apply(x_samples, y_samples, self, *_ag.est_params(self))


class CLUBSample(_QEstimator):
    """Sampled CLUB (mi_estimator.py:108-146); the negative pairs use a device permutation."""

    def forward(self, x_samples, y_samples):
        _ag._require_gpu(x_samples, y_samples)
        return _ag.MIUpperBoundFn.apply(x_samples, y_samples, self, MI_CLUBSAMPLE, *_ag.est_params(self))


class L1OutUB(_QEstimator):
    """Leave-one-out bound with the reference's exact broadcasting semantics (mi_estimator.py:149-198)."""

    def forward(self, x_samples, y_samples):
        _ag._require_gpu(x_samples, y_samples)
        return _ag.MIUpperBoundFn.apply(x_samples, y_samples, self, MI_L1OUT, *_ag.est_params(self))


class CLUB(_QEstimator):
    """The non-sampled CLUB bound (mi_estimator.py:43-55).  On the GPU the [N, N, d] negative term is evaluated
    through the column moments of y in O(N d); on CPU tensors the reference's broadcast formula."""

    def forward(self, x_samples, y_samples):
        if x_samples.device.type == "cuda":
            return _ag.MIUpperBoundFn.apply(x_samples, y_samples, self, MI_CLUB, *_ag.est_params(self))
        mu, logvar = self.get_mu_logvar(x_samples)
        positive = -((mu - y_samples) ** 2) / 2.0 / logvar.exp()
        negative = -((y_samples.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0 / logvar.exp()
        return (positive.sum(dim=-1) - negative.sum(dim=-1)).mean()


class VarUB(_QEstimator):
    """Variational upper bound (mi_estimator.py:222-224): the mean over all N * y_dim elements; independent of
    y_samples.  HIP kernels on the GPU, the reference's formula on CPU tensors."""

    def forward(self, x_samples, y_samples):
        if x_samples.device.type == "cuda":
            return _ag.MIUpperBoundFn.apply(x_samples, y_samples, self, MI_VARUB, *_ag.est_params(self))
        mu, logvar = self.get_mu_logvar(x_samples)
        return 1.0 / 2.0 * (mu**2 + logvar.exp() - 1.0 - logvar).mean()


# ----------------------------------------------------------------------------- CLUBMean, InfoNCE (backend switch)

MI_EST_BACKENDS = ("torch", "device")


def resolve_backend(backend=None) -> str:
    """"torch" or "device": the argument, else the environment variable CVHIP_MI_EST, else "torch"."""
    if backend is None:
        backend = os.environ.get("CVHIP_MI_EST") or "torch"
    if backend not in MI_EST_BACKENDS:
        raise ValueError(f"MI estimator backend must be one of {MI_EST_BACKENDS}, got {backend!r}")
    return backend


_warned = set()


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


class CLUBMean(nn.Module):
    """CLUB with logvar == 0 (mi_estimator.py:65-105).  backend="device": CUDA tensors run the CLUB kernels
    (CV_MI_CLUBMEAN) when there is a hidden layer and x_dim, y_dim, hidden_size <= 64."""

    def __init__(self, x_dim, y_dim, hidden_size=None, backend=None):
        super().__init__()
        self.backend = resolve_backend(backend)
        if hidden_size is None:
            self.p_mu = nn.Linear(x_dim, y_dim)
        else:
            self.p_mu = nn.Sequential(nn.Linear(x_dim, int(hidden_size)), nn.ReLU(), nn.Linear(int(hidden_size), y_dim))

    def device_supported(self, n=None) -> bool:
        """The geometry the device path serves (any batch of at least 2 rows)."""
        if not isinstance(self.p_mu, nn.Sequential):
            return False
        l1, l2 = self.p_mu[0], self.p_mu[2]
        return (max(l1.in_features, l1.out_features, l2.out_features) <= 64 and l1.in_features == l2.out_features
                and (n is None or n >= 2))

    def _device(self, x_samples, y_samples) -> bool:
        if self.backend != "device" or x_samples.device.type != "cuda":
            return False
        if self.device_supported(x_samples.shape[0]) and x_samples.dim() == 2:
            return True
        _warn_once(("CLUBMean", id(self)), "CLUBMean(backend='device'): outside the device envelope (a hidden layer, "
                   "x_dim == y_dim <= 64, hidden_size <= 64, n >= 2); running the torch path")
        return False

    def get_mu_logvar(self, x_samples):
        return self.p_mu(x_samples), 0

    def forward(self, x_samples, y_samples):
        if self._device(x_samples, y_samples):
            return _ag.MIUpperBoundFn.apply(x_samples, y_samples, self, MI_CLUBMEAN, *_ag.est_params(self))
        mu, _ = self.get_mu_logvar(x_samples)
        positive = -((mu - y_samples) ** 2) / 2.0
        negative = -((y_samples.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0
        return (positive.sum(dim=-1) - negative.sum(dim=-1)).mean()

    def loglikeli(self, x_samples, y_samples):
        if self._device(x_samples, y_samples):
            return -self.learning_loss(x_samples, y_samples)
        mu, _ = self.get_mu_logvar(x_samples)
        return (-((mu - y_samples) ** 2)).sum(dim=1).mean(dim=0)

    def learning_loss(self, x_samples, y_samples):
        if self._device(x_samples, y_samples):
            return _ag.LearningLossFn.apply(x_samples, y_samples, self, *_ag.est_params(self))
        return -self.loglikeli(x_samples, y_samples)


def logsumexp(x: Tensor, dim: int) -> Tensor:
    """Masked-stable logsumexp (mi_estimator.py:234-242): an all -inf slice gives -inf."""
    m, _ = x.max(dim=dim)
    mask = m == -float("inf")
    s = (x - m.masked_fill(mask, 0).unsqueeze(dim=dim)).exp().sum(dim=dim)
    return s.masked_fill(mask, 1).log() + m.masked_fill(mask, -float("inf"))


class InfoNCE(nn.Module):
    """InfoNCE lower bound (mi_estimator.py:245-273).  backend="device": CUDA tensors run cv_infonce_* (the critic's
    first Linear factored into an x part and a y part, O(N h) memory) for 2 <= n <= 16384 and x_dim, y_dim,
    hidden_size <= 64."""

    def __init__(self, x_dim, y_dim, hidden_size, backend=None):
        super().__init__()
        self.backend = resolve_backend(backend)
        self.x_dim = int(x_dim)
        self.F_func = nn.Sequential(
            nn.Linear(x_dim + y_dim, hidden_size), nn.ReLU(), nn.Linear(hidden_size, 1), nn.Softplus()
        )

    def device_supported(self, n=None, x_dim=None) -> bool:
        l1 = self.F_func[0]
        dx = self.x_dim if x_dim is None else int(x_dim)
        return bool(_lib.lib().cv_infonce_supported(2 if n is None else int(n), dx, l1.in_features - dx,
                                                    l1.out_features))

    def _device(self, x_samples, y_samples) -> bool:
        if self.backend != "device" or x_samples.device.type != "cuda":
            return False
        if (x_samples.dim() == 2 and y_samples.dim() == 2
                and x_samples.shape[1] + y_samples.shape[1] == self.F_func[0].in_features
                and self.device_supported(x_samples.shape[0], x_samples.shape[1])):
            return True
        _warn_once(("InfoNCE", id(self)), "InfoNCE(backend='device'): outside the device envelope (2 <= n <= 16384, "
                   "x_dim, y_dim, hidden_size <= 64); running the torch path")
        return False

    def forward(self, x_samples, y_samples):
        if self._device(x_samples, y_samples):
            return _ag.InfoNCEFn.apply(x_samples, y_samples, self, *_ag.est_params(self))
        n = y_samples.shape[0]
        x_tile = x_samples.unsqueeze(0).repeat((n, 1, 1))
        y_tile = y_samples.unsqueeze(1).repeat((1, n, 1))
        t0 = self.F_func(torch.cat([x_samples, y_samples], dim=-1))
        t1 = self.F_func(torch.cat([x_tile, y_tile], dim=-1))
        return t0.mean() - (t1.logsumexp(dim=1).mean() - torch.tensor(n).log())

    def learning_loss(self, x_samples, y_samples):
        if self._device(x_samples, y_samples):
            return _ag.InfoNCELearningLossFn.apply(x_samples, y_samples, self, *_ag.est_params(self))
        return -self.forward(x_samples, y_samples)
