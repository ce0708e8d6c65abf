"""Loss functions with the reference's names and signatures (code/src/losses.py).

Hot path — HIP kernels through cvhip.autograd:
  vae_loss           -> cv_mse_sum + cv_kl          (losses.py:36-50)
  contrastive_loss   -> cv_ntxent, all five sims    (losses.py:98-137)
                        "supcon_in_loss" / "supcon_out_loss" with backend="device" -> cv_supcon (losses.py:140-170)
The pairwise_* / snn_loss / supcon_*_loss / logsumexp helpers keep the reference's tensor-level semantics for
callers that use them directly (they are building blocks, not the trained path); the lam loss and the
sklearn metrics are outside the hot path and stay as in the reference (sklearn on CPU);
gMIG also has a device backend (cv_knn_mi through cvhip.metrics), chosen per call or with the environment
variable CVHIP_GMIG, and so does auc (cv_rank_auc, CVHIP_AUC).  The two supcon names of contrastive_loss
default to the reference's torch composition (backend="torch"); backend="device", or CVHIP_SUPCON=device,
runs them as HIP kernels in O(n d) memory (cvhip.autograd.SupConFn), which is what CLEARVAETrainer does when
its hyperparameter "loss_name" is one of them.
"""

from __future__ import annotations

import os
import warnings

import torch
import torch.nn.functional as F
from sklearn.feature_selection import mutual_info_classif
from sklearn.metrics import average_precision_score, roc_auc_score
from torch import Tensor

from cvhip import autograd as _ag
from cvhip._lib import SIM

# ----------------------------------------------------------------------------- metrics (CPU)


GMIG_BACKENDS = ("sklearn", "device")


def mutual_info_gap(label, latent_c, latent_s, backend=None):
    """gMIG (losses.py:10-16).  backend "sklearn" (the default) is the reference's computation: sklearn kNN MI on
    host copies of the latents.  "device" is the same estimator as a HIP kernel (cvhip.metrics.gmig): the latents
    stay on the device, ties are broken by index instead of sklearn's random noise, the value is deterministic.
    backend=None takes the environment variable CVHIP_GMIG when it is set, else "sklearn"."""
    if backend is None:
        backend = os.environ.get("CVHIP_GMIG") or "sklearn"
    if backend not in GMIG_BACKENDS:
        raise ValueError(f"mutual_info_gap: unknown backend {backend!r} (one of {', '.join(GMIG_BACKENDS)})")
    if backend == "device":
        from cvhip import metrics as _metrics

        return _metrics.gmig(label, latent_c, latent_s)
    label, latent_c, latent_s = label.cpu(), latent_c.cpu(), latent_s.cpu()
    p = torch.bincount(label) / len(label)
    H = float(-(p * torch.log(p)).sum())
    mi_c = mutual_info_classif(latent_c, label, discrete_features=False)
    mi_s = mutual_info_classif(latent_s, label, discrete_features=False)
    return (mi_c.mean() - mi_s.mean()) / H


def accurary(logit: torch.Tensor, y: torch.Tensor):
    yh = logit.argmax(dim=1).cpu()
    return (yh.view(-1) == y.view(-1)).float().mean()


AUC_BACKENDS = ("sklearn", "device")


def auc(logit: torch.Tensor, y: torch.Tensor, backend=None):
    """Per-class average precision and AUROC (losses.py:24-33).  backend "sklearn" (the default) is the reference's
    computation: sklearn on host copies of the softmax.  "device" computes the same rank statistics as a HIP kernel
    (cvhip.metrics.auc) on the logits where they are.  backend=None takes the environment variable CVHIP_AUC when
    it is set, else "sklearn"."""
    if backend is None:
        backend = os.environ.get("CVHIP_AUC") or "sklearn"
    if backend not in AUC_BACKENDS:
        raise ValueError(f"auc: unknown backend {backend!r} (one of {', '.join(AUC_BACKENDS)})")
    if backend == "device":
        from cvhip import metrics as _metrics

        return _metrics.auc(logit, y)
    num_classes = int(y.max() + 1)
    ph = logit.softmax(dim=1).detach().cpu()
    y = y.cpu()
    yb = torch.eye(num_classes)[y]
    aupr, auroc = dict(), dict()
    for i in range(num_classes):
        aupr[i] = round(average_precision_score(yb[:, i], ph[:, i]), 3)
        auroc[i] = round(roc_auc_score(yb[:, i], ph[:, i]), 3)
    return aupr, auroc


# ----------------------------------------------------------------------------- ELBO


def sample_level_reduction(tensor: Tensor):
    """sum over every non-batch dim, mean over the batch (losses.py:36-38)."""
    return tensor.sum(dim=list(range(len(tensor.shape)))[1:]).mean()


def vae_loss(x_reconstr, x, mu_c, mu_s, logvar_c, logvar_s):
    """(reconstruction, kl_c, kl_s) of losses.py:41-50 on the device."""
    _ag._require_gpu(x_reconstr, x, mu_c, mu_s, logvar_c, logvar_s)
    return _ag.VaeLossFn.apply(x_reconstr, x, mu_c, mu_s, logvar_c, logvar_s)


# ----------------------------------------------------------------------------- pairwise similarities


def pairwise_cosine(mu: torch.Tensor):
    return F.cosine_similarity(mu[None, :, :], mu[:, None, :], dim=-1)


def pairwise_l2(mu: torch.Tensor):
    return -((mu[None, :, :] - mu[:, None, :]) ** 2).sum(dim=-1)


def pairwise_jeffrey_div(mu: torch.Tensor, logvar: torch.Tensor):
    k = mu.shape[1]
    var = logvar.exp()
    t1 = logvar.sum(dim=-1)[None, :] - logvar.sum(dim=-1)[:, None] - k
    t2 = ((mu[None, :, :] - mu[:, None, :]) ** 2 / var).sum(dim=-1)
    t3 = (var[None, :, :] / (var[:, None, :] + 1e-8)).sum(dim=-1)
    kl = 0.5 * (t1 + t2 + t3)
    return -(0.5 * (kl + kl.T))


def pairwise_mahalanobis_dis(mu: torch.Tensor, logvar: torch.Tensor):
    var = 0.5 * (logvar.exp()[None, :, :] + logvar.exp()[:, None, :])
    return -((mu[None, :, :] - mu[:, None, :]) ** 2 / var).sum(dim=-1)


def pairwise_modified_l2_dis(mu: torch.Tensor, logvar: torch.Tensor):
    var = (0.5 * (logvar[None, :, :] + logvar[:, None, :])).exp()
    return -((mu[None, :, :] - mu[:, None, :]) ** 2 / var).sum(dim=-1)


def logsumexp(x: Tensor, dim: int) -> Tensor:
    """Stable logsumexp where an all -inf slice gives -inf (losses.py:87-95)."""
    m, _ = x.max(dim=dim)
    mask = m == -float("inf")
    s = (x - m.masked_fill(mask, 0).unsqueeze(dim=dim)).exp().sum(dim=dim)
    return s.masked_fill(mask, 1).log() + m.masked_fill(mask, -float("inf"))


# ----------------------------------------------------------------------------- contrastive


SUPCON_BACKENDS = ("torch", "device")
LOSS_NAMES = ("snn_loss", "supcon_in_loss", "supcon_out_loss")
_warned_supcon = False


def contrastive_loss(mu: torch.Tensor, logvar: torch.Tensor, label: torch.Tensor, sim_fn: str,
                     temperature: float, loss_name: str = "snn_loss", ps: bool = False, backend=None):
    """Contrastive loss of losses.py:98-126.  "snn_loss" is one fused HIP op (cv_ntxent): similarity, label
    masks, masked log-sum-exps and the mean over finite rows, with its analytic backward.

    "supcon_in_loss" / "supcon_out_loss" (losses.py:140-170) take a backend: "torch" (the default) is the
    reference's own composition as torch ops on the caller's tensors ([n, n] and, for three similarities, [n, n, d]
    intermediates); "device" is the same value as HIP kernels in O(n d) memory (cv_supcon through
    cvhip.autograd.SupConFn), for tensors on the ROCm device.  backend=None takes the environment variable
    CVHIP_SUPCON when it is set, else "torch".  Wider than d = 64 the device backend warns once and runs the torch
    composition.  "snn_loss" has no torch backend: naming one raises, and the environment variable is ignored."""
    if sim_fn not in SIM:
        raise ValueError("unimplemented similarity measure.")
    if loss_name in ("supcon_in_loss", "supcon_out_loss"):
        if backend is None:
            backend = os.environ.get("CVHIP_SUPCON") or "torch"
        if backend not in SUPCON_BACKENDS:
            raise ValueError(f"contrastive_loss: unknown backend {backend!r} (one of {', '.join(SUPCON_BACKENDS)})")
        if backend == "device":
            _ag._require_gpu(mu, logvar, label)
            from cvhip import _lib

            n, d = mu.shape
            if _lib.lib().cv_supcon_supported(int(n), int(d), SIM[sim_fn]):
                return _ag.SupConFn.apply(mu, logvar, label, sim_fn, temperature, bool(ps), _lib.SUPCON[loss_name])
            global _warned_supcon
            if not _warned_supcon:
                _warned_supcon = True
                warnings.warn(f"contrastive_loss: n={n}, d={d} is outside the device kernels' envelope "
                              "(1 <= n <= 131072, 1 <= d <= 64); running the torch composition")
        # The reference's own composition (losses.py:107-126 with its eval(loss_name) dispatch) over the pairwise /
        # supcon functions below, as torch ops on the caller's tensors.
        pair_mat = (label[None, :] != label[:, None]).float() if ps else (label[None, :] == label[:, None]).float()
        sim = {"cosine": lambda: pairwise_cosine(mu), "l2": lambda: pairwise_l2(mu),
               "modified_l2": lambda: pairwise_modified_l2_dis(mu, logvar),
               "jeffrey": lambda: pairwise_jeffrey_div(mu, logvar),
               "mahalanobis": lambda: pairwise_mahalanobis_dis(mu, logvar)}[sim_fn]()
        losses = (supcon_in_loss if loss_name == "supcon_in_loss" else supcon_out_loss)(sim, pair_mat, temperature)
        return losses[torch.isfinite(losses)].mean()
    if loss_name != "snn_loss":
        raise NameError(f"name '{loss_name}' is not defined")  # (what the reference's eval(loss_name) raises)
    if backend is not None and backend != "device":
        if backend not in SUPCON_BACKENDS:
            raise ValueError(f"contrastive_loss: unknown backend {backend!r} (one of {', '.join(SUPCON_BACKENDS)})")
        raise ValueError("contrastive_loss: snn_loss has no torch backend (it is always the device kernel cv_ntxent)")
    _ag._require_gpu(mu, logvar, label)
    return _ag.ContrastiveFn.apply(mu, logvar, label, sim_fn, temperature, bool(ps))


def snn_loss(sim: torch.Tensor, pair_mat: torch.Tensor, temperature: float):
    """Row losses from a similarity matrix (losses.py:129-137); fills the diagonal in place like the
    reference."""
    n = sim.shape[0]
    sim[torch.eye(n, device=sim.device).bool()] = float("-Inf")
    neg_mask = pair_mat == 0
    pos = pair_mat * sim
    pos[neg_mask] = float("-Inf")
    return -logsumexp(pos / temperature, dim=1) + logsumexp(sim / temperature, dim=1)


def supcon_in_loss(sim: torch.Tensor, pair_mat: torch.Tensor, temperature: float):
    n_k = pair_mat.sum(dim=1) - 1
    n = sim.shape[0]
    sim[torch.eye(n, device=sim.device).bool()] = float("-Inf")
    neg_mask = pair_mat == 0
    pos = pair_mat * sim
    pos[neg_mask] = float("-Inf")
    return n_k.log() - logsumexp(pos / temperature, dim=1) + logsumexp(sim / temperature, dim=1)


def supcon_out_loss(sim: torch.Tensor, pair_mat: torch.Tensor, temperature: float):
    n = sim.shape[0]
    sim[torch.eye(n, device=sim.device).bool()] = -999
    pos_mask = pair_mat * (1 - torch.eye(n)).to(sim.device)
    masked = sim * pos_mask
    n_k = pos_mask.sum(dim=1)
    select = n_k > 0
    return -masked.sum(dim=1)[select] / n_k[select] + logsumexp(sim[select] / temperature, dim=1)


def lam_loss(feature_x: torch.Tensor, feature_x_tilde: torch.Tensor, y: torch.Tensor,
             linear_w: torch.nn.Parameter):
    """Labelled LAM (losses.py:173-187), CNN baseline only."""
    w_y = linear_w[y]
    return ((feature_x * w_y - feature_x_tilde * w_y) ** 2).sum(dim=1).mean()
