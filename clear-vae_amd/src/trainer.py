"""Trainers with the reference's classes, constructor signatures, hyperparameter keys, step order,
printed values and return values (code/src/trainer.py).

CLEARVAETrainer / ClearMIMVAETrainer (the hot path) run each training step
as one fused HIP program (cvhip.engine.ClearStep: forward, ELBO, contrastive / MI terms, backward,
BatchNorm bookkeeping and Adam on a flat parameter arena, replayed as a HIP graph).  When the caller's
setup is outside what the fused step supports (e.g. an optimizer that is not a single-group Adam
over all VAE parameters), they fall back to the module-level HIP path (cvhip.autograd), which
replays the reference's loop literally.  Neither path computes on the CPU.

Per-step scalars that the reference reads with float() every step (trainer.py:486-492, 859, 888)
are kept on the device and copied once per epoch when the progress bar is disabled.
ClearTCVAETrainer runs fused too (mode "tc": the factor discriminator's density-ratio
term and its BCE step as HIP kernels), and so does HierarchicalVAETrainer (mode "group":
the GVAE / ML-VAE group evidence as label-segmented device reductions).  DownstreamMLPTrainer has an opt-in
device backend (cvhip.probe.ProbeStep: the probe's step as one HIP graph), and so does SimpleCNNTrainer
(cvhip.cnn.CnnStep: conv trunk, classifier tail, backward and Adam as one HIP graph) and LAMCNNTrainer
(cvhip.lam.LamStep: the reference's three trunk forwards as one, the LAM tail in cv_lam_step, backward and Adam as
one HIP graph).
"""

from __future__ import annotations

import math
import os
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.optim.optimizer import Optimizer
from torch.utils.data import DataLoader
from tqdm import tqdm

from src.losses import LOSS_NAMES, accurary, auc, contrastive_loss, lam_loss, mutual_info_gap, vae_loss
from src.models.vae import VAE


class LogisticAnnealer:
    """beta / (1 + exp(-(t - loc)/scale)) with t = optimizer steps taken (trainer.py:22-38)."""

    def __init__(self, loc, scale, beta) -> None:
        self.current_step = 0
        self.loc = loc
        self.scale = scale
        self.beta = beta

    def __call__(self, kl_loss) -> torch.Tensor:
        return kl_loss * self.slope()

    def slope(self) -> float:
        exponent = -(self.current_step - self.loc) / self.scale
        return self.beta / (1 + math.exp(exponent))

    def step(self) -> None:
        self.current_step += 1


class Trainer:
    def __init__(self, model: nn.Module, optimizer: Optimizer, verbose_period: int, device: torch.device,
                 transform=None) -> None:
        self.model = model
        self.optimizer = optimizer
        self.verbose_period = verbose_period
        self.device = device
        self.transform = transform

    def fit(self, epochs: int, train_loader: DataLoader, valid_loader: None | DataLoader = None):
        for epoch in range(epochs):
            verbose = (epoch % self.verbose_period) == 0
            self._train(train_loader, verbose, epoch)
            if valid_loader is not None:
                self._valid(valid_loader, verbose, epoch)

    def evaluate(self, **kwarg):
        pass

    def _train(self, **kwarg):
        pass

    def _valid(self, **kwarg):
        pass


class VAETrainer(Trainer):
    def _valid(self, dataloader, verbose, epoch_id):
        if verbose:
            mig, mse = self.evaluate(dataloader, verbose, epoch_id)
            print(f"gMIG: {round(mig, 3)}; mse: {round(float(mse), 3)}")


def _batch(batch, device, transform):
    X, label = batch[0], batch[1].reshape(-1).long()
    X, label = X.to(device), label.to(device)
    if transform:
        X = transform(X)
    return X, label


# ----------------------------------------------------------------------------- CLEAR-VAE


EVAL_BACKENDS = ("module", "fused")  # evaluate(backend=...) / CVHIP_EVAL of the VAE trainers


def _eval_backend(backend) -> str:
    """"module" or "fused": the argument, else the environment variable CVHIP_EVAL (read at the call, so the
    reference scripts switch without an edit), else "module"."""
    if backend is None:
        backend = os.environ.get("CVHIP_EVAL") or "module"
    if backend not in EVAL_BACKENDS:
        raise ValueError(f"evaluate: backend / CVHIP_EVAL must be one of {EVAL_BACKENDS}, not {backend!r}")
    return backend


class _FusedEval:
    """The fused evaluate() of the VAE trainers (cvhip.evaluate.EvalPass: each validation batch one replayed HIP
    graph, the epoch's sums and latents on the device, one host read at the end)."""

    _eval_pass = None
    _eval_warned = False

    def _eval_pass_for(self, mode, dataloader, why=None):
        """(pass, capacity), or (None, None) after warning once with the reason: the caller runs "module"."""
        from cvhip.evaluate import EvalPass

        cap = None
        if why is None:
            try:
                cap = len(dataloader.dataset)
            except (AttributeError, TypeError):
                why = "the loader has no dataset with a length (the epoch's capacity)"
        if why is None:
            ep = self._eval_pass
            if ep is None or ep.mode != mode or not ep.compatible():
                why = EvalPass.unsupported_reason(self, mode)
                ep = self._eval_pass = None if why is not None else EvalPass.build(self, mode)
            if ep is not None:
                return ep, cap
        if not self._eval_warned:
            self._eval_warned = True
            warnings.warn(f"{type(self).__name__}.evaluate(backend='fused') runs as 'module': {why}", stacklevel=3)
        return None, None

    def _evaluate_fused(self, ep, cap, dataloader, verbose, epoch_id, names, module_batch):
        """module_batch(X, label) -> (values, z): the module path's values of a batch the pass refuses (one sample,
        another image shape)."""
        ep.begin(cap)
        with torch.no_grad():
            for batch in tqdm(dataloader, disable=not verbose, desc=f"val-epoch {epoch_id}"):
                X, label = _batch(batch, self.device, None)
                if ep.accepts(X):
                    ep.batch(X, label)
                else:
                    values, z = module_batch(X, label)
                    ep.add_module_batch(values, z, label)
        totals, _, labels, lat_c, lat_s = ep.finish()
        mig = mutual_info_gap(labels, lat_c, lat_s)
        nb = len(dataloader)
        mse = float(totals[0] / nb)
        if verbose:
            print(", ".join("val_" + nm + "={:.3f}" for nm in names).format(*[t / nb for t in totals[:len(names)]]))
        return mig, mse


class _ClearEval(_FusedEval):
    """evaluate() shared by the CLEAR trainers (trainer.py:495-570, 899-965): eval-mode forward on the
    HIP path under no_grad, the same losses, gMIG by mutual_info_gap (sklearn on the CPU as in the reference, or
    the device kernel with CVHIP_GMIG=device).  backend "fused" (or CVHIP_EVAL=fused) runs the same epoch through
    cvhip.evaluate.EvalPass; a setup outside its contract warns once and runs "module"."""

    def _module_batch(self, X, label, last_fn):
        vae, hp = self.model, self.hyperparameter
        X_hat, lp, z = vae(X, explicit=True)
        rec, kl_c, kl_s = vae_loss(X_hat, X, **lp)
        c_loss = contrastive_loss(mu=lp["mu_c"], logvar=lp["logvar_c"], label=label, sim_fn=self.sim_fn,
                                  temperature=hp["temperature"], **getattr(self, "_loss_kw", {}))
        last = last_fn(lp, label, z)
        return (rec, kl_c, kl_s, c_loss, last), z

    def _evaluate(self, dataloader, verbose, epoch_id, last_name, last_fn, backend="module", mode=None):
        vae = self.model
        vae.eval()
        if backend == "fused":
            ep, cap = self._eval_pass_for(mode, dataloader)
            if ep is not None:
                return self._evaluate_fused(ep, cap, dataloader, verbose, epoch_id,
                                            ("recontr_loss", "kl_c", "kl_s", "c_loss", last_name),
                                            lambda X, label: self._module_batch(X, label, last_fn))
        totals = [0.0] * 5
        labels, lat_c, lat_s = [], [], []
        with torch.no_grad():
            for batch in tqdm(dataloader, disable=not verbose, desc=f"val-epoch {epoch_id}"):
                X, label = _batch(batch, self.device, self.transform)
                values, z = self._module_batch(X, label, last_fn)
                for i, v in enumerate(values):
                    totals[i] += v
                labels.append(label)
                lat_c.append(z[:, : vae.z_dim])
                lat_s.append(z[:, vae.z_dim:])
        mig = mutual_info_gap(torch.cat(labels), torch.cat(lat_c), torch.cat(lat_s))
        nb = len(dataloader)
        mse = float(totals[0] / nb)
        if verbose:
            print(
                ("val_recontr_loss={:.3f}, val_kl_c={:.3f}, val_kl_s={:.3f}, val_c_loss={:.3f}, val_" + last_name
                 + "={:.3f}").format(*[t / nb for t in totals])
            )
        return mig, mse


LOSS_STEPS = ("module", "fused")  # hyperparameter["loss_step"] / CVHIP_SUPCON_STEP of a supcon loss_name


class CLEARVAETrainer(VAETrainer, _ClearEval):
    def __init__(self, model: VAE, optimizer: Optimizer, sim_fn: str, hyperparameter: dict[str, float],
                 verbose_period: int, device: torch.device, transform=None) -> None:
        super().__init__(model, optimizer, verbose_period, device, transform)
        self.sim_fn = sim_fn
        self.hyperparameter = hyperparameter
        self.annealer = LogisticAnnealer(loc=hyperparameter["loc"], scale=hyperparameter["scale"],
                                         beta=hyperparameter["beta"])
        self._engine = None
        self.use_fused = True
        # "loss_name" (not a key of the reference's dict; default its snn_loss): a supcon name trains with the device
        # SupCon kernels (src.losses.contrastive_loss, backend="device") on the module path, or, opted in with
        # "loss_step": "fused" (absent: the environment's CVHIP_SUPCON_STEP, absent too: "module"), as the fused
        # engine's one-graph step (cvhip.engine.ClearStep with cv_supcon_step).  snn_loss ignores the key: its step
        # is always the fused one.
        self.loss_name = hyperparameter.get("loss_name", "snn_loss")
        if self.loss_name not in LOSS_NAMES:
            raise NameError(f"name '{self.loss_name}' is not defined")
        self._loss_kw = {} if self.loss_name == "snn_loss" else {"loss_name": self.loss_name, "backend": "device"}
        if hyperparameter.get("loss_step") not in (None,) + LOSS_STEPS:
            raise ValueError(f"loss_step must be one of {LOSS_STEPS}, not {hyperparameter.get('loss_step')!r}")
        self._check_single_process()

    def loss_step(self) -> str:
        """How a supcon loss_name trains, "module" or "fused": the hyperparameter, else CVHIP_SUPCON_STEP, else
        "module"; read when the step is asked for, so the environment may change between epochs."""
        step = self.hyperparameter.get("loss_step")
        if step is None:
            step = os.environ.get("CVHIP_SUPCON_STEP", "module")
        if step not in LOSS_STEPS:
            raise ValueError(f"loss_step / CVHIP_SUPCON_STEP must be one of {LOSS_STEPS}, not {step!r}")
        return step

    def _check_single_process(self):
        if self._loss_kw and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            raise NotImplementedError(f"CLEARVAETrainer: loss_name={self.loss_name!r} is not data parallel "
                                      "(only snn_loss has a fused multi-device step)")

    def _fused(self):
        if not self.use_fused or (self._loss_kw and self.loss_step() != "fused"):
            return None
        from cvhip.engine import ClearStep

        if self._engine is None or not self._engine.compatible():
            self._engine = ClearStep.build(self, mode="clear")
        return self._engine

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        vae = self.model
        vae.train()
        hp = self.hyperparameter
        self._check_single_process()
        engine = self._fused()
        with tqdm(dataloader, unit="batch", mininterval=0, disable=not verbose) as bar:
            bar.set_description(f"Epoch {epoch_id}")
            for batch in bar:
                X, label = _batch(batch, self.device, self.transform)
                if engine is not None and engine.accepts(X):
                    if getattr(self, "_resync", False):
                        engine.resync_from_host()
                        self._resync = False
                    losses = engine.step(X, label)
                    self.annealer.step()
                    if verbose:
                        v = losses.tolist()
                        s_loss = v[4] if hp["ps"] else -v[4]
                        bar.set_postfix(recontr_loss=v[0], kl_c=v[1], kl_s=v[2], c_loss=v[3], s_loss=s_loss)
                    continue
                if engine is not None:
                    engine.sync_host_state()
                    self._resync = True
                self.optimizer.zero_grad()
                X_hat, lp = vae(X)
                rec, kl_c, kl_s = vae_loss(X_hat, X, **lp)
                c_loss = contrastive_loss(mu=lp["mu_c"], logvar=lp["logvar_c"], label=label, sim_fn=self.sim_fn,
                                          temperature=hp["temperature"], **self._loss_kw)
                s_loss = contrastive_loss(mu=lp["mu_s"], logvar=lp["logvar_s"], label=label, sim_fn=self.sim_fn,
                                          temperature=hp["temperature"], ps=hp["ps"], **self._loss_kw)
                if not hp["ps"]:
                    s_loss = -s_loss
                loss = (rec + self.annealer(kl_c) + self.annealer(kl_s) + hp["alpha"] * c_loss
                        + hp["alpha"] * s_loss)
                loss.backward()
                self.optimizer.step()
                self.annealer.step()
                if verbose:
                    bar.set_postfix(recontr_loss=float(rec), kl_c=float(kl_c), kl_s=float(kl_s),
                                    c_loss=float(c_loss), s_loss=float(s_loss))
        if engine is not None:
            engine.sync_host_state()

    def evaluate(self, dataloader, verbose, epoch_id, backend=None):
        backend = _eval_backend(backend)
        hp = self.hyperparameter

        def s_term(lp, label, z):
            s = contrastive_loss(mu=lp["mu_s"], logvar=lp["logvar_s"], label=label, sim_fn=self.sim_fn,
                                 temperature=hp["temperature"], ps=hp["ps"], **self._loss_kw)
            return s if hp["ps"] else -s

        return self._evaluate(dataloader, verbose, epoch_id, "s_loss", s_term, backend, "clear")


# ----------------------------------------------------------------------------- CLEAR-MIM


class ClearMIMVAETrainer(VAETrainer, _ClearEval):
    def __init__(self, model: VAE, mi_estimator: nn.Module, optimizers: dict[str, Optimizer], sim_fn: str,
                 hyperparameter: dict[str, float], verbose_period: int, device: torch.device,
                 transform=None) -> None:
        super().__init__(model, optimizers["vae_optim"], verbose_period, device, transform)
        self.sim_fn = sim_fn
        self.mi_estimator_optimizer = optimizers["mi_estimator_optim"]
        self.mi_estimator = mi_estimator
        self.hyperparameter = hyperparameter
        self.annealer = LogisticAnnealer(loc=hyperparameter["loc"], scale=hyperparameter["scale"],
                                         beta=hyperparameter["beta"])
        self._engine = None
        self.use_fused = True

    def _fused(self):
        if not self.use_fused:
            return None
        from cvhip.engine import ClearStep

        if self._engine is None or not self._engine.compatible():
            self._engine = ClearStep.build(self, mode="mim")
        return self._engine

    def fit(self, epochs: int, train_loader: DataLoader, valid_loader: None | DataLoader = None):
        mi_losses, mi_learning_losses = [], []
        for epoch in range(epochs):
            verbose = (epoch % self.verbose_period) == 0
            self._train(train_loader, verbose, epoch, mi_losses, mi_learning_losses)
            if valid_loader is not None:
                self._valid(valid_loader, verbose, epoch)
        return mi_losses, mi_learning_losses

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int, mi_losses: list,
               mi_learning_losses: list):
        vae, est = self.model, self.mi_estimator
        vae.train()
        est.train()
        hp = self.hyperparameter
        engine = self._fused()
        dev_log = []  # device-side per-step scalars, converted once at the end of the epoch
        with tqdm(dataloader, unit="batch", mininterval=0, disable=not verbose) as bar:
            bar.set_description(f"Epoch {epoch_id}")
            for batch in bar:
                X, label = _batch(batch, self.device, self.transform)
                if engine is not None and engine.accepts(X):
                    if getattr(self, "_resync", False):
                        engine.resync_from_host()
                        self._resync = False
                    losses, learn = engine.step(X, label)
                    self.annealer.step()
                    dev_log.append((losses[5:6].clone(), learn))
                    if verbose:
                        v = losses.tolist()
                        bar.set_postfix(recontr_loss=v[0], kl_c=v[1], kl_s=v[2], c_loss=v[3], mi_loss=v[5])
                    continue
                if engine is not None:
                    engine.sync_host_state()
                    self._resync = True
                X_hat, lp, z = vae(X, explicit=True)
                self.optimizer.zero_grad()
                rec, kl_c, kl_s = vae_loss(X_hat, X, **lp)
                c_loss = contrastive_loss(mu=lp["mu_c"], logvar=lp["logvar_c"], label=label, sim_fn=self.sim_fn,
                                          temperature=hp["temperature"])
                mi = est(z[:, : vae.z_dim], z[:, vae.z_dim:])
                loss = (rec + self.annealer(kl_c) + self.annealer(kl_s) + hp["alpha"] * c_loss
                        + hp["lambda"] * mi)
                loss.backward()
                self.optimizer.step()
                self.annealer.step()
                learn = []
                for _ in range(5):
                    _, _, z2 = vae(X, explicit=True)
                    z2 = z2.detach()
                    ll = est.learning_loss(z2[:, : vae.z_dim], z2[:, vae.z_dim:])
                    self.mi_estimator_optimizer.zero_grad()
                    ll.backward()
                    self.mi_estimator_optimizer.step()
                    learn.append(ll.detach().reshape(1))
                dev_log.append((mi.detach().reshape(1), torch.cat(learn)))
                if verbose:
                    bar.set_postfix(recontr_loss=float(rec), kl_c=float(kl_c), kl_s=float(kl_s),
                                    c_loss=float(c_loss), mi_loss=float(mi))
        if engine is not None:
            engine.sync_host_state()
        if dev_log:
            mis = torch.cat([m for m, _ in dev_log]).tolist()
            lls = torch.cat([ll for _, ll in dev_log]).tolist()
            mi_losses.extend(mis)
            mi_learning_losses.extend(lls)

    def evaluate(self, dataloader, verbose, epoch_id, backend=None):
        backend = _eval_backend(backend)
        est = self.mi_estimator
        est.eval()

        def mi_term(lp, label, z):
            return est(z[:, : self.model.z_dim], z[:, self.model.z_dim:])

        return self._evaluate(dataloader, verbose, epoch_id, "mi_loss", mi_term, backend, "mim")


# ----------------------------------------------------------------------------- outside the hot path


class DownstreamMLPTrainer(Trainer):
    """MLP probe on mu_c of a frozen VAE (trainer.py:95-165); vae.encode runs on the HIP path.

    backend: "torch" (default) trains and evaluates the probe in PyTorch, as the reference does; "device" runs each
    training step as one HIP graph (cvhip.probe.ProbeStep: eval-mode encoder, then loss, gradients, BatchNorm running
    statistics and Adam in cv_probe_step) and the eval forward through cv_probe_forward, for the batches the engine
    accepts, and PyTorch for the rest.  None reads the environment variable CVHIP_PROBE (so the reference scripts
    switch without an edit), else "torch".  A setup outside the engine's contract warns once and runs as "torch"."""

    BACKENDS = ("torch", "device")

    def __init__(self, vae: nn.Module, model: nn.Module, optimizer: Optimizer, criterion: nn.Module,
                 verbose_period: int, device: torch.device, transform=None, backend: str | None = None) -> None:
        super().__init__(model, optimizer, verbose_period, device, transform)
        self.criterion = criterion
        self.vae = vae
        if backend is None:
            backend = os.environ.get("CVHIP_PROBE") or "torch"
        if backend not in self.BACKENDS:
            raise ValueError(f"backend must be one of {self.BACKENDS}, got {backend!r}")
        self.backend = backend
        self._engine = None
        self._engine_refused = False
        self._resync = False

    def _probe_engine(self):
        """The device probe step, or None (backend "torch", or a setup outside its contract: warned once)."""
        if self.backend != "device" or self._engine_refused:
            return None
        from cvhip.probe import ProbeStep

        if self._engine is None or not self._engine.compatible():
            if self._engine is not None:
                self._engine.sync_host_state()
            why = ProbeStep.unsupported_reason(self)
            self._engine = None if why is not None else ProbeStep.build(self)
            if self._engine is None:
                self._engine_refused = True
                warnings.warn(f"DownstreamMLPTrainer(backend='device') runs as 'torch': {why}", stacklevel=3)
        return self._engine

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        self.model.train()
        engine = self._probe_engine()
        with tqdm(dataloader, unit="batch", disable=not verbose) as bar:
            bar.set_description(f"epoch {epoch_id}")
            for batch in bar:
                X, y = batch[0], batch[1].reshape(-1).long()
                X, y = X.to(self.device), y.to(self.device)
                if self.transform:
                    X = self.transform(X)
                if engine is not None:
                    if engine.accepts(X):
                        if self._resync:
                            engine.resync_from_host()
                            self._resync = False
                        loss = engine.step(X, y)
                        if verbose:
                            bar.set_postfix(loss=float(loss))
                        continue
                    engine.sync_host_state()
                    self._resync = True
                self.optimizer.zero_grad()
                logits = self.model(self.vae.encode(X)[0])
                loss = self.criterion(logits, y)
                loss.backward()
                self.optimizer.step()
                if verbose:
                    bar.set_postfix(loss=float(loss))
        if engine is not None:
            engine.sync_host_state()

    def _valid(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        if verbose:
            (aupr, auroc), acc = self.evaluate(dataloader, verbose, epoch_id)
            print("val_aupr:", aupr)
            print(np.mean(list(aupr.values())).round(3))
            print("val_auroc:", auroc)
            print(np.mean(list(auroc.values())).round(3))
            print("val_acc:", acc.numpy().round(3))

    def evaluate(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        self.model.eval()
        engine = self._probe_engine()
        ys, logits = [], []
        with torch.no_grad():
            for batch in tqdm(dataloader, disable=not verbose, desc=f"val-epoch {epoch_id}"):
                X, y = batch[0], batch[1].reshape(-1)
                if engine is not None:
                    X = X.to(self.device)
                    if engine.accepts_eval(X):
                        logits.append(engine.logits(X))
                        ys.append(y)
                        continue
                logits.append(self.model(self.vae.encode(X.to(self.device))[0]))
                ys.append(y)
        ys, logits = torch.cat(ys), torch.cat(logits)
        return auc(logits, ys), accurary(logits, ys)


class SimpleCNNTrainer(Trainer):
    """The CNN baseline (trainer.py:168-233).

    backend: "torch" (default) trains and evaluates in PyTorch, as the reference does; "device" runs each training
    step as one HIP graph (cvhip.cnn.CnnStep: the conv trunk on the VAE encoder's kernels, the classifier tail in
    cv_cls_step, one Adam launch over a flat arena) and the eval forward through cv_cls_forward, for the batches the
    engine accepts, and PyTorch for the rest.  None reads the environment variable CVHIP_CNN (so the reference scripts
    switch without an edit), else "torch".  A setup outside the engine's contract warns once and runs as "torch"."""

    BACKENDS = ("torch", "device")

    def __init__(self, model: nn.Module, optimizer: Optimizer, criterion: nn.Module, verbose_period: int,
                 device: torch.device, transform=None, backend: str | None = None) -> None:
        super().__init__(model, optimizer, verbose_period, device, transform)
        self.criterion = criterion
        if backend is None:
            backend = os.environ.get("CVHIP_CNN") or "torch"
        if backend not in self.BACKENDS:
            raise ValueError(f"backend must be one of {self.BACKENDS}, got {backend!r}")
        self.backend = backend
        self._engine = None
        self._engine_refused = False
        self._resync = False

    @staticmethod
    def _step_class():
        from cvhip.cnn import CnnStep

        return CnnStep

    def _cnn_engine(self):
        """The device step, or None (backend "torch", or a setup outside its contract: warned once)."""
        if self.backend != "device" or self._engine_refused:
            return None
        Step = self._step_class()

        if self._engine is None or not self._engine.compatible():
            if self._engine is not None:
                self._engine.sync_host_state()
            why = Step.unsupported_reason(self)
            self._engine = None if why is not None else Step.build(self)
            if self._engine is None:
                self._engine_refused = True
                warnings.warn(f"{type(self).__name__}(backend='device') runs as 'torch': {why}", stacklevel=3)
        return self._engine

    def invalidate_packed(self):
        """Call after writing parameters through `.data` (which bypasses their version counters): the device backend
        repacks its conv weights before the next step.  No effect under backend "torch" or before the first step."""
        if self._engine is not None:
            self._engine.invalidate_packed()

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        self.model.train()
        engine = self._cnn_engine()
        with tqdm(dataloader, unit="batch", disable=not verbose) as bar:
            bar.set_description(f"epoch {epoch_id}")
            for batch in bar:
                X, y = _batch(batch, self.device, self.transform)
                if engine is not None:
                    if engine.accepts(X):
                        if self._resync:
                            engine.resync_from_host()
                            self._resync = False
                        loss = engine.step(X, y)
                        if verbose:
                            bar.set_postfix(loss=float(loss))
                        continue
                    engine.sync_host_state()
                    self._resync = True
                self.optimizer.zero_grad()
                loss = self.criterion(self.model(X), y)
                loss.backward()
                self.optimizer.step()
                if verbose:
                    bar.set_postfix(loss=float(loss))
        if engine is not None:
            engine.sync_host_state()

    def _valid(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        if verbose:
            (aupr, auroc), acc = self.evaluate(dataloader, verbose, epoch_id)
            print("val_aupr:", aupr)
            print(np.mean(list(aupr.values())).round(3))
            print("val_auroc:", auroc)
            print(np.mean(list(auroc.values())).round(3))
            print("val_acc:", acc.numpy().round(3))

    def evaluate(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        self.model.eval()
        engine = self._cnn_engine()
        ys, logits = [], []
        with torch.no_grad():
            for batch in tqdm(dataloader, disable=not verbose, desc=f"val-epoch {epoch_id}"):
                X, y = batch[0], batch[1].reshape(-1)
                X = X.to(self.device)
                if engine is not None and engine.accepts_eval(X):
                    logits.append(engine.logits(X))
                else:
                    logits.append(self.model(X))
                ys.append(y)
        ys, logits = torch.cat(ys), torch.cat(logits)
        return auc(logits, ys), accurary(logits, ys)


class LAMCNNTrainer(SimpleCNNTrainer):
    """The LAM baseline (trainer.py:236-288).

    backend: "torch" (default) is the reference's loop (three train-mode trunk forwards and lam_loss per step);
    "device" runs each training step as one HIP graph (cvhip.lam.LamStep: one trunk forward, the LAM tail in
    cv_lam_step, one trunk backward, three running-statistics updates, one Adam launch) and the eval forward through
    cv_lam_forward, for the batches the engine accepts, and PyTorch for the rest.  The device pairing is drawn by
    cv_lam_pair from the device Philox stream (keyed by torch.initial_seed()), not from torch.randperm.  None reads
    CVHIP_CNN, else "torch".  A setup outside the engine's contract warns once and runs as "torch"."""

    def __init__(self, model: nn.Module, optimizer: Optimizer, criterion: nn.Module, hyperparameter: dict,
                 verbose_period: int, device: torch.device, transform=None, backend: str | None = None) -> None:
        super().__init__(model, optimizer, criterion, verbose_period, device, transform, backend)
        self.hyperparameter = hyperparameter

    @staticmethod
    def _step_class():
        from cvhip.lam import LamStep

        return LamStep

    def ss_pairing(self, x, y):
        """Stratified shuffle: every sample is paired with a random sample of the same label
        (trainer.py:249-257)."""
        new_x = x.clone()
        for c in torch.unique(y):
            idx = (y == c).nonzero(as_tuple=True)[0]
            perm = torch.randperm(idx.shape[0])
            new_x[idx] = x[idx[perm.to(idx.device)]]
        return new_x

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        """(X, y) batches, as the reference's callers pass them (trainer.py:259-288)."""
        cnn = self.model
        cnn.train()
        engine = self._cnn_engine()
        if engine is not None:
            return self._train_device(engine, dataloader, verbose, epoch_id)
        lam_coef = self.hyperparameter["lam_coef"]
        with tqdm(dataloader, unit="batch", disable=not verbose) as bar:
            bar.set_description(f"epoch {epoch_id}")
            for batch in bar:
                X, y = _batch(batch, self.device, self.transform)
                X_tilde = self.ss_pairing(X, y)
                self.optimizer.zero_grad()
                loss_ce = self.criterion(cnn(X), y)
                loss_lam = lam_loss(cnn.net(X), cnn.net(X_tilde), y, cnn.cls_head.weight)
                loss = loss_ce + lam_coef * loss_lam
                loss.backward()
                self.optimizer.step()
                bar.set_postfix(ce_loss=float(loss_ce), lam_loss=float(loss_lam))

    def _train_device(self, engine, dataloader: DataLoader, verbose: bool, epoch_id: int):
        """The same epoch with the device step for the batches it accepts; a refused batch takes the loop above's step
        in PyTorch (the sync_host_state / resync dance of SimpleCNNTrainer._train).  The two postfix reads
        synchronise, so they happen only when the bar is enabled."""
        cnn = self.model
        with tqdm(dataloader, unit="batch", disable=not verbose) as bar:
            bar.set_description(f"epoch {epoch_id}")
            for batch in bar:
                X, y = _batch(batch, self.device, self.transform)
                if engine.accepts(X):
                    if self._resync:
                        engine.resync_from_host()
                        self._resync = False
                    losses = engine.step(X, y)
                    if verbose:
                        bar.set_postfix(ce_loss=float(losses[0]), lam_loss=float(losses[1]))
                    continue
                engine.sync_host_state()
                self._resync = True
                X_tilde = self.ss_pairing(X, y)
                self.optimizer.zero_grad()
                loss_ce = self.criterion(cnn(X), y)
                loss_lam = lam_loss(cnn.net(X), cnn.net(X_tilde), y, cnn.cls_head.weight)
                loss = loss_ce + self.hyperparameter["lam_coef"] * loss_lam
                loss.backward()
                self.optimizer.step()
                if verbose:
                    bar.set_postfix(ce_loss=float(loss_ce), lam_loss=float(loss_lam))
        engine.sync_host_state()


class HierarchicalVAETrainer(VAETrainer, _FusedEval):
    """GVAE / ML-VAE baselines (trainer.py:291-412).  Each step runs as one fused HIP program
    (cvhip.engine.ClearStep, mode "group"): the group evidence of vae.py:159-223 segmented by label on the
    device (cv_group_forward / cv_group_backward), kl_c over the groups and the B/m adjustment of rec and
    kl_s (trainer.py:322-324, 344-349) folded into the backward seed and the latent kernel.  Setups outside
    the fused contract run the reference's loop on the module-level HIP path."""

    def __init__(self, model: VAE, optimizer: Optimizer, hyperparameter: dict[str, float], verbose_period: int,
                 device: torch.device, transform=None) -> None:
        super().__init__(model, optimizer, verbose_period, device, transform)
        self.hyperparameter = hyperparameter
        self.annealer = LogisticAnnealer(loc=hyperparameter["loc"], scale=hyperparameter["scale"],
                                         beta=hyperparameter["beta"])
        self._engine = None
        self.use_fused = True

    def _fused(self):
        if not self.use_fused:
            return None
        from cvhip.engine import ClearStep

        if self._engine is None or not self._engine.compatible():
            self._engine = ClearStep.build(self, mode="group")
        return self._engine

    def fit(self, epochs: int, train_loader: DataLoader, valid_loader: None | DataLoader = None,
            eval_evidence_acc: bool = False):
        for epoch in range(epochs):
            verbose = (epoch % self.verbose_period) == 0
            self._train(train_loader, verbose, epoch)
            if valid_loader is not None:
                self._valid(valid_loader, verbose, epoch, eval_evidence_acc)

    def _group_adjust(self, B, m, *losses):
        return [loss * B / m for loss in losses]

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int):
        vae = self.model
        vae.train()
        engine = self._fused()
        with tqdm(dataloader, unit="batch", mininterval=0, disable=not verbose) as bar:
            bar.set_description(f"epoch {epoch_id}")
            for batch in bar:
                X, label = _batch(batch, self.device, None)
                if engine is not None and engine.accepts(X):
                    if getattr(self, "_resync", False):
                        engine.resync_from_host()
                        self._resync = False
                    losses = engine.step(X, label)
                    self.annealer.step()
                    if verbose:
                        v = losses.tolist()
                        bar.set_postfix(reconstr_loss=v[0], kl_c=v[1], kl_s=v[2])
                    continue
                if engine is not None:
                    engine.sync_host_state()
                    self._resync = True
                B, m = X.size(0), len(label.unique())
                if self.transform:
                    X = self.transform(X)
                self.optimizer.zero_grad()
                X_hat, lp = vae(X, label=label)
                rec, kl_c, kl_s = vae_loss(X_hat, X, **lp)
                rec, kl_s = self._group_adjust(B, m, rec, kl_s)
                loss = rec + self.annealer(kl_c) + self.annealer(kl_s)
                loss.backward()
                self.optimizer.step()
                self.annealer.step()
                if verbose:
                    bar.set_postfix(reconstr_loss=float(rec), kl_c=float(kl_c), kl_s=float(kl_s))
        if engine is not None:
            engine.sync_host_state()

    def _valid(self, dataloader, verbose, epoch_id, with_evidence_acc=False):
        if verbose:
            mig, mse = self.evaluate(dataloader, verbose, epoch_id, with_evidence_acc)
            print(f"gMIG: {round(mig, 3)}; mse: {round(float(mse), 3)}")

    def evaluate(self, dataloader, verbose, epoch_id, with_evidence_acc=False, backend=None):
        """backend "fused" (or CVHIP_EVAL=fused): the epoch through cvhip.evaluate.EvalPass (mode "group"), without
        the group evidence; with_evidence_acc=True, or a setup outside the pass's contract, warns once and runs
        "module"."""
        backend = _eval_backend(backend)
        vae = self.model
        vae.eval()
        if backend == "fused":
            why = "with_evidence_acc=True needs the group evidence in the pass" if with_evidence_acc else None
            ep, cap = self._eval_pass_for("group", dataloader, why)
            if ep is not None:
                def module_batch(X, label):
                    X_hat, lp, z = vae(X, explicit=True)
                    return tuple(vae_loss(X_hat, X, **lp)), z

                return self._evaluate_fused(ep, cap, dataloader, verbose, epoch_id, ("recontr_loss", "kl_c", "kl_s"),
                                            module_batch)
        tot = [0.0, 0.0, 0.0]
        labels, lat_c, lat_s = [], [], []
        with torch.no_grad():
            for batch in tqdm(dataloader, disable=not verbose, desc=f"val-epoch {epoch_id}"):
                X, label = _batch(batch, self.device, None)
                if with_evidence_acc:
                    X_hat, lp, z = vae(X, label, explicit=True)
                else:
                    X_hat, lp, z = vae(X, explicit=True)
                for i, v in enumerate(vae_loss(X_hat, X, **lp)):
                    tot[i] += v
                labels.append(label)
                lat_c.append(z[:, : vae.z_dim])
                lat_s.append(z[:, vae.z_dim:])
        mig = mutual_info_gap(torch.cat(labels), torch.cat(lat_c), torch.cat(lat_s))
        nb = len(dataloader)
        mse = float(tot[0] / nb)
        if verbose:
            print("val_recontr_loss={:.3f}, val_kl_c={:.3f}, val_kl_s={:.3f}".format(*[t / nb for t in tot]))
        return mig, mse


def factor_shuffling(z: torch.Tensor, strategy: str = "permute_1"):
    """(trainer.py:573-587)"""
    d = int(z.shape[1] / 2)
    z_c, z_s = z[:, :d], z[:, d:]
    if strategy == "full":
        return torch.cat([z_c, z_s[torch.randperm(z_s.shape[0])]], dim=1)
    if strategy == "permute_1":
        return torch.cat([z_c, torch.cat([z_s[1:, :], z_s[0, :][None]], dim=0)], dim=1)
    raise ValueError("this strategy is not implemented yet")


class ClearTCVAETrainer(VAETrainer, _ClearEval):
    """CLEAR-TC (trainer.py:590-778).  Each step runs as one fused HIP program (cvhip.engine.ClearStep,
    mode "tc"): the VAE step with the factor discriminator's density-ratio term relu(log(D/(1-D))).mean()
    (cv_tc_forward), a second train-mode forward with fresh noise, and the discriminator's BCE step on
    joint vs factor-shuffled z (cv_tc_learning_step + Adam).  Setups outside the fused contract (another
    discriminator architecture or optimizer) run the reference's loop with the VAE on the autograd HIP
    path and the discriminator in PyTorch."""

    def __init__(self, model: VAE, factor_cls: nn.Module, optimizers: dict[str, Optimizer], sim_fn: str,
                 hyperparameter: dict[str, float], verbose_period: int, device: torch.device,
                 transform=None) -> None:
        super().__init__(model, optimizers["vae_optim"], verbose_period, device, transform)
        self.sim_fn = sim_fn
        self.factor_optimizer = optimizers["factor_optim"]
        self.factor_cls = factor_cls
        self.hyperparameter = hyperparameter
        self.annealer = LogisticAnnealer(loc=hyperparameter["loc"], scale=hyperparameter["scale"],
                                         beta=hyperparameter["beta"])
        self._engine = None
        self.use_fused = True

    def _fused(self):
        if not self.use_fused:
            return None
        from cvhip.engine import ClearStep

        if self._engine is None or not self._engine.compatible():
            self._engine = ClearStep.build(self, mode="tc")
        return self._engine

    def fit(self, epochs: int, train_loader: DataLoader, valid_loader: None | DataLoader = None):
        factor_d_losses = []
        for epoch in range(epochs):
            verbose = (epoch % self.verbose_period) == 0
            self._train(train_loader, verbose, epoch, factor_d_losses)
            if valid_loader is not None:
                self._valid(valid_loader, verbose, epoch)
        return factor_d_losses

    def _train(self, dataloader: DataLoader, verbose: bool, epoch_id: int, factor_d_losses: list):
        vae, cls = self.model, self.factor_cls
        vae.train()
        cls.train()
        hp = self.hyperparameter
        engine = self._fused()
        log = []
        with tqdm(dataloader, unit="batch", mininterval=0, disable=not verbose) as bar:
            bar.set_description(f"Epoch {epoch_id}")
            for batch in bar:
                X, label = _batch(batch, self.device, self.transform)
                if engine is not None and engine.accepts(X):
                    if getattr(self, "_resync", False):
                        engine.resync_from_host()
                        self._resync = False
                    losses, fl = engine.step(X, label)
                    self.annealer.step()
                    log.append(fl)
                    if verbose:
                        v = losses.tolist()
                        bar.set_postfix(factor_cls_loss=float(fl), recontr_loss=v[0], kl_c=v[1], kl_s=v[2],
                                        c_loss=v[3], mi_loss=v[5])
                    continue
                if engine is not None:
                    engine.sync_host_state()
                    self._resync = True
                X_hat, lp, z = vae(X, explicit=True)
                self.optimizer.zero_grad()
                rec, kl_c, kl_s = vae_loss(X_hat, X, **lp)
                c_loss = contrastive_loss(mu=lp["mu_c"], logvar=lp["logvar_c"], label=label, sim_fn=self.sim_fn,
                                          temperature=hp["temperature"])
                d_score = cls(z)
                mi_loss = F.relu(torch.log(d_score / (1 - d_score))).mean()
                loss = (rec + self.annealer(kl_c) + self.annealer(kl_s) + hp["alpha"] * c_loss
                        + hp["lambda"] * mi_loss)
                loss.backward()
                self.optimizer.step()
                self.annealer.step()
                _, _, z = vae(X, explicit=True)
                z = z.detach()
                self.factor_optimizer.zero_grad()
                dj = cls(z)
                dm = cls(factor_shuffling(z))
                factor_loss = nn.BCELoss()(torch.cat([dj, dm], dim=0),
                                           torch.cat([torch.ones_like(dj), torch.zeros_like(dm)], dim=0))
                log.append(factor_loss.detach().reshape(1))
                factor_loss.backward()
                self.factor_optimizer.step()
                if verbose:
                    bar.set_postfix(factor_cls_loss=float(factor_loss), recontr_loss=float(rec), kl_c=float(kl_c),
                                    kl_s=float(kl_s), c_loss=float(c_loss), mi_loss=float(mi_loss))
        if engine is not None:
            engine.sync_host_state()
        if log:
            factor_d_losses.extend(torch.cat([t.reshape(1) for t in log]).tolist())

    def evaluate(self, dataloader, verbose, epoch_id, backend=None):
        backend = _eval_backend(backend)
        self.factor_cls.eval()

        def mi_term(lp, label, z):
            d = self.factor_cls(z)
            return F.relu(torch.log(d / (1 - d))).mean()

        return self._evaluate(dataloader, verbose, epoch_id, "mi_loss", mi_term, backend, "tc")
