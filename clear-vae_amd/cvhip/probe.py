"""Device downstream probe: the training step of DownstreamMLPTrainer._train (code/src/trainer.py:110-133) as one HIP
graph per step, and the eval forward of its evaluate() (code/src/trainer.py:146-165).

The probe is the reference's `mlp` (run_styledmnist_downstream_expr.py:110-117): Linear(z, h) -> BatchNorm1d(h) -> ReLU
-> Linear(h, n_class) on mu_c of the frozen VAE, nn.CrossEntropyLoss() and Adam.  A step is

  batch copy (cv_copy_many) -> [graph: eval-mode encoder + heads -> cv_probe_step on heads[:, :d] (loss, gradients,
  BatchNorm running statistics, Adam on the probe's flat arena; two launches)]

The first step at a batch size runs eagerly (it loads the code objects), every later one replays a single-chain
_lib.StepGraph.  The Adam step counter lives on the device and is advanced by the kernel, so a replay needs no host
write; the optimizer's host `step` entries are brought up to date by sync_host_state() (the trainer calls it at the end
of an epoch and before any step it takes in PyTorch).  optimizer.state[p]["exp_avg" / "exp_avg_sq"] and p.grad are
live views of the engine's flat buffers; the kernels write the BatchNorm module's own running_mean / running_var /
num_batches_tracked, so there is no copy to keep in step.

The frozen encoder's packed weights are refreshed when the VAE's parameter version counters change, and once per epoch
(a VAE trained by the fused engine in between changes its arena without touching those counters).
"""

from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import cv_probe, cv_probe_grad
from .engine import _AdamState, _dist_world
from .plan import ParamArena, Program, Workspace, ensure_arena, pack_program, ptr_array


def probe_layers(model, name: str = "the probe"):
    """(Linear, BatchNorm1d, ReLU, Linear) when `model` is exactly the reference's probe, else a reason string that
    calls the module `name`."""
    if type(model) is not nn.Sequential or len(model) != 4:
        return f"{name} is not nn.Sequential(Linear, BatchNorm1d, ReLU, Linear)"
    l0, bn, act, l2 = list(model)
    if type(l0) is not nn.Linear or type(bn) is not nn.BatchNorm1d or type(act) is not nn.ReLU \
            or type(l2) is not nn.Linear:
        return f"{name} is not nn.Sequential(Linear, BatchNorm1d, ReLU, Linear)"
    if l0.bias is None or l2.bias is None:
        return f"a Linear of {name} has no bias"
    if not bn.affine or not bn.track_running_stats or bn.running_mean is None \
            or not isinstance(bn.momentum, float):
        return f"the BatchNorm1d of {name} needs affine, track_running_stats and a float momentum"
    if l0.out_features != bn.num_features or l2.in_features != bn.num_features:
        return f"the layer widths of {name} do not chain"
    return l0, bn, act, l2


def probe_params(layers):
    l0, bn, _, l2 = layers
    return [l0.weight, l0.bias, bn.weight, bn.bias, l2.weight, l2.bias]


class ProbeStep:
    @staticmethod
    def unsupported_reason(trainer):
        """Why `trainer` is outside the device probe's contract (a string), or None when it is inside."""
        layers = probe_layers(trainer.model)
        if isinstance(layers, str):
            return layers
        params = probe_params(layers)
        bn = layers[1]
        dev = params[0].device
        if dev.type != "cuda":
            return "the probe is not on the ROCm device"
        tensors = params + [bn.running_mean, bn.running_var]
        if any(t.device != dev or t.dtype != torch.float32 for t in tensors):
            return "the probe is not fp32 on one device"
        if not all(p.requires_grad for p in params):
            return "a probe parameter does not require grad"
        crit = trainer.criterion
        if type(crit) is not nn.CrossEntropyLoss or crit.weight is not None or crit.reduction != "mean" \
                or crit.label_smoothing != 0 or crit.ignore_index != -100:
            return "the criterion is not nn.CrossEntropyLoss() with its defaults"
        if not _AdamState.supported(trainer.optimizer, params):
            return "the optimizer is not a plain single-group torch.optim.Adam over the probe's parameters"
        if trainer.transform is not None:
            return "the trainer has a transform"
        if _dist_world() > 1:
            return "a process group with more than one rank is initialised"
        vae = trainer.vae
        try:
            if next(vae.parameters()).device != dev:
                return "the VAE is on another device"
            ensure_arena(vae)
        except (NotImplementedError, AssertionError, RuntimeError, StopIteration, AttributeError) as e:
            return f"the VAE has no HIP encoder program ({e})"
        d, h, c = layers[0].in_features, bn.num_features, layers[3].out_features
        if vae._cv_spec.d != d:
            return f"the probe reads {d} features, mu_c has {vae._cv_spec.d}"
        if not _lib.lib().cv_probe_supported(2, d, h, c):
            return f"cv_probe_step does not serve d={d}, h={h}, c={c}"
        return None

    @classmethod
    def build(cls, trainer):
        """A device probe step for `trainer` (a DownstreamMLPTrainer), or None outside the contract."""
        if cls.unsupported_reason(trainer) is not None:
            return None
        return cls(trainer)

    def __init__(self, trainer):
        self.trainer = trainer
        self.vae = trainer.vae
        self.model = trainer.model
        self.layers = probe_layers(self.model)
        l0, bn, _, l2 = self.layers
        self.bn = bn
        self.d, self.h, self.c = l0.in_features, bn.num_features, l2.out_features
        self.vae_arena = ensure_arena(self.vae)
        self.spec = self.vae._cv_spec
        self.params = probe_params(self.layers)
        self.device = self.params[0].device
        self.arena = ParamArena(self.params, self.device)
        self.adam = _AdamState(trainer.optimizer, self.arena)
        for p in self.params:
            p.grad = self.arena.gview(p)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.sizes = {}  # n -> dict(ws, X, lab, work, prog, count[, graph, eval, logits])
        self.graphs_enabled = True
        self.steps_since_sync = 0
        self.steps_taken = 0
        self._packed_sig = None
        self._sig = self._signature()

    # ----------------------------------------------------------------------------- bookkeeping
    def _signature(self):
        t, bn = self.trainer, self.bn
        return (id(t.optimizer), id(t.model), id(t.criterion), id(t.vae), id(getattr(t.vae, "_cv_arena", None)),
                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(),
                float(bn.eps), bn.momentum)

    def compatible(self) -> bool:
        return (self._signature() == self._sig and self.arena.valid() and self.vae_arena.valid()
                and ProbeStep.unsupported_reason(self.trainer) is None)

    def _fits(self, X) -> bool:
        sp = self.spec
        return (X.device == self.device and X.dim() == 4 and tuple(X.shape[1:]) == (sp.in_ch, sp.H, sp.W)
                and not self.vae.training)

    def accepts(self, X) -> bool:
        """A training batch the engine takes.  A VAE left in train mode is the reference's train-mode encode (batch
        statistics, moving running statistics): that takes the torch path."""
        return (self._fits(X) and self.model.training
                and bool(_lib.lib().cv_probe_supported(int(X.shape[0]), self.d, self.h, self.c)))

    def accepts_eval(self, X) -> bool:
        n = int(X.shape[0])
        return (self._fits(X) and not self.model.training and n >= 1
                and bool(_lib.lib().cv_probe_supported(max(n, 2), self.d, self.h, self.c)))

    def resync_from_host(self):
        """After steps taken by the torch optimizer itself (its moments are the engine's buffers; its step count and
        fresh .grad tensors are not)."""
        self.sync_host_state()
        self.adam.adopt_host_step()
        for p in self.params:
            p.grad = self.arena.gview(p)

    def sync_host_state(self):
        if self.steps_since_sync:
            self.adam.sync_host(self.steps_since_sync)
            self.steps_since_sync = 0
        self._packed_sig = None

    def invalidate_packed(self):
        """Repack the encoder's weights before the next step (after VAE parameters were changed through `.data`)."""
        self._packed_sig = None

    # ----------------------------------------------------------------------------- programs
    def _probe_struct(self) -> cv_probe:
        bn = self.bn
        w1, b1, gamma, beta, w2, b2 = (p.data_ptr() for p in self.params)
        return cv_probe(w1, b1, gamma, beta, w2, b2, bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                        bn.num_batches_tracked.data_ptr(), self.d, self.h, self.c, float(bn.eps), float(bn.momentum))

    def _size(self, n: int):
        G = self.sizes.get(n)
        if G is not None:
            return G
        sp, dev = self.spec, self.device
        ws = Workspace(sp, n, dev, with_grad=False)
        X = torch.zeros(n, sp.in_ch, sp.H, sp.W, dtype=torch.float32, device=dev)
        lab = torch.zeros(n, dtype=torch.int64, device=dev)
        G = dict(ws=ws, X=X, lab=lab, count=0)
        if _lib.lib().cv_probe_supported(n, self.d, self.h, self.c):
            nbytes = int(_lib.lib().cv_probe_workspace_bytes(n, self.h, self.c))
            G["work"] = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.float32, device=dev)
            P = Program()
            ws.encoder_program(P, X, train=False)
            grad = cv_probe_grad(*[self.arena.gptr(p) for p in self.params])
            P.add("cv_probe_step", self._probe_struct(), ws.heads, 4 * sp.d, lab, n, G["work"], self.loss, grad,
                  *self.adam.args())
            G["prog"] = P
        self.sizes[n] = G
        return G

    def _eval_program(self, G):
        if "eval" not in G:
            ws = G["ws"]
            G["logits"] = torch.empty(ws.n, self.c, dtype=torch.float32, device=self.device)
            P = Program()
            ws.encoder_program(P, G["X"], train=False)
            P.add("cv_probe_forward", self._probe_struct(), ws.heads, 4 * self.spec.d, ws.n, G["logits"])
            G["eval"] = P
        return G["eval"]

    def _vae_sig(self):
        A = self.vae_arena
        return (A.flat._version,) + tuple(p._version for p in A.params)

    def _ensure_packed(self):
        sig = self._vae_sig()
        if self._packed_sig != sig:
            P = Program()
            pack_program(self.spec, P, "enc")
            P.run()
            self._packed_sig = sig

    def _load_batch(self, G, X, lab=None):
        """The batch into the programs' static inputs (one launch when no conversion is needed)."""
        raw = X.dtype == torch.float32 and X.is_contiguous() and X.shape == G["X"].shape
        if lab is not None:
            lab = lab.reshape(-1)
            if lab.shape != G["lab"].shape:
                raise ValueError(f"probe step: {tuple(lab.shape)} labels for a batch of {G['X'].shape[0]}")
            raw = raw and lab.dtype == torch.int64 and lab.is_contiguous() and lab.device == self.device
        if raw:
            pairs = [(G["X"], X)] + ([(G["lab"], lab)] if lab is not None else [])
            dst = ptr_array([a.data_ptr() for a, _ in pairs])
            src = ptr_array([b.data_ptr() for _, b in pairs])
            nb = (ctypes.c_size_t * len(pairs))(*[a.numel() * a.element_size() for a, _ in pairs])
            _lib.call("cv_copy_many", dst, src, nb, len(pairs), _lib.stream_handle())
            return
        G["X"].copy_(X, non_blocking=True)
        if lab is not None:
            G["lab"].copy_(lab, non_blocking=True)

    # ----------------------------------------------------------------------------- one step
    def step(self, X, y):
        """One training step on (X [n][C][H][W], y [n]); returns the device [1] loss (overwritten by the next step)."""
        G = self._size(int(X.shape[0]))
        self.adam.refresh_hyper()
        self._ensure_packed()
        self._load_batch(G, X, y)
        if G["count"] >= 1 and self.graphs_enabled:
            if "graph" not in G:
                G["graph"] = _lib.StepGraph(lambda s: G["prog"].run(s))
            G["graph"].replay()
        else:
            G["prog"].run()
        G["count"] += 1
        self.steps_since_sync += 1
        self.steps_taken += 1
        return self.loss

    def logits(self, X):
        """Eval-mode logits [n][c] of the probe on mu_c(X) (a fresh tensor)."""
        G = self._size(int(X.shape[0]))
        P = self._eval_program(G)
        self._ensure_packed()
        self._load_batch(G, X)
        P.run()
        return G["logits"].clone()
