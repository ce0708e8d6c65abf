"""Device LAM baseline: the training step of LAMCNNTrainer._train (code/src/trainer.py:259-288) as one HIP graph per
step, and the eval forward of its evaluate() (code/src/trainer.py:215-233).

The model is the reference's LAMCNNClassifier / LAMCNN64Classifier (code/src/models/cnn.py:57-66): the conv trunk of
the CNN baseline and cls_head = Linear(2048, n_class).  The reference step runs the trunk three times in train mode:
cnn(X), cnn.net(X) and cnn.net(X_tilde), with X_tilde = X[pair] for a permutation `pair` of the batch that ss_pairing
(code/src/trainer.py:249-257) draws inside each label.  Batch statistics do not see row order, so a conv +
train-mode-BatchNorm trunk is permutation-equivariant: net(X[pair]) = net(X)[pair], the second net(X) equals the
first, and because the backward is linear in the upstream gradient the three autograd paths sum into one backward with
a summed upstream gradient.  A step is therefore

  batch copy (cv_copy_many) -> [graph: zero the statistics and the gradient arena -> conv forwards (the VAE encoder's
  launches) -> cv_lam_pair (the device ss_pairing; skipped when a pair is given) -> cv_lam_step (BN + ReLU of the last
  block, the head, both losses, the head's gradients, the masked gradient of the last block and its BatchNorm backward
  sums; two launches) -> conv backward (data + deferred weight gradients) -> cv_step_reduce (weight-gradient tiles and
  BatchNorm2d affine gradients) -> cv_bn_update_running_sets with the trunk given three times (the three momentum
  updates of the reference's three forwards, num_batches_tracked += 3) -> cv_adam_pack_step]

on one stream, a single-chain _lib.StepGraph.  The parts shared with the CNN baseline (arena, packed weights, static
batch inputs, eager first step then replay, host-state bookkeeping) are cvhip.cnn.TrunkStep's.

lam_coef lives in a device float the step rewrites when trainer.hyperparameter["lam_coef"] changes, so a replayed
graph sees the change.  The drawn pairing takes its Philox keys from cvhip.rng.offset_tensor (keyed by
torch.initial_seed(), like the CLUB-S permutation), not from the CPU torch.randperm stream of the reference.
Test hooks: step(X, y, pair=...) uses the given permutation; record_pairs = True appends a clone of each step's pair to
pair_log, so a reference loop can replay the same pairing.

Conv biases feed a train-mode BatchNorm: as in CnnStep their gradient slots stay exactly zero and they stay
bit-unchanged.
"""

from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib, rng
from ._lib import cv_lam, cv_lam_grad
from .cnn import CnnSpec, TrunkStep, TrunkWorkspace, setup_reason, trunk_spec
from .plan import DeferGroup, Program


def lam_spec(model):
    """The layer plan of a LAMCNNClassifier / LAMCNN64Classifier (CnnSpec with head = (cls_head,)), or a reason
    string."""
    from src.models.cnn import LAMCNN64Classifier, LAMCNNClassifier

    if type(model) not in (LAMCNNClassifier, LAMCNN64Classifier):
        return f"the model is {type(model).__name__}, not LAMCNNClassifier / LAMCNN64Classifier"
    trunk = trunk_spec(model)
    if isinstance(trunk, str):
        return trunk
    in_ch, hw, enc, (c, h, w) = trunk
    head = getattr(model, "cls_head", None)
    if type(head) is not nn.Linear or head.bias is None:
        return "cls_head is not one nn.Linear with a bias"
    if head.in_features != c * h * w:
        return f"cls_head reads {head.in_features} features, net gives {c * h * w}"
    return CnnSpec(in_ch, hw, hw, enc, (c, h, w), (head,))


def lam_params(spec: CnnSpec) -> list:
    order = []
    for c in spec.enc:
        order += [c.mod.weight, c.mod.bias, c.bn.weight, c.bn.bias]
    return order + [spec.head[0].weight, spec.head[0].bias]


def _lam_coef(trainer):
    """trainer.hyperparameter["lam_coef"] as a float, or None when it is not a finite real number."""
    hp = getattr(trainer, "hyperparameter", None)
    v = hp.get("lam_coef") if isinstance(hp, dict) else None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        return None
    return float(v)


class LamStep(TrunkStep):
    NAME = "lam step"

    @staticmethod
    def unsupported_reason(trainer):
        """Why `trainer` is outside the device LAM step's contract (a string), or None when it is inside."""
        spec = lam_spec(trainer.model)
        if isinstance(spec, str):
            return spec
        params = lam_params(spec)
        if {id(p) for p in params} != {id(p) for p in trainer.model.parameters()}:
            return "the model has parameters outside net and cls_head"
        why = setup_reason(trainer, params, [c.bn for c in spec.enc])
        if why is not None:
            return why
        if _lam_coef(trainer) is None:
            return 'hyperparameter["lam_coef"] is not a finite float'
        C, Hh, Wh = spec.feat
        c = spec.head[0].out_features
        if not _lib.lib().cv_lam_supported(2, C, Hh * Wh, c):
            return f"cv_lam_step does not serve {C} channels x {Hh * Wh} pixels, c={c}"
        return None

    def __init__(self, trainer):
        sp = lam_spec(trainer.model)
        C, Hh, Wh = sp.feat
        self.ch, self.pix, self.c = C, Hh * Wh, sp.head[0].out_features
        self._setup(trainer, sp, lam_params(sp))
        self.loss = torch.zeros(2, dtype=torch.float32, device=self.device)  # (ce, lam)
        self.lam = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._lam_host = None
        # the shared (device, seed) Philox counter of the drawn pairing, taken once as ClearStep takes it: no program
        # or graph of a live engine is ever rebuilt (and none destroyed while its last replay may still be running)
        self._rng = rng.offset_tensor(self.device)
        self.record_pairs = False
        self.pair_log = []
        self._sig = self._signature()

    def _serves(self, n: int) -> bool:
        return bool(_lib.lib().cv_lam_supported(n, self.ch, self.pix, self.c))

    def _workspace(self, n: int, with_grad: bool):
        return TrunkWorkspace(self.spec, n, self.device, with_grad=with_grad)

    def _work_bytes(self, n: int) -> int:
        return int(_lib.lib().cv_lam_workspace_bytes(n, self.ch, self.pix, self.c))

    def refresh_lam(self):
        """trainer.hyperparameter["lam_coef"] into the device float the kernels read (the pattern of
        _AdamState.refresh_hyper)."""
        v = _lam_coef(self.trainer)
        if v is None:
            raise ValueError('lam step: hyperparameter["lam_coef"] is not a finite float')
        if v != self._lam_host:
            self._lam_host = v
            self.lam.copy_(torch.tensor([v], dtype=torch.float32))

    # ----------------------------------------------------------------------------- programs
    def _lam_struct(self) -> cv_lam:
        head = self.spec.head[0]
        return cv_lam(head.weight.data_ptr(), head.bias.data_ptr(), self.lam.data_ptr(), self.c, self.ch, self.pix)

    def _step_program(self, G, draw: bool = True) -> Program:
        ws, pg, n = G["ws"], self.arena.gptr, G["ws"].n
        head = self.spec.head[0]
        if "pair" not in G:
            G["pair"] = torch.zeros(n, dtype=torch.int64, device=self.device)
        P = Program()
        self._zero_program(P, ws)
        y_last = ws.conv_forward_program(P, G["X"], True)
        bn_last = ws.bn_enc[-1]
        if draw:
            seed, off = self._rng
            P.add("cv_lam_pair", G["lab"], n, ctypes.c_uint64(seed), off, G["pair"])
            P.keep.append(off)
        P.add("cv_lam_step", self._lam_struct(), y_last, bn_last.cv(True), G["lab"], G["pair"], n, G["work"],
              self.loss, ws.g_enc[-1], bn_last.gstat, cv_lam_grad(pg(head.weight), pg(head.bias)))
        defer = DeferGroup()
        ws.encoder_backward_program(P, pg, None, x=G["X"], defer=defer, heads=False)
        ws.step_reduce_program(P, defer, pg, "all", running=False)
        # (the reference's three train-mode forwards: three momentum updates with this batch's statistics)
        ws.running_sets_program(P, [ws.bn_enc] * 3)
        self._adam_program(P)
        P.keep += [G["work"], G["X"], G["lab"], G["pair"]]
        return P

    def _eval_program(self, G):
        if "eval" not in G:
            ws = G["ws"]
            G["logits"] = torch.empty(ws.n, self.c, dtype=torch.float32, device=self.device)
            P = Program()
            y_last = ws.conv_forward_program(P, G["X"], False)
            P.add("cv_lam_forward", self._lam_struct(), y_last, ws.bn_enc[-1].cv(False), ws.n, G["logits"])
            G["eval"] = P
        return G["eval"]

    # ----------------------------------------------------------------------------- one step
    def step(self, X, y, pair=None):
        """One training step on (X [n][C][H][W], y [n]); returns the device [2] losses (ce, lam; overwritten by the
        next step).  pair: the pairing to use instead of drawing one, a permutation of range(n) (validated on the
        host: the test hook)."""
        n = int(X.shape[0])
        G = self._size(n, train=True)
        key = "prog"
        if pair is not None:
            pair = torch.as_tensor(pair).reshape(-1).to(torch.int64)
            if pair.numel() != n or not torch.equal(torch.sort(pair.cpu())[0], torch.arange(n)):
                raise ValueError(f"lam step: pair is not a permutation of range({n})")
            if "given" not in G:
                G["given"] = self._step_program(G, draw=False)
            key = "given"
        self.adam.refresh_hyper()
        self.refresh_lam()
        self._ensure_packed()
        self._load_batch(G, X, y)
        if pair is not None:
            G["pair"].copy_(pair, non_blocking=True)
        self._run_step(G, key)
        if self.record_pairs:
            self.pair_log.append(G["pair"].clone())
        return self.loss
