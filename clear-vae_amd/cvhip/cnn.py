"""Device CNN baseline: the training step of SimpleCNNTrainer._train (code/src/trainer.py:181-203) as one HIP graph
per step, and the eval forward of its evaluate() (code/src/trainer.py:215-233).

The model is the reference's SimpleCNNClassifier / SimpleCNN64Classifier (code/src/models/cnn.py:6-49): `net` is layer
for layer the VAE / VAE64 encoder (Conv2d(k, 2, 1) + BatchNorm2d + ReLU, Flatten to 2048) and `cls_head` is
Linear(2048, h) -> BatchNorm1d(h) -> ReLU -> Linear(h, n_class), with nn.CrossEntropyLoss() and Adam.  A step is

  batch copy (cv_copy_many) -> [graph: zero the statistics and the gradient arena -> conv forwards (the VAE encoder's
  launches) -> cls_head[0] (cv_linear_forward on the NCHW-flattened BN + ReLU operand, not split over K: the split
  form adds its partial tiles with floating-point atomics, and this step is bit-reproducible) -> cv_cls_step
  (BatchNorm1d, ReLU, Linear, loss, their gradients, d(a); two launches) -> weight gradient and backward-data of
  cls_head[0] -> conv backward (data + deferred weight gradients) -> cv_step_reduce (weight-gradient tiles,
  BatchNorm2d affine gradients and running statistics) -> cv_adam_pack_step over the whole arena (Adam, and the
  GEMM-native copies of the conv weights it has just updated)]

on one stream: a single-chain _lib.StepGraph without side lanes.  The first step at a batch size runs eagerly (it
loads the code objects), every later one replays the graph.  All operands are fp32 (mma = 0).

Biases that feed a train-mode BatchNorm (the conv biases and cls_head[0].bias) have a gradient that is mathematically
zero: the batch mean removes them.  As in the VAE engine and the probe, the device step leaves exactly zero in their
gradient slots, so Adam leaves them bit-unchanged; PyTorch's fp32 backward moves them by rounding noise instead.

The Adam step counter lives on the device; the optimizer's host `step` entries are brought up to date by
sync_host_state() (the trainer calls it at the end of an epoch and before any step it takes in PyTorch).
optimizer.state[p]["exp_avg" / "exp_avg_sq"] and p.grad are live views of the engine's flat buffers, and the kernels
write the BatchNorm modules' own running_mean / running_var / num_batches_tracked.  The packed conv weights are
refreshed when a parameter's version counter changes (load_state_dict, a torch optimizer step); writes through `.data`
bypass the counters: call invalidate_packed() after them.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _lib
from ._lib import XF_BNRELU, cv_cls, cv_cls_grad, cv_conv_pack, cv_linear
from .engine import _AdamState, _dist_world
from .plan import (ConvSpec, DeferGroup, ParamArena, Program, Workspace, bn_arena, encoder_finalise_flags, ep_bwd,
                   ep_none, operand, ptr_array, struct_array)
from .probe import probe_layers


@dataclass
class CnnSpec:
    in_ch: int
    H: int
    W: int
    enc: list  # ConvSpec per conv block of `net`
    feat: tuple  # (C, H, W) of the flattened trunk output
    head: tuple  # (Linear, BatchNorm1d, ReLU, Linear); the LAM classifiers (cvhip.lam): (Linear,)
    mma: int = 0
    pack_items: list | None = None
    packed: torch.Tensor | None = None

    @property
    def F(self) -> int:
        c, h, w = self.feat
        return c * h * w


def trunk_spec(model):
    """(in_ch, hw, [ConvSpec], (C, H, W)) of a `net` = (Conv2d(k, 2, 1), BatchNorm2d, ReLU)* + Flatten, the trunk every
    baseline classifier of src/models/cnn.py shares, or a reason string."""
    net = getattr(model, "net", None)
    if type(net) is not nn.Sequential or len(net) < 4 or len(net) % 3 != 1 or type(net[-1]) is not nn.Flatten:
        return "net is not (Conv2d, BatchNorm2d, ReLU)* + Flatten"
    mods = list(net)[:-1]
    k0 = None
    for i in range(0, len(mods), 3):
        cv, bn, act = mods[i:i + 3]
        if type(cv) is not nn.Conv2d or type(bn) is not nn.BatchNorm2d or type(act) is not nn.ReLU:
            return "net is not (Conv2d, BatchNorm2d, ReLU)* + Flatten"
        k = cv.kernel_size[0]
        if (cv.kernel_size != (k, k) or cv.stride != (2, 2) or cv.padding != (1, 1) or cv.dilation != (1, 1)
                or cv.groups != 1 or cv.padding_mode != "zeros" or cv.bias is None or k not in (3, 4)):
            return "a conv of net is not Conv2d(k, 2, 1) with k in (3, 4) and a bias"
        if k0 is None:
            k0 = k
        if k != k0 or bn.num_features != cv.out_channels:
            return "the convs of net do not share one kernel size or a BatchNorm2d does not match its conv"
        if not bn.affine or not bn.track_running_stats or bn.running_mean is None \
                or not isinstance(bn.momentum, float) or bn.momentum != mods[1].momentum:
            return "a BatchNorm2d lacks affine / track_running_stats or the layers' (float) momenta differ"
    hw = 28 if k0 == 3 else 64  # as vae_spec: Linear(2048) fixes both
    c, h, w = mods[0].in_channels, hw, hw
    enc = []
    for i in range(0, len(mods), 3):
        cv, bn = mods[i], mods[i + 1]
        if cv.in_channels != c:
            return "the convs of net do not chain"
        ho, wo = (h + 2 - k0) // 2 + 1, (w + 2 - k0) // 2 + 1  # Conv2d(k, 2, 1)
        if ho < 1 or wo < 1:
            return "net has more stride-2 convs than the image has pixels"
        enc.append(ConvSpec(cv, bn, True, False, c, h, w, cv.out_channels, ho, wo))
        c, h, w = cv.out_channels, ho, wo
    return mods[0].in_channels, hw, enc, (c, h, w)


def cnn_spec(model):
    """The layer plan of a SimpleCNNClassifier / SimpleCNN64Classifier, or a reason string."""
    from src.models.cnn import SimpleCNN64Classifier, SimpleCNNClassifier

    if type(model) not in (SimpleCNNClassifier, SimpleCNN64Classifier):
        return f"the model is {type(model).__name__}, not SimpleCNNClassifier / SimpleCNN64Classifier"
    trunk = trunk_spec(model)
    if isinstance(trunk, str):
        return trunk
    in_ch, hw, enc, (c, h, w) = trunk
    head = probe_layers(getattr(model, "cls_head", None), name="cls_head")
    if isinstance(head, str):
        return head
    if head[0].in_features != c * h * w:
        return f"cls_head[0] reads {head[0].in_features} features, net gives {c * h * w}"
    return CnnSpec(in_ch, hw, hw, enc, (c, h, w), head)


def cnn_params(spec: CnnSpec) -> list:
    order = []
    for c in spec.enc:
        order += [c.mod.weight, c.mod.bias, c.bn.weight, c.bn.bias]
    l0, bn, _, l2 = spec.head
    return order + [l0.weight, l0.bias, bn.weight, bn.bias, l2.weight, l2.bias]


class TrunkWorkspace(Workspace):
    """Device buffers of one batch size for the conv trunk of a baseline classifier: the conv-encoder part of
    plan.Workspace (activations, gradients, the BatchNorm2d arena of plan.bn_arena with the encoder's finalise flags).
    The conv forward and backward loops, the weight-gradient calls and cv_step_reduce are plan.Workspace's own
    methods; the parts of a VAE these models do not have (latent heads, decoder) are answered as absent."""

    def __init__(self, spec: CnnSpec, n: int, device, with_grad: bool = True):  # (no super().__init__: no VaeSpec)
        self.spec, self.n, self.device = spec, n, device
        _lib.ensure_gemm_workspace(device)
        f32 = dict(dtype=torch.float32, device=device)
        self.y_enc = [torch.empty(n * c.h_out * c.w_out * c.c_out, **f32) for c in spec.enc]
        counts = [n * c.h_out * c.w_out for c in spec.enc]
        self.stats, self.bn_consts, self.bnv, _ = bn_arena([c.bn for c in spec.enc], counts, device)
        self.bn_enc, self.bn_1d, self.bn_dec = self.bnv, None, []
        encoder_finalise_flags(self.bn_enc)
        if with_grad:
            self.g_enc = [torch.empty(n * c.h_out * c.w_out * c.c_out, **f32) for c in spec.enc]
            self._defer_work = {}
            # (the shared split-K workspace of the non-deferred weight-gradient calls, Workspace._wgrad_call)
            L = _lib.lib()
            wb = [int(L.cv_conv_wgrad_workspace_bytes(ctypes.byref(c.geom(n)), 0)) for c in spec.enc]
            self.wg_bytes = max(wb + self._head_wgrad_bytes() + [16])
            self.wg_work = torch.empty(self.wg_bytes // 4, **f32)

    def _head_wgrad_bytes(self) -> list:
        """Split-K workspace bytes of the head's own weight-gradient calls through Workspace._wgrad_call."""
        return []

    def _views(self, which) -> list:
        if isinstance(which, str):
            if which not in ("all", "enc"):
                raise ValueError(f"the CNN workspace has no {which!r} BatchNorm layers")
            return self.bn_enc
        return list(which)

    def fused_heads_forward(self) -> bool:
        return False

    def fused_heads(self) -> bool:
        return False

    def fused_decoder_input(self) -> bool:
        return False


class CnnWorkspace(TrunkWorkspace):
    """The trunk's buffers plus the head's a / da (the output of cls_head[0] and its gradient)."""

    def __init__(self, spec: CnnSpec, n: int, device, with_grad: bool = True):
        super().__init__(spec, n, device, with_grad)
        f32 = dict(dtype=torch.float32, device=device)
        h = spec.head[0].out_features
        self.a = torch.zeros(n, h, **f32)
        if with_grad:
            self.da = torch.empty(n, h, **f32)

    def _head_wgrad_bytes(self) -> list:
        return [int(_lib.lib().cv_linear_wgrad_workspace_bytes(ctypes.byref(self.head_geometry()), 0))]

    def head_geometry(self) -> cv_linear:
        C, Hh, Wh = self.spec.feat
        return cv_linear(self.n, self.spec.F, self.spec.head[0].out_features, Hh * Wh, C, 1, 0, self.spec.mma)

    def trunk_program(self, P: Program, x, train: bool):
        """The conv forwards (Workspace.conv_forward_program) and cls_head[0] into self.a."""
        cur = self.conv_forward_program(P, x, train)
        # (not split over K: the split form adds its partial tiles with floating-point atomics, and the step is
        # bit-reproducible)
        l0 = self.spec.head[0]
        P.add("cv_linear_forward", self.head_geometry(), operand(cur, XF_BNRELU, self.bn_enc[-1].cv(train)),
              l0.weight.data_ptr(), l0.bias.data_ptr(), self.a, 0, ep_none())


def setup_reason(trainer, params, bns):
    """Why the trainer's setup around the parameters `params` and BatchNorm modules `bns` is outside what the device
    baseline steps share (fp32 on one ROCm device, nn.CrossEntropyLoss() defaults, plain single-group Adam, no
    transform, world size 1), or None."""
    dev = params[0].device
    if dev.type != "cuda":
        return "the model is not on the ROCm device"
    tensors = params + [t for b in bns for t in (b.running_mean, b.running_var)]
    if any(t.device != dev or t.dtype != torch.float32 for t in tensors):
        return "the model is not fp32 on one device"
    if any(b.num_batches_tracked.device != dev for b in bns):
        return "the model is not fp32 on one device"
    if not all(p.requires_grad for p in params):
        return "a parameter does not require grad"
    crit = trainer.criterion
    if type(crit) is not nn.CrossEntropyLoss or crit.weight is not None or crit.reduction != "mean" \
            or crit.label_smoothing != 0 or crit.ignore_index != -100:
        return "the criterion is not nn.CrossEntropyLoss() with its defaults"
    if not _AdamState.supported(trainer.optimizer, params):
        return "the optimizer is not a plain single-group torch.optim.Adam over the model's parameters"
    if trainer.transform is not None:
        return "the trainer has a transform"
    if _dist_world() > 1:
        return "a process group with more than one rank is initialised"
    return None


class TrunkStep:
    """What the device steps of the baseline classifiers share (CnnStep here, cvhip.lam.LamStep): the flat parameter
    arena with live p.grad and Adam-moment views, the packed conv weights and their refresh, the static batch inputs
    of a batch size, eager first step and graph replay, and the host-state bookkeeping.  A subclass gives
    unsupported_reason (static), _bns, _step_program and _eval_program, and calls _setup from its __init__."""

    NAME = "cnn step"

    @classmethod
    def build(cls, trainer):
        """A device step for `trainer`, or None outside the contract."""
        if cls.unsupported_reason(trainer) is not None:
            return None
        return cls(trainer)

    def _setup(self, trainer, spec, params):
        self.trainer = trainer
        self.model = trainer.model
        self.spec = spec
        self.params = params
        self.device = self.params[0].device
        self.arena = ParamArena(self.params, self.device)
        self.adam = _AdamState(trainer.optimizer, self.arena)
        for p in self.params:
            p.grad = self.arena.gview(p)
        self._attach_packed()
        self.sizes = {}  # n -> dict(ws, X, lab, count[, work, prog, graph, eval, logits])
        self.graphs_enabled = True
        self.steps_since_sync = 0
        self.steps_taken = 0
        self._packed_sig = None

    def _attach_packed(self):
        """The GEMM-native conv weight copies (plan.attach_packed, encoder part)."""
        sp = self.spec
        sp.packed = torch.empty(sum(2 * c.mod.weight.numel() for c in sp.enc), dtype=torch.float32,
                                device=self.device)
        sp.pack_items = []
        o = 0
        for c in sp.enc:
            w = c.mod.weight
            k = w.numel()
            c.wfwd, c.wbwd = sp.packed[o:o + k], sp.packed[o + k:o + 2 * k]
            o += 2 * k
            sp.pack_items.append(cv_conv_pack(w.data_ptr(), c.wfwd.data_ptr(), c.wbwd.data_ptr(), w.shape[0],
                                              w.shape[1], w.shape[2], w.shape[3]))

    # ----------------------------------------------------------------------------- bookkeeping
    def _head_bns(self) -> list:
        """The BatchNorm modules of the head (after the trunk's)."""
        return []

    def _bns(self):
        return [c.bn for c in self.spec.enc] + self._head_bns()

    def _signature(self):
        t = self.trainer
        sig = [id(t.optimizer), id(t.model), id(t.criterion)]
        for b in self._bns():
            sig += [b.running_mean.data_ptr(), b.running_var.data_ptr(), b.num_batches_tracked.data_ptr(),
                    float(b.eps), b.momentum]
        return tuple(sig)

    def compatible(self) -> bool:
        return (self._signature() == self._sig and self.arena.valid()
                and type(self).unsupported_reason(self.trainer) is None)

    def _fits(self, X) -> bool:
        sp = self.spec
        return (X.device == self.device and X.dim() == 4 and tuple(X.shape[1:]) == (sp.in_ch, sp.H, sp.W)
                and X.dtype.is_floating_point)

    def accepts(self, X) -> bool:
        return self._fits(X) and self.model.training and self._serves(int(X.shape[0]))

    def accepts_eval(self, X) -> bool:
        return self._fits(X) and not self.model.training and int(X.shape[0]) >= 1

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

    def invalidate_packed(self):
        """Repack the conv weights before the next step (after parameters were changed through `.data`)."""
        self._packed_sig = None

    # ----------------------------------------------------------------------------- programs
    def _zero_program(self, P: Program, ws):
        """The step's first launch: the statistics arena and the gradient arena to zero (the deferred weight gradients
        are added onto the gradient arena by cv_step_reduce, as in the VAE step)."""
        zero = [(ws.stats, ws.stats.numel() * 8), (self.arena.grad, self.arena.numel * 4)]
        P.add("cv_zero_many", ptr_array([t.data_ptr() for t, _ in zero]),
              (ctypes.c_size_t * len(zero))(*[nb for _, nb in zero]), len(zero))

    def _adam_program(self, P: Program):
        sp = self.spec
        P.add("cv_adam_pack_step", *self.adam.args(), None, None, struct_array(cv_conv_pack, sp.pack_items),
              len(sp.pack_items))

    def _size(self, n: int, train: bool):
        G = self.sizes.get(n)
        if G is None:
            sp, dev = self.spec, self.device
            G = dict(X=torch.zeros(n, sp.in_ch, sp.H, sp.W, dtype=torch.float32, device=dev),
                     lab=torch.zeros(n, dtype=torch.int64, device=dev), count=0)
            self.sizes[n] = G
        if train and "prog" not in G:
            G["ws"] = self._workspace(n, with_grad=True)
            nbytes = self._work_bytes(n)
            G["work"] = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.float32, device=self.device)
            G["prog"] = self._step_program(G)
            G.pop("eval", None)
        elif "ws" not in G:
            G["ws"] = self._workspace(n, with_grad=False)
        return G

    def _param_sig(self):
        return (self.arena.flat._version,) + tuple(p._version for p in self.params)

    def _ensure_packed(self):
        sig = self._param_sig()
        if self._packed_sig != sig:
            items = self.spec.pack_items
            self._pack_arr = struct_array(cv_conv_pack, items)
            _lib.call("cv_pack_conv_weights", self._pack_arr, len(items), _lib.stream_handle())
            self._packed_sig = sig

    def _load_batch(self, G, X, lab=None):
        """The batch into the programs' static inputs (one launch when no conversion is needed)."""
        raw = X.dtype == torch.float32 and X.is_contiguous() and X.shape == G["X"].shape
        if lab is not None:
            lab = lab.reshape(-1)
            if lab.shape != G["lab"].shape:
                raise ValueError(f"{self.NAME}: {tuple(lab.shape)} labels for a batch of {G['X'].shape[0]}")
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
    def _run_step(self, G, key: str = "prog"):
        """The program G[key] of a batch size: eagerly the first time (it loads the code objects), then as a graph."""
        ran = G.setdefault("ran", set())
        if key in ran and self.graphs_enabled:
            gk = "graph" if key == "prog" else "graph_" + key
            if gk not in G:
                G[gk] = _lib.StepGraph(lambda s: G[key].run(s))
            G[gk].replay()
        else:
            G[key].run()
            ran.add(key)
        G["count"] += 1
        self.steps_since_sync += 1
        self.steps_taken += 1

    def logits(self, X):
        """Eval-mode logits [n][c] of the model on X (a fresh tensor)."""
        G = self._size(int(X.shape[0]), train=False)
        P = self._eval_program(G)
        self._ensure_packed()
        self._load_batch(G, X)
        P.run()
        return G["logits"].clone()


class CnnStep(TrunkStep):
    @staticmethod
    def unsupported_reason(trainer):
        """Why `trainer` is outside the device CNN step's contract (a string), or None when it is inside."""
        spec = cnn_spec(trainer.model)
        if isinstance(spec, str):
            return spec
        params = cnn_params(spec)
        if {id(p) for p in params} != {id(p) for p in trainer.model.parameters()}:
            return "the model has parameters outside net and cls_head"
        why = setup_reason(trainer, params, [c.bn for c in spec.enc] + [spec.head[1]])
        if why is not None:
            return why
        h, c = spec.head[1].num_features, spec.head[3].out_features
        if not _lib.lib().cv_cls_supported(2, h, c):
            return f"cv_cls_step does not serve h={h}, c={c}"
        return None

    def __init__(self, trainer):
        sp = cnn_spec(trainer.model)
        self.bn1d = sp.head[1]
        self.h, self.c = self.bn1d.num_features, sp.head[3].out_features
        self._setup(trainer, sp, cnn_params(sp))
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._sig = self._signature()

    def _head_bns(self):
        return [self.bn1d]

    def _serves(self, n: int) -> bool:
        return bool(_lib.lib().cv_cls_supported(n, self.h, self.c))

    def _workspace(self, n: int, with_grad: bool):
        return CnnWorkspace(self.spec, n, self.device, with_grad=with_grad)

    def _work_bytes(self, n: int) -> int:
        return int(_lib.lib().cv_cls_workspace_bytes(n, self.h, self.c))

    def _cls_struct(self) -> cv_cls:
        bn, l2 = self.bn1d, self.spec.head[3]
        return cv_cls(bn.weight.data_ptr(), bn.bias.data_ptr(), l2.weight.data_ptr(), l2.bias.data_ptr(),
                      bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(),
                      self.h, self.c, float(bn.eps), float(bn.momentum))

    def _step_program(self, G) -> Program:
        ws, sp, pg, n = G["ws"], self.spec, self.arena.gptr, G["ws"].n
        l0, bn, _, l2 = sp.head
        P = Program()
        self._zero_program(P, ws)
        ws.trunk_program(P, G["X"], train=True)
        grad = cv_cls_grad(pg(bn.weight), pg(bn.bias), pg(l2.weight), pg(l2.bias))
        P.add("cv_cls_step", self._cls_struct(), ws.a, G["lab"], n, G["work"], self.loss, ws.da, grad)
        defer = DeferGroup()
        lin = ws.head_geometry()
        y_last, bn_last = ws.y_enc[-1], ws.bn_enc[-1]
        C, Hh, Wh = sp.feat
        # (gbias = NULL: cls_head[0].bias feeds a train-mode BatchNorm, its gradient slot stays exactly zero)
        ws._wgrad_call(P, "linear", lin, operand(ws.da), operand(y_last, XF_BNRELU, bn_last.cv(True)), pg(l0.weight),
                       None, ("head",), defer)
        P.add("cv_linear_backward_data", lin, operand(ws.da), l0.weight.data_ptr(), ws.g_enc[-1], 0,
              ep_bwd(bn_last, y_last, True, stat_div=Hh * Wh))
        ws.encoder_backward_program(P, pg, None, x=G["X"], defer=defer, heads=False)
        ws.step_reduce_program(P, defer, pg, "all", running=True)
        self._adam_program(P)
        P.keep += [G["work"], G["X"], G["lab"]]
        return P

    def _eval_program(self, G):
        if "eval" not in G:
            ws = G["ws"]
            G["logits"] = torch.empty(ws.n, self.c, dtype=torch.float32, device=self.device)
            P = Program()
            ws.trunk_program(P, G["X"], train=False)
            P.add("cv_cls_forward", self._cls_struct(), ws.a, ws.n, G["logits"])
            G["eval"] = P
        return G["eval"]

    def step(self, X, y):
        """One training step on (X [n][C][H][W], y [n]); returns the device [1] loss (overwritten by the next step)."""
        G = self._size(int(X.shape[0]), train=True)
        self.adam.refresh_hyper()
        self._ensure_packed()
        self._load_batch(G, X, y)
        self._run_step(G)
        return self.loss
