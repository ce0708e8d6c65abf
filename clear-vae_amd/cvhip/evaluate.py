"""Fused evaluate(): one replayed HIP graph per validation batch for the VAE trainers.

EvalPass runs the body of the trainers' evaluate() loops (code/src/trainer.py:495-570 for the CLEAR trainers,
:366-412 for the GVAE / ML-VAE one) as a fixed sequence of libclearvae_hip.so calls over device-resident buffers:

  eval-mode encoder (running statistics) -> heads + reparameterisation -> decoder up to the last ConvTranspose2d's
  pre-BN output -> the gradient-free contrastive / MI terms of the mode -> cv_eval_batch (reconstruction term without
  xhat, KL terms, the batch's latents and labels appended to the epoch's buffers, the epoch's fp64 totals advanced)

The epoch's accumulators (cv_eval_sink) live on the device and the kernels advance their cursor, so one captured graph
serves every batch of its size and the epoch needs one host read, in finish().  The pass owns its workspaces: it
writes nothing the training engine reads (its statistics, heads, parameters, BatchNorm buffers, optimizer state, the
annealer); it shares only the packed conv weights, which it refreshes from the parameters in begin(), and the Philox
counter of cvhip.rng.
"""

from __future__ import annotations

import ctypes

import torch

from . import _lib, rng
from ._lib import (GROUP, MI_CLUBSAMPLE, MI_INFONCE, SIM, SUPCON, cv_eval_sink, cv_ntxent_branch, cv_supcon_args,
                   cv_tc_disc)
from .autograd import critic_struct, est_params, mlp_struct
from .plan import Program, Workspace, ensure_arena, pack_program, ptr_array

MODES = ("clear", "mim", "tc", "group")


class EvalPass:
    @classmethod
    def unsupported_reason(cls, trainer, mode: str):
        """None when the pass serves the trainer's setup, else why not (ClearStep.build's tests without the
        optimizer ones: evaluation needs no Adam)."""
        from .engine import MI_KINDS, disc_params

        if mode not in MODES:
            raise ValueError(f"EvalPass: mode must be one of {MODES}, not {mode!r}")
        vae = trainer.model
        try:
            dev = next(vae.parameters()).device
        except StopIteration:
            return "the model has no parameters"
        if dev.type != "cuda":
            return f"the model is on {dev.type!r}, not on the ROCm device"
        if trainer.transform is not None:
            return "the trainer has a transform"
        try:
            ensure_arena(vae)
        except (NotImplementedError, AssertionError) as e:
            return f"the model is outside the HIP layer plan ({e})"
        d = vae._cv_spec.d
        if vae._cv_spec.in_ch > 4:
            return "more than 4 image channels"
        if mode == "group":
            if getattr(vae, "mode", None) not in GROUP or d > 64:
                return "group mode needs an ML-VAE / GVAE model with z_dim <= 64"
            return None
        if trainer.sim_fn not in SIM:
            return f"similarity {trainer.sim_fn!r} is not one of {sorted(SIM)}"
        if mode == "clear" and getattr(trainer, "loss_name", "snn_loss") in SUPCON:
            if not _lib.lib().cv_supcon_supported(2, d, SIM[trainer.sim_fn]):
                return f"the supcon kernels do not serve z_dim = {d}"
        if mode == "mim":
            from src.models.mi_estimator import CLUB, CLUBMean, CLUBSample, InfoNCE, L1OutUB, VarUB

            est = trainer.mi_estimator
            if type(est) in (CLUBMean, InfoNCE):
                if getattr(est, "backend", None) != "device":
                    return f"{type(est).__name__} runs on the torch backend"
                if hasattr(est, "F_func"):
                    ok = est.F_func[0].in_features == 2 * d and est.device_supported(2, d)
                else:
                    ok = est.device_supported() and est.p_mu[0].in_features == d and est.p_mu[2].out_features == d
                if not ok:
                    return f"{type(est).__name__} is outside the device kernels' envelope"
            elif type(est) not in (CLUBSample, L1OutUB, CLUB, VarUB):
                return f"estimator {type(est).__name__} has no device kernels"
            assert type(est).__name__ in MI_KINDS
            if any(p.device != dev for p in est_params(est)):
                return "the estimator is on another device"
        if mode == "tc":
            dp = disc_params(trainer.factor_cls)
            if dp is None or dp[0].shape[1] != 2 * d:
                return "the factor discriminator is not Linear(z, z) -> ReLU -> Linear(z, 1) -> Sigmoid"
            if any(p.device != dev for p in dp):
                return "the factor discriminator is on another device"
        return None

    @classmethod
    def build(cls, trainer, mode: str):
        """Return a pass for `trainer`, or None when its setup is outside the contract (unsupported_reason)."""
        if cls.unsupported_reason(trainer, mode) is not None:
            return None
        return cls(trainer, mode)

    def __init__(self, trainer, mode: str):
        from .engine import MI_KINDS

        self.trainer, self.mode = trainer, mode
        self.vae = trainer.model
        self.arena = ensure_arena(self.vae)
        self.spec = self.vae._cv_spec
        self.device = self.arena.device
        self.hp = dict(trainer.hyperparameter)
        self.sim = SIM[trainer.sim_fn] if mode != "group" else 0
        self.supcon = SUPCON.get(getattr(trainer, "loss_name", "snn_loss")) if mode == "clear" else None
        self.kind = MI_KINDS[type(trainer.mi_estimator).__name__] if mode == "mim" else None
        self.est = {"mim": getattr(trainer, "mi_estimator", None), "tc": getattr(trainer, "factor_cls", None)}.get(mode)
        # the extra terms after rec, kl_c, kl_s: (c_loss, s_loss) / (c_loss, mi) / none, with CLEAR's sign on s_loss
        self.nterm = 0 if mode == "group" else 2
        s_sign = 1.0 if (mode != "clear" or self.hp["ps"]) else -1.0
        self.term_scale = (ctypes.c_float * 2)(1.0, s_sign)
        self.seed, self.offset = rng.offset_tensor(self.device)
        self.sizes = {}  # n -> the workspace, static inputs and programs of that batch size
        self.graphs_enabled = True
        f64 = dict(dtype=torch.float64, device=self.device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.totals = torch.zeros(8, **f64)
        self.cap = 0
        self.lat_c = self.lat_s = self.label = None
        self.sink = None
        self._rows = 0  # host mirror of cursor[0] (exact unless the overflow flag is set, which finish() raises on)
        self._sig = self._signature()

    # ----------------------------------------------------------------------------- bookkeeping
    def _signature(self):
        """What the programs' pointers and constants were built from: a change rebuilds them (compatible())."""
        t = self.trainer
        ptrs = [self.arena.flat.data_ptr()]
        for b in self.spec.bn_layers:
            ptrs += [b.running_mean.data_ptr(), b.running_var.data_ptr()]
        if self.mode == "mim":
            ptrs += [p.data_ptr() for p in est_params(t.mi_estimator)]
        if self.mode == "tc":
            ptrs += [p.data_ptr() for p in t.factor_cls.parameters()]
        return (id(self.vae), getattr(t, "sim_fn", None), getattr(t, "loss_name", None),
                tuple(sorted((k, str(v)) for k, v in t.hyperparameter.items())),
                getattr(self.vae, "_cv_precision", "fp32"), id(getattr(t, "mi_estimator", None)),
                id(getattr(t, "factor_cls", None)), tuple(ptrs), self.seed, self.offset.data_ptr())

    def compatible(self) -> bool:
        if not self.arena.valid() or getattr(self.vae, "_cv_arena", None) is not self.arena:
            return False
        if rng.offset_tensor(self.device)[1] is not self.offset:  # (torch's seed changed: a new Philox stream)
            return False
        return self._signature() == self._sig

    def accepts(self, X) -> bool:
        sp = self.spec
        return (X.device.type == "cuda" and X.dim() == 4 and tuple(X.shape[1:]) == (sp.in_ch, sp.H, sp.W)
                and X.shape[0] >= 2)

    # ----------------------------------------------------------------------------- programs
    def _size(self, n: int) -> dict:
        G = self.sizes.get(n)
        if G is not None:
            return G
        sp, d, dev = self.spec, self.spec.d, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        ws = Workspace(sp, n, dev, with_grad=False)
        G = dict(ws=ws, X=torch.empty(n, sp.in_ch, sp.H, sp.W, **f32), lab=torch.zeros(n, dtype=torch.int64, device=dev),
                 eps_buf=torch.zeros(n, 2 * d, **f32), perm_buf=torch.zeros(n, dtype=torch.int64, device=dev),
                 terms=torch.zeros(4, **f32), lse=torch.empty(2, 2 * n, **f32), progs={}, graph=None, count=0)
        hw = sp.H * sp.W
        G["work"] = torch.empty(int(_lib.lib().cv_eval_workspace_bytes(n, sp.in_ch, hw)) // 8, dtype=torch.float64,
                                device=dev)
        L = _lib.lib()
        if self.supcon is not None:
            G["sc_stats"] = torch.zeros(2, int(L.cv_supcon_stats_floats(n)), **f32)
        if self.mode == "mim" and self.kind == MI_INFONCE:
            G["mi_work"] = torch.zeros(int(L.cv_infonce_workspace_bytes(n, self.est.F_func[0].out_features)) // 4 + 16,
                                       **f32)
        elif self.mode == "mim":
            G["mi_work"] = torch.zeros(int(L.cv_mi_workspace_bytes(n)) // 4 + 16, **f32)
        if self.mode == "tc":
            G["mi_work"] = torch.zeros(int(L.cv_tc_workspace_bytes(2 * d)) // 4 + 4, **f32)
        self.sizes[n] = G
        return G

    def _program(self, G: dict, inject: bool, perm: bool) -> Program:
        """The batch's program.  inject: the noise comes from G['eps_buf'] (queued through cvhip.rng) instead of the
        Philox stream; perm: CLUB-S takes G['perm_buf'] instead of drawing its permutation."""
        key = (inject, perm)
        P = G["progs"].get(key)
        if P is not None:
            return P
        sp, ws, d, n, hp = self.spec, G["ws"], self.spec.d, G["ws"].n, self.hp
        P = Program()
        rp = (G["eps_buf"] if inject else None, self.seed, self.offset)
        drew = ws.encoder_program(P, G["X"], False, reparam=rp)
        ws.decoder_program(P, ws.z, False, "none", reparam=None if drew else rp)
        hb, tp = ws.heads.data_ptr(), G["terms"].data_ptr()
        tau = ctypes.c_float(float(hp["temperature"])) if self.mode != "group" else None
        if self.mode != "group" and self.supcon is None:
            # the contrastive terms, gradient-free: content (and, for CLEAR, style) in one phase-2 launch pair
            br = [cv_ntxent_branch(hb, hb + 4 * d, 4 * d, 0, None, None, 0, None, 1.0, tp, G["lse"][0].data_ptr())]
            if self.mode == "clear":
                br.append(cv_ntxent_branch(hb + 8 * d, hb + 12 * d, 4 * d, int(bool(hp["ps"])), None, None, 0, None,
                                           1.0, tp + 4, G["lse"][1].data_ptr()))
            arr = (cv_ntxent_branch * len(br))(*br)
            P.add("cv_ntxent", arr, len(br), G["lab"], n, d, self.sim, tau, 2, 0)
            P.keep.append(arr)
        elif self.supcon is not None:
            lab = G["lab"].data_ptr()
            for k, (off, ps) in enumerate(((0, 0), (8 * d, int(bool(hp["ps"]))))):
                a = cv_supcon_args(hb + off, hb + off + 4 * d, 4 * d, lab, n, d, self.sim, ps, self.supcon,
                                   float(hp["temperature"]), G["sc_stats"][k].data_ptr(), tp + 4 * k, None, None, 0,
                                   None)
                P.add("cv_supcon", a, 0)
        zp = ws.z.data_ptr()
        if self.mode == "mim" and self.kind == MI_INFONCE:
            P.add("cv_infonce_forward", critic_struct(self.est, d), zp, 2 * d, zp + 4 * d, 2 * d, n, G["mi_work"],
                  tp + 4)
        elif self.mode == "mim":
            P.add("cv_mi_forward", self.kind, mlp_struct(self.est), zp, 2 * d, zp + 4 * d, 2 * d, n,
                  G["perm_buf"] if perm else None, ctypes.c_uint64(self.seed), self.offset, G["mi_work"], tp + 4)
        elif self.mode == "tc":
            l0w, l0b, l2w, l2b = [p for p in self.est.parameters()]
            disc = cv_tc_disc(l0w.data_ptr(), l0b.data_ptr(), l2w.data_ptr(), l2b.data_ptr(), l0w.shape[1])
            P.add("cv_tc_forward", disc, ws.z, n, ctypes.c_float(0.0), ws.heads, None, d, G["mi_work"], tp + 4)
        last = sp.dec[-1]
        terms = ptr_array([tp, tp + 4])
        P.add("cv_eval_batch", ws.bn_dec[-1].cv(False), ws.y_dec[-1], G["X"], n, sp.in_ch, last.h_out * last.w_out,
              ws.heads, ws.z, d, G["lab"], terms, self.term_scale, self.nterm, self.sink, G["work"])
        P.keep += [terms, self.term_scale, self.sink]
        G["progs"][key] = P
        return P

    # ----------------------------------------------------------------------------- one epoch
    def begin(self, capacity: int):
        """Start an epoch of at most `capacity` samples: the conv weights packed once from the parameters, the totals
        and the cursor zeroed, the sink sized."""
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError(f"EvalPass.begin: capacity {capacity} < 0")
        d, dev = self.spec.d, self.device
        if self.sink is None or capacity > self.cap:
            # (a larger sink: the programs hold the old one's pointers)
            rows = max(capacity, 1)
            self.lat_c = torch.empty(rows, d, dtype=torch.float32, device=dev)
            self.lat_s = torch.empty(rows, d, dtype=torch.float32, device=dev)
            self.label = torch.empty(rows, dtype=torch.int64, device=dev)
            self.cap = capacity
            self.sink = cv_eval_sink(self.lat_c.data_ptr(), self.lat_s.data_ptr(), self.label.data_ptr(), capacity,
                                     self.cursor.data_ptr(), self.totals.data_ptr())
            for G in self.sizes.values():
                G["progs"], G["graph"] = {}, None
        P = Program()
        pack_program(self.spec, P, "all")
        P.run(_lib.stream_handle())
        self.totals.zero_()
        self.cursor.zero_()
        self._rows = 0

    def _take_injections(self, G):
        """Consume queued test noise (cvhip.rng): eps_c then eps_s, as the module path's two sample() calls do, and
        for CLUB-S one permutation when one is queued.  Returns (inject, perm)."""
        if rng.pending_noise() < 2:
            return False, False
        d = self.spec.d
        ec, es = rng.next_noise(), rng.next_noise()
        G["eps_buf"][:, :d].copy_(ec)
        G["eps_buf"][:, d:].copy_(es)
        if self.mode == "mim" and self.kind == MI_CLUBSAMPLE:
            pm = rng.next_perm()
            if pm is not None:
                G["perm_buf"].copy_(pm)
                return True, True
        return True, False

    def _load_batch(self, G, X, label):
        lab = label.reshape(-1)
        if (X.shape == G["X"].shape and lab.shape == G["lab"].shape and X.dtype == torch.float32 and X.is_contiguous()
                and X.device == G["X"].device and lab.dtype == torch.int64 and lab.is_contiguous()
                and lab.device == G["lab"].device):
            dst = ptr_array([G["X"].data_ptr(), G["lab"].data_ptr()])
            src = ptr_array([X.data_ptr(), lab.data_ptr()])
            nb = (ctypes.c_size_t * 2)(G["X"].numel() * 4, G["lab"].numel() * 8)
            _lib.call("cv_copy_many", dst, src, nb, 2, _lib.stream_handle())
        else:
            if tuple(X.shape) != tuple(G["X"].shape) or lab.numel() != G["lab"].numel():
                raise ValueError(f"EvalPass.batch: X {tuple(X.shape)} / label {tuple(label.shape)} do not fit the "
                                 f"pass's {tuple(G['X'].shape)} input")
            G["X"].copy_(X, non_blocking=True)
            G["lab"].copy_(lab, non_blocking=True)

    def batch(self, X, label):
        """One validation batch: copied into the static buffers, then the replayed graph (the first batch of a size,
        a batch with injected noise, or graphs_enabled = False: the same calls eagerly)."""
        if self.sink is None:
            raise RuntimeError("EvalPass.batch before begin()")
        n = X.shape[0]
        G = self._size(n)
        inject, perm = self._take_injections(G)
        self._load_batch(G, X, label)
        if G["count"] >= 1 and not inject and self.graphs_enabled:
            if G["graph"] is None:
                P = self._program(G, False, False)
                G["graph"] = _lib.StepGraph(lambda s: P.run(s))
            G["graph"].replay()
        else:
            self._program(G, inject, perm).run(_lib.stream_handle())
        G["count"] += 1
        self._rows += n

    def add_module_batch(self, values, z, label):
        """A batch the pass refused (accepts(X) false), from the module path's values (rec, kl_c, kl_s and the mode's
        extra terms, signed as printed), its latents z [n][2d] and labels."""
        if self.sink is None:
            raise RuntimeError("EvalPass.add_module_batch before begin()")
        n, d = z.shape[0], self.spec.d
        if self._rows + n > self.cap:
            self.cursor[1] = 1
            return
        r = self._rows
        self.lat_c[r:r + n].copy_(z[:, :d])
        self.lat_s[r:r + n].copy_(z[:, d:])
        self.label[r:r + n].copy_(label.reshape(-1))
        vals = torch.stack([torch.as_tensor(v, device=self.device).detach().reshape(()).double() for v in values])
        self.totals[:vals.numel()] += vals
        self.totals[7] += 1
        self.cursor[0] += n
        self._rows += n

    def finish(self):
        """(totals [5] as Python floats: rec, kl_c, kl_s and the two extra terms summed over the batches, the batch
        count, label [m], lat_c [m][d], lat_s [m][d]): views of the sink's first m = cursor[0] rows.  The epoch's one
        host read.  Raises RuntimeError when a batch did not fit under the capacity given to begin()."""
        host = torch.cat([self.cursor.double(), self.totals]).cpu().tolist()
        rows, flag, totals = int(host[0]), int(host[1]), host[2:]
        if flag:
            raise RuntimeError(f"EvalPass: the epoch holds more than the {self.cap} samples begin() was given "
                               f"({rows} appended before the batch that did not fit)")
        return totals[:5], int(totals[7]), self.label[:rows], self.lat_c[:rows], self.lat_s[:rows]
