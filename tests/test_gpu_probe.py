"""The device downstream probe on the GPU: cv_probe_step / cv_probe_forward at the C-ABI against the fp64 reference of
tests/probe_ref.py, the Adam tail against tests/adam_ref.py, eager against replayed, and DownstreamMLPTrainer with
backend="device" against the fp64 oracle (oracle.cpu_ref.encode(train=False) + the probe in fp64 with torch's Adam).

Inputs and the seed rule: tests/probe_ref.py (no |gamma xhat + beta| under 1e-5 in the fp64 reference, so no ReLU mask
flips on fp32 rounding).  Every buffer a kernel writes sits between sentinel words, checked after every launch.

Bounds.  Loss, dW2, db2, dgamma, dbeta, dW1, running_mean, running_var and the eval logits: relative L2 1e-5 against
fp64 — about 30x the error of the fp32 restatement of the same step (1 - 3.5e-7 per tensor on these inputs) and two
orders below the smallest real defect (one flipped ReLU mask moves a tensor by >= 1e-3 at these sizes).  One exception:
at n = 2 BatchNorm maps every column to +-1 (but for eps), dW1 is a cancellation residue, and its bound is 30x the
restatement's own error computed in the test.  d(b1) is exactly zero; the parameters are bit-unchanged without an
arena.  The Adam tail follows tests/test_gpu_adam.py: adam_ref.Case fed the gradients each launch itself wrote, 8 x e32.
The trainer cases use the bounds of tests/test_gpu_downstream.py (TOL = 1e-4 relative on the probe's parameters, its
running_mean allowance restated for the number of steps taken here).

Measured on an MI355X (relative L2 against fp64; the tests print them as PROBEERR / ADAMERR lines):
  cv_probe_step, params = NULL     seed  loss     dW2      db2      dgamma   dbeta    dW1      rm       rv
  n128-d8-h256-c10-ld32               0  4.0e-08  1.5e-07  8.6e-08  7.4e-08  5.8e-08  2.2e-07  2.4e-08  2.4e-08
  n32-d32-h256-c10-ld128              0  2.6e-08  1.2e-07  7.5e-08  1.1e-07  6.1e-08  1.4e-07  2.4e-08  2.4e-08
  n5-d3-h20-c3-ld3                    0  1.9e-08  8.0e-08  5.0e-08  1.2e-07  7.6e-08  8.4e-08  2.6e-08  2.7e-08
  n3-d4-h16-c2-ld4                    0  8.7e-09  5.7e-08  1.8e-08  5.8e-08  5.4e-08  2.0e-07  2.5e-08  2.3e-08
  n2-d4-h16-c3-ld16                   0  6.8e-08  5.0e-08  4.8e-08  6.8e-08  4.3e-08  9.4e-07  2.3e-08  2.3e-08
    (dW1 bound 7.82e-05)
  n1000-d8-h256-c10-ld8               1  6.7e-08  3.8e-07  7.6e-08  7.2e-08  6.1e-08  5.6e-07  2.4e-08  2.4e-08
  n37-d17-h130-c7-ld40                0  2.2e-08  1.3e-07  1.0e-07  1.2e-07  7.9e-08  1.4e-07  2.7e-08  2.4e-08
  n1024-d64-h64-c4-ld256              0  3.5e-08  3.9e-07  7.2e-08  4.4e-08  2.7e-08  5.6e-07  2.8e-08  2.2e-08
  n64-d8-h512-c32-ld32                0  2.9e-08  1.3e-07  6.7e-08  1.3e-07  1.0e-07  1.9e-07  2.6e-08  2.5e-08
  cv_probe_forward logits: n128-d8-h256-c10-ld32 2.1e-07, n5-d3-h20-c3-ld3 7.2e-08, n37-d17-h130-c7-ld40 2.0e-07,
    n64-d8-h512-c32-ld32 2.9e-07
  Adam tail (p in lr, m in |g|, v in g^2; kernel | e32): step 0: 2.82e-05 4.87e-08 6.3e-08 | 2.82e-05 4.87e-08
    6.3e-08; step 1: 5.1e-05 6.8e-08 9.16e-08 | 5.1e-05 7.37e-08 1.02e-07; step 2: 6.33e-05 5.66e-08 9.74e-08 |
    6.33e-05 6.7e-08 1.25e-07; step 3: 6.17e-05 6.75e-08 1.27e-07 | 6.17e-05 6.75e-08 1.27e-07
  trainer against the fp64 oracle, largest over the three trainer tests: 0.weight 1.5e-06, 1.weight 7.9e-08, 1.bias
    3.6e-05, 1.running_var 1.4e-07, 3.weight 5.3e-07, 3.bias 1.2e-07
"""

import copy
import functools
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import adam_ref as AR
import probe_ref as PR

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel 4-byte words on either side of every buffer a kernel writes
SENT = 0x5A5A5A5A
BOUND = 1e-5
TOL = 1e-4  # tests/test_gpu_downstream.py
LR = 3e-4


class Buf:
    """A device buffer holding `data` (fp32, or int64 with dtype=np.int64) between two runs of sentinel words."""

    def __init__(self, data, dtype=np.float32):
        data = np.ascontiguousarray(data, dtype=dtype).reshape(-1)
        self.n, self.dtype = data.size, dtype
        self.k = 2 if dtype == np.int64 else 1  # 4-byte words per element
        self.words = torch.empty(self.n * self.k + 2 * GUARD, dtype=torch.int32, device="cuda")
        self.words.fill_(SENT)
        body = self.words[GUARD:GUARD + self.n * self.k]
        self.t = body.view(torch.int64 if dtype == np.int64 else torch.float32)
        self.t.copy_(torch.from_numpy(data))

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * self.k * off

    def host(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        w = self.words.cpu()
        return bool((w[:GUARD] == SENT).all() and (w[GUARD + self.n * self.k:] == SENT).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


class Dev:
    """The device side of one probe_ref input set: the six parameters (separately, or inside a p / m / v / g arena
    with padding words), running statistics, the step's outputs and workspace."""

    def __init__(self, inp, arena=False, x_word_offset=0):
        from cvhip import _lib

        self.inp = inp
        n, d, h, c, ldx = self.shape = inp["shape"]
        # x: rows of stride ldx; with x_word_offset = 1 every row starts off the 16-byte grid
        xbuf = torch.zeros(n * ldx + 4, dtype=torch.float32, device="cuda")
        xbuf[x_word_offset:x_word_offset + n * ldx].copy_(torch.from_numpy(inp["xfull"].reshape(-1)))
        self.xbuf, self.xoff = xbuf, x_word_offset
        self.label = torch.from_numpy(inp["label"]).cuda()
        self.rm, self.rv = Buf(inp["rm"]), Buf(inp["rv"])
        self.nbt = Buf(np.array([PR.NBT0]), np.int64)
        self.loss = Buf(np.array([np.nan]))
        nbytes = int(_lib.lib().cv_probe_workspace_bytes(n, h, c))
        assert nbytes % 16 == 0
        self.work = Buf(np.zeros(nbytes // 4))
        self.arena = arena
        if arena:
            # padding words before, between and after the parameters; each parameter on a 16-byte boundary
            self.off, self.pad, o = {}, list(range(4)), 4
            for k in PR.NAMES:
                self.off[k] = o
                o += inp[k].size
                gap = (-o) % 4 + (4 if k in ("b1", "w2") else 0)
                self.pad += list(range(o, o + gap))
                o += gap
            self.pad += list(range(o, o + 8))
            self.numel = o + 8
            rng = np.random.default_rng(77)
            self.p0 = (0.3 * rng.standard_normal(self.numel)).astype(np.float32)
            for k in PR.NAMES:
                self.p0[self.off[k]:self.off[k] + inp[k].size] = inp[k].reshape(-1)
            self.m0 = (0.01 * rng.standard_normal(self.numel)).astype(np.float32)
            self.v0 = (self.m0.astype(np.float64) ** 2 * rng.uniform(0.5, 2.0, self.numel)).astype(np.float32)
            self.p, self.m, self.v = Buf(self.p0), Buf(self.m0), Buf(self.v0)
            self.g = Buf(np.zeros(self.numel))
            pp = {k: self.p.ptr(self.off[k]) for k in PR.NAMES}
            gp = {k: self.g.ptr(self.off[k]) for k in PR.NAMES}
            self.written = [self.p, self.m, self.v, self.g]
        else:
            self.par = {k: Buf(inp[k]) for k in PR.NAMES}
            self.grad = {k: Buf(np.full(inp[k].size, np.nan)) for k in PR.NAMES}
            pp = {k: self.par[k].ptr() for k in PR.NAMES}
            gp = {k: self.grad[k].ptr() for k in PR.NAMES}
            self.written = list(self.grad.values()) + list(self.par.values())
        self.written += [self.rm, self.rv, self.nbt, self.loss, self.work]
        self.P = _lib.cv_probe(*[pp[k] for k in PR.NAMES], self.rm.ptr(), self.rv.ptr(), self.nbt.ptr(), d, h, c,
                               PR.EPS, PR.MOMENTUM)
        self.G = _lib.cv_probe_grad(*[gp[k] for k in PR.NAMES])

    def x_ptr(self):
        return self.xbuf.data_ptr() + 4 * self.xoff

    def set_x(self, xfull):
        n, _, _, _, ldx = self.shape
        self.xbuf[self.xoff:self.xoff + n * ldx].copy_(torch.from_numpy(np.ascontiguousarray(xfull).reshape(-1)))

    def step_args(self, hyper=None, step=None):
        n, d, h, c, ldx = self.shape
        if self.arena:
            adam = (self.p.ptr(), self.g.ptr(), self.m.ptr(), self.v.ptr(), self.numel, hyper.data_ptr(),
                    step.data_ptr())
        else:
            adam = (None, None, None, None, 0, None, None)
        return (self.P, self.x_ptr(), ldx, self.label.data_ptr(), n, self.work.ptr(), self.loss.ptr(), self.G) + adam

    def guards(self, what):
        torch.cuda.synchronize()
        for b in self.written:
            assert b.guards_intact(), what


def _ids(shapes):
    return [PR.shape_id(s) for s in shapes]


# ------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize("shape", PR.SHAPES, ids=_ids(PR.SHAPES))
def test_step_gradients(shape):
    """cv_probe_step with params = NULL: loss, gradients, running statistics and nbt against the fp64 reference."""
    from cvhip import _lib

    inp, ref = PR.case(shape)
    n = shape[0]
    dev = Dev(inp, x_word_offset=1 if shape == (5, 3, 20, 3, 3) else 0)
    _lib.call("cv_probe_step", *dev.step_args(), _lib.stream_handle())
    dev.guards(shape)
    errs = {"loss": abs(float(dev.loss.host()[0]) - float(ref["loss"])) / abs(float(ref["loss"]))}
    for k in ("w2", "b2", "gamma", "beta", "w1"):
        errs["d" + k] = PR.rel_l2(dev.grad[k].host(), ref[k])
    errs["rm"] = PR.rel_l2(dev.rm.host(), ref["rm"])
    errs["rv"] = PR.rel_l2(dev.rv.host(), ref["rv"])
    bounds = {k: BOUND for k in errs}
    if n == 2:  # dW1 is a cancellation residue: 30 x the fp32 restatement's own error on it
        bounds["dw1"] = 30.0 * PR.rel_l2(PR.step_ref(inp, dtype=torch.float32)["w1"], ref["w1"])
    print(f"PROBEERR step {PR.shape_id(shape)} seed {inp['seed']}: "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + (f" (dw1 bound {bounds['dw1']:.2e})" if n == 2 else ""))
    for k, v in errs.items():
        assert v <= bounds[k], (k, v, bounds[k])
    assert not _bits(dev.grad["b1"].host()).any(), "d(b1) must be exact zeros"
    assert int(dev.nbt.host()[0]) == PR.NBT0 + 1
    for k in PR.NAMES:
        assert np.array_equal(_bits(dev.par[k].host()), _bits(inp[k].reshape(-1))), k


# ------------------------------------------------------------------------------------------------ 2. Adam tail
def test_step_adam_tail():
    """The Adam tail of probe_bwd_kernel, as test_mi_learning_step_adam: the reference consumes the gradients each
    launch itself wrote into `grads`.  Hyper set B, t0 = 7, warm moments, an arena with padding words before, between
    and after the parameters that carry live gradients, 4 launches with a fresh x each; two slabs (h = 20)."""
    from cvhip import _lib

    shape, steps, t0 = (37, 8, 20, 3, 8), 4, 7
    inp = PR.make_inputs(shape, 0)
    dev = Dev(inp, arena=True)
    pad = dev.pad
    assert len(pad) >= 12 and pad[0] == 0 and pad[-1] == dev.numel - 1
    rng = np.random.default_rng(78)
    gpad = rng.standard_normal((steps, len(pad))).astype(np.float32)
    hyper = torch.tensor(list(AR.HYPER_B) + [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    step = torch.tensor([t0, 0], dtype=torch.int64, device="cuda")
    padi = torch.tensor(pad, device="cuda")
    grads, got = [], []
    for k in range(steps):
        dev.set_x(rng.standard_normal((shape[0], shape[4])).astype(np.float32))
        dev.g.t.fill_(float("nan"))  # (every parameter's gradient is overwritten by the launch)
        dev.g.t[padi] = torch.from_numpy(gpad[k]).cuda()
        _lib.call("cv_probe_step", *dev.step_args(hyper, step), _lib.stream_handle())
        dev.guards(k)
        assert step.tolist() == [t0 + k + 1, 0], (k, step.tolist())
        assert np.isfinite(float(dev.loss.host()[0]))
        grads.append(dev.g.host().copy())
        assert np.isfinite(grads[-1]).all() and np.array_equal(grads[-1][pad], gpad[k])
        o = dev.off["b1"]
        assert not _bits(grads[-1][o:o + shape[2]]).any()
        got.append((dev.p.host().copy(), dev.m.host().copy(), dev.v.host().copy()))
        assert int(dev.nbt.host()[0]) == PR.NBT0 + k + 1
    case = AR.Case(dev.p0, dev.m0, dev.v0, np.stack(grads), AR.HYPER_B, t0)
    for k in range(steps):
        err, ok = case.errors(k, *got[k])
        print(f"ADAMERR probe_step step {k}: kernel p {err[0]:.3g} m {err[1]:.3g} v {err[2]:.3g}"
              f" | e32 p {case.e32_p[k]:.3g} m {case.e32_m[k]:.3g} v {case.e32_v[k]:.3g}")
        assert ok, (k, err, (case.e32_p[k], case.e32_m[k], case.e32_v[k]))
        # the padding words moved like every other (a kernel that skipped them would leave p0 there)
        assert not np.array_equal(got[k][0][pad], dev.p0[pad] if k == 0 else got[k - 1][0][pad])


# ------------------------------------------------------------------------------------------------ 3. replay
def _run3(mode):
    """Three steps from the same initial state; mode 'eager' or 'graph'.  Returns every piece of state as bits."""
    from cvhip import _lib

    shape = (37, 17, 130, 7, 40)
    inp, _ = PR.case(shape)
    dev = Dev(inp, arena=True)
    hyper = torch.tensor(list(AR.HYPER_A) + [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    step = torch.tensor([3, 0], dtype=torch.int64, device="cuda")
    args = dev.step_args(hyper, step)
    graph = _lib.StepGraph(lambda s: _lib.call("cv_probe_step", *args, s)) if mode == "graph" else None
    out = []
    for k in range(3):
        if graph is not None:
            graph.replay()
        else:
            _lib.call("cv_probe_step", *args, _lib.stream_handle())
        dev.guards((mode, k))
        out.append([_bits(b.host()).copy() for b in (dev.loss, dev.p, dev.m, dev.v, dev.g, dev.rm, dev.rv, dev.nbt)]
                   + [np.array(step.tolist())])
    assert step.tolist() == [6, 0]
    return out


def test_step_replay_bit_identical():
    """Eager and replayed launches from identical state give identical bits (loss, parameters, moments, gradients,
    running statistics, counters), and so do two eager runs."""
    a, b, g = _run3("eager"), _run3("eager"), _run3("graph")
    for k in range(3):
        for i, (x, y, z) in enumerate(zip(a[k], b[k], g[k])):
            assert np.array_equal(x, y), ("eager vs eager", k, i)
            assert np.array_equal(x, z), ("eager vs graph", k, i)
    assert not np.array_equal(a[0][1], a[2][1])  # (the parameters did move)


# ------------------------------------------------------------------------------------------------ 4. eval forward
EVAL_SHAPES = [PR.SHAPES[0], PR.SHAPES[2], PR.SHAPES[6], PR.SHAPES[8]]


@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=_ids(EVAL_SHAPES))
def test_eval_forward(shape):
    from cvhip import _lib

    inp, _ = PR.case(shape)
    n, d, h, c, ldx = shape
    dev = Dev(inp, x_word_offset=1 if ldx == 3 else 0)
    out = Buf(np.full(n * c, np.nan))
    _lib.call("cv_probe_forward", dev.P, dev.x_ptr(), ldx, n, out.ptr(), _lib.stream_handle())
    dev.guards(shape)
    assert out.guards_intact()
    err = PR.rel_l2(out.host(), PR.eval_ref(inp))
    print(f"PROBEERR eval {PR.shape_id(shape)}: logits {err:.2e}")
    assert err <= BOUND
    assert np.array_equal(_bits(dev.rm.host()), _bits(inp["rm"]))
    assert np.array_equal(_bits(dev.rv.host()), _bits(inp["rv"]))
    assert int(dev.nbt.host()[0]) == PR.NBT0
    assert np.isnan(dev.loss.host()[0])  # (untouched)
    for k in PR.NAMES:
        assert np.array_equal(_bits(dev.par[k].host()), _bits(inp[k].reshape(-1))), k


# ------------------------------------------------------------------------------------------------ 5. trainer
def _rel(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _vae(arch, zt, C, sd):
    from src.models.vae import VAE, VAE64

    vae = (VAE if arch == "VAE" else VAE64)(zt, C).cuda()
    vae.load_state_dict({k: torch.as_tensor(np.asarray(v)).float() if np.asarray(v).dtype != np.int64
                         else torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    vae.eval()
    for p in vae.parameters():
        p.requires_grad = False
    return vae


def _probe(d, n_cls, extra=False):
    torch.manual_seed(7)
    layers = [nn.Linear(d, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, n_cls)]
    if extra:
        layers.insert(3, nn.Dropout(0.0))
    return nn.Sequential(*layers)


@functools.lru_cache(maxsize=None)
def _setting(arch, zt, C, n, n_cls=10):
    """The frozen VAE's state, three batches of n and one of 20, and their fp64 mu_c (computed once, shared)."""
    from oracle import cpu_ref as R

    sd = R.det_state(arch, zt, C)
    P = R.to_torch(sd, requires_grad=False)
    batches, mus = [], []
    for s, m in enumerate((n, n, n, 20)):
        x, label, _, _, _ = R.det_inputs(m, C, R.IMAGE[arch], zt, n_cls, seed=11 + s)
        X = torch.tensor(x, dtype=torch.float32)
        batches.append((X, torch.tensor(label).reshape(-1, 1)))
        with torch.no_grad():
            mus.append(R.encode(P, X.double(), arch, train=False)[0])
    return sd, batches, mus


def _oracle(probe0, batches, mus, epochs):
    """The fp64 probe trained straight through with torch's Adam; returns it in eval mode."""
    omlp = copy.deepcopy(probe0).double()
    oopt = torch.optim.Adam(omlp.parameters(), lr=LR)
    omlp.train()
    for _ in range(epochs):
        for (X, y), mu in zip(batches, mus):
            oopt.zero_grad()
            nn.functional.cross_entropy(omlp(mu), y.reshape(-1).long()).backward()
            oopt.step()
    return omlp.eval()


def _bias_drift(steps_oracle, steps_device_side):
    """The allowance of tests/test_gpu_downstream.py for 1.running_mean, restated for T steps: 0.bias feeds a
    train-mode BatchNorm, its gradient is mathematically zero and Adam turns rounding noise into steps of up to lr, so
    after t updates |b_t - b_0| <= t lr on a side whose bias moves at all.  The device step writes exact zeros: from
    zero moments it never moves the bias (steps_device_side = 0); after torch-side steps the first moment those left
    behind keeps moving it for as long as it decays, so every update counts.  running_mean = sum_t 0.1 * 0.9^(T-1-t)
    * mean(W_t mu + b_t) carries that drift."""
    T = steps_oracle
    per_side = lambda moved: sum(0.1 * 0.9 ** (T - 1 - t) * min(t, moved) for t in range(T)) * LR * 1.01  # noqa: E731
    return per_side(T) + per_side(steps_device_side)


def _compare_probe(mlp, omlp, probe0, noise_steps_device):
    T = int(mlp[1].num_batches_tracked)
    assert T == int(omlp[1].num_batches_tracked)
    for (k, a), (_, b) in zip(mlp.state_dict().items(), omlp.state_dict().items()):
        if k == "0.bias":
            b0 = probe0.state_dict()[k].double()
            if noise_steps_device == 0:
                assert torch.equal(a.cpu(), probe0.state_dict()[k]), "0.bias moved under exact-zero gradients"
            else:
                assert float((a.double().cpu() - b0).abs().max()) <= noise_steps_device * LR * 1.01
        elif k == "1.running_mean":
            diff = (a.double().cpu() - b.double()).abs()
            assert float(diff.max()) <= _bias_drift(T, noise_steps_device) + TOL * float(b.abs().max()), k
        elif a.dtype.is_floating_point:
            err = _rel(a, b)
            print(f"PROBEERR trainer {k}: {err:.2e}")
            assert err < TOL, (k, err)


@pytest.mark.parametrize("arch,zt,C,n", [("VAE", 16, 1, 128), ("VAE64", 64, 3, 32)])
def test_trainer_device_backend_matches_oracle(arch, zt, C, n):
    from src.trainer import DownstreamMLPTrainer

    sd, batches, mus = _setting(arch, zt, C, n)
    vae = _vae(arch, zt, C, sd)
    before = {k: v.clone() for k, v in vae.state_dict().items()}
    probe0 = _probe(zt // 2, 10)
    mlp = copy.deepcopy(probe0).cuda()
    opt = torch.optim.Adam(mlp.parameters(), lr=LR)
    tr = DownstreamMLPTrainer(vae, mlp, opt, nn.CrossEntropyLoss(), 10, torch.device("cuda"), backend="device")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for epoch in range(2):
            tr._train(batches, verbose=False, epoch_id=epoch)
    assert not [w for w in rec if "DownstreamMLPTrainer" in str(w.message)], "the device backend was refused"
    eng = tr._engine
    assert eng is not None and eng.steps_taken == 8, "the device engine did not take every step"
    assert all("graph" in eng.sizes[m] and eng.sizes[m]["count"] == cnt for m, cnt in ((n, 6), (20, 2)))
    params = list(mlp.parameters())
    for p in params:
        st = opt.state[p]
        assert float(st["step"]) == 8.0
        o, ln = eng.arena.offset[id(p)]
        assert st["exp_avg"].data_ptr() == eng.adam.m.data_ptr() + 4 * o  # (a live view of the engine's moments)
        assert p.grad is not None and p.grad.data_ptr() == eng.arena.grad.data_ptr() + 4 * o
    assert float(opt.state[params[0]]["exp_avg"].abs().max()) > 0

    omlp = _oracle(probe0, batches, mus, 2)
    _compare_probe(mlp, omlp, probe0, 0)
    for k, v in vae.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in vae.parameters())

    (aupr, auroc), acc = tr.evaluate(batches, verbose=False, epoch_id=0)
    with torch.no_grad():
        ologits = torch.cat([omlp(mu) for mu in mus])
    oy = torch.cat([y.reshape(-1) for _, y in batches])
    oacc = float((ologits.argmax(1) == oy).double().mean())
    assert abs(float(acc) - oacc) <= 1.0 / len(oy) + 1e-12
    assert set(aupr) == set(auroc) == set(range(int(oy.max()) + 1))
    assert eng.steps_taken == 8  # (evaluate trains nothing)


# ------------------------------------------------------------------------------------------------ 6. fallback
def _fit(backend, probe0, criterion, vae, batches, epochs=2):
    from src.trainer import DownstreamMLPTrainer

    mlp = copy.deepcopy(probe0).cuda()
    opt = torch.optim.Adam(mlp.parameters(), lr=LR)
    tr = DownstreamMLPTrainer(vae, mlp, opt, criterion, 10, torch.device("cuda"), backend=backend)
    for epoch in range(epochs):
        tr._train(batches, verbose=False, epoch_id=epoch)
    (_, _), acc = tr.evaluate(batches, verbose=False, epoch_id=0)
    return tr, mlp, opt, acc


@pytest.mark.parametrize("what", ["dropout", "label_smoothing"])
def test_outside_contract_warns_once_and_runs_as_torch(what):
    sd, batches, _ = _setting("VAE", 16, 1, 128)
    vae = _vae("VAE", 16, 1, sd)
    probe0 = _probe(8, 10, extra=what == "dropout")
    crit = nn.CrossEntropyLoss(label_smoothing=0.1 if what == "label_smoothing" else 0.0)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr, mlp, _, acc = _fit("device", probe0, crit, vae, batches)
    ours = [w for w in rec if "DownstreamMLPTrainer" in str(w.message)]
    assert len(ours) == 1, [str(w.message) for w in rec]
    assert tr._engine is None
    _, ref, _, racc = _fit("torch", probe0, crit, vae, batches)
    for (k, a), (_, b) in zip(mlp.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(acc, racc)


def test_torch_epoch_then_device_adopts_the_optimizer_state():
    """One epoch by the torch backend, then the device backend on the same probe and optimizer: the engine adopts the
    Adam moments and the step count, and the two epochs match the fp64 oracle running straight through."""
    from src.trainer import DownstreamMLPTrainer

    sd, batches, mus = _setting("VAE", 16, 1, 128)
    vae = _vae("VAE", 16, 1, sd)
    probe0 = _probe(8, 10)
    mlp = copy.deepcopy(probe0).cuda()
    opt = torch.optim.Adam(mlp.parameters(), lr=LR)
    crit = nn.CrossEntropyLoss()
    DownstreamMLPTrainer(vae, mlp, opt, crit, 10, torch.device("cuda"), backend="torch")._train(batches, verbose=False,
                                                                                          epoch_id=0)
    assert float(opt.state[mlp[0].weight]["step"]) == 4.0
    tr = DownstreamMLPTrainer(vae, mlp, opt, crit, 10, torch.device("cuda"), backend="device")
    tr._train(batches, verbose=False, epoch_id=1)
    assert tr._engine is not None and tr._engine.steps_taken == 4
    assert all(float(opt.state[p]["step"]) == 8.0 for p in mlp.parameters())
    assert tr._engine.adam.step.tolist() == [8, 0]
    _compare_probe(mlp, _oracle(probe0, batches, mus, 2), probe0, 8)
