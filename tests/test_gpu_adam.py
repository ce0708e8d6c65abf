"""The three hand-written Adam implementations at the C-ABI against the fp64 reference of tests/adam_ref.py, over
several steps: adam_kernel (cv_adam_step), the Adam fused into pack_small_kernel / pack_kernel (cv_adam_pack_step,
cv_adam_pack_step_part) and the tail of mi_learn_reduce_kernel (cv_mi_learning_step with params != NULL).

Reference: torch.optim.Adam, foreach form (tests/test_adam_ref.py checks adam_ref against it to 1e-12).  Inputs
(adam_ref.make_case): parameters ~N(0, 0.1^2); gradient magnitudes log-uniform over 1e-9 .. 10 per element with
fresh signs every step, a block that is exactly 0 at every step, a few elements of ~1e15; hyper sets
A = (5e-4, 0.9, 0.999, 1e-8, 0) and B = (2e-3, 0.8, 0.95, 1e-6, 0.01) with grad_scale 0.25; step counters starting at
0, at 7 (moments and parameters from 7 reference steps) and at 100000 (the same warm moments).

Tolerance (adam_ref.Case): p, m and v after every launch may differ from the reference by 8 x e32, e32 being the
error of the fp32 restatement of the same trajectory against fp64 (per step, p in units of lr, m in units of the
element's gradient magnitude, v of its square), with a floor of one fp32 ulp of the value.  tests/test_adam_ref.py
pins that every wrong restatement (a bias correction one step late, eps on the wrong side of sqrt(bc2), ...) misses
this by more than 10x.  Exact: the zero-gradient block keeps its parameters bit for bit without weight decay and its
moments at 0; step == [t0 + k + 1, 0] after every launch; aux_counter advances by one; the sentinel words around
p, m, v (and the packed copies) are untouched; the packed copies are the kernel's own new parameters, permuted as
include/clearvae.h defines (gather [tap][cb][cs], scatter [tap][cs][cb]).

Measured on an MI355X (largest over the steps; p in lr, m in |g|, v in g^2; the kernels may use 8 x e32):
                                              e32  p       m       v      kernel  p       m       v
  cv_adam_step 3077, A, t0 0 (12 steps)           1.4e-4  7.5e-8  3.6e-9         2.1e-4  6.5e-8  4.1e-9
  cv_adam_step 3077, B, t0 7                      4.1e-5  2.3e-7  2.2e-7         4.1e-5  2.3e-7  2.3e-7
  cv_adam_step 4, A, t0 0                         3.7e-5  1.1e-8  1.6e-9         6.7e-5  1.1e-8  9.3e-10
  cv_adam_step 2098179, B, t0 7 (2 steps)         1.5e-5  1.1e-6  5.5e-7         1.5e-5  8.2e-7  4.2e-7
  cv_adam_pack_step tiled, B, t0 0 (3 steps)      2.2e-4  3.7e-6  9.4e-7         2.2e-4  3.7e-6  9.4e-7
  cv_adam_pack_step tiled-strided, B, t0 7        2.2e-5  2.5e-6  1.1e-6         2.2e-5  1.9e-6  5.1e-7
  cv_adam_pack_step small-strided, A, t0 0        8.7e-5  3.5e-8  6.3e-10        8.9e-5  2.9e-8  5.2e-10
  cv_mi_learning_step (4 steps)                   3.6e-5  6.7e-8  2.1e-7         3.6e-5  6.7e-8  2.1e-7
Over all cases the kernels' errors are 0.6 .. 2.4 x e32 of the same step, but for the parameters of the 4-element
case (two live elements: 6.1 x at one step).  A copy of the library with one error per kernel (adam_kernel: bias
corrections one step late; adam_consts: beta1 in the v decay; mi_learn_reduce_kernel: eps before the division by
sqrt(bc2)) fails every test here but the six cv_adam_step cases at t0 = 100000, where a late bias correction is 1
either way."""

import functools

import numpy as np
import pytest
import torch

import adam_ref as AR

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel fp32 words on either side of every buffer a kernel writes
SENT = 0x5A5A5A5A
AUX0 = 41


class Buf:
    """A device fp32 buffer holding `data` between two runs of sentinel words."""

    def __init__(self, data):
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        self.n = data.size
        self.full = torch.empty(self.n + 2 * GUARD, dtype=torch.float32, device="cuda")
        self.full.view(torch.int32).fill_(SENT)
        self.t = self.full[GUARD:GUARD + self.n]
        self.t.copy_(torch.from_numpy(data))

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off

    def host(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        w = self.full.view(torch.int32).cpu()
        return bool((w[:GUARD] == SENT).all() and (w[GUARD + self.n:] == SENT).all())


class Dev:
    """The device side of a Case: p / m / v / g, the hyper block, the step words, grad_scale and aux_counter."""

    def __init__(self, case, hyper_set, aux=True):
        hyper, scale = AR.SETS[hyper_set]
        assert (AR.TOL_FACTOR * case.e32_p < 0.02).all(), case.e32_p  # (the rule's condition: no mutant fits under it)
        self.case = case
        self.wd = hyper[4]
        self.p, self.m, self.v, self.g = Buf(case.p0), Buf(case.m0), Buf(case.v0), Buf(case.g[0])
        self.hyper = torch.tensor(list(hyper) + [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
        self.step = torch.tensor([case.t0, 0], dtype=torch.int64, device="cuda")
        self.gscale = None if scale == 1.0 else torch.tensor([scale], dtype=torch.float32, device="cuda")  # (A: NULL)
        self.aux = torch.tensor([AUX0], dtype=torch.int64, device="cuda") if aux else None

    def load_grad(self, k):
        self.g.t.copy_(torch.from_numpy(self.case.g[k]))

    def args(self, off=0, numel=None):
        """The leading arguments of the three cv_adam_* entry points (for the arena part starting at word `off`)."""
        from cvhip import _lib

        return (self.p.ptr(off), self.g.ptr(off), self.m.ptr(off), self.v.ptr(off),
                self.case.numel - off if numel is None else numel, self.hyper.data_ptr(), self.step.data_ptr(),
                _lib.ptr(self.gscale), _lib.ptr(self.aux))

    def check(self, k, what, lo=0, hi=None):
        """After launch k: elements [lo, hi) against the reference, the exact properties and the sentinels."""
        torch.cuda.synchronize()
        c = self.case
        hi = c.numel if hi is None else hi
        p, m, v = self.p.host(), self.m.host(), self.v.host()
        sub = _Slice(c, lo, hi)
        err, ok = sub.errors(k, p[lo:hi], m[lo:hi], v[lo:hi])
        print(f"ADAMERR {what} step {k}: kernel p {err[0]:.3g} m {err[1]:.3g} v {err[2]:.3g}"
              f" | e32 p {c.e32_p[k]:.3g} m {c.e32_m[k]:.3g} v {c.e32_v[k]:.3g}")
        assert ok, (what, k, err, (c.e32_p[k], c.e32_m[k], c.e32_v[k]))
        z0, z1 = AR.zero_block(c.numel)
        z0, z1 = max(z0, lo), min(z1, hi)
        if self.wd == 0 and z1 > z0:
            assert np.array_equal(p[z0:z1].view(np.int32), c.p0[z0:z1].view(np.int32)), (what, k)
            assert not m[z0:z1].view(np.int32).any() and not v[z0:z1].view(np.int32).any(), (what, k)
        for b in (self.p, self.m, self.v):
            assert b.guards_intact(), (what, k)
        return p

    def counters(self):
        torch.cuda.synchronize()
        return self.step.tolist(), (None if self.aux is None else int(self.aux))


class _Slice:
    """Case.errors over the elements [lo, hi)."""

    def __init__(self, c, lo, hi):
        self.P, self.M, self.V = c.P[:, lo:hi], c.M[:, lo:hi], c.V[:, lo:hi]
        self.tol_p, self.tol_m, self.tol_v = c.tol_p[:, lo:hi], c.tol_m[:, lo:hi], c.tol_v[:, lo:hi]
        self.gmag, self.lr = c.gmag[lo:hi], c.lr

    errors = AR.Case.errors


@functools.lru_cache(maxsize=None)
def _case(numel, hyper_set, t0, steps=AR.STEPS):
    return AR.make_case(numel, hyper_set, t0, steps)


def _expect_counters(dev, t, naux, what):
    step, aux = dev.counters()
    assert step == [t, 0], (what, step, t)
    assert aux is None or aux == AUX0 + naux, (what, aux, naux)


# ------------------------------------------------------------------------------------------------ cv_adam_step
@pytest.mark.parametrize("t0", [0, 7, 100000])
@pytest.mark.parametrize("hyper_set", ["A", "B"])
@pytest.mark.parametrize("numel", [4, 1027, 3077])
def test_adam_step(numel, hyper_set, t0):
    """adam_kernel: one float4 (4), a scalar tail of 3 (1027), several workgroups and a tail of 1 (3077)."""
    from cvhip import _lib

    case = _case(numel, hyper_set, t0)
    dev = Dev(case, hyper_set, aux=t0 != 7)  # (t0 = 7: NULL aux_counter; set A: NULL grad_scale)
    for k in range(case.steps):
        dev.load_grad(k)
        _lib.call("cv_adam_step", *dev.args(), _lib.stream_handle())
        dev.check(k, f"adam_step[{numel}-{hyper_set}-{t0}]")
        _expect_counters(dev, t0 + k + 1, k + 1, (numel, hyper_set, t0, k))


@pytest.mark.parametrize("hyper_set,t0", [("A", 0), ("B", 7)])
def test_adam_step_grid_stride(hyper_set, t0):
    """More float4s than 2048 workgroups x 256 threads: a second grid-stride trip, and a scalar tail of 3."""
    from cvhip import _lib

    numel = 2 * 1024 * 1024 + 1024 + 3
    assert numel // 4 > 2048 * 256 and numel % 4 == 3
    case = AR.make_case(numel, hyper_set, t0, 2)  # (not kept: ~0.3 GB of fp64 reference and tolerances)
    dev = Dev(case, hyper_set)
    for k in range(case.steps):
        dev.load_grad(k)
        _lib.call("cv_adam_step", *dev.args(), _lib.stream_handle())
        dev.check(k, f"adam_step[{numel}-{hyper_set}-{t0}]")
        _expect_counters(dev, t0 + k + 1, k + 1, (numel, hyper_set, t0, k))


def test_adam_step_replayed():
    """One captured launch replayed with fresh gradients in the same buffer: the step counter is read on the device,
    so every replay takes its own t (bias corrections of steps 8 .. 11, not four times step 8's)."""
    from cvhip import _lib

    case = _case(3077, "B", 7)
    dev = Dev(case, "B")
    args = dev.args()
    graph = _lib.StepGraph(lambda s: _lib.call("cv_adam_step", *args, s))
    _expect_counters(dev, 7, 0, "capture runs nothing")
    for k in range(4):
        dev.load_grad(k)
        graph.replay()
        dev.check(k, "adam_step[replay]")
        _expect_counters(dev, 7 + k + 1, k + 1, ("replay", k))


# ------------------------------------------------------------------------------------------- cv_adam_pack_step
# name -> (items (cs, cb, kh, kw, copies) in arena order, gaps before / between / after them, listing order)
ARENAS = {
    # every item under 256K elements: pack_small_kernel
    "small": ([(8, 4, 4, 4, "gs"), (5, 3, 3, 3, "g"), (17, 33, 1, 1, "s")], [5, 3, 9, 6], [2, 0, 1]),
    # one item covering the arena exactly: no plain range (nplain == 0)
    "exact": ([(6, 10, 3, 3, "gs")], [0, 0], [0]),
    # 280,704 elements, both dimensions off the 16 x 32 tile: pack_kernel, and a tiny item through it too
    "tiled": ([(5, 3, 3, 3, "s"), (136, 129, 4, 4, "gs")], [7, 2, 11], [1, 0]),
    # 33 x 33 = 1089 tiles > the 1024 workgroups an item gets: the tile loop strides
    "tiled-strided": ([(528, 1056, 1, 1, "gs")], [3, 5], [0]),
    # 25 taps > 16 force pack_small_kernel at 275,000 elements: 1075 > 1024 workgroups, the element loop strides
    "small-strided": ([(100, 110, 5, 5, "gs")], [1, 2], [0]),
}


def _layout(name, base=0):
    """[(offset, cs, cb, kh, kw, copies)] in listing order and the arena's length."""
    items, gaps, order = ARENAS[name]
    out, o = [], base
    for it, gap in zip(items, gaps):
        o += gap
        out.append((o,) + it)
        o += it[0] * it[1] * it[2] * it[3]
    return [out[i] for i in order], o + gaps[-1] - base


class Packed:
    """The cv_conv_pack items of a layout over dev.p, with guarded destinations."""

    def __init__(self, dev, layout):
        from cvhip import _lib

        self.layout, self.bufs, items = layout, [], []
        for o, cs, cb, kh, kw, copies in layout:
            ln = cs * cb * kh * kw
            ga = Buf(np.full(ln, 12345.0)) if "g" in copies else None
            sc = Buf(np.full(ln, 12345.0)) if "s" in copies else None
            self.bufs.append((ga, sc))
            items.append(_lib.cv_conv_pack(dev.p.ptr(o), ga.ptr() if ga else None, sc.ptr() if sc else None,
                                           cs, cb, kh, kw))
        self.arr = (_lib.cv_conv_pack * len(items))(*items)
        self.n = len(items)

    def check(self, p, what):
        """Both copies bit-equal to the kernel's new parameters `p` (host), permuted on the host."""
        for (o, cs, cb, kh, kw, copies), (ga, sc) in zip(self.layout, self.bufs):
            W = p[o:o + cs * cb * kh * kw].reshape(cs, cb, kh, kw)
            for buf, perm in ((ga, (2, 3, 1, 0)), (sc, (2, 3, 0, 1))):
                if buf is None:
                    continue
                want = np.ascontiguousarray(W.transpose(perm)).reshape(-1)
                assert np.array_equal(buf.host().view(np.int32), want.view(np.int32)), (what, (cs, cb, kh, kw), perm)
                assert buf.guards_intact(), (what, (cs, cb, kh, kw), perm)


@pytest.mark.parametrize("name,hyper_set,t0", [
    ("small", "A", 0), ("small", "B", 7), ("exact", "B", 100000), ("tiled", "A", 7), ("tiled", "B", 0),
    ("tiled-strided", "B", 7), ("small-strided", "A", 0)])
def test_adam_pack_step(name, hyper_set, t0):
    from cvhip import _lib

    layout, numel = _layout(name)
    case = _case(numel, hyper_set, t0, 3)
    dev = Dev(case, hyper_set, aux=name != "exact")
    pk = Packed(dev, layout)
    for k in range(case.steps):
        dev.load_grad(k)
        _lib.call("cv_adam_pack_step", *dev.args(), pk.arr, pk.n, _lib.stream_handle())
        p = dev.check(k, f"adam_pack_step[{name}-{hyper_set}-{t0}]")  # (the whole arena, gaps included)
        _expect_counters(dev, t0 + k + 1, k + 1, (name, k))
        pk.check(p, (name, k))


def test_adam_pack_step_part():
    """A split update: the arena's tail (a tiled item and a tiny one) with advance = 0, then its head (small items)
    with advance = 1.  The first call leaves step[0] and aux_counter alone; both take the bias corrections of the same
    t; the second advances both once."""
    from cvhip import _lib

    head, cut = _layout("small")
    tail, ntail = _layout("tiled", cut)
    t0 = 7
    case = _case(cut + ntail, "B", t0, 2)
    dev = Dev(case, "B")
    pk_head, pk_tail = Packed(dev, head), Packed(dev, tail)
    for k in range(case.steps):
        dev.load_grad(k)
        before = dev.p.host().copy()
        _lib.call("cv_adam_pack_step_part", *dev.args(cut), pk_tail.arr, pk_tail.n, 0, _lib.stream_handle())
        p = dev.check(k, "adam_pack_step_part[tail]", cut, case.numel)
        _expect_counters(dev, t0 + k, k, ("tail", k))
        assert np.array_equal(p[:cut].view(np.int32), before[:cut].view(np.int32))
        pk_tail.check(p, ("tail", k))
        _lib.call("cv_adam_pack_step_part", *dev.args(0, cut), pk_head.arr, pk_head.n, 1, _lib.stream_handle())
        p = dev.check(k, "adam_pack_step_part[both]")
        _expect_counters(dev, t0 + k + 1, k + 1, ("head", k))
        pk_head.check(p, ("head", k))
        pk_tail.check(p, ("tail after head", k))


# ----------------------------------------------------------------------------------------- cv_mi_learning_step
def test_mi_learning_step_adam():
    """The Adam tail of mi_learn_reduce_kernel, isolated from the estimator's gradient (tests/test_gpu_mi_*.py check
    that): the reference consumes the gradients each launch itself wrote into `grads`.  Hyper set B (the entry point
    has no grad_scale), t0 = 7, an arena with padding words before, between and after the parameters that carry
    non-zero gradients, parameters and moments."""
    from cvhip import _lib

    dx = dy = 8
    h, n, steps, t0 = 16, 64, 4, 7
    sizes = [("w1", h * dx), ("b1", h), ("pad", 4), ("w2", dy * h), ("b2", dy), ("w3", h * dx), ("b3", h),
             ("w4", dy * h), ("b4", dy)]
    off, o = {}, 4  # (4 padding words first; every parameter on a 16-byte boundary, as in a ParamArena)
    pad = list(range(4))
    for name, ln in sizes:
        if name == "pad":
            pad += list(range(o, o + ln))
        else:
            off[name] = o
        o += ln
    pad += list(range(o, o + 8))
    numel = o + 8
    rng = np.random.default_rng(77)
    p0 = (0.3 * rng.standard_normal(numel)).astype(np.float32)
    m0 = (0.01 * rng.standard_normal(numel)).astype(np.float32)
    v0 = (m0.astype(np.float64) ** 2 * rng.uniform(0.5, 2.0, numel)).astype(np.float32)
    gpad = rng.standard_normal((steps, len(pad))).astype(np.float32)
    p, m, v, g = Buf(p0), Buf(m0), Buf(v0), Buf(np.zeros(numel))
    hyper = torch.tensor(list(AR.HYPER_B) + [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    step = torch.tensor([t0, 0], dtype=torch.int64, device="cuda")
    x = torch.tensor(rng.standard_normal((n, dx)), dtype=torch.float32, device="cuda")
    y = torch.tensor(rng.standard_normal((n, dy)), dtype=torch.float32, device="cuda")
    work = torch.zeros(int(_lib.lib().cv_mi_workspace_bytes(n)) // 4 + 16, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    names = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
    mlp = _lib.cv_mlp(*[p.ptr(off[k]) for k in names], dx, h, dy)
    G = _lib.cv_mlp_grad(*[g.ptr(off[k]) for k in names])
    grads, got = [], []
    for k in range(steps):
        g.t.fill_(float("nan"))  # (every parameter's gradient is overwritten by the launch)
        g.t[torch.tensor(pad, device="cuda")] = torch.from_numpy(gpad[k]).cuda()
        _lib.call("cv_mi_learning_step", mlp, x.data_ptr(), dx, y.data_ptr(), dy, n, work.data_ptr(), loss.data_ptr(),
                  G, p.ptr(), g.ptr(), m.ptr(), v.ptr(), numel, hyper.data_ptr(), step.data_ptr(),
                  _lib.stream_handle())
        torch.cuda.synchronize()
        assert step.tolist()[0] == t0 + k + 1, (k, step.tolist())
        assert np.isfinite(float(loss))
        grads.append(g.host().copy())
        assert np.isfinite(grads[-1]).all() and np.array_equal(grads[-1][pad], gpad[k])
        got.append((p.host().copy(), m.host().copy(), v.host().copy()))
        for b in (p, m, v, g):
            assert b.guards_intact(), k
    case = AR.Case(p0, m0, v0, np.stack(grads), AR.HYPER_B, t0)
    for k in range(steps):
        err, ok = case.errors(k, *got[k])
        print(f"ADAMERR mi_learning_step step {k}: kernel p {err[0]:.3g} m {err[1]:.3g} v {err[2]:.3g}"
              f" | e32 p {case.e32_p[k]:.3g} m {case.e32_m[k]:.3g} v {case.e32_v[k]:.3g}")
        assert ok, (k, err, (case.e32_p[k], case.e32_m[k], case.e32_v[k]))
        # the padding words moved like every other (a kernel that skipped them would leave p0 there)
        assert not np.array_equal(got[k][0][pad], p0[pad] if k == 0 else got[k - 1][0][pad])
