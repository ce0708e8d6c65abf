"""The classifier tail of the device CNN baseline on the GPU: cv_cls_step / cv_cls_forward at the C-ABI against the
fp64 numpy reference of tests/cnn_ref.py, and eager against replayed launches.

Inputs and the seed rule: tests/cnn_ref.py (no |gamma xhat + beta| under 1e-5 in the fp64 reference, so no ReLU mask
flips on fp32 rounding).  Every buffer a kernel writes sits between sentinel words, checked after every launch.

Bounds.  Loss, dW2, db2, dgamma, dbeta, da, running_mean, running_var and the eval logits: relative L2 1e-5 against
fp64, the bound of tests/test_gpu_probe.py for the same arithmetic.  One exception: at n = 2 BatchNorm maps every
column to +-1 (but for eps), da is a cancellation residue, and its bound is 30x the error of the fp32 numpy
restatement against fp64, computed in the test.  num_batches_tracked is exact.

Measured on an MI355X (relative L2 against fp64; the tests print them as CLSERR lines):
  cv_cls_step        seed  loss     dW2      db2      dgamma   dbeta    da       rm       rv
  n128-h256-c10         0  1.3e-08  1.4e-07  4.2e-08  6.4e-08  5.6e-08  8.0e-08  2.6e-08  2.0e-08
  n2-h16-c2             0  1.4e-07  6.9e-08  5.8e-08  8.5e-08  8.7e-08  2.8e-07  2.7e-08  2.1e-08
    (da bound 6.95e-05)
  n5-h20-c3             0  1.1e-09  7.0e-08  8.7e-08  7.8e-08  8.9e-08  1.0e-07  2.4e-08  2.0e-08
  n37-h130-c7           0  8.4e-08  1.0e-07  1.3e-07  7.8e-08  6.9e-08  8.4e-08  2.8e-08  2.4e-08
  n1024-h64-c4          0  5.7e-08  4.0e-07  7.1e-08  3.0e-08  3.4e-08  7.3e-08  2.6e-08  2.2e-08
  n64-h512-c32          0  6.6e-08  1.1e-07  9.0e-08  1.2e-07  1.0e-07  1.2e-07  2.5e-08  2.4e-08
  cv_cls_forward logits: n1-h20-c3 7.0e-08, n5-h20-c3 7.0e-08, n128-h256-c10 2.1e-07, n1500-h20-c3 6.8e-08
"""

import numpy as np
import pytest
import torch

import cnn_ref as CR

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel 4-byte words on either side of every buffer a kernel writes
SENT = 0x5A5A5A5A
BOUND = 1e-5

# (n, h, c)
SHAPES = [
    (128, 256, 10),  # the scripts'
    (2, 16, 2),      # smallest
    (5, 20, 3),      # ragged
    (37, 130, 7),    # partial slab and row tile
    (1024, 64, 4),   # contract corner
    (64, 512, 32),   # contract corner
]


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

    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        w = self.words.cpu()
        return bool((w[:GUARD] == SENT).all() and (w[GUARD + self.n * self.k:] == SENT).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


class Dev:
    """The device side of one cnn_ref tail input set."""

    def __init__(self, inp):
        from cvhip import _lib

        self.inp = inp
        n, h, c = self.shape = inp["shape"]
        self.a = torch.from_numpy(inp["a"]).cuda()
        self.label = torch.from_numpy(inp["label"]).cuda()
        self.par = {k: Buf(inp[k]) for k in CR.TAIL_NAMES}
        self.grad = {k: Buf(np.full(inp[k].size, np.nan)) for k in CR.TAIL_NAMES}
        self.rm, self.rv = Buf(inp["rm"]), Buf(inp["rv"])
        self.nbt = Buf(np.array([CR.NBT0]), np.int64)
        self.loss = Buf(np.array([np.nan]))
        self.da = Buf(np.full(n * h, np.nan))
        nbytes = int(_lib.lib().cv_cls_workspace_bytes(n, h, c))
        assert nbytes % 16 == 0
        self.work = Buf(np.zeros(nbytes // 4))
        assert self.work.ptr() % 16 == 0
        self.written = (list(self.grad.values()) + list(self.par.values())
                        + [self.rm, self.rv, self.nbt, self.loss, self.da, self.work])
        self.P = _lib.cv_cls(*[self.par[k].ptr() for k in CR.TAIL_NAMES], self.rm.ptr(), self.rv.ptr(),
                             self.nbt.ptr(), h, c, CR.EPS, CR.MOMENTUM)
        self.G = _lib.cv_cls_grad(*[self.grad[k].ptr() for k in CR.TAIL_NAMES])

    def step_args(self):
        return (self.P, self.a.data_ptr(), self.label.data_ptr(), self.shape[0], self.work.ptr(), self.loss.ptr(),
                self.da.ptr(), self.G)

    def guards(self, what):
        torch.cuda.synchronize()
        for b in self.written:
            assert b.guards_intact(), what

    def counters(self):
        """The workspace's arrival counters (its first 64 bytes)."""
        return self.work.host()[:16].view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the step
@pytest.mark.parametrize("shape", SHAPES, ids=[CR.shape_id(s) for s in SHAPES])
def test_step_against_fp64(shape):
    from cvhip import _lib

    inp, ref = CR.tail_case(shape)
    n = shape[0]
    dev = Dev(inp)
    _lib.call("cv_cls_step", *dev.step_args(), _lib.stream_handle())
    dev.guards(shape)
    errs = {"loss": abs(float(dev.loss.host()[0]) - float(ref["loss"])) / abs(float(ref["loss"]))}
    for k in ("w2", "b2", "gamma", "beta"):
        errs["d" + k] = CR.rel_l2(dev.grad[k].host(), ref[k])
    errs["da"] = CR.rel_l2(dev.da.host(), ref["da"])
    errs["rm"] = CR.rel_l2(dev.rm.host(), ref["rm"])
    errs["rv"] = CR.rel_l2(dev.rv.host(), ref["rv"])
    bounds = {k: BOUND for k in errs}
    if n == 2:  # da is a cancellation residue: 30 x the fp32 restatement's own error on it
        bounds["da"] = 30.0 * CR.rel_l2(CR.tail_step(inp, dtype=np.float32)["da"], ref["da"])
    print(f"CLSERR step {CR.shape_id(shape)} seed {inp['seed']}: "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + (f" (da bound {bounds['da']:.2e})" if n == 2 else ""))
    for k, v in errs.items():
        assert v <= bounds[k], (k, v, bounds[k])
    assert int(dev.nbt.host()[0]) == CR.NBT0 + 1
    assert not dev.counters().any(), "the arrival counters did not reset"
    for k in CR.TAIL_NAMES:
        assert np.array_equal(_bits(dev.par[k].host()), _bits(inp[k].reshape(-1))), k


def test_step_label_out_of_range_gives_nan_and_indexes_nothing():
    from cvhip import _lib

    inp, _ = CR.tail_case((5, 20, 3))
    inp = dict(inp, label=inp["label"].copy())
    inp["label"][3] = 3
    dev = Dev(inp)
    _lib.call("cv_cls_step", *dev.step_args(), _lib.stream_handle())
    dev.guards("label")
    assert np.isnan(dev.loss.host()[0])
    assert np.isnan(dev.grad["b2"].host()).all()


def test_step_without_nbt():
    from cvhip import _lib

    inp, ref = CR.tail_case((5, 20, 3))
    dev = Dev(inp)
    dev.P.nbt = None
    _lib.call("cv_cls_step", *dev.step_args(), _lib.stream_handle())
    dev.guards("nbt")
    assert int(dev.nbt.host()[0]) == CR.NBT0
    assert CR.rel_l2(dev.da.host(), ref["da"]) <= BOUND


# ------------------------------------------------------------------------------------------------ 2. eval forward
@pytest.mark.parametrize("n", [1, 5, 128, 1500])
def test_eval_forward(n):
    """n = 1500: the eval forward has no batch limit (the step's 1024 does not apply to it)."""
    from cvhip import _lib

    shape = {1: (5, 20, 3), 5: (5, 20, 3), 128: (128, 256, 10), 1500: (1500, 20, 3)}[n]
    # (beyond the step's contract there is no step reference and no ReLU-margin rule: logits are continuous in a)
    inp = CR.make_tail(shape, 0) if n > 1024 else CR.tail_case(shape)[0]
    _, h, c = shape
    dev = Dev(inp)
    out = Buf(np.full(n * c, np.nan))
    _lib.call("cv_cls_forward", dev.P, dev.a.data_ptr(), n, out.ptr(), _lib.stream_handle())
    dev.guards(n)
    assert out.guards_intact()
    err = CR.rel_l2(out.host(), CR.tail_eval(inp, a=inp["a"][:n]))
    print(f"CLSERR eval n{n}-h{h}-c{c}: logits {err:.2e}")
    assert err <= BOUND
    assert np.array_equal(_bits(dev.rm.host()), _bits(inp["rm"]))
    assert np.array_equal(_bits(dev.rv.host()), _bits(inp["rv"]))
    assert int(dev.nbt.host()[0]) == CR.NBT0
    assert np.isnan(dev.loss.host()[0]) and np.isnan(dev.da.host()).all()  # (untouched)
    assert np.isnan(dev.grad["w2"].host()).all()
    assert not _bits(dev.work.host()).any()
    for k in CR.TAIL_NAMES:
        assert np.array_equal(_bits(dev.par[k].host()), _bits(inp[k].reshape(-1))), k


# ------------------------------------------------------------------------------------------------ 3. determinism
def _run(mode):
    """One launch on fresh buffers; mode 'eager' or 'graph'.  Returns every output as bits."""
    from cvhip import _lib

    inp, _ = CR.tail_case((37, 130, 7))
    dev = Dev(inp)
    args = dev.step_args()
    if mode == "graph":
        _lib.StepGraph(lambda s: _lib.call("cv_cls_step", *args, s)).replay()
    else:
        _lib.call("cv_cls_step", *args, _lib.stream_handle())
    dev.guards(mode)
    assert not dev.counters().any(), "the arrival counters did not reset"
    return [_bits(b.host()).copy() for b in (dev.loss, dev.da, dev.rm, dev.rv, dev.nbt, *dev.grad.values())]


def test_step_replay_bit_identical():
    a, b, g = _run("eager"), _run("eager"), _run("graph")
    for i, (x, y, z) in enumerate(zip(a, b, g)):
        assert np.array_equal(x, y), ("eager vs eager", i)
        assert np.array_equal(x, z), ("eager vs graph", i)
