"""The LAM tail on the GPU: cv_lam_step / cv_lam_forward / cv_lam_pair at the C-ABI against the fp64 numpy reference
of tests/lam_ref.py, and eager against replayed launches.

Inputs and the seed rule: tests/lam_ref.py (no BatchNorm output under 1e-5 in the fp64 reference, so no ReLU mask flips
on fp32 rounding).  Every buffer a kernel writes sits between sentinel words, checked after every launch.  The
BatchNorm's forward sums are filled as tests/test_gpu_declinear.py::test_heads_backward fills them (replica 0, fp64).

Bounds.  ce, lam, gW, gb, gin, the two backward sums and the eval logits: relative L2 1e-5 against fp64, the bound of
tests/test_gpu_cnn.py and tests/test_gpu_probe.py for this arithmetic.  At n = 2 a quantity that is a cancellation
residue would take 30x the error of the fp32 numpy restatement instead (the exception rule of tests/test_gpu_cnn.py);
the test computes that figure and prints it, and no quantity of this tail needed it.  The ReLU mask is the reference's
away from |BN output| < 1e-5 (nowhere, by the seed rule).

Each shape runs at lam_coef 0.1 and 8 (the LAM terms dominate at 8) with one pair kind: a label-preserving shuffle, a
permutation that crosses labels, one with fixed points, or a shuffle with an absent class.

Measured on an MI355X (relative L2 against fp64, the larger of the lam 0.1 and lam 8 runs; the tests print both as
LAMERR lines):
  cv_lam_step                     seed  ce       lam      gw       gb       gin      gs1      gs2
  n128-ch128-pix16-c10-shuffle      28  3.8e-09  1.9e-09  1.3e-07  9.9e-08  8.1e-08  8.0e-08  9.5e-08
  n128-ch512-pix4-c4-cross          19  4.3e-08  4.6e-08  1.3e-07  3.9e-08  7.8e-08  6.9e-08  8.4e-08
  n2-ch4-pix1-c2-cross               0  9.9e-08  7.7e-07  1.1e-06  1.1e-06  6.5e-07  6.5e-07  1.2e-06
    (30 x the fp32 restatement would have been 8.6e-06 2.3e-05 3.2e-05 3.2e-05 1.9e-05 1.9e-05 3.6e-05)
  n5-ch8-pix9-c3-fixed               0  1.8e-08  2.8e-09  9.7e-08  3.5e-08  6.5e-08  4.5e-08  5.4e-08
  n37-ch12-pix16-c7-absent           0  5.7e-08  3.0e-08  9.7e-08  8.6e-08  7.9e-08  5.8e-08  4.0e-08
  n1024-ch16-pix4-c32-shuffle        0  7.1e-08  2.9e-08  1.1e-07  1.6e-07  1.0e-07  4.9e-08  5.1e-08
  cv_lam_forward logits: n1-ch8-pix9-c3 1.5e-07, n5-ch8-pix9-c3 7.9e-08, n128-ch128-pix16-c10 1.3e-07,
    n1500-ch512-pix4-c4 1.3e-07
"""

import ctypes

import numpy as np
import pytest
import torch

import lam_ref as LR

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel 4-byte words on either side of every buffer a kernel writes
SENT = 0x5A5A5A5A
BOUND = 1e-5

# (n, ch, pix, c), pair kind
SHAPES = [
    ((128, 128, 16, 10), "shuffle"),  # LAMCNNClassifier's trunk
    ((128, 512, 4, 4), "cross"),      # LAMCNN64Classifier's
    ((2, 4, 1, 2), "cross"),          # smallest
    ((5, 8, 9, 3), "fixed"),          # ragged
    ((37, 12, 16, 7), "absent"),      # partial slab and row tile
    ((1024, 16, 4, 32), "shuffle"),   # contract corner
]
IDS = [f"{LR.shape_id(s)}-{k}" for s, k in SHAPES]
_WORDS = {np.float32: (torch.float32, 1), np.int64: (torch.int64, 2), np.float64: (torch.float64, 2)}


class Buf:
    """A device buffer holding `data` (fp32, fp64 or int64) between two runs of sentinel words."""

    def __init__(self, data, dtype=np.float32):
        data = np.ascontiguousarray(data, dtype=dtype).reshape(-1)
        self.n, (self.tdtype, self.k) = data.size, _WORDS[dtype]
        self.words = torch.empty(self.n * self.k + 2 * GUARD, dtype=torch.int32, device="cuda")
        self.words.fill_(SENT)
        self.t = self.words[GUARD:GUARD + self.n * self.k].view(self.tdtype)
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
    """The device side of one lam_ref tail input set."""

    def __init__(self, inp, lam, pair=None, label=None, train=True):
        from cvhip import _lib

        self.inp = inp
        n, ch, pix, c = self.shape = inp["shape"]
        F, R = ch * pix, _lib.stat_repl(ch)
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.y = cuda(inp["y"])
        self.label = cuda(inp["label"] if label is None else label)
        self.pair = cuda(inp["pair"] if pair is None else pair)
        self.lam = torch.tensor([lam], dtype=torch.float32, device="cuda")
        self.gamma, self.beta, self.rm, self.rv = (Buf(inp[k]) for k in ("gamma", "beta", "rm", "rv"))
        self.w, self.b = Buf(inp["w"]), Buf(inp["b"])
        yc = inp["y"].astype(np.float64).reshape(n * pix, ch)
        stat = np.zeros((R, 2, ch))
        stat[0, 0], stat[0, 1] = yc.sum(0), (yc * yc).sum(0)
        self.stat = Buf(stat, np.float64)
        self.gstat = Buf(np.zeros((R, 2, ch)), np.float64)
        self.gw, self.gb = Buf(np.full(c * F, np.nan)), Buf(np.full(c, np.nan))
        self.loss = Buf(np.full(2, np.nan))
        self.gin = Buf(np.full(n * F, np.nan))
        nbytes = int(_lib.lib().cv_lam_workspace_bytes(min(max(n, 2), 1024), ch, pix, c))  # (eval: any n)
        assert nbytes > 0 and nbytes % 16 == 0
        self.work = Buf(np.zeros(nbytes // 4))
        assert self.work.ptr() % 16 == 0
        self.consts = [self.gamma, self.beta, self.rm, self.rv, self.w, self.b, self.stat]
        self.outputs = [self.loss, self.gw, self.gb, self.gin, self.gstat]
        self.P = _lib.cv_lam(self.w.ptr(), self.b.ptr(), self.lam.data_ptr(), c, ch, pix)
        self.bn = _lib.cv_bn(self.gamma.ptr(), self.beta.ptr(), self.stat.ptr(), self.gstat.ptr(), self.rm.ptr(),
                             self.rv.ptr(), ch, n * pix, int(train), LR.EPS, None, None, None)
        self.G = _lib.cv_lam_grad(self.gw.ptr(), self.gb.ptr())

    def step_args(self):
        return (self.P, self.y.data_ptr(), ctypes.byref(self.bn), self.label.data_ptr(), self.pair.data_ptr(),
                self.shape[0], self.work.ptr(), self.loss.ptr(), self.gin.ptr(), self.gstat.ptr(), self.G)

    def guards(self, what):
        torch.cuda.synchronize()
        for b in self.consts + self.outputs + [self.work]:
            assert b.guards_intact(), what
        for b, k in zip(self.consts[:6], ("gamma", "beta", "rm", "rv", "w", "b")):
            assert np.array_equal(_bits(b.host()), _bits(self.inp[k].reshape(-1))), k

    def counters(self):
        """The workspace's arrival counters (its first 64 bytes)."""
        return self.work.host()[:16].view(np.int32)

    def results(self):
        n, ch, pix, c = self.shape
        gs = self.gstat.host().reshape(-1, 2, ch)
        assert not gs[1:].any(), "a replica other than 0 was written"
        loss = self.loss.host()
        return dict(ce=loss[0], lam=loss[1], gw=self.gw.host().reshape(c, -1), gb=self.gb.host(),
                    gin=self.gin.host().reshape(n, pix, ch), gs1=gs[0, 0], gs2=gs[0, 1])


def _step(dev):
    from cvhip import _lib

    _lib.call("cv_lam_step", *dev.step_args(), _lib.stream_handle())
    dev.guards(dev.shape)
    assert not dev.counters().any(), "the arrival counter did not reset"
    return dev.results()


# ------------------------------------------------------------------------------------------------ 1. the step
@pytest.mark.parametrize("lam", [0.1, 8.0])
@pytest.mark.parametrize("shape,kind", SHAPES, ids=IDS)
def test_step_against_fp64(shape, kind, lam):
    inp, ref = LR.tail_case(shape, kind), LR.tail_ref(shape, kind, lam)
    got = _step(Dev(inp, lam))
    keys = ("ce", "lam", "gw", "gb", "gin", "gs1", "gs2")
    errs = {k: LR.rel_l2(got[k], ref[k]) for k in keys}
    note = ""
    if shape[0] == 2:  # what the exception rule for cancellation residues would allow (not needed: printed only)
        r32 = LR.tail_step(inp, lam, dtype=np.float32)
        note = " (30 x fp32 restatement: " + " ".join(f"{k} {30 * LR.rel_l2(r32[k], ref[k]):.1e}" for k in keys) + ")"
    print(f"LAMERR step {LR.shape_id(shape)}-{kind} lam {lam} seed {inp['seed']}: "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + note)
    for k, v in errs.items():
        assert v <= BOUND, (k, v)
    mask, edge = got["gin"] != 0, np.abs(ref["pre"]) < 1e-5
    assert ((ref["pre"] > 0) == mask)[~edge].all(), "ReLU mask differs away from the edge"


def test_identity_pair_has_no_lam_term():
    shape, kind = SHAPES[4]
    inp = LR.tail_case(shape, kind)
    ident = np.arange(shape[0], dtype=np.int64)
    a, b = _step(Dev(inp, 0.1, pair=ident)), _step(Dev(inp, 0.0))
    assert a["lam"] == 0.0 and b["lam"] > 0.0
    for k in ("ce", "gw", "gb", "gin", "gs1", "gs2"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("what", ["label", "negative_label", "pair", "negative_pair", "not_a_permutation"])
def test_invalid_input_gives_nan_and_indexes_nothing(what):
    shape, kind = SHAPES[3]
    inp = LR.tail_case(shape, kind)
    label, pair = inp["label"].copy(), inp["pair"].copy()
    if what == "label":
        label[3] = shape[3]
    elif what == "negative_label":
        label[0] = -1
    elif what == "pair":
        pair[2] = shape[0]
    elif what == "negative_pair":
        pair[4] = -(2 ** 40)
    else:
        pair[:] = np.arange(shape[0])
        pair[1] = 0
    got = _step(Dev(inp, 0.1, pair=pair, label=label))
    assert np.isnan(got["ce"]) and np.isnan(got["lam"])


# ------------------------------------------------------------------------------------------------ 2. eval forward
@pytest.mark.parametrize("n", [1, 5, 128, 1500])
def test_eval_forward(n):
    """n = 1500: the eval forward has no batch limit (the step's 1024 does not apply to it)."""
    from cvhip import _lib

    shape = {1: (5, 8, 9, 3), 5: (5, 8, 9, 3), 128: (128, 128, 16, 10), 1500: (1500, 512, 4, 4)}[n]
    # (beyond the step's contract there is no step reference and no ReLU-margin rule: logits are continuous in y)
    inp = LR.make_tail(shape, "shuffle", 0) if n > 1024 else LR.tail_case(shape, "fixed" if n <= 5 else "shuffle")
    c = shape[3]
    dev = Dev(inp, 0.1, train=False)
    y = torch.from_numpy(inp["y"][:n]).cuda()
    out = Buf(np.full(n * c, np.nan))
    _lib.call("cv_lam_forward", dev.P, y.data_ptr(), ctypes.byref(dev.bn), n, out.ptr(), _lib.stream_handle())
    dev.guards(n)
    assert out.guards_intact()
    err = LR.rel_l2(out.host(), LR.tail_eval(inp, y=inp["y"][:n]))
    print(f"LAMERR eval {LR.shape_id((n,) + shape[1:])}: logits {err:.2e}")
    assert err <= BOUND
    for b in (dev.loss, dev.gw, dev.gb, dev.gin):  # (untouched)
        assert np.isnan(b.host()).all()
    assert not dev.gstat.host().any() and not _bits(dev.work.host()).any()


# ------------------------------------------------------------------------------------------------ 3. determinism
def _run(mode):
    """One launch on fresh buffers; mode 'eager' or 'graph'.  Returns every output as bits."""
    from cvhip import _lib

    shape, kind = SHAPES[4]
    dev = Dev(LR.tail_case(shape, kind), 0.1)
    args = dev.step_args()
    if mode == "graph":
        _lib.StepGraph(lambda s: _lib.call("cv_lam_step", *args, s)).replay()
    else:
        _lib.call("cv_lam_step", *args, _lib.stream_handle())
    dev.guards(mode)
    assert not dev.counters().any(), "the arrival counter did not reset"
    return [_bits(b.host()).copy() for b in dev.outputs]


def test_step_replay_bit_identical():
    a, b, g = _run("eager"), _run("eager"), _run("graph")
    for i, (x, y, z) in enumerate(zip(a, b, g)):
        assert np.array_equal(x, y), ("eager vs eager", i)
        assert np.array_equal(x, z), ("eager vs graph", i)


# ------------------------------------------------------------------------------------------------ 4. the pairing
def _draw(label, seed, offset):
    """cv_lam_pair on `label` from (seed, offset); returns (pair, the counter afterwards)."""
    from cvhip import _lib

    n = len(label)
    lab = torch.from_numpy(np.asarray(label, dtype=np.int64)).cuda()
    off = torch.tensor([offset], dtype=torch.int64, device="cuda")
    out = Buf(np.full(n, -7), np.int64)
    _lib.call("cv_lam_pair", lab.data_ptr(), n, ctypes.c_uint64(seed), off.data_ptr(), out.ptr(), _lib.stream_handle())
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.host().copy(), int(off[0])


@pytest.mark.parametrize("n,c", [(64, 4), (1, 1), (1024, 32), (37, 7)])
def test_pair_is_a_stratified_permutation(n, c):
    label = np.random.default_rng([n, c]).integers(0, c, n)
    if n == 37:
        label[::5] = -3          # (labels only compare: values outside any [0, c) index nothing)
        label[1::5] = 2 ** 40
    pair, after = _draw(label, 11, 5)
    assert after == 6
    assert sorted(pair.tolist()) == list(range(n))
    assert (label[pair] == label).all()
    again, _ = _draw(label, 11, 5)
    assert np.array_equal(pair, again)
    if n == 64:
        nxt, _ = _draw(label, 11, 6)
        other, _ = _draw(label, 12, 5)
        assert not np.array_equal(pair, nxt) and not np.array_equal(pair, other)


def test_pair_reaches_every_arrangement():
    """Labels [0, 0, 0, 1]: 200 draws show all six arrangements of the first class (missed with probability about
    6 (5/6)^200 = 9e-16)."""
    from cvhip import _lib

    lab = torch.tensor([0, 0, 0, 1], dtype=torch.int64, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((200, 4), -1, dtype=torch.int64, device="cuda")
    for k in range(200):
        _lib.call("cv_lam_pair", lab.data_ptr(), 4, ctypes.c_uint64(3), off.data_ptr(), out[k].data_ptr(),
                  _lib.stream_handle())
    torch.cuda.synchronize()
    assert int(off[0]) == 200
    draws = out.cpu().numpy()
    assert (draws[:, 3] == 3).all()
    assert len({tuple(r[:3]) for r in draws}) == 6
