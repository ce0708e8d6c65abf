"""cv_eval_batch alone through the C-ABI against an fp64 torch reference on the CPU.

Synthetic y (NHWC pre-BN decoder output), x (NCHW), heads, z, labels and running statistics.  The bar for every value is
the project's LOSS_TOL (tests/test_gpu_parity.py): |value - ref| <= 1e-4 * max(|ref|, 1e-3).  The kernel evaluates each
element in fp32 (BatchNorm, sigmoid, difference, square: a few ulp, 2^-24 each, against values of order 0.1) and sums
fp32 per thread over at most a few elements before every further sum runs in fp64, so its relative error is of order
1e-6; the bar is not widened for any shape.  Appended rows, cursor and batch count are exact."""

import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
EPS = 1e-5
SHAPES = [(1, 1, 784, 1), (2, 1, 784, 8), (37, 1, 784, 8), (5, 3, 784, 3), (3, 4, 49, 64), (16, 3, 4096, 32)]


def close(v, ref):
    return abs(v - ref) <= LOSS_TOL * max(abs(ref), 1e-3)


@functools.lru_cache(maxsize=None)
def case(n, c, hw, d, seed=0):
    """Host inputs (fp32) and the fp64 reference (rec, kl_c, kl_s), computed once per shape and never written to."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + 3 * c + hw + d)
    y = torch.randn(n, hw, c, generator=g) * 1.5 + 0.3
    x = torch.rand(n, c, hw, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.2
    rmean = torch.randn(c, generator=g) * 0.3
    rvar = torch.rand(c, generator=g) + 0.4
    heads = torch.randn(n, 4 * d, generator=g) * 0.7
    z = torch.randn(n, 2 * d, generator=g)
    label = torch.randint(0, 10, (n,), generator=g, dtype=torch.int64)
    Y, X = y.double().permute(0, 2, 1), x.double()  # [n, c, hw]
    bn = (Y - rmean.double()[None, :, None]) / torch.sqrt(rvar.double() + EPS)[None, :, None]
    xh = torch.sigmoid(bn * gamma.double()[None, :, None] + beta.double()[None, :, None])
    rec = float(((xh - X) ** 2).sum() / n)
    H = heads.double()
    kl = lambda mu, lv: float(-0.5 * (1 + lv - mu ** 2 - lv.exp()).sum() / n)  # noqa: E731
    ref = (rec, kl(H[:, :d], H[:, d:2 * d]), kl(H[:, 2 * d:3 * d], H[:, 3 * d:]))
    return dict(n=n, c=c, hw=hw, d=d, y=y, x=x, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar, heads=heads, z=z,
                label=label, ref=ref)


class Sink:
    """Device accumulators of one epoch; rows: the allocated length (>= cap), filled with a canary."""

    CANARY = -777.0

    def __init__(self, cap, d, rows=None):
        from cvhip import _lib

        rows = cap if rows is None else rows
        dev = torch.device("cuda", 0)
        self.lat_c = torch.full((max(rows, 1), d), self.CANARY, dtype=torch.float32, device=dev)
        self.lat_s = torch.full((max(rows, 1), d), self.CANARY, dtype=torch.float32, device=dev)
        self.label = torch.full((max(rows, 1),), -777, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=dev)
        self.totals = torch.zeros(8, dtype=torch.float64, device=dev)
        self.c = _lib.cv_eval_sink(self.lat_c.data_ptr(), self.lat_s.data_ptr(), self.label.data_ptr(), cap,
                                   self.cursor.data_ptr(), self.totals.data_ptr())

    def state(self):
        torch.cuda.synchronize()
        return [t.cpu().clone() for t in (self.lat_c, self.lat_s, self.label, self.cursor, self.totals)]


def run(cs, sink, terms=(), scales=()):
    """One cv_eval_batch call on the case's inputs (copied to the device here)."""
    from cvhip import _lib

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    t = {k: cs[k].to(dev) for k in ("y", "x", "gamma", "beta", "rmean", "rvar", "heads", "z", "label")}
    n, c, hw, d = cs["n"], cs["c"], cs["hw"], cs["d"]
    bn = _lib.cv_bn(t["gamma"].data_ptr(), t["beta"].data_ptr(), None, None, t["rmean"].data_ptr(),
                    t["rvar"].data_ptr(), c, n * hw, 0, EPS, None, None, None)
    nb = int(L.cv_eval_workspace_bytes(n, c, hw))
    assert nb > 0 and nb % 24 == 0
    work = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=dev)  # (need not be zeroed)
    tp = (ctypes.c_void_p * 2)(*[x.data_ptr() for x in terms], *([None] * (2 - len(terms))))
    ts = (ctypes.c_float * 2)(*scales, *([0.0] * (2 - len(scales))))
    _lib.call("cv_eval_batch", ctypes.byref(bn), t["y"].data_ptr(), t["x"].data_ptr(), n, c, hw, t["heads"].data_ptr(),
              t["z"].data_ptr(), d, t["label"].data_ptr(), tp, ts, len(terms), ctypes.byref(sink.c), work.data_ptr(),
              _lib.stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n{}_c{}_hw{}_d{}".format(*s))
def test_terms_and_rows_match_the_fp64_reference(shape):
    cs = case(*shape)
    n, d = cs["n"], cs["d"]
    sink = Sink(n, d)
    run(cs, sink)
    lat_c, lat_s, label, cursor, totals = sink.state()
    for i, name in enumerate(("rec", "kl_c", "kl_s")):
        print(name, float(totals[i]), cs["ref"][i])
    for i, name in enumerate(("rec", "kl_c", "kl_s")):
        assert close(float(totals[i]), cs["ref"][i]), (name, float(totals[i]), cs["ref"][i])
    assert totals[3:7].tolist() == [0.0] * 4 and float(totals[7]) == 1.0
    assert cursor.tolist() == [n, 0]
    assert torch.equal(lat_c, cs["z"][:, :d]) and torch.equal(lat_s, cs["z"][:, d:])  # bit for bit
    assert torch.equal(label, cs["label"])


@pytest.mark.parametrize("nterm", [0, 1, 2])
def test_terms_are_scaled_and_added(nterm):
    cs = case(5, 3, 784, 3)
    dev = torch.device("cuda", 0)
    vals, scales = [3.25, 0.625][:nterm], [-1.0, 2.5][:nterm]
    terms = [torch.tensor([v], dtype=torch.float32, device=dev) for v in vals]
    sink = Sink(16, 3)
    run(cs, sink, terms, scales)
    run(cs, sink, terms, scales)
    totals = sink.state()[4]
    want = [2 * s * v for s, v in zip(scales, vals)] + [0.0] * (2 - nterm)
    assert totals[3:5].tolist() == want  # (exact in fp64: small dyadic values)
    assert totals[5:7].tolist() == [0.0, 0.0] and float(totals[7]) == 2.0


def test_a_nan_term_poisons_only_its_total():
    cs = case(5, 3, 784, 3)
    dev = torch.device("cuda", 0)
    terms = [torch.tensor([float("nan")], dtype=torch.float32, device=dev),
             torch.tensor([1.5], dtype=torch.float32, device=dev)]
    sink = Sink(8, 3)
    run(cs, sink, terms, [1.0, -1.0])
    totals = sink.state()[4]
    assert math.isnan(float(totals[3]))
    assert float(totals[4]) == -1.5 and float(totals[7]) == 1.0
    for i in range(3):
        assert close(float(totals[i]), cs["ref"][i])


THREE = [(5, 1, 784, 8), (7, 1, 784, 8), (2, 1, 784, 8)]


def test_three_calls_append_in_order_and_sum():
    cases3 = [case(*s, seed=k + 1) for k, s in enumerate(THREE)]
    sink = Sink(16, 8)
    for cs in cases3:
        run(cs, sink)
    lat_c, lat_s, label, cursor, totals = sink.state()
    assert cursor.tolist() == [14, 0] and float(totals[7]) == 3.0
    zc = torch.cat([cs["z"][:, :8] for cs in cases3])
    zs = torch.cat([cs["z"][:, 8:] for cs in cases3])
    lab = torch.cat([cs["label"] for cs in cases3])
    assert torch.equal(lat_c[:14], zc) and torch.equal(lat_s[:14], zs) and torch.equal(label[:14], lab)
    assert (lat_c[14:] == Sink.CANARY).all() and (label[14:] == -777).all()
    for i, name in enumerate(("rec", "kl_c", "kl_s")):
        ref = sum(cs["ref"][i] for cs in cases3)  # the fp64 sum of the three per-call references
        print(name, float(totals[i]), ref)
        assert close(float(totals[i]), ref), (name, float(totals[i]), ref)


def test_overflow_guard_appends_nothing_and_sticks():
    cases3 = [case(*s, seed=k + 1) for k, s in enumerate(THREE)]
    sink = Sink(10, 8, rows=16)
    run(cases3[0], sink)
    first = sink.state()
    assert first[3].tolist() == [5, 0]
    run(cases3[1], sink)  # rows 5..11 do not fit under cap = 10
    second = sink.state()
    assert second[3].tolist() == [5, 1]
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(a, b)
    assert torch.equal(first[4], second[4])
    assert (second[0][5:] == Sink.CANARY).all() and (second[1][5:] == Sink.CANARY).all()
    assert (second[2][5:] == -777).all()
    run(cases3[2], sink)  # would fit (5 + 2 <= 10), but the flag is sticky
    third = sink.state()
    for a, b in zip(second, third):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(37, 1, 784, 8), (16, 3, 4096, 32)], ids=lambda s: "n{}_c{}_hw{}_d{}".format(*s))
def test_two_runs_give_equal_bits(shape):
    cs = case(*shape)
    dev = torch.device("cuda", 0)
    term = [torch.tensor([0.3], dtype=torch.float32, device=dev)]
    states = []
    for _ in range(2):
        sink = Sink(cs["n"], cs["d"])
        run(cs, sink, term, [-2.0])
        states.append(sink.state())
    for a, b in zip(*states):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b)
