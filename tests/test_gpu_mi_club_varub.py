"""CLUB and VarUB (reference mi_estimator.py:43-55, 222-224) on the HIP kernels: cv_mi_forward / cv_mi_backward
with CV_MI_CLUB / CV_MI_VARUB against the reference's formulas in fp64 on the CPU.

The fp64 references are written here (oracle/cpu_ref.py has neither estimator): the reference's literal
[N, N, d] broadcast for n <= 257, and for n = 8192 the same sum taken in blocks of rows (the literal form would
need 8192 * 8192 * 8 doubles), differentiated block by block.  Each reference is computed once and shared by the
tests below; nothing modifies it.

Shapes (n, d, hidden_size; the MLP's hidden width is hidden_size // 2), each for something specific:
  (2, 2, 4)       the minimum n, lanes beyond dy idle;
  (5, 3, 8)       odd widths, n not a multiple of the 4 rows per workgroup;
  (64, 8, 16), (16, 32, 64)   the two fixture geometries;
  (40, 64, 128)   the widest MLP (DM = 64);
  (257, 8, 16)    one row past 64 workgroups x 4 rows: the rows kernel grid-strides;
  (8192, 8, 16)   past the 128-workgroup cap of the gradient kernel; the [N, N, d] form needs gigabytes here.
y has a non-zero mean and a non-unit scale (1.5 * randn + 0.7), so a wrong moment term cannot hide.

Bars (tests/test_gpu_bigbatch.py:77-81): |value - ref| <= 1e-4 * max(|ref|, 1); rel-L2 < 1e-4 on x.grad, y.grad and
each of the eight parameter gradients.  VarUB does not depend on y: y.grad is exactly zero, and an accumulating
backward leaves dy bit-identical."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 4), (5, 3, 8), (64, 8, 16), (16, 32, 64), (40, 64, 128), (257, 8, 16), (8192, 8, 16)]
STRIDED = [(5, 3, 8), (16, 32, 64), (257, 8, 16), (8192, 8, 16)]
KINDS = ["CLUB", "VarUB"]
LITERAL_MAX = 257


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1).cpu(), torch.as_tensor(b).double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def club_literal(mu, lv, y):
    """CLUB.forward as the reference writes it (mi_estimator.py:46-55)."""
    positive = -((mu - y) ** 2) / 2.0 / lv.exp()
    negative = -((y.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0 / lv.exp()
    return (positive.sum(dim=-1) - negative.sum(dim=-1)).mean()


def club_blockwise_backward(mu, lv, y, block=16):
    """The same sum over blocks of rows; returns the value and accumulates its gradients into mu.grad, lv.grad and
    y.grad block by block (mu, lv, y: leaf tensors).  16 rows: the [block, N, d] temporaries stay in the CPU's
    cache at N = 8192 (measured several times faster than 128)."""
    n = y.shape[0]
    total = 0.0
    for r0 in range(0, n, block):
        m, l_, yy = mu[r0:r0 + block], lv[r0:r0 + block], y[r0:r0 + block]
        positive = -((m - yy) ** 2) / 2.0 / l_.exp()
        negative = -((y.unsqueeze(0) - m.unsqueeze(1)) ** 2).mean(dim=1) / 2.0 / l_.exp()
        part = (positive.sum(dim=-1) - negative.sum(dim=-1)).sum() / n
        part.backward()
        total += float(part.detach())
    return total


def varub_literal(mu, lv):
    """VarUB.forward (mi_estimator.py:222-224): the mean runs over all n * dy elements."""
    return 1.0 / 2.0 * (mu ** 2 + lv.exp() - 1.0 - lv).mean()


@functools.lru_cache(maxsize=None)
def reference(kind, n, d, hidden):
    """fp64 value and gradients (x, y, the eight parameters) on deterministic weights and inputs; the inputs are
    fp32 values, so the device sees exactly what the reference differentiates."""
    from oracle import cpu_ref as R

    g = torch.Generator().manual_seed(1000 * n + d)
    x32 = torch.randn(n, d, generator=g, dtype=torch.float32)
    y32 = 1.5 * torch.randn(n, d, generator=g, dtype=torch.float32) + 0.7
    md = R.det_mlp(d, hidden)
    M = R.to_torch({k: torch.tensor(v, dtype=torch.float32).numpy() for k, v in md.items()})
    x = x32.double().requires_grad_(True)
    y = y32.double().requires_grad_(True)
    mu, lv = R.mlp_forward(M, x)
    if kind == "VarUB":
        val = varub_literal(mu, lv)
        val.backward()
        value = float(val.detach())
    elif n <= LITERAL_MAX:
        val = club_literal(mu, lv, y)
        val.backward()
        value = float(val.detach())
    else:
        mu_l, lv_l = mu.detach().requires_grad_(True), lv.detach().requires_grad_(True)
        value = club_blockwise_backward(mu_l, lv_l, y)
        torch.autograd.backward([mu, lv], [mu_l.grad, lv_l.grad])
    gy = y.grad if y.grad is not None else torch.zeros_like(y)
    return dict(x=x32, y=y32, md=md, value=value, gx=x.grad.clone(), gy=gy.clone(),
                gp={k: v.grad.clone() for k, v in M.items()})


def _estimator(kind, d, hidden, md):
    from src.models import mi_estimator as MI

    est = getattr(MI, kind)(d, d, hidden).cuda()
    est.load_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in md.items()})
    return est


def test_blockwise_reference_is_the_literal_one():
    """The row-block form used at n = 8192, against the literal broadcast at a size both can hold."""
    g = torch.Generator().manual_seed(7)
    n, d = 257, 8
    mu, lv = torch.randn(n, d, generator=g, dtype=torch.float64), 0.5 * torch.randn(n, d, generator=g,
                                                                                       dtype=torch.float64)
    y = 1.5 * torch.randn(n, d, generator=g, dtype=torch.float64) + 0.7
    a = [t.clone().requires_grad_(True) for t in (mu, lv, y)]
    b = [t.clone().requires_grad_(True) for t in (mu, lv, y)]
    va = club_literal(*a)
    va.backward()
    vb = club_blockwise_backward(*b, block=100)
    assert abs(float(va.detach()) - vb) <= 1e-13 * max(abs(vb), 1.0)
    for p, q in zip(a, b):
        assert _rel(q.grad, p.grad) < 1e-13


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hidden", SHAPES, ids=lambda v: str(v))
def test_forward_backward_vs_fp64(kind, n, d, hidden):
    """est(x, y) and .backward() on CUDA tensors (cvhip.autograd.MIUpperBoundFn): the value, x.grad, y.grad and
    the eight parameter gradients."""
    from cvhip import rng

    ref = reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["md"])
    rng.clear_injections()
    xd, yd = ref["x"].cuda().requires_grad_(True), ref["y"].cuda().requires_grad_(True)
    mi = est(xd, yd)
    mi.backward()
    torch.cuda.synchronize()
    mi = mi.detach()
    figures = dict(value=(float(mi), ref["value"]), x=_rel(xd.grad, ref["gx"]),
                   y=(float(yd.grad.abs().max()) if kind == "VarUB" else _rel(yd.grad, ref["gy"])),
                   **{k: _rel(p.grad, ref["gp"][k]) for k, p in est.named_parameters()})
    print(kind, (n, d, hidden), figures)
    assert abs(float(mi) - ref["value"]) <= 1e-4 * max(abs(ref["value"]), 1.0), figures
    assert _rel(xd.grad, ref["gx"]) < 1e-4, figures
    if kind == "VarUB":
        assert torch.count_nonzero(yd.grad) == 0, figures
    else:
        assert _rel(yd.grad, ref["gy"]) < 1e-4, figures
    for k, p in est.named_parameters():
        assert _rel(p.grad, ref["gp"][k]) < 1e-4, (k, figures)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hidden", STRIDED, ids=lambda v: str(v))
def test_strided_inputs_and_accumulate(kind, n, d, hidden):
    """x and y as the two halves of one [n, 2d] buffer (ldx = ldy = 2d, as the fused step passes z), no
    permutation, an RNG offset that must advance by one as for L1OutUB; then cv_mi_backward with accumulate = 1
    onto pre-filled dx / dy (the two halves of one [n, 2d] buffer, gld = 2d).  The pre-fill has the gradient's
    own scale (its rms), so the fp32 addition does not mask the gradient: result - pre-fill meets the bar of
    the test above.  VarUB: dy keeps the pre-fill's bits, a negative zero included."""
    from cvhip import _lib
    from cvhip.autograd import mlp_struct

    ref = reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["md"])
    code = {"CLUB": _lib.MI_CLUB, "VarUB": _lib.MI_VARUB}[kind]
    z = torch.cat([ref["x"], ref["y"]], dim=1).cuda().contiguous()
    work = torch.zeros(int(_lib.lib().cv_mi_workspace_bytes(n)) // 4 + 16, dtype=torch.float32, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.empty((), device="cuda")
    mlp = mlp_struct(est)
    zp = z.data_ptr()
    _lib.call("cv_mi_forward", code, mlp, zp, 2 * d, zp + 4 * d, 2 * d, n, None, 99, off.data_ptr(),
              work.data_ptr(), out.data_ptr(), _lib.stream_handle())
    gx, gy = ref["gx"], ref["gy"]
    g = torch.Generator().manual_seed(n + d)
    rms = lambda t: float(t.pow(2).mean().sqrt()) or 1.0  # noqa: E731  (VarUB's dy is zero: unit pre-fill)
    pre = torch.cat([torch.randn(n, d, generator=g) * rms(gx), torch.randn(n, d, generator=g) * rms(gy)], dim=1)
    pre[0, d] = -0.0
    acc = pre.cuda().contiguous()
    ap = acc.data_ptr()
    _lib.call("cv_mi_backward", code, mlp, zp, 2 * d, zp + 4 * d, 2 * d, n, work.data_ptr(), None, 1.0, ap,
              ap + 4 * d, 2 * d, 1, None, None, None, None, 0, _lib.stream_handle())
    torch.cuda.synchronize()
    assert int(off.item()) == 1
    assert abs(float(out) - ref["value"]) <= 1e-4 * max(abs(ref["value"]), 1.0), (float(out), ref["value"])
    got = acc.cpu()
    dxg = got[:, :d].double() - pre[:, :d].double()
    print(kind, (n, d, hidden), "dx", _rel(dxg, gx))
    assert _rel(dxg, gx) < 1e-4, _rel(dxg, gx)
    assert _rel(got[:, :d], pre[:, :d].double() + gx) < 1e-4
    if kind == "VarUB":
        assert torch.equal(got[:, d:].contiguous().view(torch.int32), pre[:, d:].contiguous().view(torch.int32))
    else:
        dyg = got[:, d:].double() - pre[:, d:].double()
        print(kind, (n, d, hidden), "dy", _rel(dyg, gy))
        assert _rel(dyg, gy) < 1e-4, _rel(dyg, gy)
        assert _rel(got[:, d:], pre[:, d:].double() + gy) < 1e-4
