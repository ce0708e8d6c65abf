"""InfoNCE and CLUBMean (reference mi_estimator.py:245-273, 65-105) with backend="device": the cv_infonce_* kernels
and cv_mi_* with CV_MI_CLUBMEAN against the reference's formulas in fp64 on the CPU (tests/nce_ref.py: the literal
broadcast form for n <= 257, row blocks above; fp32 inputs widened to fp64).

Shapes (n, d, H; x_dim = y_dim = d, hidden_size = H), each for something specific:
  (2, 2, 4)       the minimum n, lanes beyond the widths idle;
  (5, 3, 8)       odd widths, n not a multiple of the 4 rows per workgroup;
  (64, 8, 16), (16, 32, 64)   the factory geometries for z_dim 16 and 64;
  (40, 64, 64)    the widest networks (every width bucket at 64);
  (257, 8, 16)    one past 64 workgroups x 4 rows (the row kernels grid-stride), one past four 64-owner groups of the
                  InfoNCE pass, 17 chunks of 16 with a 1-row tail;
  (1025, 8, 16)   one past the 1024-thread stride of the InfoNCE finalise, 30 chunks of 35 (an LDS tile of 32 plus a
                  3-row tail tile), a last owner group with one live lane.
y = 1.5 * randn + 0.7, as in tests/test_gpu_mi_club_varub.py.

Bars (tests/test_gpu_bigbatch.py:77-81): |value - ref| <= 1e-4 * max(|ref|, 1); rel-L2 < 1e-4 on x.grad, y.grad and
each parameter gradient (CLUBMean's d forward / d p_mu.2.bias is zero identically: its error is taken relative to
the positive term's gradient, tests/nce_ref.py).  One fused Adam step against torch.optim.Adam in fp64 on the fp64
gradients: per-tensor rel-L2 median < 1e-5, worst < 5e-3 (tests/test_mi_golden_club_varub.py)."""

import pytest
import torch

import nce_ref as NR

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 4), (5, 3, 8), (64, 8, 16), (16, 32, 64), (40, 64, 64), (257, 8, 16), (1025, 8, 16)]
SOME = [(5, 3, 8), (16, 32, 64), (257, 8, 16), (1025, 8, 16)]
KINDS = ["InfoNCE", "CLUBMean"]
VAL, GRAD = 1e-4, 1e-4


def _estimator(kind, d, hidden, W):
    from src.models import mi_estimator as MI

    est = getattr(MI, kind)(d, d, hidden, backend="device").cuda()
    est.load_state_dict({k: v.clone() for k, v in W.items()})
    return est


def _value_ok(got, ref):
    return abs(got - ref) <= VAL * max(abs(ref), 1.0)


def test_blockwise_references_are_the_literal_ones():
    """The row-block forms used above 257 rows, against the literal broadcasts at a size both can hold."""
    for kind in KINDS:
        W = NR.det_weights(kind, 8, 16)
        x32, y32 = NR.inputs(100, 8)
        a = NR.forward_backward(kind, W, x32, y32)
        P = {k: v.double().requires_grad_(True) for k, v in W.items()}
        x, y = x32.double().requires_grad_(True), y32.double().requires_grad_(True)
        fn = NR.infonce_blockwise_backward if kind == "InfoNCE" else NR.clubmean_blockwise_backward
        vb = fn(P, x, y, block=32)
        assert abs(a["value"] - vb) <= 1e-13 * max(abs(vb), 1.0)
        assert NR.rel(x.grad, a["gx"]) < 1e-12 and NR.rel(y.grad, a["gy"]) < 1e-12
        for k in W:
            if not (kind == "CLUBMean" and k == "p_mu.2.bias"):  # (identically zero: nce_ref.reference)
                assert NR.rel(P[k].grad, a["gp"][k]) < 1e-12, k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hidden", SHAPES, ids=lambda v: str(v))
def test_forward_backward_vs_fp64(kind, n, d, hidden):
    """est(x, y) and .backward() on CUDA tensors: the value, x.grad, y.grad and every parameter gradient."""
    ref = NR.reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["W"])
    xd, yd = ref["x"].cuda().requires_grad_(True), ref["y"].cuda().requires_grad_(True)
    mi = est(xd, yd)
    mi.backward()
    torch.cuda.synchronize()
    figures = dict(value=(float(mi), ref["value"]), x=NR.rel(xd.grad, ref["gx"]), y=NR.rel(yd.grad, ref["gy"]),
                   **{k: NR.grad_error(ref, k, p.grad) for k, p in est.named_parameters()})
    print(kind, (n, d, hidden), figures)
    assert _value_ok(float(mi), ref["value"]), figures
    assert figures["x"] < GRAD and figures["y"] < GRAD, figures
    for k, _ in est.named_parameters():
        assert figures[k] < GRAD, (k, figures)


def _device_calls(kind, est, d):
    """(forward, backward) closures over the C-ABI for z = [x | y] buffers with leading dimension 2d."""
    from cvhip import _lib
    from cvhip.autograd import critic_struct, mlp_struct

    st = _lib.stream_handle()
    if kind == "InfoNCE":
        cr = critic_struct(est, d)

        def work(n):
            return torch.zeros(int(_lib.lib().cv_infonce_workspace_bytes(n, cr.h)) // 4 + 16, device="cuda")

        def fwd(zp, n, w, out):
            _lib.call("cv_infonce_forward", cr, zp, 2 * d, zp + 4 * d, 2 * d, n, w.data_ptr(), out.data_ptr(), st)

        def bwd(zp, n, w, gmul, dxp, dyp, gld, acc, heads=None, z=None, dheads=None):
            _lib.call("cv_infonce_backward", cr, zp, 2 * d, zp + 4 * d, 2 * d, n, w.data_ptr(), None, gmul, dxp, dyp,
                      gld, acc, None, heads, z, dheads, d if dheads else 0, st)
    else:
        mlp = mlp_struct(est)
        assert not mlp.w3 and not mlp.b4

        def work(n):
            return torch.zeros(int(_lib.lib().cv_mi_workspace_bytes(n)) // 4 + 16, device="cuda")

        def fwd(zp, n, w, out):
            _lib.call("cv_mi_forward", _lib.MI_CLUBMEAN, mlp, zp, 2 * d, zp + 4 * d, 2 * d, n, None, 0, None,
                      w.data_ptr(), out.data_ptr(), st)

        def bwd(zp, n, w, gmul, dxp, dyp, gld, acc, heads=None, z=None, dheads=None):
            _lib.call("cv_mi_backward", _lib.MI_CLUBMEAN, mlp, zp, 2 * d, zp + 4 * d, 2 * d, n, w.data_ptr(), None,
                      gmul, dxp, dyp, gld, acc, None, heads, z, dheads, d if dheads else 0, st)
    return work, fwd, bwd


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hidden", SOME, ids=lambda v: str(v))
def test_strided_inputs_and_accumulate(kind, n, d, hidden):
    """x and y as the two halves of one [n, 2d] buffer (as the fused step passes z); then the backward with
    accumulate = 1 onto pre-filled dx / dy (the halves of one [n, 2d] buffer).  The pre-fill has the gradient's own
    scale (its rms), so result - pre-fill meets the bar of the test above."""
    ref = NR.reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["W"])
    work, fwd, bwd = _device_calls(kind, est, d)
    z = torch.cat([ref["x"], ref["y"]], dim=1).cuda().contiguous()
    w, out = work(n), torch.empty((), device="cuda")
    fwd(z.data_ptr(), n, w, out)
    gx, gy = ref["gx"], ref["gy"]
    g = torch.Generator().manual_seed(n + d)
    rms = lambda t: float(t.pow(2).mean().sqrt()) or 1.0  # noqa: E731
    pre = torch.cat([torch.randn(n, d, generator=g) * rms(gx), torch.randn(n, d, generator=g) * rms(gy)], dim=1)
    acc = pre.cuda().contiguous()
    bwd(z.data_ptr(), n, w, 1.0, acc.data_ptr(), acc.data_ptr() + 4 * d, 2 * d, 1)
    torch.cuda.synchronize()
    assert _value_ok(float(out), ref["value"]), (float(out), ref["value"])
    got = acc.cpu().double()
    fx, fy = NR.rel(got[:, :d] - pre[:, :d].double(), gx), NR.rel(got[:, d:] - pre[:, d:].double(), gy)
    print(kind, (n, d, hidden), "dx", fx, "dy", fy)
    assert fx < GRAD and fy < GRAD, (fx, fy)


@pytest.mark.parametrize("kind", KINDS)
def test_chain_mode_vs_autograd(kind):
    """Chain mode (the fused step's form): lambda * d(value)/d(heads) through z = mu + eps * exp(lv / 2), accumulated
    onto a pre-filled d(heads), against fp64 autograd through the same reparameterisation."""
    n, d, hidden, lam = 64, 8, 16, 0.37
    W = NR.det_weights(kind, d, hidden)
    g = torch.Generator().manual_seed(5)
    heads32 = torch.randn(n, 4 * d, generator=g) * 0.5
    eps32 = torch.randn(n, 2 * d, generator=g)
    mu32 = torch.cat([heads32[:, :d], heads32[:, 2 * d:3 * d]], dim=1)
    lv32 = torch.cat([heads32[:, d:2 * d], heads32[:, 3 * d:]], dim=1)
    z32 = mu32 + eps32 * (lv32 / 2).exp()
    # fp64: the noise that reproduces the fp32 z exactly, so both sides differentiate at the same point
    heads = heads32.double().requires_grad_(True)
    mu = torch.cat([heads[:, :d], heads[:, 2 * d:3 * d]], dim=1)
    lv = torch.cat([heads[:, d:2 * d], heads[:, 3 * d:]], dim=1)
    eps = ((z32.double() - mu) / (lv / 2).exp()).detach()
    z = mu + eps * (lv / 2).exp()
    P = {k: v.double() for k, v in W.items()}
    val = NR.infonce_literal(P, z[:, :d], z[:, d:]) if kind == "InfoNCE" else NR.clubmean_literal(
        NR.p_mu(P, z[:, :d]), z[:, d:])
    (lam * val).backward()
    est = _estimator(kind, d, hidden, W)
    work, fwd, bwd = _device_calls(kind, est, d)
    zd, hd = z32.cuda().contiguous(), heads32.cuda().contiguous()
    pre = torch.randn(n, 4 * d, generator=g) * float(heads.grad.pow(2).mean().sqrt())
    dh = pre.cuda().contiguous()
    w, out = work(n), torch.empty((), device="cuda")
    fwd(zd.data_ptr(), n, w, out)
    bwd(zd.data_ptr(), n, w, lam, None, None, 0, 1, hd.data_ptr(), zd.data_ptr(), dh.data_ptr())
    torch.cuda.synchronize()
    fig = NR.rel(dh.cpu().double() - pre.double(), heads.grad)
    print(kind, "chain", fig, float(out), float(val))
    assert _value_ok(float(out), float(val.detach()))
    assert fig < GRAD, fig


def test_infonce_large_scores():
    """Critic output layer scaled so that s_ij is of order 1e2 - 1e3: the log-sum-exp subtracts the row maximum, the
    value is finite and within the bar, softplus runs in its linear branch."""
    n, d, hidden = 64, 8, 16
    ref = NR.reference("InfoNCE", n, d, hidden, 2000.0)
    P = {k: v.double() for k, v in ref["W"].items()}
    s = NR.critic(P, torch.cat([ref["x"], ref["y"]], dim=-1).double())
    assert 1e2 <= float(s.max()) <= 5e3, float(s.max())
    est = _estimator("InfoNCE", d, hidden, ref["W"])
    out = est(ref["x"].cuda(), ref["y"].cuda())
    torch.cuda.synchronize()
    print("large scores", float(out), ref["value"], float(s.max()))
    assert torch.isfinite(out)
    assert _value_ok(float(out), ref["value"]), (float(out), ref["value"])


@pytest.mark.parametrize("kind", KINDS)
def test_forward_backward_twice_is_bit_identical(kind):
    n, d, hidden = 257, 8, 16
    ref = NR.reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["W"])
    runs = []
    for _ in range(2):
        est.zero_grad()
        xd, yd = ref["x"].cuda().requires_grad_(True), ref["y"].cuda().requires_grad_(True)
        mi = est(xd, yd)
        mi.backward()
        ll = est.learning_loss(ref["x"].cuda(), ref["y"].cuda())
        lg = torch.autograd.grad(ll, list(est.parameters()))
        torch.cuda.synchronize()
        runs.append([mi.detach(), xd.grad, yd.grad, ll.detach()] + list(lg)
                    + ([p.grad.clone() for p in est.parameters()] if kind == "InfoNCE" else []))
    # (CLUBMean's forward-parameter gradients on the autograd path are atomics, as CLUB's: not compared)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,d,hidden", SOME, ids=lambda v: str(v))
def test_learning_step_and_adam(kind, n, d, hidden):
    """learning_loss (InfoNCE: -forward; CLUBMean: -loglikeli) and its parameter gradients through autograd, then the
    same launch with the estimator's Adam step against torch.optim.Adam in fp64 on the fp64 gradients."""
    from cvhip import _lib
    from cvhip.autograd import critic_struct, est_params, mlp_grad_struct, mlp_struct
    from cvhip.engine import _AdamState
    from cvhip.plan import ParamArena

    ref = NR.reference(kind, n, d, hidden)
    est = _estimator(kind, d, hidden, ref["W"])
    xd, yd = ref["x"].cuda(), ref["y"].cuda()
    ll = est.learning_loss(xd, yd)
    ll.backward()
    torch.cuda.synchronize()
    figures = dict(loss=(float(ll), ref["loss"]),
                   **{k: NR.rel(p.grad, ref["lgp"][k]) for k, p in est.named_parameters()})
    print(kind, (n, d, hidden), figures)
    assert _value_ok(float(ll), ref["loss"]), figures
    for k, _ in est.named_parameters():
        assert figures[k] < GRAD, (k, figures)

    lr = 1e-3
    P64 = {k: v.double().requires_grad_(True) for k, v in ref["W"].items()}
    opt64 = torch.optim.Adam(list(P64.values()), lr=lr)
    for k, p in P64.items():
        p.grad = ref["lgp"][k].clone()
    opt64.step()
    est.zero_grad(set_to_none=True)
    ps = est_params(est)
    arena = ParamArena(ps, torch.device("cuda"))
    adam = _AdamState(torch.optim.Adam(est.parameters(), lr=lr), arena)
    z = torch.cat([ref["x"], ref["y"]], dim=1).cuda().contiguous()
    zp = z.data_ptr()
    loss = torch.empty((), device="cuda")
    targs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in adam.args()]
    if kind == "InfoNCE":
        cr = critic_struct(est, d)
        w = torch.zeros(int(_lib.lib().cv_infonce_workspace_bytes(n, cr.h)) // 4 + 16, device="cuda")
        G = _lib.cv_critic_grad(*[arena.gptr(p) for p in ps])
        _lib.call("cv_infonce_learning_step", cr, zp, 2 * d, zp + 4 * d, 2 * d, n, w.data_ptr(), loss.data_ptr(), G,
                  *targs, _lib.stream_handle())
    else:
        w = torch.zeros(int(_lib.lib().cv_mi_workspace_bytes(n)) // 4 + 16, device="cuda")
        G = mlp_grad_struct(est, [arena.gptr(p) for p in ps])
        _lib.call("cv_mi_learning_step", mlp_struct(est), zp, 2 * d, zp + 4 * d, 2 * d, n, w.data_ptr(),
                  loss.data_ptr(), G, *targs, _lib.stream_handle())
    torch.cuda.synchronize()
    assert _value_ok(float(loss), ref["loss"])
    assert int(adam.step[0]) == 1
    rels = sorted(NR.rel(p, P64[k]) for k, p in est.named_parameters())
    moved = min(NR.rel(p, ref["W"][k]) for k, p in est.named_parameters())
    print(kind, (n, d, hidden), "adam", rels, "moved", moved)
    assert moved > 1e-5  # (the step did move every tensor)
    assert rels[len(rels) // 2] < 1e-5 and rels[-1] < 5e-3, rels
