"""The small module-path kernels of csrc/cv_latent.hip (cv_kl, cv_mse_sum, cv_sample_forward, cv_sample_backward:
the device side of VaeLossFn and SampleFn) called directly, at the sizes where their launch arithmetic has an edge,
against fp64 restatements (oracle/cpu_ref.py vae_loss, sample).

Inputs: mu ~ N(0,1), logvar = 0.3 N(0,1), images uniform in [0,1), all rounded to fp32 before either side sees them.

Bars.  cv_kl: value 1e-6 relative (the kernel sums fp32 terms in fp64), gradients 1e-5 rel-L2.  cv_mse_sum: every
term (xhat - x)^2 is two fp32 roundings of a positive number (<= 1.8e-7 relative), the sum is fp64 and the result is
rounded once more: <= 2.4e-7, bar 1e-6; the gradient g (xhat - x) with g = gscale * 2 / n is four roundings per
element, <= 2.4e-7, bar 1e-6 rel-L2.  cv_sample_forward: z = mu + eps exp(logvar / 2) is an expf (2 ulp) and three
roundings, <= 3e-7 (|mu| + |eps| sd) per element, bar 1e-6 of that scale per element and 1e-6 rel-L2.
cv_sample_backward: d mu = dz exactly; d logvar = dz (z - mu) / 2 inherits the rounding of the stored z,
<= 6e-7 in the worst case, bar 1e-5 rel-L2 (the bar of the KL gradients).

Accumulating calls are checked on the added part (after - before in fp64); the pre-filled values have the scale of
the gradient they receive, so the fp32 rounding of the sum (6e-8 of the larger operand) stays below the bars."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1).cpu(), torch.as_tensor(b).double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    from cvhip import _lib

    return _lib.stream_handle()


# ----------------------------------------------------------------------------- cv_kl


def _kl_ref(mu, lv, gscale):
    from oracle import cpu_ref as R

    m, l_ = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    z = torch.zeros(1, 1, dtype=torch.float64)
    _, kl, _ = R.vae_loss(z, z, m, m, l_, l_)
    (gscale * kl).backward()
    return float(kl.detach()), m.grad, l_.grad


@pytest.mark.parametrize("n,d", [(1, 3), (37, 5), (300, 32)])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_kl(n, d, strided, accumulate):
    """One 1024-thread workgroup over n * d elements (3, 185, 9600: below one pass, and more than nine) with e / d,
    e % d indexing; contiguous rows or the heads layout (ld = 4d); gradients into rows of another pitch (gld = 2d + 3:
    the columns between them stay untouched); accumulate and gscale."""
    from cvhip import _lib

    g = torch.Generator().manual_seed(1000 * n + 10 * d + 2 * strided + accumulate)
    ld = 4 * d if strided else d
    heads = torch.randn(n, 4 * d, generator=g)
    heads[:, d:2 * d] *= 0.3
    hd = heads.to(DEV)
    if strided:
        mu_d, lv_d = hd[:, :d], hd[:, d:2 * d]
    else:
        mu_d, lv_d = hd[:, :d].contiguous(), hd[:, d:2 * d].contiguous()
    gscale = 0.6 if accumulate else 1.0
    kl_ref, gm_ref, gl_ref = _kl_ref(heads[:, :d], heads[:, d:2 * d], gscale)
    gld = 2 * d + 3
    before = torch.randn(n, gld, generator=g) / n
    gbuf = before.to(DEV)
    gsc = torch.tensor([gscale], dtype=torch.float32, device=DEV) if accumulate else None
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("cv_kl", _p(mu_d), _p(lv_d), ld, n, d, _p(out), _p(gsc), _p(gbuf[:, :d]), _p(gbuf[:, d:]), gld,
              accumulate, _stream())
    torch.cuda.synchronize()
    after = gbuf.cpu()
    e_val = abs(float(out) - kl_ref) / abs(kl_ref)
    base = before.double() if accumulate else torch.zeros(n, gld, dtype=torch.float64)
    added = after.double() - base
    e_mu, e_lv = _rel(added[:, :d], gm_ref), _rel(added[:, d:2 * d], gl_ref)
    print(f"KL n={n} d={d} ld={ld} acc={accumulate} kl={float(out):.7g} ref={kl_ref:.7g} e_val={e_val:.3g} "
          f"e_dmu={e_mu:.3g} e_dlv={e_lv:.3g}")
    assert e_val <= 1e-6, e_val
    assert e_mu <= 1e-5 and e_lv <= 1e-5, (e_mu, e_lv)
    assert torch.equal(after[:, 2 * d:].view(torch.int32), before[:, 2 * d:].view(torch.int32))
    # value only (no gradient pointers) and gradients only (no value pointer)
    out2 = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("cv_kl", _p(mu_d), _p(lv_d), ld, n, d, _p(out2), None, None, None, 0, 0, _stream())
    g2 = before.to(DEV)
    _lib.call("cv_kl", _p(mu_d), _p(lv_d), ld, n, d, None, _p(gsc), _p(g2[:, :d]), _p(g2[:, d:]), gld, accumulate,
              _stream())
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu().view(torch.int32), out.cpu().view(torch.int32))
    assert torch.equal(g2.cpu().view(torch.int32), after.view(torch.int32))


# ----------------------------------------------------------------------------- cv_mse_sum


@pytest.mark.parametrize("n,per", [(3, 7), (9, 784), (43, 12288)])
@pytest.mark.parametrize("with_gscale", [False, True])
def test_mse_sum(n, per, with_gscale):
    """n * per_sample = 21 (below one block), 7056 (not a multiple of 1024) and 528384 (above the 512 x 1024 grid:
    the grid-stride loop runs); forward only, backward only and both in one call; gscale NULL and not."""
    from cvhip import _lib
    from oracle import cpu_ref as R

    g = torch.Generator().manual_seed(n * per + with_gscale)
    xh, x = torch.rand(n, per, generator=g), torch.rand(n, per, generator=g)
    gs = 0.35 if with_gscale else 1.0
    xh64 = xh.double().requires_grad_(True)
    zero = torch.zeros(n, 1, dtype=torch.float64)
    rec_ref = R.vae_loss(xh64, x.double(), zero, zero, zero, zero)[0]
    (gs * rec_ref).backward()
    rec_ref = float(rec_ref.detach())
    xd, xx = xh.to(DEV), x.to(DEV)
    gsc = torch.tensor([gs], dtype=torch.float32, device=DEV) if with_gscale else None
    res = {}
    for mode in ("fwd", "bwd", "both"):
        rec = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV) if mode != "bwd" else None
        dx = torch.full((n, per), float("nan"), dtype=torch.float32, device=DEV) if mode != "fwd" else None
        work = torch.zeros(1, dtype=torch.float64, device=DEV) if rec is not None else None
        _lib.call("cv_mse_sum", _p(xd), _p(xx), n, per, _p(rec), _p(gsc), _p(dx), _p(work), _stream())
        torch.cuda.synchronize()
        res[mode] = (None if rec is None else float(rec), None if dx is None else dx.cpu())
    for mode in ("fwd", "both"):
        e = abs(res[mode][0] - rec_ref) / rec_ref
        print(f"MSE n={n} per={per} {mode} rec={res[mode][0]:.7g} ref={rec_ref:.7g} e={e:.3g}")
        assert e <= 1e-6, (mode, e)
    for mode in ("bwd", "both"):
        e = _rel(res[mode][1], xh64.grad)
        print(f"MSE n={n} per={per} {mode} e_dxhat={e:.3g}")
        assert e <= 1e-6, (mode, e)
    assert torch.equal(res["bwd"][1].view(torch.int32), res["both"][1].view(torch.int32))


def test_vae_loss_twice():
    """cv_mse_sum adds into an fp64 work word that the caller zeroes: VaeLossFn (src.losses.vae_loss) allocates a
    zeroed word per call, so two calls give the same values, and they are the oracle's (values and gradients)."""
    from oracle import cpu_ref as R
    from src.losses import vae_loss

    n, d = 9, 5
    g = torch.Generator().manual_seed(11)
    xh, x = torch.rand(n, 1, 28, 28, generator=g), torch.rand(n, 1, 28, 28, generator=g)
    heads = torch.randn(n, 4 * d, generator=g)
    heads[:, d:2 * d] *= 0.3
    heads[:, 3 * d:] *= 0.3
    h64 = heads.double().requires_grad_(True)
    xh64 = xh.double().requires_grad_(True)
    ref = R.vae_loss(xh64, x.double(), h64[:, :d], h64[:, 2 * d:3 * d], h64[:, d:2 * d], h64[:, 3 * d:])
    (ref[0] + 0.5 * ref[1] + 0.25 * ref[2]).backward()
    hd = heads.to(DEV).requires_grad_(True)
    xd = xh.to(DEV).requires_grad_(True)
    outs = []
    for _ in range(2):
        o = vae_loss(xd, x.to(DEV), hd[:, :d], hd[:, 2 * d:3 * d], hd[:, d:2 * d], hd[:, 3 * d:])
        outs.append([float(v.detach()) for v in o])
    (o[0] + 0.5 * o[1] + 0.25 * o[2]).backward()
    torch.cuda.synchronize()
    for vals in outs:
        for v, r in zip(vals, ref):
            assert abs(v - float(r)) <= 1e-6 * abs(float(r)), (vals, [float(r) for r in ref])
    assert _rel(xd.grad, xh64.grad) <= 1e-6
    assert _rel(hd.grad, h64.grad) <= 1e-5


# ----------------------------------------------------------------------------- cv_sample_forward / cv_sample_backward

SAMPLE_SHAPES = [(7, 5), (1, 1), (1, 600001)]  # numel 35 (odd), 1, and 600001 (odd, above the 1024-block grid)


@pytest.mark.parametrize("shape", SAMPLE_SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sample_injected(shape, accumulate):
    """One thread serves two elements: odd sizes end on a half pair.  With injected eps, z against fp64; the backward
    with and without accumulation."""
    from cvhip import _lib
    from oracle import cpu_ref as R

    numel = shape[0] * shape[1]
    g = torch.Generator().manual_seed(numel + accumulate)
    mu, eps, dz = (torch.randn(shape, generator=g) for _ in range(3))
    lv = 0.3 * torch.randn(shape, generator=g)
    m64, l64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    z_ref = R.sample(m64, l64, eps.double())
    z_ref.backward(dz.double())
    mu_d, lv_d, eps_d, dz_d = (t.to(DEV) for t in (mu, lv, eps, dz))
    z = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.call("cv_sample_forward", _p(mu_d), _p(lv_d), numel, _p(eps_d), 1234, _p(off), _p(z), _stream())
    bm, bl = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    dmu, dlv = bm.to(DEV), bl.to(DEV)
    _lib.call("cv_sample_backward", _p(mu_d), _p(z), _p(dz_d), numel, _p(dmu), _p(dlv), accumulate, _stream())
    torch.cuda.synchronize()
    zc = z.cpu().double()
    scale = mu.double().abs() + eps.double().abs() * torch.exp(0.5 * lv.double())
    e_el = float(((zc - z_ref.detach()).abs() / scale).max())
    e_z = _rel(zc, z_ref.detach())
    base_m = bm.double() if accumulate else torch.zeros(shape, dtype=torch.float64)
    base_l = bl.double() if accumulate else torch.zeros(shape, dtype=torch.float64)
    e_mu, e_lv = _rel(dmu.cpu().double() - base_m, m64.grad), _rel(dlv.cpu().double() - base_l, l64.grad)
    print(f"SAMPLE numel={numel} acc={accumulate} e_z={e_z:.3g} e_z_el={e_el:.3g} e_dmu={e_mu:.3g} e_dlv={e_lv:.3g}")
    assert e_z <= 1e-6 and e_el <= 1e-6, (e_z, e_el)
    if not accumulate:
        assert torch.equal(dmu.cpu().view(torch.int32), dz.view(torch.int32))
    assert e_mu <= 1e-6, e_mu
    assert e_lv <= 1e-5, e_lv


@pytest.mark.parametrize("shape", SAMPLE_SHAPES)
def test_sample_device_noise(shape):
    """Without injected noise the kernel draws from (seed, offset[0], pair index): offset[0] moves by exactly one per
    call and the arrival count offset[1] returns to zero, at every grid size; consecutive calls draw different noise
    and the same (seed, offset) draws the same; every element is written."""
    from cvhip import _lib

    numel = shape[0] * shape[1]
    mu = torch.zeros(shape, dtype=torch.float32, device=DEV)
    lv = torch.zeros(shape, dtype=torch.float32, device=DEV)  # (z = eps)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    draws = []
    for call in range(3):
        z = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("cv_sample_forward", _p(mu), _p(lv), numel, None, 1234, _p(off), _p(z), _stream())
        torch.cuda.synchronize()
        assert off.cpu().tolist() == [call + 1, 0]
        draws.append(z.cpu())
        assert bool(torch.isfinite(draws[-1]).all())
    for a, b in zip(draws, draws[1:]):
        assert not torch.equal(a, b)
    off.zero_()
    z = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("cv_sample_forward", _p(mu), _p(lv), numel, None, 1234, _p(off), _p(z), _stream())
    torch.cuda.synchronize()
    assert torch.equal(z.cpu().view(torch.int32), draws[0].view(torch.int32))
    if numel > 100000:  # (standard normal draws: the standard error of the mean is 1.3e-3 at this size)
        assert abs(float(draws[0].mean())) < 0.01 and abs(float(draws[0].std()) - 1.0) < 0.01
