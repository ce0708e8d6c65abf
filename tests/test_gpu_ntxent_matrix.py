"""Every NT-Xent kernel family of cv_ntxent (csrc/cv_latent.hip, csrc/cv_ntxent.hpp) against the fp64 oracle
(oracle/cpu_ref.py contrastive_loss / contrastive_loss_blockwise, themselves pinned to the reference by
tests/test_oracle_golden.py), with the launched kernels read back from the launch log for every case.

Families (the rows launch and the gradient launch choose separately: ntl_bytes differs with `grad`):
  reg   ntxent_*_reg_kernel<8,8> / <32,4>   cosine, d % 4 == 0, 16-byte rows, n <= 512 & d <= 8 or n <= 256 & d <= 32
  lds   ntxent_*_lds_kernel<8|16|32|64>     ntl_bytes(n, d, need_lv, grad) <= 144 KiB (float4 or scalar staging)
  walk  ntxent_*_kernel<DM,false>           the LDS does not fit, n <= 4096
  walk  ntxent_*_kernel<DM,true>  (BIG)     n > 4096

Inputs: mu ~ N(0,1), logvar = 0.3 N(0,1) from a seeded generator, labels uniform in 0..9, tau = 0.1 unless a case
says otherwise; the same values go to the device (rounded to fp32) and to the oracle (fp64 on the CPU).

Bars (the project's parity bars, tests/test_gpu_bigbatch.py): loss within 1e-4 * max(|ref|, 1e-3), each gradient
tensor within 1e-4 rel-L2.  The oracle evaluated in fp32 differs from fp64 by at most 1.6e-7 (loss) and 5.5e-6 (a
gradient tensor) at (70,10) and (288,64), so a correct fp32 kernel has more than an order of magnitude of room.
No bar is raised.  The row log-sum-exps read back by the C-ABI tests are held to 1e-5 * max(|ref|, 1): they are
sums of at most n terms of S / tau with |S / tau| up to a few hundred, a few fp32 ulps (6e-8 relative) each.

Two shapes differ from the first plan because ntl_bytes puts the planned ones elsewhere: mahalanobis d = 8 has
84 n bytes of rows-launch LDS, so both launches walk global memory only from n = 1756 (1758 here, not 1540);
cosine d = 6 has 40 n, so from n = 3687 (3690 here, not 2840).

The module path (src.losses.contrastive_loss -> ContrastiveFn) issues three launches: rows, the loss-only
gradient launch of the forward, and the gradient launch of the backward.  The launch log is per thread, so the
backward runs on the calling thread here (torch.autograd.set_multithreading_enabled(False))."""

import ctypes
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

SIMS = ("cosine", "l2", "modified_l2", "jeffrey", "mahalanobis")
USES_LV = ("modified_l2", "jeffrey", "mahalanobis")
LDS_LIMIT = 144 * 1024


# ----------------------------------------------------------------------------- helpers


def _ntl_bytes(n, d, need_lv, grad):
    """cv_ntxent.hpp ntl_bytes."""
    return n * 8 + n * (d + 1) * 4 * (2 if need_lv else 1) + n * 4 * (4 if grad else 1)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1).cpu(), torch.as_tensor(b).double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _inputs(n, d, seed, classes=10):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, d, generator=g, dtype=torch.float64)
    lv = 0.3 * torch.randn(n, d, generator=g, dtype=torch.float64)
    label = torch.randint(0, classes, (n,), generator=g)
    # the device sees fp32: the oracle starts from the same rounded values
    return mu.float().double(), lv.float().double(), label


def _oracle(mu, lv, label, sim, tau, ps, blockwise=False):
    """(loss, d mu, d logvar or None) in fp64."""
    from oracle import cpu_ref as R

    m64, l64 = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    if blockwise:
        loss = R.contrastive_loss_blockwise(m64, l64, label, sim, tau, ps)
    else:
        loss = R.contrastive_loss(m64, l64, label, sim, tau, ps)
        if torch.isfinite(loss):
            loss.backward()
    gm = m64.grad if m64.grad is not None else torch.zeros_like(mu)
    gl = l64.grad if sim in USES_LV else None
    return float(loss.detach()), gm, gl


def _oracle_rows(mu, lv, label, sim, tau, ps):
    """(lse_all, lse_pos, row losses) of the oracle, fp64."""
    from oracle import cpu_ref as R

    with torch.no_grad():
        n = mu.shape[0]
        s = R.pairwise(sim, mu, lv).masked_fill(torch.eye(n, dtype=torch.bool), float("-inf"))
        pair = (label[None, :] != label[:, None]) if ps else (label[None, :] == label[:, None])
        la = R.logsumexp(s / tau, dim=1)
        lp = R.logsumexp(s.masked_fill(~pair, float("-inf")) / tau, dim=1)
    return la, lp, la - lp


class _KernelLog:
    """The kernels the enclosed calls launched from this thread (cv_debug_kernel_log / cv_debug_kernel_names)."""

    def __enter__(self):
        from cvhip import _lib

        self.L = _lib.lib()
        self.names = []
        self.prev = self.L.cv_debug_kernel_log(1)
        return self

    def __exit__(self, *exc):
        try:
            buf = ctypes.create_string_buffer(1 << 16)
            k = self.L.cv_debug_kernel_names(buf, len(buf))
            self.names = buf.value.decode().split("\n") if k else []
        finally:
            self.L.cv_debug_kernel_log(self.prev)
        return False


_KERNEL = re.compile(r"ntxent_(rows|grad)(?:_(lds|reg))?_kernel<([^>]*)>")


def _launches(names):
    """[(phase, family, template args)] of the NT-Xent launches in a log: ("rows", "lds", (16,)),
    ("grad", "walk", (64, False)), ("rows", "reg", (32, 4)) ..."""
    out = []
    for nm in names:
        m = _KERNEL.search(nm)
        if not m:
            continue
        args = tuple({"true": True, "false": False}.get(a.strip(), a.strip()) for a in m.group(3).split(","))
        args = tuple(a if isinstance(a, bool) else int(a) for a in args)
        out.append((m.group(1), m.group(2) or "walk", args))
    return out


def _dm(d):
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def _family(n, d, sim, grad, reg):
    """The family ntxent_launch picks for this launch, restated from cv_latent.hip for the cross-check below (the
    tests state their expectation explicitly; this only says whether a stated shape is where ntl_bytes puts it)."""
    if _ntl_bytes(n, d, sim in USES_LV, grad) <= LDS_LIMIT:
        if reg:
            return ("reg", (8, 8) if d <= 8 else (32, 4))
        return ("lds", (_dm(d),))
    return ("walk", (_dm(d), n > 4096))


def _assert_path(names, rows, grad, n_grad):
    """The log holds one rows launch of family `rows` followed by n_grad gradient launches of family `grad`."""
    got = _launches(names)
    want = [("rows",) + rows] + [("grad",) + grad] * n_grad
    assert got == want, (got, want, names)


def _device_module(mu, lv, label, sim, tau, ps):
    from src.losses import contrastive_loss

    m = mu.float().cuda().requires_grad_(True)
    l_ = lv.float().cuda().requires_grad_(True)
    lab = label.cuda()
    with _KernelLog() as log, torch.autograd.set_multithreading_enabled(False):
        loss = contrastive_loss(m, l_, lab, sim, tau, ps=ps)
        loss.backward()
        torch.cuda.synchronize()
    return float(loss.detach()), m.grad.cpu(), (l_.grad.cpu() if sim in USES_LV else None), log.names


def _check(tag, dev, ref, sim):
    (loss, gm, gl), (rloss, rgm, rgl) = dev, ref
    e_loss = abs(loss - rloss) / max(abs(rloss), 1e-3)
    e_mu = _rel(gm, rgm)
    e_lv = _rel(gl, rgl) if sim in USES_LV else 0.0
    print(f"NTX {tag} loss={loss:.7g} ref={rloss:.7g} e_loss={e_loss:.3g} e_dmu={e_mu:.3g} e_dlv={e_lv:.3g}")
    assert abs(loss - rloss) <= 1e-4 * max(abs(rloss), 1e-3), (tag, loss, rloss)
    assert e_mu < 1e-4, (tag, "dmu", e_mu)
    if sim in USES_LV:
        assert e_lv < 1e-4, (tag, "dlogvar", e_lv)


def _module_case(tag, mu, lv, label, sim, tau, ps, rows, grad, blockwise=False):
    loss, gm, gl, names = _device_module(mu, lv, label, sim, tau, ps)
    _assert_path(names, rows, grad, 2)
    _check(tag, (loss, gm, gl), _oracle(mu, lv, label, sim, tau, ps, blockwise), sim)


def _seed(n, d, sim, ps, salt=0):
    return 100003 * n + 101 * d + 10 * SIMS.index(sim) + int(ps) + 7919 * salt


# ----------------------------------------------------------------------------- a. module path

LDS_SHAPES = [(70, 5), (70, 10), (37, 20), (130, 64)]  # DM = 8 / 16 (scalar staging), 32, 64; n % 4 != 0


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("n,d", LDS_SHAPES)
def test_module_lds(n, d, sim, ps):
    """The LDS family at every DM; cosine at (37, 20) has 16-byte rows and d % 4 == 0: the <32,4> register variant."""
    fam = ("reg", (32, 4)) if (sim == "cosine" and (n, d) == (37, 20)) else ("lds", (_dm(d),))
    assert _family(n, d, sim, False, fam[0] == "reg") == fam and _family(n, d, sim, True, fam[0] == "reg") == fam
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps))
    _module_case(f"{fam[0]}{fam[1]} n={n} d={d} {sim} ps={int(ps)}", mu, lv, label, sim, 0.1, ps, fam, fam)


WALK_CASES = ([(288, 64, s, ps) for s in ("jeffrey", "mahalanobis", "modified_l2") for ps in (False, True)]
              + [(544, 64, s, ps) for s in ("cosine", "l2") for ps in (False, True)]
              + [(1758, 8, "mahalanobis", ps) for ps in (False, True)]
              + [(3690, 6, "cosine", ps) for ps in (False, True)])


@pytest.mark.parametrize("n,d,sim,ps", WALK_CASES)
def test_module_global_walk(n, d, sim, ps):
    """Neither launch fits the LDS and n <= 4096: ntxent_rows_kernel / ntxent_grad_kernel<DM,false>; d = 6: the
    k < d guards of the DM = 8 template and scalar row loads."""
    fam = ("walk", (_dm(d), False))
    assert _family(n, d, sim, False, False) == fam and _family(n, d, sim, True, False) == fam
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps))
    _module_case(f"walk{fam[1]} n={n} d={d} {sim} ps={int(ps)}", mu, lv, label, sim, 0.1, ps, fam, fam,
                 blockwise=n > 1000)


@pytest.mark.parametrize("n,d,sim,ps", [(274, 64, "jeffrey", False), (274, 64, "jeffrey", True),
                                        (528, 64, "cosine", False), (528, 64, "cosine", True)])
def test_module_mixed(n, d, sim, ps):
    """The rows launch fits the LDS (532 n / 272 n bytes), the gradient launch (544 n / 284 n) does not: the
    log-sum-exps of an LDS rows kernel feed a global-walk gradient kernel."""
    rows, grad = ("lds", (64,)), ("walk", (64, False))
    assert _family(n, d, sim, False, False) == rows and _family(n, d, sim, True, False) == grad
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps))
    _module_case(f"mixed n={n} d={d} {sim} ps={int(ps)}", mu, lv, label, sim, 0.1, ps, rows, grad)


@pytest.mark.parametrize("n,d,sim,ps", [(4100, 10, "mahalanobis", False), (4100, 20, "modified_l2", True)])
def test_module_big(n, d, sim, ps):
    """n > 4096: the BIG kernels (<16,true>, <32,true>), which re-count the finite rows per block; one singleton label
    makes that count n - 1 under ps = False."""
    fam = ("walk", (_dm(d), True))
    assert _family(n, d, sim, False, False) == fam and _family(n, d, sim, True, False) == fam
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps))
    label[n // 3] = 77
    if not ps:
        assert int(torch.isfinite(_oracle_rows_blockwise(mu, lv, label, sim, 0.1, ps)).sum()) == n - 1
    _module_case(f"big{fam[1]} n={n} d={d} {sim} ps={int(ps)}", mu, lv, label, sim, 0.1, ps, fam, fam, blockwise=True)


def _oracle_rows_blockwise(mu, lv, label, sim, tau, ps, block=128):
    from oracle import cpu_ref as R

    n = mu.shape[0]
    with torch.no_grad():
        return torch.cat([R.contrastive_rows(mu, lv, label, sim, tau, ps, torch.arange(i, min(n, i + block)))
                          for i in range(0, n, block)])


# ----------------------------------------------------------------------------- b. C-ABI path


def _branch(mu, lv, ld, ps, dmu, dlv, gld, gscale, gmul, loss, lse):
    from cvhip import _lib

    def p(t):
        return t.data_ptr() if t is not None else None

    return _lib.cv_ntxent_branch(p(mu), p(lv), ld, int(ps), p(dmu), p(dlv), gld, p(gscale), gmul, p(loss), p(lse))


def _call(branches, label, n, d, sim, tau, phases, accumulate):
    from cvhip import _lib

    arr = (_lib.cv_ntxent_branch * len(branches))(*branches)
    with _KernelLog() as log:
        for ph in phases:
            _lib.call("cv_ntxent", arr, len(branches), label.data_ptr(), n, d, _lib.SIM[sim], tau, ph, accumulate,
                      _lib.stream_handle())
        torch.cuda.synchronize()
    return log.names


def _heads_case(sim, seed):
    """A heads block [n][4d] = (mu_c, lv_c, mu_s, lv_s), a pre-filled d(heads) and labels, n = 70, d = 8."""
    n, d = 70, 8
    g = torch.Generator().manual_seed(seed)
    heads = torch.randn(n, 4 * d, generator=g, dtype=torch.float64)
    heads[:, d:2 * d] *= 0.3
    heads[:, 3 * d:] *= 0.3
    heads = heads.float()
    label = torch.randint(0, 10, (n,), generator=g)
    before = torch.randn(n, 4 * d, generator=g, dtype=torch.float64).float()
    return n, d, heads, label, before


def _run_heads(sim, heads, label, before, n, d, phases):
    dev = torch.device("cuda")
    h = heads.to(dev)
    dh = before.to(dev).clone()
    lab = label.to(dev)
    gsc = torch.tensor([0.75], dtype=torch.float32, device=dev)
    lse = torch.full((2, 2 * n), 7.0, dtype=torch.float32, device=dev)
    loss = torch.zeros(2, dtype=torch.float32, device=dev)
    br = [_branch(h[:, 2 * b * d:], h[:, (2 * b + 1) * d:], 4 * d, b, dh[:, 2 * b * d:], dh[:, (2 * b + 1) * d:], 4 * d,
                  gsc, 1.25, loss[b:], lse[b]) for b in (0, 1)]
    names = _call(br, lab, n, d, sim, 0.1, phases, 1)
    return lse.cpu(), loss.cpu(), dh.cpu(), names


@pytest.mark.parametrize("sim", ["jeffrey", "modified_l2"])
def test_abi_two_branches_accumulate(sim):
    """Two branches in one call over a heads block (ld = gld = 4d; branch 0 = columns 0..2d with ps = 0, branch 1 =
    2d..4d with ps = 1), accumulate = 1 onto a random d(heads), gmul = 1.25, gscale = 0.75: d(heads) = before +
    1.25 * 0.75 * the oracle's gradient (the added part held to 1e-4 rel-L2), both losses and all four log-sum-exp
    rows; the same call as phase 0 then phase 1 equals phase 2 bit for bit."""
    n, d, heads, label, before = _heads_case(sim, 4242 + SIMS.index(sim))
    lse, loss, dh, names = _run_heads(sim, heads, label, before, n, d, (2,))
    _assert_path(names, ("lds", (8,)), ("lds", (8,)), 1)
    h64 = heads.double()
    for b in (0, 1):
        mu, lv = h64[:, 2 * b * d:(2 * b + 1) * d].contiguous(), h64[:, (2 * b + 1) * d:(2 * b + 2) * d].contiguous()
        rloss, rgm, rgl = _oracle(mu, lv, label, sim, 0.1, bool(b))
        added = dh.double() - before.double()
        gm, gl = added[:, 2 * b * d:(2 * b + 1) * d], added[:, (2 * b + 1) * d:(2 * b + 2) * d]
        _check(f"abi2 {sim} branch={b}", (float(loss[b]), gm, gl), (rloss, 1.25 * 0.75 * rgm, 1.25 * 0.75 * rgl), sim)
        la, lp, _ = _oracle_rows(mu, lv, label, sim, 0.1, bool(b))
        for got, ref, nm in ((lse[b, :n].double(), la, "lse_all"), (lse[b, n:].double(), lp, "lse_pos")):
            fin = torch.isfinite(ref)
            assert torch.equal(got[~fin], ref[~fin]), (b, nm)
            err = ((got[fin] - ref[fin]).abs() / ref[fin].abs().clamp_min(1.0)).max()
            print(f"NTX abi2 {sim} branch={b} {nm} err={float(err):.3g}")
            assert err <= 1e-5, (b, nm, float(err))
    lse2, loss2, dh2, names2 = _run_heads(sim, heads, label, before, n, d, (0, 1))
    _assert_path(names2, ("lds", (8,)), ("lds", (8,)), 1)
    for x, y, nm in ((lse, lse2, "lse"), (loss, loss2, "loss"), (dh, dh2, "dheads")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), nm


@pytest.mark.parametrize("sim", ["cosine", "mahalanobis"])
@pytest.mark.parametrize("ps", [False, True])
def test_abi_unaligned_rows(sim, ps):
    """Rows that start one float past a 16-byte boundary with ld = 4d + 1: the scalar staging path with a stride;
    cosine must not take the register variant (it needs 16-byte rows)."""
    n, d = 70, 8
    ld = 4 * d + 1
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps, salt=1))
    dev = torch.device("cuda")
    buf = torch.full((1 + n * ld + 3,), float("nan"), dtype=torch.float32, device=dev)
    rows = buf[1:1 + n * ld].view(n, ld)
    assert rows.data_ptr() % 16 == 4
    rows[:, :d] = mu.float().to(dev)
    rows[:, d:2 * d] = lv.float().to(dev)
    dmu = torch.full((n, d), 3.0, dtype=torch.float32, device=dev)
    dlv = torch.full((n, d), 3.0, dtype=torch.float32, device=dev)
    lse = torch.empty(2 * n, dtype=torch.float32, device=dev)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    br = _branch(rows, rows[:, d:], ld, ps, dmu, dlv, d, None, 1.0, loss, lse)
    names = _call([br], label.to(dev), n, d, sim, 0.1, (2,), 0)
    _assert_path(names, ("lds", (8,)), ("lds", (8,)), 1)
    _check(f"unaligned {sim} ps={int(ps)}", (float(loss), dmu.cpu(), dlv.cpu()), _oracle(mu, lv, label, sim, 0.1, ps),
           sim)
    if sim == "cosine":  # (no logvar gradient: the kernel writes its zero)
        assert not dlv.any()


# ----------------------------------------------------------------------------- c. edges


def _edge_shapes(sim):
    """(n, d, rows family, gradient family): one LDS shape and the global-walk shape of this similarity."""
    walk = (544, 64) if sim in ("cosine", "l2") else (288, 64)
    return [(70, 10, ("lds", (16,)), ("lds", (16,))), walk + (("walk", (64, False)), ("walk", (64, False)))]


EDGE_SIMS = [(sim, i) for sim in SIMS for i in (0, 1)]


@pytest.mark.parametrize("sim,which", EDGE_SIMS)
def test_singleton_labels(sim, which):
    """Three rows with unique labels under ps = False: non-finite rows that leave the mean (the finite-row count is
    n - 3) but still act as columns in the other rows' denominators."""
    n, d, rows, grad = _edge_shapes(sim)[which]
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, False, salt=2))
    for q, r in enumerate((0, n // 2, n - 1)):
        label[r] = 100 + q
    _, _, terms = _oracle_rows(mu, lv, label, sim, 0.1, False)
    assert int(torch.isfinite(terms).sum()) == n - 3
    _module_case(f"singletons n={n} d={d} {sim}", mu, lv, label, sim, 0.1, False, rows, grad)


@pytest.mark.parametrize("sim,which", [("cosine", 0), ("cosine", 1), ("jeffrey", 0), ("jeffrey", 1)])
def test_no_finite_row(sim, which):
    """All labels equal under ps = True: no row has a positive.  The loss is NaN as the oracle's is and every
    gradient element is exactly 0; with accumulate = 1 a pre-filled buffer is unchanged bit for bit."""
    n, d, rows, grad = _edge_shapes(sim)[which]
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, True, salt=3))
    label[:] = 4
    rloss, _, _ = _oracle(mu, lv, label, sim, 0.1, True)
    assert rloss != rloss
    loss, gm, gl, names = _device_module(mu, lv, label, sim, 0.1, True)
    _assert_path(names, rows, grad, 2)
    assert loss != loss
    assert not gm.any() and (gl is None or not gl.any())
    dev = torch.device("cuda")
    m, l_ = mu.float().to(dev), lv.float().to(dev)
    g = torch.Generator().manual_seed(5)
    seed_mu, seed_lv = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    dmu, dlv = seed_mu.to(dev), seed_lv.to(dev)
    lse = torch.empty(2 * n, dtype=torch.float32, device=dev)
    lo = torch.zeros((), dtype=torch.float32, device=dev)
    names = _call([_branch(m, l_, d, True, dmu, dlv, d, None, 1.0, lo, lse)], label.to(dev), n, d, sim, 0.1, (2,), 1)
    _assert_path(names, rows, grad, 1)
    assert float(lo) != float(lo)
    assert torch.equal(dmu.cpu().view(torch.int32), seed_mu.view(torch.int32))
    assert torch.equal(dlv.cpu().view(torch.int32), seed_lv.view(torch.int32))


def _tiny(tag, mu, lv, label, sim, ps, fam):
    rloss, rgm, rgl = _oracle(mu, lv, label, sim, 0.1, ps)
    assert abs(rloss) <= 1e-9 and float(rgm.abs().max()) <= 1e-9, (rloss, float(rgm.abs().max()))
    loss, gm, gl, names = _device_module(mu, lv, label, sim, 0.1, ps)
    _assert_path(names, fam, fam, 2)
    worst = max(float(gm.abs().max()), float(gl.abs().max()) if gl is not None else 0.0)
    print(f"NTX {tag} loss={loss:.3g} grad_max={worst:.3g}")
    assert abs(loss) <= 1e-6, loss
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("sim", SIMS)
def test_two_rows(sim):
    """n = 2 with one label under ps = False: each row's only column is its positive, so the loss is 0 and the two
    softmax weights cancel in the gradient."""
    mu, lv, _ = _inputs(2, 8, _seed(2, 8, sim, False))
    fam = ("reg", (8, 8)) if sim == "cosine" else ("lds", (8,))
    _tiny(f"n=2 {sim}", mu, lv, torch.tensor([3, 3]), sim, False, fam)


def test_three_rows_l2():
    """n = 3, labels [0, 0, 1], l2, ps = True: rows 0 and 1 have row 2 as their positive and each other as the only
    negative; with this seed row 2 is so much nearer that the negative's exp underflows (the oracle's loss is 0 and
    its gradients are below 1e-40, asserted first)."""
    mu, lv, _ = _inputs(3, 8, _seed(3, 8, "l2", True))
    _tiny("n=3 l2", mu, lv, torch.tensor([0, 0, 1]), "l2", True, ("lds", (8,)))


@pytest.mark.parametrize("n,d,rows,grad", [(64, 8, ("reg", (8, 8)), ("reg", (8, 8))),
                                           (70, 10, ("lds", (16,)), ("lds", (16,))),
                                           (544, 64, ("walk", (64, False)), ("walk", (64, False)))])
@pytest.mark.parametrize("ps", [False, True])
def test_zero_row_cosine(n, d, rows, grad, ps):
    """A zero mu row under cosine: the fp64 oracle is finite (the eps = 1e-8 clamp of the norm); the zero row's
    gradient is ~1e6-1e7 through that clamp, so it is compared on its own and the other rows together, each at 1e-4
    rel-L2."""
    mu, lv, label = _inputs(n, d, _seed(n, d, "cosine", ps, salt=4))
    z = 3
    mu[z] = 0.0
    rloss, rgm, _ = _oracle(mu, lv, label, "cosine", 0.1, ps)
    assert rloss == rloss and bool(torch.isfinite(rgm).all())
    loss, gm, _, names = _device_module(mu, lv, label, "cosine", 0.1, ps)
    _assert_path(names, rows, grad, 2)
    keep = torch.arange(n) != z
    e_zero, e_rest = _rel(gm[z], rgm[z]), _rel(gm[keep], rgm[keep])
    print(f"NTX zero-row n={n} d={d} ps={int(ps)} loss={loss:.7g} ref={rloss:.7g} |g_zero|={float(rgm[z].norm()):.3g} "
          f"e_zero={e_zero:.3g} e_rest={e_rest:.3g}")
    assert abs(loss - rloss) <= 1e-4 * max(abs(rloss), 1e-3), (loss, rloss)
    assert e_zero < 1e-4, e_zero
    assert e_rest < 1e-4, e_rest


@pytest.mark.parametrize("n,d,sim,rows,grad", [(64, 8, "cosine", ("reg", (8, 8)), ("reg", (8, 8))),
                                               (70, 10, "jeffrey", ("lds", (16,)), ("lds", (16,))),
                                               (288, 64, "mahalanobis", ("walk", (64, False)), ("walk", (64, False))),
                                               (544, 64, "cosine", ("walk", (64, False)), ("walk", (64, False)))])
@pytest.mark.parametrize("ps", [False, True])
def test_labels_above_bit_31(n, d, sim, rows, grad, ps):
    """Classes k and k + 2**40 differ only above bit 31.  The device equals the oracle on the true int64 labels, and
    that oracle differs from the one on labels truncated to 32 bits by far more than the bars (checked first)."""
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps, salt=5), classes=5)
    g = torch.Generator().manual_seed(n + d)
    label = label + (torch.rand(n, generator=g) < 0.5).long() * (1 << 40)
    trunc = label & 0xFFFFFFFF
    assert len(torch.unique(label)) > len(torch.unique(trunc))
    ref = _oracle(mu, lv, label, sim, 0.1, ps)
    bad = _oracle(mu, lv, trunc, sim, 0.1, ps)
    assert abs(ref[0] - bad[0]) > 1e-2 * abs(ref[0]) and _rel(bad[1], ref[1]) > 1e-2
    loss, gm, gl, names = _device_module(mu, lv, label, sim, 0.1, ps)
    _assert_path(names, rows, grad, 2)
    _check(f"labels64 n={n} d={d} {sim} ps={int(ps)}", (loss, gm, gl), ref, sim)


@pytest.mark.parametrize("n,d,fam", [(70, 8, ("lds", (8,))), (544, 64, ("walk", (64, False)))])
@pytest.mark.parametrize("ps", [False, True])
def test_large_logits_l2(n, d, fam, ps):
    """l2 with mu scaled by 30: logits of about -1e5 and a loss of about 3.5e4 at (70, 8), ps = False; without the
    max subtraction every exp underflows.  The LDS kernels and the global-walk kernels each have their own
    log-sum-exp loop."""
    mu, lv, label = _inputs(n, d, _seed(n, d, "l2", ps, salt=6))
    mu = (30.0 * mu).float().double()
    ref = _oracle(mu, lv, label, "l2", 0.1, ps)
    assert ref[0] > 1e3
    _module_case(f"large-logits n={n} d={d} l2 ps={int(ps)}", mu, lv, label, "l2", 0.1, ps, fam, fam)


@pytest.mark.parametrize("tau", [0.07, 0.5])
@pytest.mark.parametrize("sim", ["jeffrey", "cosine"])
@pytest.mark.parametrize("ps", [False, True])
def test_temperatures(tau, sim, ps):
    n, d = 70, 10
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, ps, salt=7))
    _module_case(f"tau={tau} n={n} d={d} {sim} ps={int(ps)}", mu, lv, label, sim, tau, ps, ("lds", (16,)), ("lds", (16,)))
