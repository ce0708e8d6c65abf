"""The device SupCon losses (csrc/cv_supcon.hip through src.losses.contrastive_loss(..., backend="device") ->
cvhip.autograd.SupConFn) against the torch composition of src/losses.py evaluated in fp64 on the CPU
(contrastive_loss(..., backend="torch"), itself pinned to the reference at 1e-12 by tests/test_supcon.py), with
autograd for the gradients.

Inputs as tests/test_gpu_ntxent_matrix.py::_inputs: mu ~ N(0,1) * scale, logvar = 0.3 N(0,1), seeded, labels uniform
in 0..classes-1; the device sees the fp32 rounding, the reference starts from the same rounded values in fp64.

Bars (the project's parity bars, tests/test_gpu_ntxent_matrix.py): loss within 1e-4 * max(|ref|, 1e-3), each
gradient tensor within 1e-4 rel-L2.  The fp32 torch composition differs from fp64 by at most 3.7e-6 (loss) and 1.1e-5
(a gradient) over the first five shapes below, so a correct fp32 kernel has about 10x room.  No bar is raised.

Variants (cv_supcon.hip): sc_*_kernel<DM, true> stages all n rows in LDS when n * (d + 1) * 4 * (2 with logvar)
<= 144 KiB, else sc_*_kernel<DM, false> walks the columns in tiles of 256 rows; for d = 8 the tiled variant starts
at n = 4097 (cosine, l2) and n = 2049 (the logvar similarities).  The launch log is per thread, so the backward runs
on the calling thread (torch.autograd.set_multithreading_enabled(False))."""

import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIMS = ("cosine", "l2", "modified_l2", "jeffrey", "mahalanobis")
USES_LV = ("modified_l2", "jeffrey", "mahalanobis")
LOSSES = ("supcon_in_loss", "supcon_out_loss")
LDS_LIMIT = 144 * 1024


# ----------------------------------------------------------------------------- helpers


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1).cpu(), torch.as_tensor(b).double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _inputs(n, d, seed, classes=10, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, d, generator=g, dtype=torch.float64) * scale
    lv = 0.3 * torch.randn(n, d, generator=g, dtype=torch.float64)
    label = torch.randint(0, classes, (n,), generator=g)
    return mu.float().double(), lv.float().double(), label


def _seed(n, d, sim, salt=0):
    return 100003 * n + 101 * d + 10 * SIMS.index(sim) + 7919 * salt


def _oracle(mu, lv, label, sim, tau, loss_name, ps):
    """(loss, d mu, d logvar or None): the torch composition in fp64 on the CPU."""
    from src.losses import contrastive_loss

    m64, l64 = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    loss = contrastive_loss(m64, l64, label, sim, tau, loss_name=loss_name, ps=ps, backend="torch")
    if torch.isfinite(loss):
        loss.backward()
    gm = m64.grad if m64.grad is not None else torch.zeros_like(mu)
    gl = (l64.grad if l64.grad is not None else torch.zeros_like(lv)) if sim in USES_LV else None
    return float(loss.detach()), gm, gl


@functools.lru_cache(maxsize=None)
def _case(n, d, classes, scale, tau, sim, loss_name, ps):
    """Inputs and their fp64 reference, computed once per case and shared (never modified)."""
    mu, lv, label = _inputs(n, d, _seed(n, d, sim), classes, scale)
    return mu, lv, label, _oracle(mu, lv, label, sim, tau, loss_name, ps)


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


_KERNEL = re.compile(r"sc_(rows|grad|loss)_kernel(?:<(\d+), (true|false)>)?")


def _launches(names):
    """[("rows", 16, True), ("loss",), ("grad", 16, True)] ...: the SupCon launches of a log; the bool is FULL (all
    rows staged in LDS)."""
    out = []
    for nm in names:
        m = _KERNEL.search(nm)
        if m:
            out.append((m.group(1),) if m.group(1) == "loss" else (m.group(1), int(m.group(2)), m.group(3) == "true"))
    return out


def _dm(d):
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def _full(n, d, sim):
    return n * (d + 1) * 4 * (2 if sim in USES_LV else 1) <= LDS_LIMIT


def _device(mu, lv, label, sim, tau, loss_name, ps, upstream=None):
    from src.losses import contrastive_loss

    m = mu.float().cuda().requires_grad_(True)
    l_ = lv.float().cuda().requires_grad_(True)
    lab = label.cuda()
    with _KernelLog() as log, torch.autograd.set_multithreading_enabled(False):
        loss = contrastive_loss(m, l_, lab, sim, tau, loss_name=loss_name, ps=ps, backend="device")
        (loss if upstream is None else upstream * loss).backward()
        torch.cuda.synchronize()
    gl = None
    if sim in USES_LV:
        gl = l_.grad.cpu()
    else:
        assert l_.grad is None or not l_.grad.any()
    return float(loss.detach()), m.grad.cpu(), gl, log.names


def _check(tag, dev, ref, sim):
    (loss, gm, gl), (rloss, rgm, rgl) = dev, ref
    e_loss = abs(loss - rloss) / max(abs(rloss), 1e-3)
    e_mu = _rel(gm, rgm)
    e_lv = _rel(gl, rgl) if sim in USES_LV else 0.0
    print(f"SUPCON {tag} loss={loss:.7g} ref={rloss:.7g} e_loss={e_loss:.3g} e_dmu={e_mu:.3g} e_dlv={e_lv:.3g}")
    assert abs(loss - rloss) <= 1e-4 * max(abs(rloss), 1e-3), (tag, loss, rloss)
    assert e_mu < 1e-4, (tag, "dmu", e_mu)
    if sim in USES_LV:
        assert e_lv < 1e-4, (tag, "dlogvar", e_lv)


def _assert_path(names, n, d, sim):
    full = _full(n, d, sim)
    want = [("rows", _dm(d), full), ("loss",), ("grad", _dm(d), full)]
    assert _launches(names) == want, (names, want)


# ----------------------------------------------------------------------------- a. the shape table

TABLE = ([(70, 10, 10, 1.0, 0.1, s) for s in SIMS]                  # ragged n vs 64 lanes / 4 rows, d % 4 != 0
         + [(288, 64, 10, 1.0, 0.1, s) for s in SIMS]               # the widest DM
         + [(257, 33, 10, 1.0, 0.5, s) for s in ("cosine", "jeffrey")]   # d < DM = 64 padding, another tau
         + [(130, 8, 60, 1.0, 0.1, s) for s in ("cosine", "l2")]    # many dropped rows (singleton classes)
         + [(96, 32, 10, 8.0, 0.1, s) for s in ("l2", "modified_l2", "mahalanobis", "jeffrey")])  # S < -999


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,d,classes,scale,tau,sim", TABLE)
def test_table(n, d, classes, scale, tau, sim, loss_name, ps):
    mu, lv, label, ref = _case(n, d, classes, scale, tau, sim, loss_name, ps)
    loss, gm, gl, names = _device(mu, lv, label, sim, tau, loss_name, ps)
    _assert_path(names, n, d, sim)
    _check(f"n={n} d={d} {sim} {loss_name} ps={int(ps)}", (loss, gm, gl), ref, sim)


def test_dropped_rows_are_really_dropped():
    """(130, 8) with 60 classes: under ps = False the singleton classes leave the mean (both losses), so the table
    case above exercises the kept-row count; (96, 32) at scale 8: every off-diagonal S / tau is far below -999 / tau,
    so supcon_out's diagonal term dominates its log-sum-exp."""
    mu, lv, label, _ = _case(130, 8, 60, 1.0, 0.1, "cosine", "supcon_in_loss", False)
    counts = torch.bincount(label)
    singles = int((counts[label] == 1).sum())
    assert 5 <= singles < 130
    from src.losses import pairwise_l2

    mu, lv, label, ref = _case(96, 32, 10, 8.0, 0.1, "l2", "supcon_out_loss", False)
    s = pairwise_l2(mu)
    s.fill_diagonal_(-1e30)
    assert float(s.max()) < -999
    assert -7e3 < ref[0] < -5e3
    assert _case(96, 32, 10, 8.0, 0.1, "l2", "supcon_in_loss", False)[3][0] > 5e3


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,d,ps,sim", [(5, 3, True, "cosine"), (5, 3, True, "jeffrey"), (1, 4, False, "cosine"),
                                        (1, 4, True, "mahalanobis")])
def test_no_kept_row(n, d, ps, sim, loss_name):
    """One class under ps = True, or a single row: no kept row.  The loss is NaN as the reference's mean of an empty
    tensor is, every gradient element is exactly 0, and nothing faults."""
    mu, lv, label = _inputs(n, d, _seed(n, d, sim, salt=3), classes=1)
    rloss, _, _ = _oracle(mu, lv, label, sim, 0.1, loss_name, ps)
    assert rloss != rloss
    loss, gm, gl, names = _device(mu, lv, label, sim, 0.1, loss_name, ps)
    _assert_path(names, n, d, sim)
    assert loss != loss
    assert not gm.any() and (gl is None or not gl.any())


# ----------------------------------------------------------------------------- b. the tiled (non-LDS) variant


def _supcon_rows(S, rows, label, tau, loss_name, ps):
    """The row values of supcon_in_loss / supcon_out_loss (src/losses.py) for the rows `rows` of the similarity,
    S = pairwise[rows, :]: the same expressions with the row operand restricted; non-kept rows are NaN / inf."""
    from src.losses import logsumexp

    lab_r = label[rows]
    # (.float(): the composition's pair matrix is fp32 whatever the inputs are, so its log n_k is an fp32 log)
    pair = ((label[None, :] != lab_r[:, None]) if ps else (label[None, :] == lab_r[:, None])).float()
    diag = torch.zeros_like(S, dtype=torch.bool)
    diag[torch.arange(len(rows)), rows] = True
    if loss_name == "supcon_in_loss":
        n_k = pair.sum(dim=1) - 1
        sim = S.masked_fill(diag, float("-inf"))
        pos = (pair * sim).masked_fill(pair == 0, float("-inf"))
        return n_k.log() - logsumexp(pos / tau, dim=1) + logsumexp(sim / tau, dim=1)
    sim = S.masked_fill(diag, -999.0)
    pos_mask = pair * (~diag).to(S.dtype)
    n_k = pos_mask.sum(dim=1)
    # (rows with n_k = 0 are dropped by the composition's `select`; NaN here, with a finite quotient for autograd)
    out = -(sim * pos_mask).sum(dim=1) / n_k.clamp_min(1) + logsumexp(sim / tau, dim=1)
    return out.masked_fill(n_k == 0, float("nan"))


@functools.lru_cache(maxsize=None)
def _big_reference(n, d, sim, tau, block=256, only=None):
    """{(loss_name, ps): (loss, d mu, d logvar)} in fp64, block by block over oracle.cpu_ref.pairwise_rows so that
    no [n, n, d] tensor is built; one similarity block serves the four (loss, ps) combinations, and the result is
    cached: the four cases of a shape share one pass, about 10 s of host time at n = 4097 (its cost is the fp64
    backward through the [block, n, d] broadcast, once per combination), paid by the first of them.  The row
    functions are checked against the torch composition at a small n by
    test_blockwise_reference_is_the_composition."""
    from oracle import cpu_ref as R

    mu, lv, label = _inputs(n, d, _seed(n, d, sim))
    m64, l64 = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    keys = [only] if only else [(ln, ps) for ln in LOSSES for ps in (False, True)]
    tot = {k: 0.0 for k in keys}
    cnt = {k: 0 for k in keys}
    gm = {k: torch.zeros_like(mu) for k in keys}
    gl = {k: torch.zeros_like(lv) for k in keys}
    for i in range(0, n, block):
        rows = torch.arange(i, min(n, i + block))
        S = R.pairwise_rows(sim, m64, l64, rows)
        sums = []
        for k in keys:
            t = _supcon_rows(S, rows, label, tau, k[0], k[1])
            fin = torch.isfinite(t)
            cnt[k] += int(fin.sum())
            s = t[fin].sum()
            tot[k] += float(s.detach())
            sums.append(s)
        for q, k in enumerate(keys):
            if not sums[q].requires_grad:
                continue
            g = torch.autograd.grad(sums[q], [m64, l64], retain_graph=q + 1 < len(keys), allow_unused=True)
            gm[k] += g[0]
            if g[1] is not None:
                gl[k] += g[1]
    return (mu, lv, label), {k: (tot[k] / cnt[k], gm[k] / cnt[k], gl[k] / cnt[k] if sim in USES_LV else None)
                             for k in keys}


@pytest.mark.parametrize("sim", ["cosine", "jeffrey"])
def test_blockwise_reference_is_the_composition(sim):
    n, d, tau = 70, 8, 0.1
    (mu, lv, label), ref = _big_reference(n, d, sim, tau, 32)
    for (loss_name, ps), (loss, gm, gl) in ref.items():
        rloss, rgm, rgl = _oracle(mu, lv, label, sim, tau, loss_name, ps)
        assert abs(loss - rloss) <= 1e-12 * max(abs(rloss), 1.0)
        assert _rel(gm, rgm) < 1e-12 and (gl is None or _rel(gl, rgl) < 1e-12)


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,sim", [(4097, "cosine"), (2049, "modified_l2")])
def test_tiled_variant_at_its_threshold(n, sim, loss_name, ps):
    """d = 8: the smallest n at which the rows do not fit the LDS (one row less does, asserted): the tiled kernels
    run, read from the launch log, with a ragged last tile (n % 256 == 1) and a last workgroup with one row."""
    d, tau = 8, 0.1
    assert _full(n - 1, d, sim) and not _full(n, d, sim)
    (mu, lv, label), ref = _big_reference(n, d, sim, tau)
    loss, gm, gl, names = _device(mu, lv, label, sim, tau, loss_name, ps)
    assert _launches(names) == [("rows", 8, False), ("loss",), ("grad", 8, False)], names
    _check(f"tiled n={n} d={d} {sim} {loss_name} ps={int(ps)}", (loss, gm, gl), ref[(loss_name, ps)], sim)


def test_largest_lds_batch():
    """n = 4096, d = 8, cosine: exactly 144 KiB of LDS, the largest fully staged launch."""
    n, d, sim, tau = 4096, 8, "cosine", 0.1
    assert _full(n, d, sim)
    (mu, lv, label), ref = _big_reference(n, d, sim, tau, only=("supcon_in_loss", False))
    loss, gm, gl, names = _device(mu, lv, label, sim, tau, "supcon_in_loss", False)
    assert _launches(names) == [("rows", 8, True), ("loss",), ("grad", 8, True)], names
    _check(f"full n={n} d={d} {sim}", (loss, gm, gl), ref[("supcon_in_loss", False)], sim)


# ----------------------------------------------------------------------------- c. fixture, strides, upstream, bits


def _fx():
    with np.load(os.path.join(HERE, "golden", "supcon.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_golden_fixture_on_the_device():
    """tests/golden/supcon.npz: its inputs rounded to fp32 on the device against the scalars the real reference
    recorded, every case it holds, at the loss bar."""
    from src.losses import contrastive_loss

    fx = _fx()
    mu = torch.tensor(fx["mu"]).float().cuda()
    lv = torch.tensor(fx["logvar"]).float().cuda()
    lab = torch.tensor(fx["label"]).cuda()
    seen = 0
    for key in fx:
        if "__" not in key:
            continue
        loss_name, sim, ps = key.split("__")
        v = float(contrastive_loss(mu, lv, lab, sim, float(fx["tau"]), loss_name=loss_name, ps=ps == "ps1",
                                   backend="device"))
        ref = float(fx[key])
        print(f"SUPCON golden {key} dev={v:.7g} ref={ref:.7g} e={abs(v - ref) / max(abs(ref), 1e-3):.3g}")
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (key, v, ref)
        seen += 1
    assert seen == 20


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("sim", ["cosine", "mahalanobis"])
def test_strided_heads_views(sim, loss_name):
    """mu / logvar as column slices of an [n, 4d] heads tensor (what the trainers pass): row stride 4d, no copy;
    the gradient reaches the heads tensor through the slices."""
    from src.losses import contrastive_loss

    n, d, tau, ps = 70, 10, 0.1, True
    mu, lv, label, ref = _case(n, d, 10, 1.0, tau, sim, loss_name, ps)
    heads = torch.randn(n, 4 * d, generator=torch.Generator().manual_seed(5)).cuda()
    heads[:, 2 * d:3 * d] = mu.float().cuda()
    heads[:, 3 * d:] = lv.float().cuda()
    heads.requires_grad_(True)
    loss = contrastive_loss(heads[:, 2 * d:3 * d], heads[:, 3 * d:], label.cuda(), sim, tau, loss_name=loss_name,
                            ps=ps, backend="device")
    loss.backward()
    g = heads.grad.cpu()
    assert not g[:, :2 * d].any()
    _check(f"strided {sim} {loss_name}", (float(loss.detach()), g[:, 2 * d:3 * d], g[:, 3 * d:]), ref, sim)
    if sim == "cosine":
        assert not g[:, 3 * d:].any()


@pytest.mark.parametrize("loss_name", LOSSES)
def test_upstream_gradient(loss_name):
    n, d, tau, sim, ps = 70, 10, 0.1, "jeffrey", False
    mu, lv, label, (rloss, rgm, rgl) = _case(n, d, 10, 1.0, tau, sim, loss_name, ps)
    loss, gm, gl, _ = _device(mu, lv, label, sim, tau, loss_name, ps, upstream=-2.5)
    _check(f"upstream {loss_name}", (loss, gm, gl), (rloss, -2.5 * rgm, -2.5 * rgl), sim)


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,d,sim", [(288, 64, "jeffrey"), (2049, 8, "modified_l2")])
def test_two_runs_are_bit_identical(n, d, sim, loss_name):
    mu, lv, label = _inputs(n, d, _seed(n, d, sim))
    a = _device(mu, lv, label, sim, 0.1, loss_name, False)
    b = _device(mu, lv, label, sim, 0.1, loss_name, False)
    assert np.float32(a[0]).view(np.int32) == np.float32(b[0]).view(np.int32)
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("loss_name", LOSSES)
def test_memory_has_no_n_squared_term(loss_name):
    """n = 4096, d = 32, jeffrey, forward + backward: the growth of the peak allocation stays below one n x n fp32
    matrix (64 MiB); inputs, gradients and row statistics are about 2.1 MB (the torch composition holds several
    [n, n, d] tensors of 2 GiB)."""
    from src.losses import contrastive_loss

    n, d = 4096, 32
    mu, lv, label = _inputs(n, d, _seed(n, d, "jeffrey"))
    m = mu.float().cuda().requires_grad_(True)
    l_ = lv.float().cuda().requires_grad_(True)
    lab = label.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    loss = contrastive_loss(m, l_, lab, "jeffrey", 0.1, loss_name=loss_name, backend="device")
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"SUPCON memory {loss_name} n={n} d={d}: +{grown} bytes")
    assert torch.isfinite(loss) and bool(torch.isfinite(m.grad).all()) and bool(torch.isfinite(l_.grad).all())
    assert grown < n * n * 4, grown


@pytest.mark.parametrize("loss_name", LOSSES)
def test_wider_than_the_envelope_warns_once_and_runs_the_composition(loss_name, monkeypatch):
    """d = 65 > 64: backend="device" warns (once per process) and returns the torch composition's value, no
    SupCon kernel launched."""
    from src import losses

    monkeypatch.setattr(losses, "_warned_supcon", False)
    mu, lv, label = _inputs(40, 65, 11)
    m, l_, lab = mu.float().cuda(), lv.float().cuda(), label.cuda()
    ref = losses.contrastive_loss(m, l_, lab, "l2", 0.1, loss_name=loss_name, backend="torch")
    with _KernelLog() as log:
        with pytest.warns(UserWarning, match="outside the device kernels' envelope"):
            v = losses.contrastive_loss(m, l_, lab, "l2", 0.1, loss_name=loss_name, backend="device")
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("error")
            v2 = losses.contrastive_loss(m, l_, lab, "l2", 0.1, loss_name=loss_name, backend="device")
        torch.cuda.synchronize()
    assert _launches(log.names) == []
    assert float(v) == float(ref) == float(v2)


# ----------------------------------------------------------------------------- d. trainer


@pytest.mark.parametrize("loss_name", LOSSES)
def test_trainer_trains_with_a_supcon_loss(loss_name, monkeypatch):
    """get_clearvae_trainer(loss_name=...) on VAE z = 16, two batches of 32 synthetic 28x28 images: SupConFn.apply
    runs twice per step, the fused engine is never built, parameters move and stay finite, evaluate() is finite."""
    from cvhip import autograd as ag
    from cvhip.engine import ClearStep
    from oracle import cpu_ref as R
    from src.utils.trainer_utils import get_clearvae_trainer

    calls = []
    real = ag.SupConFn.apply

    def counting(*a):
        calls.append(a[6])
        return real(*a)

    def no_engine(*a, **k):
        raise AssertionError("the fused engine must not be built for a supcon loss")

    monkeypatch.setattr(ag.SupConFn, "apply", staticmethod(counting))
    monkeypatch.setattr(ClearStep, "build", staticmethod(no_engine))
    torch.manual_seed(0)
    tr = get_clearvae_trainer(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=16, alpha=100, temperature=0.1, device="cuda",
                              loss_name=loss_name)
    x, label, _, _, _ = R.det_inputs(64, 1, 28, 16, 10)
    ds = torch.utils.data.TensorDataset(torch.tensor(x, dtype=torch.float32), torch.tensor(label))
    dl = torch.utils.data.DataLoader(ds, batch_size=32, shuffle=False)
    before = [p.detach().clone() for p in tr.model.parameters()]
    steps = 0
    for epoch in range(2):
        tr._train(dl, False, epoch)
        steps += len(dl)
        assert len(calls) == 2 * steps
        assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    assert steps >= 3 and tr._engine is None
    from cvhip import _lib

    assert set(calls) == {_lib.SUPCON[loss_name]}
    assert any(not torch.equal(p.detach(), b) for p, b in zip(tr.model.parameters(), before))
    n_train = len(calls)
    mig, mse = tr.evaluate(dl, False, 0)
    assert len(calls) == n_train + 2 * len(dl)
    assert np.isfinite(mig) and np.isfinite(mse)
