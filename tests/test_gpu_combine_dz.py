"""The latent combine kernels (csrc/cv_latent.hip) called directly, against an fp64 torch restatement of
trainer.py:452-480 through the decoder Linear (vae.py:33), z = mu + eps exp(lv / 2) (vae.py:56-60), the KL terms
(losses.py:48-49) and the logistic annealer (trainer.py:32-34):

  heads = [n][4d] = mu_c | lv_c | mu_s | lv_s,  mu / lv the [n][2d] concatenations,  z = mu + eps exp(lv / 2) (fp32)
  wgt   = beta / (1 + exp(-(t - loc) / scale))
  dz    = d(h) W                 (W [F][K] in PyTorch feature order, d(h) stored pixel-major: _storage)
  dmu   = wgt mu / n + dz        dlv = wgt (-0.5 / n)(1 - exp(lv)) + dz (z - mu) / 2
  losses[1], [2] = -0.5 / n sum(1 + lv - mu^2 - exp(lv)) over the content / style half, [7] = wgt, [0] = sum(rec_in)

cv_latent_combine_dz (combine_dz_kernel: MFMA contraction, storage-column -> feature map, per-tile split-K with
tickets, the combine of 256 elements per tile) at shapes with ragged row / column tiles, a tile that straddles the
content / style boundary, pix > 1, 1 / 2 / 4 slices; cv_latent_combine / _acc (combine_kernel, combine_multi_kernel)
at one shape per launch form of combine_launch.

Tolerances: 1e-5 relative L2 against fp64 (test_gpu_declinear.py's bar for fp32 contractions) and, on dz,
max|err| <= 1e-5 max|ref| (one wrong element cannot hide in the norm); the KL terms and the weight 1e-5 relative.
An fp32 CPU restatement of the formulas sits at 1.4e-7 .. 3.7e-7 relative L2 and <= 8e-8 on the KL terms with these
input distributions, a dropped 4-column chunk at F = 2048 moves dz by ~4e-2; the kernels measure 7e-8 .. 2.3e-7 on
dz and d(heads) (cv_latent_combine / _acc 3.6e-8) on an MI355X.  Every sum of the kernels has a fixed
order: launches repeated on one workspace without a host synchronisation between them are bit-identical, and every
launch leaves its tickets at zero."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_declinear import _rel, _storage

pytestmark = pytest.mark.gpu

SLOTS = 1024  # CMB_SLOTS: KL partial slots of the workspace; the tickets follow them
GUARD = 16  # rows past n of the output buffers that no launch may touch
SENT = -12345.5  # their fill
LSENT = 7.25  # fill of the losses words the kernels do not write

CASES_DZ = [  # n, d, ch, pix: the slices the host picks with CV_CDZ_S unset (4)
    (16, 8, 64, 1),  # S=1: one full tile, identity feature map
    (5, 4, 64, 1),  # S=1: rows and columns ragged in the only tile
    (37, 12, 32, 4),  # S=2: tile 0 straddles j = d, second column tile half empty, ragged last row tile, pix > 1
    (50, 8, 128, 16),  # S=4: the MNIST geometry at a ragged batch
    (33, 32, 512, 4),  # S=4: the VAE64 geometry, 4 column tiles x 3 row tiles
    (16, 8, 48, 4),  # S=1: F % 128 != 0
]
ANNEAL = [(0, 0.0, 1.0, 1 / 8), (7, 5.0, 2.0, 1 / 32)]  # t, loc, scale, beta

CASES_PLAIN = [  # n, d: the launch forms of combine_launch
    (16, 4),  # 128 elements: one workgroup
    (37, 8),  # 592: one workgroup, ragged
    (512, 8),  # 8192: 4 workgroups
    (2100, 32),  # 134400: capped at 64 workgroups, grid-stride tail
]


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(n, d, F, pix, ch):
    """Host inputs of one shape (F = 0: no contraction, dz ~ N(0, 1) given) with their fp64 restatement's parts;
    built once, never written."""
    g = np.random.default_rng(1000 * n + 10 * d + F)
    K = 2 * d
    heads = torch.tensor(g.standard_normal((n, 4 * d)) * 0.5, dtype=torch.float32)
    eps = torch.tensor(g.standard_normal((n, K)), dtype=torch.float32)
    mu = torch.cat([heads[:, 0:d], heads[:, 2 * d:3 * d]], 1)
    lv = torch.cat([heads[:, d:2 * d], heads[:, 3 * d:4 * d]], 1)
    z = mu + eps * torch.exp(0.5 * lv)  # (fp32, as the forward builds it)
    prior = torch.tensor(g.standard_normal((n, 4 * d)), dtype=torch.float32)
    rec = torch.tensor(g.uniform(0, 1, 32), dtype=torch.float64)
    r = 0.0
    for v in rec.tolist():  # (the kernels' order)
        r += v
    I = dict(n=n, d=d, heads=heads, z=z, mu=mu.double(), lv=lv.double(), prior=prior, rec=rec, rec_sum=np.float32(r))
    if F:
        I["W"] = torch.tensor(g.uniform(-0.3, 0.3, (F, K)), dtype=torch.float32)
        dh = torch.tensor(g.standard_normal((n, F)), dtype=torch.float32)
        I["dh"] = _storage(dh, pix, ch).contiguous()
        I["dz"] = dh.double() @ I["W"].double()
    else:
        dz = torch.tensor(g.standard_normal((n, K)), dtype=torch.float32)
        I["dz32"] = dz
        I["dz"] = dz.double()
    return I


def _expected(I, dz, anneal, accumulate):
    """fp64: (dheads [n][4d], kl_c, kl_s, wgt) for the given dz."""
    t, loc, scale, beta = anneal
    n, d, mu, lv = I["n"], I["d"], I["mu"], I["lv"]
    wgt = float(np.float32(beta)) / (1.0 + np.exp(-(t - loc) / scale))
    dmu = wgt * mu / n + dz
    dlv = wgt * (-0.5 / n) * (1 - torch.exp(lv)) + dz * (I["z"].double() - mu) / 2
    dheads = torch.cat([dmu[:, :d], dlv[:, :d], dmu[:, d:], dlv[:, d:]], 1)
    if accumulate:
        dheads = dheads + I["prior"].double()
    term = 1 + lv - mu * mu - torch.exp(lv)
    return dheads, float(-0.5 / n * term[:, :d].sum()), float(-0.5 / n * term[:, d:].sum()), wgt


def _dev(t):
    return t.to("cuda")


def _out_buffers(I, accumulate, with_dz):
    n, d = I["n"], I["d"]
    dheads = torch.full((n + GUARD, 4 * d), SENT, device="cuda")
    dheads[:n] = _dev(I["prior"]) if accumulate else float("nan")
    dz_out = None
    if with_dz:
        dz_out = torch.full((n + GUARD, 2 * d), SENT, device="cuda")
        dz_out[:n] = float("nan")
    losses = torch.full((24,), LSENT, device="cuda")
    return dheads, dz_out, losses


def _dz_workspace(n, d):
    from cvhip import _lib

    return torch.zeros(int(_lib.lib().cv_latent_combine_dz_workspace_bytes(n, d)) // 8 + 1, dtype=torch.float64,
                       device="cuda")


def _dz_tickets(work):
    """The grid ticket (2 words) and the tile tickets (SLOTS words) of a cv_latent_combine_dz workspace."""
    return work.view(torch.int32)[2 * 2 * SLOTS:2 * 2 * SLOTS + 2 + SLOTS]


class _DzOperands:
    """Device operands of one shape, shared by its launches."""

    def __init__(self, n, d, ch, pix):
        from cvhip import _lib

        self.I = I = _inputs(n, d, ch * pix, pix, ch)
        self.heads, self.z, self.dh, self.W = _dev(I["heads"]), _dev(I["z"]), _dev(I["dh"]), _dev(I["W"])
        self.rec = _dev(I["rec"])
        self.lin = _lib.cv_linear(n, 2 * d, ch * pix, 1, 0, pix, ch, 0)
        self.steps = {}

    def launch(self, anneal, with_rec, accumulate, work, with_dz=True):
        """One cv_latent_combine_dz launch into fresh output buffers (no synchronisation)."""
        from cvhip import _lib

        t, loc, scale, beta = anneal
        if t not in self.steps:
            self.steps[t] = torch.tensor([t], dtype=torch.int64, device="cuda")
        dheads, dz_out, losses = _out_buffers(self.I, accumulate, with_dz)
        _lib.call("cv_latent_combine_dz", self.heads.data_ptr(), self.z.data_ptr(), self.dh.data_ptr(),
                  self.W.data_ptr(), ctypes.byref(self.lin), beta, loc, scale, self.steps[t].data_ptr(),
                  self.rec.data_ptr() if with_rec else None, dheads.data_ptr(), losses.data_ptr(),
                  dz_out.data_ptr() if with_dz else None, int(accumulate), work.data_ptr(), _lib.stream_handle())
        return dheads, dz_out, losses


def _check_guard(I, dheads, dz_out):
    n = I["n"]
    assert bool((_bits(dheads[n:]) == _bits(torch.full_like(dheads[n:], SENT))).all()), "dheads rows past n written"
    assert not bool(torch.isnan(dheads[:n]).any()), "a live dheads element was not written"
    if dz_out is not None:
        assert bool((_bits(dz_out[n:]) == _bits(torch.full_like(dz_out[n:], SENT))).all()), "dz rows past n written"
        assert not bool(torch.isnan(dz_out[:n]).any()), "a live dz element was not written"


def _check_losses(I, losses, ref, with_rec):
    _, kc, ks, wgt = ref
    lo = losses.cpu()
    for i, want in ((1, kc), (2, ks), (7, wgt)):
        assert abs(float(lo[i]) - want) <= 1e-5 * abs(want), (i, float(lo[i]), want)
    if with_rec:
        assert float(lo[0]) == float(I["rec_sum"])
    untouched = [3, 4, 5, 6] + list(range(8, 24)) + ([] if with_rec else [0])
    assert bool((lo[untouched] == LSENT).all()), lo


def _check_dheads(I, dheads, ref):
    n = I["n"]
    e = _rel(dheads[:n], ref[0])
    print("dheads rel", e)
    assert e <= 1e-5, e


@pytest.mark.parametrize("anneal", ANNEAL, ids=["t0", "t7"])
@pytest.mark.parametrize("with_rec", [True, False], ids=["rec", "norec"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("n,d,ch,pix", CASES_DZ)
def test_combine_dz_against_fp64(n, d, ch, pix, accumulate, with_rec, anneal):
    op = _DzOperands(n, d, ch, pix)
    I = op.I
    work = _dz_workspace(n, d)
    dheads, dz_out, losses = op.launch(anneal, with_rec, accumulate, work)
    torch.cuda.synchronize()
    assert int(_dz_tickets(work).abs().max()) == 0, "a ticket was not reset"
    _check_guard(I, dheads, dz_out)
    ref = _expected(I, I["dz"], anneal, accumulate)
    dz = dz_out[:n].double().cpu()
    e2, emax = _rel(dz, I["dz"]), float((dz - I["dz"]).abs().max() / I["dz"].abs().max())
    print("dz rel", e2, "max", emax)
    assert e2 <= 1e-5, e2
    assert emax <= 1e-5, emax
    _check_dheads(I, dheads, ref)
    _check_losses(I, losses, ref, with_rec)


def test_combine_dz_kl_gradient_alone():
    """d(h) = 0: d(heads) is the KL term alone (at the other cases' beta it is ~1e-4 of the decoder term)."""
    n, d, ch, pix = 37, 12, 32, 4
    op = _DzOperands(n, d, ch, pix)
    op.dh = torch.zeros_like(op.dh)
    anneal = (0, 0.0, 1.0, 1.0)
    work = _dz_workspace(n, d)
    dheads, dz_out, losses = op.launch(anneal, True, 0, work)
    torch.cuda.synchronize()
    _check_guard(op.I, dheads, dz_out)
    assert float(dz_out[:n].abs().max()) == 0.0
    ref = _expected(op.I, torch.zeros(n, 2 * d, dtype=torch.float64), anneal, 0)
    _check_dheads(op.I, dheads, ref)
    _check_losses(op.I, losses, ref, True)


@pytest.mark.parametrize("n,d,ch,pix", [CASES_DZ[2], CASES_DZ[5]])
def test_combine_dz_without_dz_out(n, d, ch, pix):
    """dz_out = NULL: the same d(heads) and losses, bit for bit."""
    op = _DzOperands(n, d, ch, pix)
    work = _dz_workspace(n, d)
    a = op.launch(ANNEAL[1], True, 1, work)
    b = op.launch(ANNEAL[1], True, 1, work, with_dz=False)
    torch.cuda.synchronize()
    assert int(_dz_tickets(work).abs().max()) == 0
    _check_guard(op.I, b[0], None)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[2]), _bits(b[2]))
    _check_dheads(op.I, b[0], _expected(op.I, op.I["dz"], ANNEAL[1], 1))


@pytest.mark.parametrize("n,d,ch,pix", CASES_DZ)
def test_combine_dz_replays_are_bit_identical(n, d, ch, pix):
    """8 launches back to back on one workspace, no host synchronisation between them: the fixed-order claim of the
    kernel's header comment, and every ticket reset by the launch that took it."""
    op = _DzOperands(n, d, ch, pix)
    work = _dz_workspace(n, d)
    outs = [op.launch(ANNEAL[1], True, 1, work) for _ in range(8)]
    torch.cuda.synchronize()
    assert int(_dz_tickets(work).abs().max()) == 0
    _check_dheads(op.I, outs[0][0], _expected(op.I, op.I["dz"], ANNEAL[1], 1))
    for k, (dheads, dz_out, losses) in enumerate(outs[1:], 1):
        assert torch.equal(_bits(dz_out), _bits(outs[0][1])), k
        assert torch.equal(_bits(dheads), _bits(outs[0][0])), k
        assert torch.equal(_bits(losses[:8]), _bits(outs[0][2][:8])), k


def _plain_workspace():
    from cvhip import _lib

    return torch.zeros(int(_lib.lib().cv_latent_combine_workspace_bytes()) // 8 + 1, dtype=torch.float64,
                       device="cuda")


def _plain_launch(I, dz, anneal, with_rec, accumulate, work, dev):
    """cv_latent_combine (accumulate = 0) / cv_latent_combine_acc into fresh output buffers (no synchronisation)."""
    from cvhip import _lib

    t, loc, scale, beta = anneal
    dheads, _, losses = _out_buffers(I, accumulate, False)
    _lib.call("cv_latent_combine_acc" if accumulate else "cv_latent_combine", dev["heads"].data_ptr(),
              dev["z"].data_ptr(), dz.data_ptr(), I["n"], I["d"], beta, loc, scale, dev["step"][t].data_ptr(),
              dev["rec"].data_ptr() if with_rec else None, dheads.data_ptr(), losses.data_ptr(),
              work.data_ptr() if work is not None else None, _lib.stream_handle())
    return dheads, losses


def _plain_dev(I):
    return dict(heads=_dev(I["heads"]), z=_dev(I["z"]), rec=_dev(I["rec"]),
                step={t: torch.tensor([t], dtype=torch.int64, device="cuda") for t, *_ in ANNEAL})


@pytest.mark.parametrize("n,d,ch,pix", [CASES_DZ[2], CASES_DZ[3]])
@pytest.mark.parametrize("anneal", ANNEAL, ids=["t0", "t7"])
def test_combine_dz_matches_combine_acc_on_its_own_dz(n, d, ch, pix, anneal):
    """The two schedules: cv_latent_combine_acc fed the kernel's own dz_out runs the same per-element arithmetic
    (only the compiler's contraction may differ)."""
    op = _DzOperands(n, d, ch, pix)
    I = op.I
    work = _dz_workspace(n, d)
    dheads, dz_out, losses = op.launch(anneal, True, 1, work)
    pwork = _plain_workspace()
    dh2, lo2 = _plain_launch(I, dz_out, anneal, True, 1, pwork, _plain_dev(I))
    torch.cuda.synchronize()
    assert int(pwork.view(torch.int32)[2 * 2 * SLOTS]) == 0
    _check_guard(I, dh2, None)
    a, b = dh2[:n].double().cpu(), dheads[:n].double().cpu()
    assert _rel(a, b) <= 1e-6, _rel(a, b)
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    la, lb = lo2[:8].double().cpu(), losses[:8].double().cpu()
    assert bool(((la - lb).abs() <= 1e-6 * lb.abs()).all()), (la, lb)


@pytest.mark.parametrize("anneal", ANNEAL, ids=["t0", "t7"])
@pytest.mark.parametrize("with_rec", [True, False], ids=["rec", "norec"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("n,d", CASES_PLAIN)
def test_combine_against_fp64(n, d, accumulate, with_rec, anneal):
    """cv_latent_combine / _acc with a given dz: without a workspace (the one-workgroup kernel), and 8 launches back
    to back on one workspace (several workgroups from 2 x 2048 elements), bit-identical, the ticket left at zero."""
    I = _inputs(n, d, 0, 0, 0)
    dev = _plain_dev(I)
    dz = _dev(I["dz32"])
    ref = _expected(I, I["dz"], anneal, accumulate)
    one = _plain_launch(I, dz, anneal, with_rec, accumulate, None, dev)
    work = _plain_workspace()
    outs = [_plain_launch(I, dz, anneal, with_rec, accumulate, work, dev) for _ in range(8)]
    torch.cuda.synchronize()
    assert int(work.view(torch.int32)[2 * 2 * SLOTS]) == 0, "the ticket was not reset"
    for dheads, losses in (one, outs[0]):
        _check_guard(I, dheads, None)
        _check_dheads(I, dheads, ref)
        _check_losses(I, losses, ref, with_rec)
    for k, (dheads, losses) in enumerate(outs[1:], 1):
        assert torch.equal(_bits(dheads), _bits(outs[0][0])), k
        assert torch.equal(_bits(losses[:8]), _bits(outs[0][1][:8])), k
