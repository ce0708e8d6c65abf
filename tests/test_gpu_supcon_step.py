"""cv_supcon_step (csrc/cv_supcon.hip: the step form of the SupCon kernels), called directly through the C-ABI on a
synthetic [n][4d] heads buffer — content mu at column 0, logvar at d, style mu at 2d, logvar at 3d, row stride 4d, as
the fused step passes them — against the torch composition of src/losses.py in fp64 on the CPU
(tests/test_gpu_supcon.py::_oracle, the reference of the existing SupCon tests).

Bars (tests/test_gpu_supcon.py): loss within 1e-4 * max(|ref|, 1e-3), each gradient block within 1e-4 rel-L2.  Phase 1
accumulates, so the gradient is read as dheads_after - dheads_before, the difference taken in fp64, over a pre-fill
of the gradient's own magnitude: one fp32 add of two numbers of the gradient's size rounds at 6e-8 of their sum, far
below the bar.  Where the reference keeps no row (n = 2 under some labels) the loss must be NaN and the difference
exactly zero.

The draws: seeded as tests/test_gpu_supcon.py seeds its inputs; per (n, d, similarity) the first draw of the seed
sequence that is measurable (_measurable, a property of the reference alone).  Measured on the one shape where the
first draw is not, (5, 3, cosine), labels [5, 8, 1, 0, 8], supcon_in under ps = 1: |d mu| = 2.0e-5 beside a loss of
0.94, the torch composition in fp32 is 7.1e-4 rel-L2 from its fp64 value there and cv_supcon_step 2.5e-3 (1.4e-8 and
5e-8 absolute): a cancellation residue (rows whose every other row is a positive have the constant value log n_k),
not a gradient a 1e-4 bar can be held to.  With (5, 3, jeffrey)'s first draw all labels are distinct and the
reference gradient is exactly zero; the kernels return the fp32 residue of softmax_all - softmax_pos there, 1e-8 of
the weights, as cv_supcon does."""

import ctypes
import functools

import pytest
import torch

from test_gpu_supcon import LOSSES, USES_LV, _big_reference, _full, _inputs, _KernelLog, _oracle, _rel, _seed

pytestmark = pytest.mark.gpu

TAU = 0.1


# ----------------------------------------------------------------------------- helpers


COND = 2e-5  # a draw is measurable when the fp32 composition's own gradient error is a fifth of the 1e-4 bar


@functools.lru_cache(maxsize=None)
def _draw(n, d, sim, salt, classes=10):
    """((mu_c, lv_c), (mu_s, lv_s), label): fp64 values of fp32-representable inputs, shared and never modified."""
    mu_c, lv_c, label = _inputs(n, d, _seed(n, d, sim, salt=2 * salt), classes)
    mu_s, lv_s, _ = _inputs(n, d, _seed(n, d, sim, salt=2 * salt + 1), classes)
    return (mu_c, lv_c), (mu_s, lv_s), label


@functools.lru_cache(maxsize=None)
def _ref_of(n, d, sim, salt, loss_name, ps, b):
    br = _draw(n, d, sim, salt)
    return _oracle(br[b][0], br[b][1], br[2], sim, TAU, loss_name, ps)


def _measurable(n, d, sim, salt):
    """Judged from the reference alone: every (branch, loss, ps) of the draw either keeps no row (NaN: checked
    exactly) or has a gradient that the torch composition itself reproduces in fp32 within COND of its fp64 value.
    A draw fails this when the gradient is a cancellation residue: at n = 5 with ten classes most rows have every
    other row as a positive under ps = 1, their supcon_in value is the constant log n_k, and the whole gradient is
    zero (all labels distinct) or 1e-5 of the loss (one equal pair), which no fp32 evaluation resolves to 1e-4."""
    from src.losses import contrastive_loss

    br = _draw(n, d, sim, salt)
    for b in range(2):
        for loss_name in LOSSES:
            for ps in (False, True):
                rloss, rgm, rgl = _ref_of(n, d, sim, salt, loss_name, ps, b)
                if rloss != rloss:
                    continue
                m = br[b][0].float().requires_grad_(True)
                v = br[b][1].float().requires_grad_(True)
                contrastive_loss(m, v, br[2], sim, TAU, loss_name=loss_name, ps=ps, backend="torch").backward()
                if not float(rgm.norm()) > 0 or _rel(m.grad, rgm) > COND:
                    return False
                if sim in USES_LV and (not float(rgl.norm()) > 0 or _rel(v.grad, rgl) > COND):
                    return False
    return True


@functools.lru_cache(maxsize=None)
def _salt(n, d, sim):
    """The first measurable draw of the seed sequence (0 for every shape but the smallest)."""
    for salt in range(16):
        if _measurable(n, d, sim, salt):
            return salt
    raise AssertionError(f"no measurable draw for n={n} d={d} {sim}")


def _branches(n, d, sim):
    return _draw(n, d, sim, _salt(n, d, sim))


def _ref(n, d, sim, loss_name, ps, b):
    """(loss, d mu, d logvar or None) of branch b in fp64, computed once per case."""
    return _ref_of(n, d, sim, _salt(n, d, sim), loss_name, ps, b)


def _heads(br, d):
    (mu_c, lv_c), (mu_s, lv_s), _ = br
    return torch.cat([mu_c, lv_c, mu_s, lv_s], dim=1).float().cuda().contiguous()


def _prefill(n, d, scales):
    """[n][4d], deterministic, no zero of either sign: block q (of width d) is +-scales[q] * (0.5 .. 1.5)."""
    i = torch.arange(n, dtype=torch.float64)[:, None]
    j = torch.arange(4 * d, dtype=torch.float64)[None, :]
    mag = 0.5 + ((7 * i + 13 * j) % 17) / 17.0
    sign = 1.0 - 2.0 * ((3 * i + 5 * j) % 2)
    sc = torch.tensor(scales, dtype=torch.float64).repeat_interleave(d)[None, :]
    out = (mag * sign * sc).float()
    assert bool((out != 0).all())
    return out.cuda().contiguous()


def _scales(refs, ups, d, sim):
    """The pre-fill's magnitude per [mu_c, lv_c, mu_s, lv_s] block: the largest expected gradient element there."""
    out = []
    for b in range(2):
        for g in (refs[b][1], refs[b][2]) if b < len(refs) else (None, None):
            m = float(g.abs().max()) * abs(ups[b]) if g is not None else 0.0
            out.append(m if m > 0 and m == m else 1.0)
    return out


class _Call:
    """One cv_supcon_step setup over heads / dheads: the branch array with everything it points to kept alive."""

    def __init__(self, heads, dheads, label, n, d, sim, kind, ps, gmul, gscale, nbr=2, with_lv=True):
        from cvhip import _lib

        self.L = _lib.lib()
        self._lib = _lib
        self.n, self.d, self.sim, self.kind, self.nbr = n, d, sim, kind, nbr
        self.lab = label.cuda()
        self.gscale = torch.tensor([gscale], dtype=torch.float32, device="cuda")
        self.stats = torch.zeros(2, int(self.L.cv_supcon_stats_floats(n)), dtype=torch.float32, device="cuda")
        self.loss = torch.full((2,), 12345.0, dtype=torch.float32, device="cuda")
        hb, dh = heads.data_ptr(), dheads.data_ptr()
        self.keep = (heads, dheads)
        brs = []
        for b in range(2):
            o = 8 * b * d  # bytes: the style branch starts at column 2d
            brs.append(_lib.cv_supcon_branch(hb + o, hb + o + 4 * d if with_lv else None, 4 * d, int(ps[b]),
                                             dh + o, dh + o + 4 * d, 4 * d, self.gscale.data_ptr(), float(gmul[b]),
                                             self.loss.data_ptr() + 4 * b, self.stats[b].data_ptr()))
        self.arr = (_lib.cv_supcon_branch * 2)(*brs)

    def phase(self, ph):
        rc = self.L.cv_supcon_step(self.arr, self.nbr, self.lab.data_ptr(), self.n, self.d, self._lib.SIM[self.sim],
                                   self.kind, ctypes.c_float(TAU), ph, self._lib.stream_handle())
        self._lib.check(rc, "cv_supcon_step")

    def run(self):
        self.phase(0)
        self.phase(1)
        torch.cuda.synchronize()
        return self.loss.cpu()


def _check_branch(tag, loss, delta_mu, delta_lv, ref, up, sim):
    rloss, rgm, rgl = ref
    if rloss != rloss:  # no kept row: NaN and nothing added
        assert loss != loss, (tag, loss)
        assert not delta_mu.any() and not delta_lv.any(), tag
        return
    e_loss = abs(loss - rloss) / max(abs(rloss), 1e-3)
    e_mu = _rel(delta_mu, up * rgm)
    e_lv = _rel(delta_lv, up * rgl) if sim in USES_LV else 0.0
    print(f"SUPCON_STEP {tag} loss={loss:.7g} ref={rloss:.7g} e_loss={e_loss:.3g} e_dmu={e_mu:.3g} e_dlv={e_lv:.3g}")
    assert abs(loss - rloss) <= 1e-4 * max(abs(rloss), 1e-3), (tag, loss, rloss)
    assert e_mu < 1e-4, (tag, "dmu", e_mu)
    if sim in USES_LV:
        assert e_lv < 1e-4, (tag, "dlogvar", e_lv)


def _run_case(n, d, sim, loss_name, ps, nbr, gmul, gscale, refs=None, br=None):
    """Both phases over a pre-filled dheads; the losses, the fp64 difference per block and the untouched columns."""
    from cvhip import _lib

    br = br or _branches(n, d, sim)
    # branch 0 takes `ps`, branch 1 the other value (the step's content branch has ps = 0, its style branch the
    # trainer's; over the table's two `ps` values both branches see both); branch 1's gmul is negated
    pss = (ps, not ps)
    gm = (gmul, -gmul)
    refs = refs or [_ref(n, d, sim, loss_name, pss[b], b) for b in range(nbr)]
    ups = [gm[b] * gscale for b in range(2)]
    heads = _heads(br, d)
    before = _prefill(n, d, _scales(refs, ups, d, sim))
    dheads = before.clone()
    call = _Call(heads, dheads, br[2], n, d, sim, _lib.SUPCON[loss_name], pss, gm, gscale, nbr=nbr)
    loss = call.run()
    delta = (dheads.double() - before.double()).cpu()
    for b in range(nbr):
        c0 = 2 * b * d
        _check_branch(f"n={n} d={d} {sim} {loss_name} ps={int(pss[b])} b={b}/{nbr} up={ups[b]:g}", float(loss[b]),
                      delta[:, c0:c0 + d], delta[:, c0 + d:c0 + 2 * d], refs[b], ups[b], sim)
        if sim not in USES_LV:  # cosine / l2: the logvar columns keep their bits
            assert torch.equal(dheads[:, c0 + d:c0 + 2 * d], before[:, c0 + d:c0 + 2 * d])
    if nbr == 1:  # the style columns are not the call's
        assert torch.equal(dheads[:, 2 * d:], before[:, 2 * d:])
        assert float(loss[1]) == 12345.0
    return loss, dheads


# ----------------------------------------------------------------------------- 1.-3. the table

SHAPES = [(2, 8), (5, 3), (66, 8), (257, 32), (33, 33)]
TABLE = ([(n, d, s) for (n, d) in SHAPES for s in ("cosine", "jeffrey")]
         + [(66, 8, "l2"), (257, 32, "modified_l2"), (33, 33, "mahalanobis")])


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,d,sim", TABLE)
def test_table(n, d, sim, loss_name, ps):
    """Every (nbr, gmul, gscale) combination of the case: nbr = 1 leaves the style columns bit-identical, cosine / l2
    leave the logvar columns bit-identical (_run_case)."""
    for nbr in (1, 2):
        for gmul in (100.0, -100.0):
            for gscale in (1.0, 0.5):
                _run_case(n, d, sim, loss_name, ps, nbr, gmul, gscale)


def test_null_logvar_is_allowed_for_cosine_and_l2():
    from cvhip import _lib

    n, d = 66, 8
    for sim in ("cosine", "l2"):
        br = _branches(n, d, sim)
        heads = _heads(br, d)
        outs = []
        for with_lv in (True, False):
            dheads = _prefill(n, d, [1.0] * 4)
            call = _Call(heads, dheads, br[2], n, d, sim, _lib.SUPCON_IN, (0, 1), (100.0, 100.0), 1.0, with_lv=with_lv)
            outs.append((call.run(), dheads))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- 4. the tiled variant


@pytest.mark.parametrize("n,sim,loss_name", [(4097, "cosine", "supcon_in_loss"),
                                             (2049, "modified_l2", "supcon_out_loss")])
def test_tiled_variant_at_its_threshold(n, sim, loss_name):
    """d = 8, the smallest n whose rows do not fit the LDS: the tiled step kernels (read from the launch log), both
    branches on the inputs of tests/test_gpu_supcon.py's blockwise fp64 reference (ps = 0 and ps = 1 of one pass)."""
    from cvhip import _lib

    d = 8
    assert _full(n - 1, d, sim) and not _full(n, d, sim)
    (mu, lv, label), ref = _big_reference(n, d, sim, TAU)
    br = ((mu, lv), (mu, lv), label)
    refs = [ref[(loss_name, False)], ref[(loss_name, True)]]
    with _KernelLog() as log:
        _run_case(n, d, sim, loss_name, False, 2, 100.0, 1.0, refs=refs, br=br)
    names = [nm for nm in log.names if "sc_step_" in nm]
    assert len(names) == 3 and all("sc_step_loss" in nm or "<8, false>" in nm for nm in names), log.names
    assert _lib.lib().cv_supcon_supported(n, d, _lib.SIM[sim]) == 1


# ----------------------------------------------------------------------------- 5. no kept row


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("distinct,ps", [(True, False), (False, True)])
@pytest.mark.parametrize("sim", ["cosine", "jeffrey"])
def test_no_kept_row(sim, distinct, ps, loss_name):
    """All labels distinct under ps = 0, all equal under ps = 1: no positive anywhere, both branches.  NaN losses and
    a dheads that equals its pre-fill."""
    from cvhip import _lib

    n, d = 37, 8
    br = _branches(n, d, sim)
    label = torch.arange(n) if distinct else torch.zeros(n, dtype=torch.int64)
    rloss, _, _ = _oracle(br[0][0], br[0][1], label, sim, TAU, loss_name, ps)
    assert rloss != rloss
    heads = _heads(br, d)
    before = _prefill(n, d, [1.0, 0.25, 3.0, 1e-3])
    dheads = before.clone()
    call = _Call(heads, dheads, label, n, d, sim, _lib.SUPCON[loss_name], (ps, ps), (100.0, -100.0), 1.0)
    loss = call.run()
    assert bool(torch.isnan(loss).all()), loss
    assert torch.equal(dheads, before)


# ----------------------------------------------------------------------------- 6. bit-identical repeats


@pytest.mark.parametrize("loss_name", LOSSES)
@pytest.mark.parametrize("n,d,sim", [(257, 32, "jeffrey"), (2049, 8, "modified_l2")])
def test_two_runs_are_bit_identical(n, d, sim, loss_name):
    from cvhip import _lib

    br = _draw(n, d, sim, 0)  # (no reference needed)
    heads = _heads(br, d)
    outs = []
    for _ in range(2):
        dheads = _prefill(n, d, [1.0, 0.5, 2.0, 0.1])
        call = _Call(heads, dheads, br[2], n, d, sim, _lib.SUPCON[loss_name], (0, 1), (100.0, -100.0), 1.0)
        outs.append((call.run(), dheads))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


# ----------------------------------------------------------------------------- 7. the launch log


@pytest.mark.parametrize("loss_name", LOSSES)
def test_a_step_is_at_most_three_launches(loss_name):
    from cvhip import _lib

    n, d, sim = 66, 8, "cosine"
    br = _branches(n, d, sim)
    dheads = _prefill(n, d, [1.0] * 4)
    call = _Call(_heads(br, d), dheads, br[2], n, d, sim, _lib.SUPCON[loss_name], (0, 1), (100.0, 100.0), 1.0)
    with _KernelLog() as log:
        call.run()
    names = [nm for nm in log.names if nm]
    assert 1 <= len(names) <= 3, names
    assert all("sc_step_" in nm for nm in names), names
    assert not any("nt_" in nm or "ntxent" in nm for nm in names), names


# ----------------------------------------------------------------------------- 8. host validation


def test_host_validation_rejects_before_any_launch():
    from cvhip import _lib

    L = _lib.lib()
    n, d = 16, 8
    heads = torch.randn(n, 4 * d, device="cuda")
    dheads = torch.zeros(n, 4 * d, device="cuda")
    lab = torch.zeros(n, dtype=torch.int64, device="cuda")
    gs = torch.ones(1, device="cuda")
    loss = torch.zeros(2, device="cuda")
    stats = torch.zeros(2, int(L.cv_supcon_stats_floats(n)), device="cuda")
    hb, dh = heads.data_ptr(), dheads.data_ptr()

    def branch(b=0, **over):
        o = 8 * b * d
        f = dict(mu=hb + o, logvar=hb + o + 4 * d, ld=4 * d, ps=0, dmu=dh + o, dlogvar=dh + o + 4 * d, gld=4 * d,
                 gscale=gs.data_ptr(), gmul=100.0, loss_out=loss.data_ptr() + 4 * b, stats=stats[b].data_ptr())
        f.update(over)
        return _lib.cv_supcon_branch(*[f[k] for k, _ in _lib.cv_supcon_branch._fields_])

    def call(brs, nbr=2, label=lab.data_ptr(), n_=n, d_=d, sim=0, kind=0, tau=0.1, phase=0):
        arr = (_lib.cv_supcon_branch * 2)(*brs)
        return L.cv_supcon_step(arr, nbr, label, n_, d_, sim, kind, ctypes.c_float(tau), phase, _lib.stream_handle())

    good = [branch(0), branch(1)]
    bad = {
        "nbr=0": dict(nbr=0), "nbr=3": dict(nbr=3), "label": dict(label=None), "tau=0": dict(tau=0.0),
        "tau<0": dict(tau=-0.1), "kind": dict(kind=2), "sim=-1": dict(sim=-1), "sim=5": dict(sim=5),
        "phase=2": dict(phase=2), "phase=-1": dict(phase=-1), "n=0": dict(n_=0), "d=65": dict(d_=65),
        "n too large": dict(n_=131073),
    }
    bad_branch = {
        "mu": (dict(mu=None), {}), "stats": (dict(stats=None), {}), "logvar jeffrey": (dict(logvar=None), dict(sim=3)),
        "ld<d": (dict(ld=d - 1), {}), "phase 1 dmu": (dict(dmu=None), dict(phase=1)),
        "phase 1 gscale": (dict(gscale=None), dict(phase=1)), "phase 1 gld<d": (dict(gld=d - 1), dict(phase=1)),
        "phase 0 loss_out": (dict(loss_out=None), {}),
    }
    with _KernelLog() as log:
        for tag, kw in bad.items():
            assert call(good, **kw) != 0, tag
            assert L.cv_last_error(), tag
        for tag, (over, kw) in bad_branch.items():
            for b in (0, 1):  # in either slot
                brs = [branch(0, **over) if b == 0 else branch(0), branch(1, **over) if b == 1 else branch(1)]
                assert call(brs, **kw) != 0, (tag, b)
                assert L.cv_last_error(), (tag, b)
        assert L.cv_supcon_step(None, 2, lab.data_ptr(), n, d, 0, 0, ctypes.c_float(0.1), 0, None) != 0
        torch.cuda.synchronize()
    assert [nm for nm in log.names if nm] == [], log.names
    # a bad second slot is not looked at when nbr = 1, and the good set runs
    assert call([branch(0), branch(1, mu=None)], nbr=1) == 0
    assert call(good) == 0 and call(good, phase=1) == 0
    torch.cuda.synchronize()
