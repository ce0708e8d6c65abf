"""cv_blobs / cv_snn_bounds (csrc/cv_bound.hip), cvhip.bounds and src.utils.mi_bounds on the device.

The bounds are compared with tests/bound_ref.py (fp64, tied to the reference notebook by tests/test_mi_bounds_ref.py)
on the same fp32 inputs:

    bound:  |got - ref| <= 1e-4 |ref| + 2 (d + 4) 2^-24 / tau
    rows:   |got - ref| <= 1e-5 max(|ref|, 1) + 2 (d + 4) 2^-24 / tau, and -inf exactly where the reference has -inf
    count:  equal, always (a kernel cannot hide a wrong row by dropping it)

The first term is the project's NT-Xent bar (test_gpu_ntxent_matrix.py).  The second propagates fp32 rounding: a
normalised d-term fp32 dot product is off by at most about (d + 4) 2^-24, every log-sum-exp is 1-Lipschitz in its
arguments s / tau, and a bound is the difference of two of them.  NaN compares as NaN with count 0."""

import functools
import os

import numpy as np
import pytest
import torch

import bound_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mi_bounds.npz")
CASES = ("blobs", "antipodal", "antipodal_singletons", "d1", "one_label", "wide_labels", "zero_row")
# the kernel's tiles (cv_bound.hip): BD_NT rows of i per workgroup, bd_tj<DM>() streamed points of j per LDS tile
ROW_TILE = 256
STREAM_TILE = {8: 512, 16: 256, 32: 128, 64: 64}  # by d class (d <= 8, 16, 32, 64)
TAUS4 = (0.01, 0.1, 0.3, 1.0)
TAUS8 = (0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0, 2.0)


def bound_tol(ref, d, tau):
    return 1e-4 * abs(ref) + 2 * (d + 4) * 2.0 ** -24 / tau


def check_bounds(snn, pssnn, count, x, label, taus, what=""):
    """(snn, pssnn, count) of the device against bound_ref, trial by trial; x [B, n, d] fp32, label [n] or [B, n]."""
    got = torch.stack([snn, pssnn], dim=-1).cpu().numpy()
    cnt = count.cpu().numpy()
    x, label = np.asarray(x), np.asarray(label)
    B, n, d = x.shape
    assert got.shape == (B, len(taus), 2) and got.dtype == np.float64 and cnt.shape == got.shape
    for b in range(B):
        ref, rc, _ = bound_ref.bounds(x[b], label[b] if label.ndim == 2 else label, taus)
        assert np.array_equal(cnt[b], rc), (what, b, cnt[b], rc)
        assert np.array_equal(np.isnan(got[b]), np.isnan(ref)), (what, b, got[b], ref)
        for t, tau in enumerate(taus):
            for c in range(2):
                if not np.isnan(ref[t, c]):
                    err, tol = abs(got[b, t, c] - ref[t, c]), bound_tol(ref[t, c], d, tau)
                    assert err <= tol, (what, b, tau, c, got[b, t, c], ref[t, c], err, tol)


@functools.lru_cache(maxsize=None)
def make_inputs(B, n, d, seed=0, classes=3):
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    label = rng.integers(0, classes, n)
    x = (rng.standard_normal((B, n, d)) + 0.7 * label[None, :, None]).astype(np.float32)
    x.setflags(write=False)
    label.setflags(write=False)
    return x, label


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------- 1. the golden cases
@pytest.mark.parametrize("case", CASES)
def test_golden_cases(golden, case):
    from cvhip.bounds import snn_bounds

    x, label, taus = golden[case + "__x"], golden[case + "__label"], golden["taus"].tolist()
    n, d = x.shape
    snn, ps, count, rows = snn_bounds(dev(x), dev(label), taus, return_rows=True)
    check_bounds(snn, ps, count, x[None], label, taus, case)
    # the notebook's own values and counts (fp64 on the same fp32 inputs)
    got = torch.stack([snn, ps], dim=-1).cpu().numpy()[0]
    want, want_count = golden[case + "__value"], golden[case + "__count"]
    assert np.array_equal(count.cpu().numpy()[0], want_count)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for t, tau in enumerate(taus):
        for c in range(2):
            if not np.isnan(want[t, c]):
                assert abs(got[t, c] - want[t, c]) <= bound_tol(want[t, c], d, tau), (case, tau, c, got[t, c], want[t, c])
    # the row values
    _, _, ref_rows = bound_ref.bounds(x, label, taus)
    r = rows.cpu().numpy()[0].astype(np.float64)
    assert r.shape == (len(taus), 3, n)
    for t, tau in enumerate(taus):
        ninf = np.isneginf(ref_rows[t])
        assert np.array_equal(np.isneginf(r[t]), ninf), (case, tau)
        tol = 1e-5 * np.maximum(np.abs(ref_rows[t][~ninf]), 1.0) + 2 * (d + 4) * 2.0 ** -24 / tau
        err = np.abs(r[t][~ninf] - ref_rows[t][~ninf])
        assert (err <= tol).all(), (case, tau, err.max(), tol.min())


# ---------------------------------------------------------------- 2. shapes across the tile boundaries
SHAPES = [
    (3, 2, 3, TAUS4),
    (3, 5, 3, TAUS4),
    (3, ROW_TILE + 1, 3, TAUS4[1:2]),             # one more than the row tile, T = 1
    (3, STREAM_TILE[8] + 1, 3, TAUS4),            # one more than the streamed tile, d = 3 (and three row tiles)
    (3, STREAM_TILE[64] + 1, 64, TAUS8),          # one more than the streamed tile, d = 64, T = 8
    (3, STREAM_TILE[16] + 1, 12, TAUS4),          # the d <= 16 class
    (3, STREAM_TILE[32] + 1, 17, TAUS8),          # the d <= 32 class
    (3, 40, 1, TAUS4),
    (3, 40, 5, TAUS4),
    (300, 6, 3, TAUS4),
]


@pytest.mark.parametrize("B, n, d, taus", SHAPES, ids=[f"B{s[0]}-n{s[1]}-d{s[2]}-T{len(s[3])}" for s in SHAPES])
def test_shapes(B, n, d, taus):
    from cvhip.bounds import snn_bounds

    x, label = make_inputs(B, n, d)
    snn, ps, count = snn_bounds(dev(x), dev(label), taus)
    check_bounds(snn, ps, count, x, label, taus, (B, n, d))


def test_more_trials_than_a_grid_dimension_holds():
    """B = 70000 > 65535: trials on both sides of the y / z grid limit have the bits of the single-trial call."""
    from cvhip.bounds import snn_bounds

    B, n, d = 70000, 4, 3
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, n, d, generator=g, device="cuda")
    label = dev([0, 0, 1, 1])
    snn, ps, count = snn_bounds(x, label, TAUS4)
    assert int(count.min()) == n and bool(torch.isfinite(snn).all()) and bool(torch.isfinite(ps).all())
    pick = [0, 65534, 65535, 65536, B - 1]
    for b in pick:
        s1, p1, c1 = snn_bounds(x[b], label, TAUS4)
        assert torch.equal(s1[0], snn[b]) and torch.equal(p1[0], ps[b]) and torch.equal(c1[0], count[b])
    check_bounds(snn[pick], ps[pick], count[pick], x[pick].cpu().numpy(), [0, 0, 1, 1], TAUS4)


# ---------------------------------------------------------------- 3. labels
def test_shared_and_per_trial_labels():
    from cvhip.bounds import snn_bounds

    B, n, d = 3, 70, 5
    x, label = make_inputs(B, n, d)
    xd = dev(x)
    a = snn_bounds(xd, dev(label), TAUS4)
    b = snn_bounds(xd, dev(np.tile(label, (B, 1))), TAUS4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # labels that differ per trial
    lab2 = np.stack([label, (label + np.arange(n) % 2) % 3, np.roll(label, 5)])
    check_bounds(*snn_bounds(xd, dev(lab2), TAUS4), x, lab2, TAUS4, "per-trial labels")
    # int32 labels are taken too
    c = snn_bounds(xd, dev(label, torch.int32), TAUS4)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


def test_row_shuffle_changes_nothing_beyond_rounding():
    from cvhip.bounds import snn_bounds

    B, n, d = 3, 300, 3
    x, label = make_inputs(B, n, d)
    rng = np.random.default_rng(4)
    perm = np.stack([rng.permutation(n) for _ in range(B)])
    xs = np.stack([x[b][perm[b]] for b in range(B)])
    ls = np.stack([label[perm[b]] for b in range(B)])
    a = snn_bounds(dev(x), dev(label), TAUS4)
    s = snn_bounds(dev(xs), dev(ls), TAUS4)
    assert torch.equal(a[2], s[2])
    for k in range(2):
        u, v = a[k].cpu().numpy(), s[k].cpu().numpy()
        for t, tau in enumerate(TAUS4):
            for b in range(B):
                assert abs(u[b, t] - v[b, t]) <= bound_tol(u[b, t], d, tau), (k, b, tau, u[b, t], v[b, t])


# ---------------------------------------------------------------- 4. strides
def test_strides_give_the_same_bits():
    from cvhip.bounds import snn_bounds

    B, n, d = 3, 130, 5
    x, label = make_inputs(B, n, d)
    xd, lab = dev(x), dev(label)
    base = snn_bounds(xd, lab, TAUS4, return_rows=True)
    perm = xd.permute(1, 0, 2).contiguous().permute(1, 0, 2)  # [n, B, d] storage
    assert perm.stride() == (d, B * d, 1)
    wide = torch.full((B, n, d + 3), float("nan"), device="cuda")
    wide[..., :d] = xd
    for other in (perm, wide[..., :d]):
        assert not other.is_contiguous()
        got = snn_bounds(other, lab, TAUS4, return_rows=True)
        for u, v in zip(base, got):
            assert torch.equal(u, v)
    # a stride along d that is not 1 is made contiguous
    col = xd.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert col.stride(2) != 1
    for u, v in zip(base, snn_bounds(col, lab, TAUS4, return_rows=True)):
        assert torch.equal(u, v)


# ---------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_nan_stays_in_its_trial(bad):
    from cvhip.bounds import snn_bounds

    B, n, d = 3, 300, 3
    x, label = make_inputs(B, n, d)
    xd, lab = dev(x), dev(label)
    clean = snn_bounds(xd, lab, TAUS4)
    xb = xd.clone()
    xb[1, 270, 1] = bad
    snn, ps, count = snn_bounds(xb, lab, TAUS4)
    assert bool(torch.isnan(snn[1]).all()) and bool(torch.isnan(ps[1]).all()) and int(count[1].abs().max()) == 0
    for b in (0, 2):
        assert torch.equal(snn[b], clean[0][b]) and torch.equal(ps[b], clean[1][b])
        assert torch.equal(count[b], clean[2][b])
    if bad != bad:
        xn = x.copy()
        xn[1, 270, 1] = bad
        check_bounds(snn, ps, count, xn, label, TAUS4, "nan")


# ---------------------------------------------------------------- 6. determinism
def test_deterministic_and_batch_independent():
    from cvhip.bounds import snn_bounds

    B, n, d = 3, STREAM_TILE[8] + 1, 3
    x, label = make_inputs(B, n, d)
    xd, lab = dev(x), dev(label)
    a = snn_bounds(xd, lab, TAUS4, return_rows=True)
    b = snn_bounds(xd.clone(), lab.clone(), TAUS4, return_rows=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for t in range(B):
        one = snn_bounds(xd[t], lab, TAUS4, return_rows=True)
        for u, v in zip(a, one):
            assert torch.equal(u[t], v[0])


# ---------------------------------------------------------------- 7. the modules
def test_modules():
    from cvhip.bounds import snn_bounds
    from src.utils.mi_bounds import PSSNN, SNN

    B, n, d = 3, 96, 3
    x, label = make_inputs(B, n, d)
    xd, lab = dev(x), dev(label)
    taus = (0.1, 0.3, 1.0)
    snn, ps, _ = snn_bounds(xd, lab, taus)
    for t, tau in enumerate(taus):
        for cls, batched in ((SNN, snn), (PSSNN, ps)):
            m = cls(tau).cuda()
            v3 = m(xd, lab)
            assert v3.shape == (B,) and v3.dtype == torch.float64 and torch.equal(v3, batched[:, t])
            for b in range(B):
                v2 = float(m(xd[b], lab))  # the cv_ntxent path
                ref = float(batched[b, t])
                print(cls.__name__, tau, b, v2, ref)
                assert abs(v2 - ref) <= bound_tol(ref, d, tau), (cls.__name__, tau, b, v2, ref)
    x2 = xd[0].clone().requires_grad_(True)
    for cls in (SNN, PSSNN):
        x2.grad = None
        cls(0.3)(x2, lab).backward()
        assert bool(torch.isfinite(x2.grad).all()) and float(x2.grad.abs().max()) > 0
    x3 = xd.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        SNN(0.3)(x3, lab)
    with torch.no_grad():
        assert torch.equal(SNN(0.3)(x3, lab), snn[:, 1])


def test_the_notebook_loop_body_runs_unchanged():
    from cvhip import rng
    from src.utils.mi_bounds import PSSNN, generate_gaussian_blobs

    torch.manual_seed(3)
    rng.reset_counters()
    pssnn = PSSNN(tau=0.3).cuda()
    x, y = generate_gaussian_blobs(n_samples=150, centers=[-1., 2., 7.], cluster_std=np.float64(2.5))
    assert x.shape == (150, 3) and y.shape == (150,) and x.is_cuda and y.is_cuda and y.dtype == torch.int64
    indices = torch.randperm(x.size(0))
    x, y = x[indices].cuda(), y[indices].cuda()
    v = float(pssnn(x, y))
    ref, cnt, _ = bound_ref.bounds(x.cpu().numpy(), y.cpu().numpy(), [0.3])
    assert cnt[0, 1] == 150 and abs(v - ref[0, 1]) <= bound_tol(ref[0, 1], 3, 0.3)
    xb, yb = generate_gaussian_blobs(n_samples=150, cluster_std=[1.0, 2.0])
    assert xb.shape == (2, 150, 3) and yb.shape == (150,)


# ---------------------------------------------------------------- blobs
CENTERS = np.array([-1.0, 2.0, 7.0])


def _draw(stds=(1.0, 2.0, 3.0, 4.0), n=1536):
    from cvhip.bounds import gaussian_blobs

    return gaussian_blobs(list(stds), n)


def test_blobs_are_standard_normal_around_their_centres():
    import math

    from scipy import stats

    from cvhip import rng

    torch.manual_seed(11)
    rng.reset_counters()
    stds, n, d = (1.0, 2.0, 3.0, 4.0), 1536, 3
    x, label = _draw(stds, n)
    B = len(stds)
    assert x.shape == (B, n, d) and x.dtype == torch.float32 and x.stride() == (d, B * d, 1)
    assert x.permute(1, 0, 2).reshape(n, B * d).data_ptr() == x.data_ptr()  # the free view knn_mi takes
    lab = label.cpu().numpy()
    assert np.array_equal(lab, np.arange(n) // (n // 3)) and label.dtype == torch.int64
    z = (x.double().cpu().numpy() - CENTERS[lab][None, :, None]) / np.array(stds)[:, None, None]
    assert np.isfinite(z).all()
    for v in [z.reshape(-1)] + [z[b].reshape(-1) for b in range(B)]:
        N = v.size
        assert abs(v.mean()) < 5 / math.sqrt(N), v.mean()
        assert abs(v.var() - 1) < 5 * math.sqrt(2 / N), v.var()
        assert stats.kstest(v, "norm").pvalue > 1e-6
    # the dimensions of a trial and the trials among each other: the [n, B d] columns are pairwise uncorrelated
    c = np.corrcoef(z.transpose(1, 0, 2).reshape(n, B * d), rowvar=False)
    off = np.abs(c[~np.eye(B * d, dtype=bool)])
    assert off.max() < 5 / math.sqrt(n), off.max()
    # a second call draws fresh blobs (the counter advanced on the device)
    x2, _ = _draw(stds, n)
    assert not torch.equal(x, x2)
    z2 = (x2.double().cpu().numpy() - CENTERS[lab][None, :, None]) / np.array(stds)[:, None, None]
    r = np.corrcoef(z.reshape(-1), z2.reshape(-1))[0, 1]
    assert abs(r) < 5 / math.sqrt(z.size), r
    # the seed and the counters reproduce the first call bit for bit
    torch.manual_seed(11)
    rng.reset_counters()
    x3, _ = _draw(stds, n)
    assert torch.equal(x, x3)
    # a device tensor of stds is the same draw
    torch.manual_seed(11)
    rng.reset_counters()
    from cvhip.bounds import gaussian_blobs

    x4, _ = gaussian_blobs(dev(stds, torch.float32), n)
    assert torch.equal(x, x4)
    with pytest.raises(ValueError):
        gaussian_blobs(dev([1.0, -1.0], torch.float32), n)


def test_blob_layout_matches_the_notebook(golden):
    from cvhip.bounds import gaussian_blobs

    x, label = gaussian_blobs([1.0], 100)
    assert x.shape == (1, 99, 3) == (1, int(golden["blob_rows_100_3"]), 3)
    assert np.array_equal(label.cpu().numpy(), golden["blob_label_100_3"])
    x, label = gaussian_blobs([1.0, 2.0], 96, dim=2, centers=(-1.0, 2.0, 7.0, 11.0), n_blobs=4)
    assert x.shape == (2, int(golden["blob_rows_96_4"]), 2)
    assert np.array_equal(label.cpu().numpy(), golden["blob_label_96_4"])
    m = x[0].double().cpu().numpy().reshape(4, 24, 2).mean(axis=(1, 2))
    assert np.abs(m - np.array([-1.0, 2.0, 7.0, 11.0])).max() < 5 / np.sqrt(48)


def test_blobs_fill_exactly_their_output():
    """[B][n][d] storage through out=, an odd number of elements (the last Philox draw is half used) and a guard behind
    the output that must stay untouched."""
    from cvhip.bounds import gaussian_blobs

    for B, n, d in ((1, 3, 1), (3, 33, 5), (2, 1536, 3)):
        total = B * n * d
        buf = torch.full((total + 64,), float("nan"), device="cuda")
        out = buf[:total].view(B, n, d)
        x, label = gaussian_blobs([1.0 + b for b in range(B)], n, dim=d, out=out)
        assert x.data_ptr() == buf.data_ptr()
        assert bool(torch.isfinite(buf[:total]).all()) and bool(torch.isnan(buf[total:]).all())
        z = (out.double().cpu().numpy() - CENTERS[label.cpu().numpy()][None, :, None]) / \
            (1.0 + np.arange(B))[:, None, None]
        assert abs(z.mean()) < 5 / np.sqrt(total) and (total < 100 or abs(z.var() - 1) < 5 * np.sqrt(2 / total))


# ---------------------------------------------------------------- the sweep
def test_sweep():
    from knn_mi_oracle import knn_mi_oracle

    from cvhip import rng
    from cvhip.bounds import gaussian_blobs, snn_bounds
    from cvhip.metrics import knn_mi
    from src.utils.mi_bounds import mi_bound_sweep

    stds, R, taus = (1.0, 4.0), 3, (0.1, 0.3, 0.5, 1.0)
    torch.manual_seed(21)
    rng.reset_counters()
    res = mi_bound_sweep(stds, repeats=R, n_samples=96)
    B = len(stds) * R
    assert res["std"].cpu().tolist() == [1.0, 1.0, 1.0, 4.0, 4.0, 4.0]  # the std outer, the repeat inner
    assert res["knn_mi"].shape == (B, 3) and res["knn_mi"].dtype == torch.float64
    assert res["snn"].shape == (B, 4) == res["pssnn"].shape and res["snn"].dtype == torch.float64
    assert res["count"].shape == (B, 4, 2) and res["taus"] == taus
    assert all(res[k].is_cuda for k in ("std", "knn_mi", "snn", "pssnn", "count"))
    # the same blobs again
    torch.manual_seed(21)
    rng.reset_counters()
    x, label = gaussian_blobs([s for s in stds for _ in range(R)], 96)
    snn, ps, count = snn_bounds(x, label, taus)
    assert torch.equal(snn, res["snn"]) and torch.equal(ps, res["pssnn"]) and torch.equal(count, res["count"])
    check_bounds(snn, ps, count, x.cpu().numpy(), label.cpu().numpy(), taus, "sweep")
    lab = label.cpu().numpy()
    for b in range(B):
        assert torch.equal(knn_mi(x[b], label), res["knn_mi"][b])
        ref = knn_mi_oracle(x[b].cpu().numpy(), lab, 3)[0]
        assert np.abs(res["knn_mi"][b].cpu().numpy() - ref).max() <= 1e-9  # test_gpu_knn_mi.py's MI_TOL
    # tighter blobs carry more information about their label
    assert float(res["knn_mi"][:R].mean()) > float(res["knn_mi"][R:].mean())
