"""cvhip.tsne on the device (csrc/cv_tsne.hip) against the fp64 restatement tests/tsne_ref.py, which
tests/test_tsne_ref.py holds against sklearn's own functions.

Cases (tsne_ref.case): min N=4 D=1 perplexity 2; n257 N=257 D=5 at perplexity 30 and 5 (ragged tiles); d64 N=300 D=64;
d20 N=130 D=20 (the 32-column build of the kernels; the others cover 4, 8, 16 and 64); n1000 N=1000 D=3 (several row
tiles and slabs of j); n4096 N=4096 D=16; dups N=128 with 16 duplicated rows and a constant column; scaled = n257 times
1e3 and 1e-3 (the doubling and the halving branch of the search); view = the left 5 columns of a [257, 9] tensor.  The
restatement's search converges on every row of every case (asserted).

Bars.  Those the definition fixes:
  H            |H_i(beta_i of the device, in fp64) - ln perplexity| <= 2e-5: sklearn's 1e-5 stopping rule plus as much
               again for the kernel's own evaluation of H (fp64 sums of fp32 exponentials)
Those measured on an MI355X against the restatement, set to 8 x the largest error over the cases and capped:
  logz         |logz_i - ln S_i(beta_i)|                       measured 7.9e-7, bar 6.3e-6 (cap 1e-5)
  gradient     max|grad - ref| / max|ref|                      measured 2.4e-6, bar 1.9e-5 (cap 1e-4)
  KL           |kl - ref| / |ref|                              measured 8.2e-7, bar 6.5e-6 (cap 1e-5)
  trajectory   max|Y - ref| / max|ref| after 5 and 2 + 4 its   measured 1.8e-6, bar 1.4e-5 (cap 5e-3)
(the largest H error measured was 1.02e-5, of which 1e-5 is the search's own window).
kl_grad and the trajectories are compared with the restatement evaluated at the device's own (beta, logz), so the
1e-5 window of the search does not enter.  Every test prints its figures before it asserts."""

import functools

import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu

MEASURED_LOGZ, LOGZ_BAR = 7.9e-7, 6.3e-6    # largest at n257_p5 (logz down to -12.4 in fp32)
MEASURED_GRAD, GRAD_BAR = 2.4e-6, 1.9e-5    # largest at n1000, late embedding; 8e-8 .. 2e-7 at the init
MEASURED_KL, KL_BAR = 8.2e-7, 6.5e-6        # largest at dups, late embedding
MEASURED_TRAJ, TRAJ_BAR = 1.8e-6, 1.4e-5    # largest at d64 after 5 iterations; 1e-7 .. 4e-7 across the switch
H_BAR = 2e-5

NAMES = ["min", "n257", "n257_p5", "d64", "d20", "n1000", "n4096", "dups", "scaled_up", "scaled_down"]


@functools.lru_cache(maxsize=None)
def ref(name):
    """(X, perplexity, D): the case and its dense fp64 distances, computed once."""
    X, perplexity = R.case(name)
    return X, perplexity, R.sqdist(X)


@functools.lru_cache(maxsize=None)
def dev(name):
    """(x on the device, beta, logz on the device, their fp64 host copies, the restatement's P at them)."""
    from cvhip import tsne

    X, perplexity, D = ref(name)
    x = torch.as_tensor(X).cuda()
    beta, logz = tsne.affinities(x, perplexity)
    b, l = beta.cpu().numpy().astype(np.float64), logz.cpu().numpy().astype(np.float64)
    return x, beta, logz, b, l, R.joint_P(X, b, l, D)


@functools.lru_cache(maxsize=None)
def init(name):
    """The PCA initialisation at 1e-4 scale, rounded to fp32: what both sides start from."""
    return R.pca_init(ref(name)[0]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def late(name):
    """The restatement's embedding after 300 iterations (50 past the switch), rounded to fp32."""
    return R.descend(dev(name)[5], init(name), 300).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_affinities(name):
    X, perplexity, D = ref(name)
    _, _, _, conv = R.search_beta(X, perplexity, D)
    assert conv.all(), ("the restatement's search did not converge: change the input", np.flatnonzero(~conv))
    x, beta, logz, b, l, _ = dev(name)
    assert beta.dtype == logz.dtype == torch.float32 and beta.shape == logz.shape == (len(X),)
    assert beta.is_cuda and logz.is_cuda
    assert np.isfinite(b).all() and (b > 0).all() and np.isfinite(l).all()
    H, lnS = R.row_entropy(D, b)
    h_err, z_err = np.abs(H - np.log(perplexity)).max(), np.abs(l - lnS).max()
    print(f"{name}: max|H - ln perplexity| = {h_err:.3e} (bar {H_BAR}), max|logz - ln S| = {z_err:.3e} "
          f"(bar {LOGZ_BAR}), beta in [{b.min():.3e}, {b.max():.3e}], logz in [{l.min():.3f}, {l.max():.3f}]")
    assert h_err <= H_BAR
    assert z_err <= LOGZ_BAR


def _embeddings(name):
    if name == "n4096":
        return [("init", 1.0)]
    return [("init", 1.0), ("late", 1.0), ("late", 12.0)]


@pytest.mark.parametrize("name,which,exaggeration", [(n, w, e) for n in NAMES for w, e in _embeddings(n)])
def test_kl_grad(name, which, exaggeration):
    from cvhip import tsne

    x, beta, logz, _, _, P = dev(name)
    Y = init(name) if which == "init" else late(name)
    kl, grad = tsne.kl_grad(x, beta, logz, torch.as_tensor(Y).cuda(), exaggeration)
    assert kl.dtype == torch.float64 and kl.dim() == 0 and kl.is_cuda
    assert grad.dtype == torch.float32 and grad.shape == (len(Y), 2) and grad.is_cuda
    ref_kl, ref_grad = R.kl_grad(P, Y, exaggeration)
    g_err = np.abs(grad.cpu().numpy() - ref_grad).max() / np.abs(ref_grad).max()
    k_err = abs(float(kl) - ref_kl) / abs(ref_kl)
    print(f"{name} {which} e={exaggeration}: grad error / max|grad| = {g_err:.3e} (bar {GRAD_BAR}), "
          f"KL {float(kl):.12g} vs {ref_kl:.12g}: relative {k_err:.3e} (bar {KL_BAR})")
    assert g_err <= GRAD_BAR
    assert k_err <= KL_BAR


@pytest.mark.parametrize("name", ["n257", "dups", "d64"])
@pytest.mark.parametrize("n_iter,exploration", [(5, 250), (6, 2)])
def test_trajectory(name, n_iter, exploration):
    """Short on purpose: the early phase amplifies rounding (an fp32 emulation parts from fp64 by 6e-5 after 5
    iterations and by O(1) after 20).  6 iterations with exploration_iter=2 cross the reset of update and gains."""
    from cvhip import tsne

    x, beta, logz, _, _, P = dev(name)
    y0 = torch.as_tensor(init(name)).cuda()
    keep = y0.clone()
    y = tsne.descend(x, beta, logz, y0, n_iter, exploration_iter=exploration)
    assert torch.equal(y0, keep) and y.dtype == torch.float32 and y.shape == y0.shape and y.is_cuda
    want = R.descend(P, init(name), n_iter, exploration_iter=exploration)
    err = np.abs(y.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"{name} {n_iter} iterations, switch at {exploration}: error / max|Y| = {err:.3e} (bar {TRAJ_BAR})")
    assert err <= TRAJ_BAR
    # without the reset the restatement itself lands elsewhere: the test can tell
    if exploration < n_iter:
        assert np.abs(want - R.descend(P, init(name), n_iter, exploration_iter=n_iter)).max() > 0


def test_two_fits_are_bit_identical():
    from cvhip import tsne

    X = ref("n257")[0]
    a = tsne.TSNE(perplexity=30).fit(X)
    b = tsne.TSNE(perplexity=30).fit(X)
    assert a.embedding_.tobytes() == b.embedding_.tobytes()
    assert np.float64(a.kl_divergence_).tobytes() == np.float64(b.kl_divergence_).tobytes()
    assert np.isfinite(a.embedding_).all() and a.n_iter_ == 1000 and a.learning_rate_ == 50.0
    assert np.abs(a.embedding_).max() > 1.0  # it has left the 1e-4 initialisation


def test_a_strided_view_gives_the_bits_of_its_contiguous_copy():
    from cvhip import tsne

    wide = torch.as_tensor(R.view_case()).cuda()
    view = wide[:, :5]
    assert not view.is_contiguous() and view.stride(0) == 9
    copy = view.contiguous()
    assert torch.equal(copy, dev("n257")[0])
    bv, lv = tsne.affinities(view, 30.0)
    bc, lc = tsne.affinities(copy, 30.0)
    assert torch.equal(bv, bc) and torch.equal(lv, lc)
    y0 = torch.as_tensor(init("n257")).cuda()
    for a, b in zip(tsne.kl_grad(view, bv, lv, y0, 12.0), tsne.kl_grad(copy, bc, lc, y0, 12.0)):
        assert torch.equal(a, b)
    assert torch.equal(tsne.descend(view, bv, lv, y0, 6, exploration_iter=2),
                       tsne.descend(copy, bc, lc, y0, 6, exploration_iter=2))
    ev = tsne.TSNE(perplexity=30, max_iter=20, exploration_iter=10).fit_transform(view)
    ec = tsne.TSNE(perplexity=30, max_iter=20, exploration_iter=10).fit_transform(copy)
    assert ev.is_cuda and torch.equal(ev, ec)


def test_pca_init_matches_the_restatement():
    from cvhip import tsne

    for name in ("n257", "d64", "min"):
        got = tsne.pca_init(dev(name)[0])
        want = R.pca_init(ref(name)[0])
        assert got.dtype == torch.float32 and got.shape == want.shape and got.is_cuda
        err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"{name}: pca_init error / max|Y| = {err:.3e}")
        assert err <= 1e-5  # fp32 output (6e-8) and the eigenvectors of two fp64 solvers


def test_end_to_end_on_three_clusters():
    """The notebooks' call on 192 points in three clusters: every point's nearest neighbour in the embedding carries
    its own label, and the KL divergence of the embedding (fp64, the restatement's own P) is at most 1.05 x the worse
    of the restatement's own 1000 iterations and sklearn's method="exact" from init="pca" (0.3565 and 0.3625 with
    sklearn 1.7.2; sklearn's random inits spread by about 2 %)."""
    from sklearn.manifold import TSNE as SkTSNE

    from cvhip import tsne

    X, lab = R.three_clusters()
    D = R.sqdist(X)
    beta, logz, _, conv = R.search_beta(X, 30.0, D)
    assert conv.all()
    P = R.joint_P(X, beta, logz, D)

    model = tsne.TSNE(n_components=2, perplexity=30, learning_rate=200, init="pca")
    emb = model.fit_transform(X)
    assert isinstance(emb, np.ndarray) and emb.dtype == np.float32 and emb.shape == (192, 2)
    assert emb is model.embedding_ and model.n_iter_ == 1000 and model.learning_rate_ == 200.0
    assert np.isfinite(emb).all()

    E = R.sqdist(emb)
    np.fill_diagonal(E, np.inf)
    same = float((lab[E.argmin(axis=1)] == lab).mean())
    kl_dev = R.kl_grad(P, emb)[0]
    a = R.kl_grad(P, R.descend(P, R.pca_init(X).astype(np.float32), 1000, learning_rate=200.0))[0]
    sk = SkTSNE(n_components=2, perplexity=30, learning_rate=200, init="pca", method="exact", max_iter=1000,
                random_state=0).fit(X)
    b = R.kl_grad(P, sk.embedding_)[0]
    print(f"nearest neighbour in its own cluster: {same}; KL device {kl_dev:.6f}, restatement {a:.6f}, "
          f"sklearn exact {b:.6f} (its own report {sk.kl_divergence_:.6f}, {sk.n_iter_} iterations)")
    assert same == 1.0
    assert kl_dev <= 1.05 * max(a, b)

    # kl_divergence_ is the KL at the returned embedding, for the device's own (beta, logz)
    x = torch.as_tensor(X).cuda()
    bd, ld = tsne.affinities(x, 30.0)
    Pd = R.joint_P(X, bd.cpu().numpy().astype(np.float64), ld.cpu().numpy().astype(np.float64), D)
    want = R.kl_grad(Pd, emb)[0]
    rel = abs(model.kl_divergence_ - want) / want
    print(f"kl_divergence_ {model.kl_divergence_:.12g} vs fp64 {want:.12g}: relative {rel:.3e} (bar {KL_BAR})")
    assert isinstance(model.kl_divergence_, float) and rel <= KL_BAR

    # a device tensor in, a device tensor out, the same bits
    m2 = tsne.TSNE(n_components=2, perplexity=30, learning_rate=200, init="pca")
    out = m2.fit_transform(x)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == (192, 2)
    assert np.array_equal(out.cpu().numpy(), emb) and m2.kl_divergence_ == model.kl_divergence_


def test_random_and_array_init():
    from cvhip import tsne

    X = ref("dups")[0]
    a = tsne.TSNE(perplexity=20, init="random", random_state=7, max_iter=30).fit_transform(X)
    b = tsne.TSNE(perplexity=20, init="random", random_state=7, max_iter=30).fit_transform(X)
    c = tsne.TSNE(perplexity=20, init="random", random_state=8, max_iter=30).fit_transform(X)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    y0 = init("dups")
    d = tsne.TSNE(perplexity=20, init=y0, max_iter=5, learning_rate=200).fit_transform(X)
    x, beta, logz = dev("dups")[:3]
    e = tsne.descend(x, beta, logz, torch.as_tensor(y0).cuda(), 5)
    assert np.array_equal(d, e.cpu().numpy())


def test_bad_inputs_raise_before_any_launch(monkeypatch):
    from cvhip import _lib, tsne

    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    x = dev("n257")[0]
    bad = x.clone()
    bad[100, 3] = float("nan")
    inf = x.clone()
    inf[0, 0] = float("inf")
    wide = torch.zeros((70, 65), device="cuda")
    with pytest.raises(ValueError, match="perplexity"):
        tsne.affinities(x, 257.0)
    with pytest.raises(ValueError, match="perplexity"):
        tsne.TSNE(perplexity=300).fit(x)
    with pytest.raises(ValueError, match="NaN or infinity"):
        tsne.TSNE().fit(bad)
    with pytest.raises(ValueError, match="NaN or infinity"):
        tsne.TSNE().fit(inf.cpu().numpy())
    with pytest.raises(ValueError, match=r"1\.\.64"):
        tsne.affinities(wide, 30.0)
    with pytest.raises(ValueError, match=r"1\.\.64"):
        tsne.TSNE().fit(wide)
    with pytest.raises(ValueError, match="float32"):
        tsne.affinities(x.double(), 30.0)
    with pytest.raises(ValueError, match=r"\[257, 2\]"):
        tsne.kl_grad(x, dev("n257")[1], dev("n257")[2], torch.zeros((257, 3), device="cuda"))
    with pytest.raises(ValueError, match="one entry per row"):
        tsne.kl_grad(x, dev("n257")[1][:100], dev("n257")[2], torch.zeros((257, 2), device="cuda"))
    assert launched == []
    # the C entry points refuse the same sizes themselves, without a launch
    L = _lib.lib()
    assert L.cv_tsne_affinity(x.data_ptr(), 5, 257, 5, 257.0, x.data_ptr(), x.data_ptr(), None) != 0
    assert b"perplexity" in L.cv_last_error()
    assert L.cv_tsne_affinity(x.data_ptr(), 5, 257, 65, 30.0, x.data_ptr(), x.data_ptr(), None) != 0
    assert b"1..64" in L.cv_last_error()
    assert L.cv_tsne_workspace_bytes(65537) == 0 and L.cv_tsne_workspace_bytes(1) == 0
    tsne.affinities(x, 30.0)
    assert launched == ["cv_tsne_affinity"]
