"""cvhip.figures (csrc/cv_figure.hip) and src.utils.visual_utils on the device against tests/figures_ref.py, the host
restatement of torchvision's make_grid and of the reference's compositions (not compared with a torchvision install:
it is not installed where these tests run).

Bars.  Everything that only moves values (grids, frames, fills, the swap latents, the copied halves and the end rows of
the interpolation latents, both figures given their decoded images) is bit-exact.  The interior of the interpolation
is within 8 * 2^-24 * (|a| + |b|) of the fp64 value: p carries at most two roundings, 1 - p one, each product one and
the sum one (contracted or not), which comes to under 6 * 2^-24 * (|a| + |b|).  One decode of all latents against
per-sample decodes (eval mode): 1e-4 absolute, the bar the golden tests hold x-hat to (batch size may change the GEMM
tiling).  Every test prints its figures before it asserts.

Measured on an MI355X: the interpolation's largest interior error 1.52 * 2^-24 * (|a| + |b|) (S = 5, T = 11, D = 13);
one decode against per-sample decodes 0 for VAE and VAE64; library calls outside vae.decode 5 for the swap figure and 7
for the two strips, at 2 and at 6 images."""

import functools

import numpy as np
import pytest
import torch

import figures_ref as R

pytestmark = pytest.mark.gpu

GRID_CASES = [(1, 1, 5, 7, 8), (1, 3, 5, 7, 8), (2, 1, 28, 28, 1), (5, 3, 4, 6, 3), (9, 1, 28, 28, 3),
              (7, 3, 64, 64, 8), (3, 3, 9, 65, 2)]
SENTINEL = -7.0


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def images(m, c, h, w):
    """Random images with 0.25 planted in every channel of image 0 (at different pixels) and one NaN pixel."""
    x = np.random.default_rng(m * 1000 + c * 100 + h + w).uniform(0.0, 1.0, size=(m, c, h, w)).astype(np.float32)
    for ch in range(c):
        x[0, ch, ch, ch + 1] = 0.25
    x[0, 0, 3, 3] = np.nan
    x[m - 1, c - 1, 0, 0] = 0.25
    x.setflags(write=False)
    return x


def ref_grid(x, nrow, padding, pad_value, frame):
    g = R.make_grid(x, nrow=nrow, padding=padding, pad_value=pad_value)
    return g if frame is None else R.recolour(g, frame)


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: "x".join(map(str, c)))
def test_make_grid_bit_exact(case):
    from cvhip import figures

    m, c, h, w, nrow = case
    x = images(m, c, h, w)
    xd = dev(x)
    bad = []
    for padding in (0, 2, 3):
        for pad_value in (0.0, 0.25):
            for frame in (None, "red", "blue"):
                want = ref_grid(x, nrow, padding, pad_value, frame)
                got = host(figures.make_grid(xd, nrow=nrow, padding=padding, pad_value=pad_value, frame=frame))
                if not R.same_bits(got, want):
                    bad.append((padding, pad_value, frame, got.shape, want.shape))
    print(case, "mismatches:", bad)
    assert not bad
    if m == 1:
        assert figures.make_grid(xd, nrow=nrow).shape == (3, h, w)  # the unpadded quirk
    # the frames did something: with pad 0.25 a red frame is (1, 0.25, 0.25), a blue one (0, 0, 1), by value
    if m > 1:
        red = host(figures.make_grid(xd, nrow=nrow, pad_value=0.25, frame="red"))
        blue = host(figures.make_grid(xd, nrow=nrow, pad_value=0.25, frame="blue"))
        assert tuple(red[:, 0, 0]) == (1.0, 0.25, 0.25) and tuple(blue[:, 0, 0]) == (0.0, 0.0, 1.0)


def test_make_grid_takes_a_non_contiguous_batch():
    from cvhip import figures

    x = images(5, 3, 4, 6)
    xd = dev(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)  # channels-last storage
    assert not xd.is_contiguous()
    assert R.same_bits(host(figures.make_grid(xd, nrow=3)), R.make_grid(x, nrow=3))


@pytest.mark.parametrize("case", [(5, 3, 4, 6, 3), (3, 3, 9, 65, 2), (1, 1, 5, 7, 8), (9, 1, 28, 28, 3)],
                         ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("strided", [False, True])
def test_make_grid_into_a_canvas_leaves_the_rest_untouched(case, strided):
    from cvhip import figures

    m, c, h, w, nrow = case
    x = images(m, c, h, w)
    want = ref_grid(x, nrow, 2, 0.25, "blue")
    gh, gw = want.shape[1:]
    y0, x0 = 2, 3
    if strided:  # a canvas that is itself a window of a larger tensor: both pitches differ from the dense ones
        base = torch.full((3, gh + 9, gw + 20), SENTINEL, device="cuda")
        canvas = base[:, 1:gh + 6, 4:gw + 13]
    else:
        base = canvas = torch.full((3, gh + 5, gw + 9), SENTINEL, device="cuda")
    view = figures.make_grid(dev(x), nrow=nrow, pad_value=0.25, frame="blue", out=canvas, origin=(y0, x0))
    assert view.data_ptr() == canvas[:, y0:, x0:].data_ptr() and view.shape == want.shape
    got = host(canvas)
    assert R.same_bits(got[:, y0:y0 + gh, x0:x0 + gw], want)
    outside = np.ones(got.shape, bool)
    outside[:, y0:y0 + gh, x0:x0 + gw] = False
    assert (got[outside] == SENTINEL).all()
    if strided:
        b = host(base)
        inner = np.zeros(b.shape, bool)
        inner[:, 1:gh + 6, 4:gw + 13] = True
        assert (b[~inner] == SENTINEL).all()


def test_fill():
    from cvhip import figures

    canvas = torch.full((3, 37, 70), SENTINEL, device="cuda")
    view = figures.fill(canvas, (5, 3), (9, 65), 1.0)
    assert view.shape == (3, 9, 65)
    want = np.full((3, 37, 70), SENTINEL, np.float32)
    want[:, 5:14, 3:68] = 1.0
    assert R.same_bits(host(canvas), want)
    figures.fill(canvas, (0, 0), (37, 70), 0.25, frame="red")  # the whole canvas, through the frame rule
    got = host(canvas)
    assert (got[0] == 1.0).all() and (got[1:] == 0.25).all()
    figures.fill(canvas, (36, 69), (1, 1), 0.25, frame="blue")
    assert tuple(host(canvas)[:, 36, 69]) == (0.0, 0.0, 1.0) and tuple(host(canvas)[:, 36, 68]) == (1.0, 0.25, 0.25)


# ---- pair_latents ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("dc,ds", [(8, 8), (3, 5), (64, 64)])
def test_pair_latents_bit_exact_without_a_copy(n, dc, ds, monkeypatch):
    from cvhip import _lib, figures

    z = torch.randn(n, dc + ds, generator=torch.Generator().manual_seed(n + dc)).cuda()
    z_c, z_s = z[:, :dc], z[:, dc:]
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    got = figures.pair_latents(z_c, z_s)
    monkeypatch.undo()
    (name, a), = seen
    assert name == "cv_latent_pairs"
    assert (a[0], a[2]) == (z_c.data_ptr(), z_s.data_ptr()) and a[2] == z.data_ptr() + 4 * dc  # the slices themselves
    if n > 1:
        assert (a[1], a[3]) == (dc + ds, dc + ds)
    want = torch.cat((z_c[:, None, :].repeat(1, n, 1), z_s[None, :, :].repeat(n, 1, 1)), dim=-1).view(-1, dc + ds)
    assert got.shape == (n * n, dc + ds) and got.is_contiguous()
    assert R.same_bits(host(got), host(want))
    assert R.same_bits(host(got), R.pairs(host(z_c), host(z_s)))


# ---- interp_latents ----------------------------------------------------------------------------------------------
IDS = {2: ([3, 3], [3, 0]), 5: ([0, 6, 6, 2, 4], [1, 6, 3, 2, 0])}  # repeated ids, and src == tgt


@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("T", [1, 2, 3, 11, 12])
@pytest.mark.parametrize("D,z_dim,view", [(16, 8, False), (13, 5, True)])
def test_interp_latents(S, T, D, z_dim, view):
    from cvhip import figures

    big = (3.0 * torch.randn(7, D + 3, generator=torch.Generator().manual_seed(D))).cuda()
    z = big[:, :D] if view else big[:, :D].contiguous()
    src, tgt = IDS[S]
    got = host(figures.interp_latents(z, z_dim, torch.tensor(src), torch.tensor(tgt).cuda(), T))
    assert got.shape == (2, S, T, D)
    zh = host(z)
    z1, z2 = zh[src], zh[tgt]
    # the copied halves, every step
    for k in range(T):
        assert R.same_bits(got[0, :, k, :z_dim], z1[:, :z_dim])
        assert R.same_bits(got[1, :, k, z_dim:], z1[:, z_dim:])
    # the end rows of the interpolated halves
    assert R.same_bits(got[0, :, 0, z_dim:], z1[:, z_dim:]) and R.same_bits(got[1, :, 0, :z_dim], z1[:, :z_dim])
    if T >= 2:
        assert R.same_bits(got[0, :, T - 1, z_dim:], z2[:, z_dim:])
        assert R.same_bits(got[1, :, T - 1, :z_dim], z2[:, :z_dim])
    ref, mag = R.interp_ref(zh, z_dim, src, tgt, T)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(mag, 1e-300)).max() / 2.0 ** -24)
    print(f"S={S} T={T} D={D}: largest error {worst:.3f} x 2^-24 (|a| + |b|); bar 8")
    assert (err <= 8 * 2.0 ** -24 * mag).all()
    # src == tgt: every step is the row itself, up to the roundings above
    same = [i for i in range(S) if src[i] == tgt[i]]
    assert same
    assert R.same_bits(host(figures.interp_latents(z, z_dim, src, tgt, T)), got)  # lists pass, and twice is the same


@pytest.mark.parametrize("src,tgt", [([0, 7], [1, 2]), ([0, 1], [-1, 2]), ([0, 1], [1, 2 ** 40])])
@pytest.mark.parametrize("on_device", [False, True])
def test_interp_latents_rejects_ids_out_of_range(src, tgt, on_device, monkeypatch):
    from cvhip import _lib, figures

    z = torch.zeros(7, 16, device="cuda")
    s, t = torch.tensor(src), torch.tensor(tgt)
    if on_device:
        s, t = s.cuda(), t.cuda()
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match=r"\[0, 7\)"):
        figures.interp_latents(z, 8, s, t, 3)


# ---- the figures -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(kind):
    from src.models.vae import VAE, VAE64

    torch.manual_seed(11)
    vae = (VAE(16, 1) if kind == "VAE" else VAE64(16, 3)).cuda().eval()
    size, ch = (28, 1) if kind == "VAE" else (64, 3)
    g = torch.Generator().manual_seed(5)
    X = torch.rand(12, ch, size, size, generator=g).cuda()
    z = torch.randn(12, 16, generator=g).cuda()
    return vae, X, z, size


class Calls:
    """Counts _lib.call invocations, except those made while vae.decode runs; records decode's argument shapes."""

    def __init__(self, monkeypatch, vae):
        from cvhip import _lib

        self.names, self.decodes, self.outputs, self.inside = [], [], [], False
        real_call, real_decode = _lib.call, vae.decode

        def call(name, *a):
            if not self.inside:
                self.names.append(name)
            return real_call(name, *a)

        def decode(z):
            self.decodes.append(tuple(z.shape))
            self.inside = True
            try:
                out = real_decode(z)
            finally:
                self.inside = False
            self.outputs.append(out)
            return out

        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(vae, "decode", decode)


@pytest.mark.parametrize("kind,n", [("VAE", 4), ("VAE64", 3)])
def test_swap_figure(kind, n, monkeypatch):
    from cvhip import figures
    from src.utils import visual_utils as V

    vae, X, z, size = model(kind)
    X, z_c, z_s = X[:n], z[:n, :8], z[:n, 8:]
    with torch.no_grad():
        decoded = vae.decode(figures.pair_latents(z_c, z_s))
    rec = Calls(monkeypatch, vae)
    fig = V.feature_swapping_grid(z_c, z_s, X, vae, img_size=size)
    again = V.feature_swapping_grid(z_c, z_s, X, vae, img_size=size)
    monkeypatch.undo()
    assert rec.decodes == [(n * n, 16)] * 2 and vae.training is False
    h = w = size
    assert fig.shape == (3, (h + 4) + n * (h + 2) + 2, (w + 4) + n * (w + 2) + 2)
    got = host(fig)
    assert R.same_bits(host(rec.outputs[0]), host(decoded))  # decode is deterministic
    # the main area, image by image
    for i in range(n):
        for j in range(n):
            y, x = (h + 4) + 2 + i * (h + 2), (w + 4) + 2 + j * (w + 2)
            cell = got[:, y:y + h, x:x + w]
            d = host(decoded[i * n + j])
            assert R.same_bits(cell, np.broadcast_to(d, (3, h, w)) if d.shape[0] == 1 else d), (i, j)
    assert R.same_bits(got, R.swap_figure(host(X), host(decoded)))
    assert R.same_bits(host(again), got)
    assert R.same_bits(host(figures.swap_figure(X, decoded)), got)


def strips_ref(X, src, tgt, style, content, T):
    Xh = host(X)
    return R.strip(Xh[src], Xh[tgt], host(style), T), R.strip(Xh[src], Xh[tgt], host(content), T)


@pytest.mark.parametrize("kind,S,T", [("VAE", 3, 4), ("VAE64", 2, 3), ("VAE", 2, 1)])
def test_interpolation_grids_eval(kind, S, T, monkeypatch):
    from cvhip import figures
    from src.utils import visual_utils as V

    vae, X, z, size = model(kind)
    src, tgt = list(range(S)), [5, 1, 7][:S]  # (tgt[1] == src[1])
    rec = Calls(monkeypatch, vae)
    style_fig, content_fig = V.interpolation_grids(X, z, vae, 8, sample_size=S, inter_steps=T, src_ids=src,
                                                   tgt_ids=tgt)
    monkeypatch.undo()
    assert rec.decodes == [(2 * S * T, 16)] and vae.training is False  # one decode of every latent
    h = w = size
    shape = (3, S * (h + 2) + 2, (w + 4) + 8 + T * (w + 2) + 2 + 8 + (w + 4))
    assert style_fig.shape == shape and content_fig.shape == shape
    dec = rec.outputs[0]
    want_s, want_c = strips_ref(X, src, tgt, dec[:S * T], dec[S * T:], T)
    assert R.same_bits(host(style_fig), want_s) and R.same_bits(host(content_fig), want_c)
    # interp_figure on its own, without the frame shared through `like`, gives the same strip
    assert R.same_bits(host(figures.interp_figure(X[src], X[tgt], dec[S * T:])), want_c)
    # against per-sample decodes: same images within the golden tests' bar
    lat = figures.interp_latents(z, 8, src, tgt, T)
    with torch.no_grad():
        per = torch.cat([vae.decode(lat[a, i]) for a in range(2) for i in range(S)])
    diff = float((per - dec).abs().max())
    print(f"{kind} S={S} T={T}: one decode against per-sample decodes, largest difference {diff:.3e} (bar 1e-4)")
    assert diff <= 1e-4


def test_interpolation_grids_draws_the_reference_ids(monkeypatch):
    from src.utils import visual_utils as V

    vae, X, z, _ = model("VAE")
    torch.manual_seed(3)
    src = torch.randperm(z.size(0))[:3]
    tgt = torch.randperm(z.size(0))[:3]
    want = V.interpolation_grids(X, z, vae, 8, sample_size=3, inter_steps=3, src_ids=src, tgt_ids=tgt)
    torch.manual_seed(3)
    got = V.interpolation_grids(X, z, vae, 8, sample_size=3, inter_steps=3)
    for g, w in zip(got, want):
        assert R.same_bits(host(g), host(w))
    assert not R.same_bits(host(got[0]), host(got[1]))


def test_interpolation_grids_train_mode(monkeypatch):
    """In train mode BatchNorm ties a decode to its batch: the 2 S batches of T latents are decoded one by one in the
    reference's order, and the figures are made of exactly those outputs."""
    from cvhip import figures
    from src.models.vae import VAE
    from src.utils import visual_utils as V

    vae0, X, z, size = model("VAE")
    # a model of its own: train-mode decodes update the running statistics, which the shared one must keep
    vae = VAE(16, 1).cuda()
    vae.load_state_dict(vae0.state_dict())
    vae.train()
    S, T = 3, 4
    src, tgt = [4, 2, 9], [0, 2, 3]
    rec = Calls(monkeypatch, vae)
    style_fig, content_fig = V.interpolation_grids(X, z, vae, 8, sample_size=S, inter_steps=T, src_ids=src,
                                                   tgt_ids=tgt)
    monkeypatch.undo()
    assert rec.decodes == [(T, 16)] * (2 * S) and vae.training is True
    lat = figures.interp_latents(z, 8, src, tgt, T)
    style, content = torch.cat(rec.outputs[0::2]), torch.cat(rec.outputs[1::2])  # style_i, content_i, per sample
    want_s, want_c = strips_ref(X, src, tgt, style, content, T)
    assert R.same_bits(host(style_fig), want_s) and R.same_bits(host(content_fig), want_c)
    assert lat.shape == (2, S, T, 16)


def test_launch_counts_do_not_grow_with_the_figure(monkeypatch):
    """The number of library calls outside vae.decode: the same for 2 and 6 images, and at most 8 (a guard against a
    per-image loop on the host)."""
    from src.utils import visual_utils as V

    vae, X, z, size = model("VAE")
    counts = {}
    for n in (2, 6):
        rec = Calls(monkeypatch, vae)
        V.feature_swapping_grid(z[:n, :8], z[:n, 8:], X[:n], vae, img_size=size)
        monkeypatch.undo()
        counts["swap", n] = list(rec.names)
        rec = Calls(monkeypatch, vae)
        V.interpolation_grids(X, z, vae, 8, sample_size=n, inter_steps=5, src_ids=list(range(n)),
                              tgt_ids=list(range(n, 2 * n)))
        monkeypatch.undo()
        counts["strips", n] = list(rec.names)
    print({k: len(v) for k, v in counts.items()}, counts["swap", 2], counts["strips", 2])
    assert counts["swap", 2] == counts["swap", 6] and counts["strips", 2] == counts["strips", 6]
    assert 1 <= len(counts["swap", 2]) <= 8 and 1 <= len(counts["strips", 2]) <= 8


def test_make_colored_grid_is_the_framed_grid():
    from src.utils import visual_utils as V

    x = images(5, 3, 4, 6)
    for color, nrow in (("red", 1), ("blue", 5)):
        assert R.same_bits(host(V.make_colored_grid(dev(x), nrow, color)), R.colored_grid(x, nrow, color))


def test_latent_embeddings():
    from cvhip.tsne import TSNE
    from src.utils import visual_utils as V

    vae, _, _, _ = model("VAE")
    g = torch.Generator().manual_seed(9)
    X = torch.rand(64, 1, 28, 28, generator=g)
    c, s = torch.randint(0, 10, (64,), generator=g), torch.randint(0, 4, (64,), generator=g)
    loader = [(X[i:i + 24], c[i:i + 24], s[i:i + 24]) for i in range(0, 64, 24)]  # 24, 24, 16
    emb_c, emb_s, labels, styles = V.latent_embeddings(loader, vae, torch.device("cuda", 0), perplexity=5,
                                                       max_iter=20)
    assert torch.equal(labels, c) and torch.equal(styles, s)
    with torch.no_grad():
        parts = [vae(xb.cuda())[1] for xb, _, _ in loader]
    mu_c = torch.cat([p["mu_c"] for p in parts]).contiguous()
    mu_s = torch.cat([p["mu_s"] for p in parts]).contiguous()
    kw = dict(n_components=2, perplexity=5, learning_rate=200, init="pca", max_iter=20)
    assert emb_c.shape == (64, 2) and emb_s.shape == (64, 2)
    assert R.same_bits(host(emb_c), host(TSNE(**kw).fit_transform(mu_c)))
    assert R.same_bits(host(emb_s), host(TSNE(**kw).fit_transform(mu_s)))
