"""cvhip.figures and src.utils.visual_utils without a device: every ValueError that is raised before anything is
launched, the host-side validation of the three C entry points, and what the module needs in order to import.  The
restatement the device tests compare against (tests/figures_ref.py) is checked here for the facts the figures rest on:
the frame values, the figure shapes and the exact end rows of the interpolation."""

import subprocess
import sys

import numpy as np
import pytest
import torch

import figures_ref as R


@pytest.fixture
def no_launch(monkeypatch):
    from cvhip import _lib

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a kernel was launched"))


def img(m=4, c=1, h=28, w=28, dtype=torch.float32):
    return torch.zeros(m, c, h, w, dtype=dtype)


class Decoder(torch.nn.Module):
    def decode(self, z):
        pytest.fail("decode was called")


def test_cpu_tensors_are_rejected(no_launch):
    from cvhip import figures
    from src.utils import visual_utils as V

    z = torch.zeros(4, 16)
    cases = [
        lambda: figures.pair_latents(z[:, :8], z[:, 8:]),
        lambda: figures.interp_latents(z, 8, [0, 1], [1, 2], 3),
        lambda: figures.make_grid(img()),
        lambda: figures.make_grid(img(), out=torch.zeros(3, 200, 200)),
        lambda: figures.fill(torch.zeros(3, 8, 8), (0, 0), (2, 2), 1.0),
        lambda: figures.swap_figure(img(2), img(4)),
        lambda: figures.interp_figure(img(2), img(2), img(6)),
        lambda: V.make_colored_grid(img(), 1, "red"),
        lambda: V.feature_swapping_grid(z[:, :8], z[:, 8:], img(), Decoder()),
        lambda: V.interpolation_grids(img(), z, Decoder(), 8, sample_size=2, inter_steps=3),
        lambda: figures.pair_latents(np.zeros((4, 8), np.float32), z[:, 8:]),  # not a tensor at all
    ]
    for fn in cases:
        with pytest.raises(ValueError, match="ROCm device"):
            fn()


@pytest.mark.parametrize("fn,match", [
    (lambda F: F.make_grid(img(c=2)), "1 or 3 channels"),
    (lambda F: F.make_grid(img(dtype=torch.float64)), "float32"),
    (lambda F: F.make_grid(img(dtype=torch.float16)), "float32"),
    (lambda F: F.make_grid(img()[0]), r"\[M, C, H, W\]"),
    (lambda F: F.make_grid(img(m=0)), r"1\.\.65536"),
    (lambda F: F.make_grid(img(h=1, w=4097)), r"1\.\.4096"),
    (lambda F: F.make_grid(img(), nrow=0), "nrow"),
    (lambda F: F.make_grid(img(), padding=-1), "padding"),
    (lambda F: F.make_grid(img(), frame="green"), "frame"),
    (lambda F: F.make_grid(img(), out=torch.zeros(3, 10, 10)), "does not fit"),
    (lambda F: F.make_grid(img(), out=torch.zeros(3, 200, 200), origin=(-1, 0)), "does not fit"),
    (lambda F: F.make_grid(img(), out=torch.zeros(1, 200, 200)), r"\[3, Hd, Wd\]"),
    (lambda F: F.make_grid(img(), out=torch.zeros(3, 200, 200, dtype=torch.float64)), r"\[3, Hd, Wd\]"),
    (lambda F: F.make_grid(img(), out=torch.zeros(3, 200, 400)[:, :, ::2]), "unit column stride"),
    (lambda F: F.fill(torch.zeros(3, 8, 8), (4, 4), (5, 5), 1.0), "does not fit"),
    (lambda F: F.fill(torch.zeros(3, 8, 8), (0, 0), (0, 5), 1.0), "empty"),
    (lambda F: F.pair_latents(torch.zeros(4, 8), torch.zeros(5, 8)), "rows"),
    (lambda F: F.pair_latents(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 8)), "float32"),
    (lambda F: F.pair_latents(torch.zeros(4), torch.zeros(4, 8)), "2-D"),
    (lambda F: F.pair_latents(torch.zeros(0, 8), torch.zeros(0, 8)), "empty"),
    (lambda F: F.interp_latents(torch.zeros(4, 16), 16, [0], [1], 3), "z_dim"),
    (lambda F: F.interp_latents(torch.zeros(4, 16), 0, [0], [1], 3), "z_dim"),
    (lambda F: F.interp_latents(torch.zeros(4, 16), 8, [0], [1], 0), "steps"),
    (lambda F: F.interp_latents(torch.zeros(4, 16), 8, [0, 1], [1], 3), "same length"),
    (lambda F: F.interp_latents(torch.zeros(4, 16), 8, [0.5], [1.0], 3), "integer"),
    (lambda F: F.interp_latents(torch.zeros(4, 16).double(), 8, [0], [1], 3), "float32"),
    (lambda F: F.swap_figure(img(1), img(1)), "n >= 2"),
    (lambda F: F.swap_figure(img(3), img(8)), "n \\* n"),
    (lambda F: F.swap_figure(img(2), img(4, c=3)), "agree"),
    (lambda F: F.swap_figure(img(2, c=2), img(4, c=2)), "1 or 3 channels"),
    (lambda F: F.interp_figure(img(1), img(1), img(3)), "S >= 2"),
    (lambda F: F.interp_figure(img(2), img(3), img(6)), "differ in shape"),
    (lambda F: F.interp_figure(img(2), img(2), img(5)), "multiple"),
    (lambda F: F.interp_figure(img(2), img(2), img(6, h=14)), "agree"),
])
def test_figures_reject_before_any_launch(fn, match, no_launch):
    from cvhip import figures

    with pytest.raises(ValueError, match=match):
        fn(figures)


@pytest.mark.parametrize("fn,match", [
    (lambda V: V.make_colored_grid(img(), 1, "green"), "other color not implemented yet"),
    (lambda V: V.feature_swapping_grid(torch.zeros(1, 8), torch.zeros(1, 8), img(1), Decoder()), "n >= 2"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(4, 8), img(4), Decoder(), img_size=32),
     "img_size"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(4, 8), img(4, h=28, w=32), Decoder()),
     "img_size"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(3, 8), img(4), Decoder()), "rows"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(4, 8), img(5), Decoder()), "images"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(4, 8), img(4, c=2), Decoder()),
     "1 or 3 channels"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8).double(), torch.zeros(4, 8), img(4), Decoder()), "float32"),
    (lambda V: V.feature_swapping_grid(torch.zeros(4, 8), torch.zeros(4, 8), img(4).double(), Decoder()), "float32"),
    (lambda V: V.interpolation_grids(img(4), torch.zeros(4, 16), Decoder(), 8, sample_size=1), "sample_size"),
    (lambda V: V.interpolation_grids(img(4), torch.zeros(4, 16), Decoder(), 8, sample_size=2, inter_steps=0),
     "inter_steps"),
    (lambda V: V.interpolation_grids(img(5), torch.zeros(4, 16), Decoder(), 8, sample_size=2), "images"),
    (lambda V: V.interpolation_grids(img(4), torch.zeros(4, 16), Decoder(), 8, sample_size=2, src_ids=[0, 1]),
     "both"),
    (lambda V: V.interpolation_grids(img(4, c=2), torch.zeros(4, 16), Decoder(), 8, sample_size=2),
     "1 or 3 channels"),
])
def test_visual_utils_reject_before_any_launch(fn, match, no_launch):
    from src.utils import visual_utils

    with pytest.raises(ValueError, match=match):
        fn(visual_utils)


def test_c_entry_points_refuse_bad_arguments_without_a_launch():
    """Host-side validation of the three entry points: each call is rejected before anything is enqueued, so the
    (never dereferenced) pointers may be anything non-null."""
    from cvhip import _lib

    L = _lib.lib()
    p = 4096  # stands for any non-null pointer

    def refused(rc, word):
        assert rc != 0
        err = L.cv_last_error()
        assert err and word in err, err

    # cv_latent_pairs(z_c, ldc, z_s, lds, n, dc, ds, out, stream)
    for args, word in [((None, 8, p, 8, 4, 8, 8, p), b"must be given"), ((p, 8, None, 8, 4, 8, 8, p), b"must be given"),
                       ((p, 8, p, 8, 4, 8, 8, None), b"must be given"), ((p, 8, p, 8, 0, 8, 8, p), b"positive"),
                       ((p, 8, p, 8, 4, 0, 8, p), b"positive"), ((p, 7, p, 8, 4, 8, 8, p), b"row stride"),
                       ((p, 8, p, 3, 4, 8, 8, p), b"row stride"), ((p, 64, p, 64, 46341, 1, 1, p), b"2^31")]:
        refused(L.cv_latent_pairs(*args, None), word)
    # cv_latent_interp(z, ldz, n, d, z_dim, src_ids, tgt_ids, s, steps, out, stream)
    for args, word in [((None, 16, 4, 16, 8, p, p, 2, 3, p), b"must be given"),
                       ((p, 16, 4, 16, 8, None, p, 2, 3, p), b"must be given"),
                       ((p, 16, 4, 16, 8, p, None, 2, 3, p), b"must be given"),
                       ((p, 16, 4, 16, 8, p, p, 2, 3, None), b"must be given"),
                       ((p, 15, 4, 16, 8, p, p, 2, 3, p), b"row stride"), ((p, 16, 0, 16, 8, p, p, 2, 3, p), b"n >= 1"),
                       ((p, 16, 4, 16, 0, p, p, 2, 3, p), b"z_dim"), ((p, 16, 4, 16, 16, p, p, 2, 3, p), b"z_dim"),
                       ((p, 16, 4, 16, 8, p, p, 0, 3, p), b"positive"), ((p, 16, 4, 16, 8, p, p, 2, 0, p), b"positive"),
                       ((p, 64, 4, 64, 8, p, p, 65536, 256, p), b"2^31")]:
        refused(L.cv_latent_interp(*args, None), word)

    # cv_make_grid(images, m, c, h, w, nrow, padding, pad_value, frame, mode, dst, dst_h, dst_w, cpitch, rpitch, y0,
    #              x0, stream)
    def grid(images=p, m=4, c=1, h=28, w=28, nrow=2, padding=2, pad_value=0.0, frame=0, mode=0, dst=p, dst_h=62,
             dst_w=62, cpitch=62 * 62, rpitch=62, y0=0, x0=0):
        return L.cv_make_grid(images, m, c, h, w, nrow, padding, pad_value, frame, mode, dst, dst_h, dst_w, cpitch,
                              rpitch, y0, x0, None)

    for kw, word in [(dict(images=None), b"images must be given"), (dict(dst=None), b"destination must be given"),
                     (dict(c=2), b"1 or 3 channels"), (dict(c=0), b"1 or 3 channels"), (dict(padding=-1), b"padding"),
                     (dict(nrow=0), b"nrow"), (dict(m=65537), b"1..65536"), (dict(m=0), b"1..65536"),
                     (dict(h=4097), b"at most 4096"), (dict(w=4097), b"at most 4096"), (dict(h=0), b"positive"),
                     (dict(frame=3), b"frame"), (dict(mode=2), b"mode"), (dict(y0=1), b"does not fit"),
                     (dict(x0=-1), b"does not fit"), (dict(dst_h=61), b"does not fit"), (dict(nrow=4), b"does not fit"),
                     (dict(rpitch=61), b"pitches"), (dict(cpitch=62 * 62 - 1), b"pitches"),
                     (dict(cpitch=2 ** 30), b"2^31"), (dict(mode=1, m=4), b"takes no images"),
                     (dict(mode=1, m=0, h=63), b"does not fit"),
                     (dict(m=65536, nrow=1, h=4096, w=4096), b"does not fit")]:
        refused(grid(**kw), word)


def test_module_imports_without_torchvision_and_matplotlib():
    code = ("import sys, importlib.abc\n"
            "class Block(importlib.abc.MetaPathFinder):\n"
            "    def find_spec(self, name, path, target=None):\n"
            "        if name.split('.')[0] in ('torchvision', 'matplotlib', 'sklearn'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path[:0] = {[p for p in sys.path if p]!r}\n"
            "import src.utils.visual_utils as V, cvhip.figures\n"
            "assert not {'torchvision', 'matplotlib', 'sklearn'} & set(sys.modules), sorted(sys.modules)\n"
            "print(sorted(n for n in dir(V) if not n.startswith('_')))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("make_colored_grid", "feature_swapping_grid", "feature_swapping_plot", "interpolation_grids",
                 "interpolation_plot", "latent_embeddings", "tsne_plot"):
        assert name in r.stdout, (name, r.stdout)


def test_plot_functions_keep_the_reference_signatures():
    import inspect

    from src.utils import visual_utils as V

    assert list(inspect.signature(V.feature_swapping_plot).parameters) == ["z_c", "z_s", "X", "vae", "img_size"]
    assert list(inspect.signature(V.interpolation_plot).parameters) == ["X", "z", "vae", "z_dim", "sample_size",
                                                                        "inter_steps"]
    assert list(inspect.signature(V.tsne_plot).parameters) == ["dataloader", "vae", "device", "content_labels",
                                                               "style_labels"]
    assert list(inspect.signature(V._tsne_plot).parameters) == ["tsne_2d", "class_labels", "classes"]
    sig = inspect.signature(V.interpolation_plot).parameters
    assert (sig["sample_size"].default, sig["inter_steps"].default) == (10, 11)
    assert inspect.signature(V.feature_swapping_plot).parameters["img_size"].default == 28


# ---- the restatement itself --------------------------------------------------------------------------------------
def test_restatement_frame_values_and_shapes():
    rng = np.random.default_rng(0)
    X = rng.uniform(0.3, 0.9, size=(3, 1, 5, 5)).astype(np.float32)
    red, blue = R.colored_grid(X, 1, "red"), R.colored_grid(X, 3, "blue")
    assert red.shape == (3, 3 * 7 + 2, 9) and blue.shape == (3, 9, 3 * 7 + 2)
    assert tuple(red[:, 0, 0]) == (1.0, 0.25, 0.25)  # not red: the later masks see channel 0 already changed
    assert tuple(blue[:, 0, 0]) == (0.0, 0.0, 1.0)
    assert np.array_equal(red[:, 2:7, 2:7], np.repeat(X[0], 3, axis=0))
    Y = X.copy()
    Y[1, 0, 2, 3] = 0.25  # an image pixel at the pad value is recoloured too
    assert tuple(R.colored_grid(Y, 1, "red")[:, 7 + 2 + 2, 2 + 3]) == (1.0, 0.25, 0.25)
    assert tuple(R.colored_grid(Y, 1, "blue")[:, 7 + 2 + 2, 2 + 3]) == (0.0, 0.0, 1.0)
    Y[1, 0, 2, 3] = np.nan
    assert np.isnan(R.colored_grid(Y, 1, "red")[:, 7 + 2 + 2, 2 + 3]).all()
    dec = rng.uniform(size=(9, 1, 5, 5)).astype(np.float32)
    fig = R.swap_figure(X, dec)
    assert fig.shape == (3, 32, 32) == (3, 9 + 3 * 7 + 2, 9 + 3 * 7 + 2)
    assert (fig[:, :9, :9] == 1.0).all()
    assert np.array_equal(fig[0, 9 + 2 + 7:9 + 2 + 7 + 5, 9 + 2 + 14:9 + 2 + 14 + 5], dec[1 * 3 + 2, 0])
    st = R.strip(X[:2], X[1:], rng.uniform(size=(2 * 4, 1, 5, 5)).astype(np.float32), 4)
    assert st.shape == (3, 2 * 7 + 2, 9 + 8 + 4 * 7 + 2 + 8 + 9)
    assert R.make_grid(X[:1]).shape == (3, 5, 5)  # one image: no border
    assert R.make_grid(rng.uniform(size=(5, 3, 4, 6)).astype(np.float32), nrow=3, padding=3).shape == (3, 17, 30)


@pytest.mark.parametrize("steps", [1, 2, 3, 11, 12])
def test_torch_interpolation_has_exact_end_rows(steps):
    """What cv_latent_interp promises for its end rows holds for the reference's own fp32 formula on the host."""
    from src.utils.display_utils import interpolate_latent

    g = torch.Generator().manual_seed(steps)
    a, b = torch.randn(16, generator=g), torch.randn(16, generator=g)
    out = interpolate_latent(a, b, steps)
    assert R.same_bits(out[0].numpy(), a.numpy())
    if steps >= 2:
        assert R.same_bits(out[-1].numpy(), b.numpy())
    z = torch.stack([a, b]).numpy()
    ref, mag = R.interp_ref(z, 8, [0], [1], steps)
    err = np.abs(out.numpy().astype(np.float64)[:, 8:] - ref[0, 0, :, 8:])
    assert (err <= 8 * 2.0 ** -24 * mag[0, 0, :, 8:]).all()
