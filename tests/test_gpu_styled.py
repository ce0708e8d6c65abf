"""The device Styled-MNIST generator (cv_style_mnist via cvhip.styled / src.utils.data_utils.DeviceStyledMNIST)
against the fp64 restatement tests/styled_ref.py (pinned by tests/test_styled_ref.py): every style with the style
injected, the mixed batch, the on-device draws and the public path down to one fused training step.

Tolerances (0-255 scale): identity / stripe exact; scale / brightness 1e-4 (the fp64 reference rounds to fp32 at the
end, one fp32 ulp at 255 is 1.5e-5); zigzag 1e-2 (an fp32 logf on an fp64 line distance, |d term / d dist| <= 1.2
where the term is non-zero: about 1e-3); canny exact for every image whose reference decision margin is >= 1e-5 (the
fp32 error of a 9-tap blur, a Sobel and a square root on values up to 4 is about 1e-6; the kernel's front end is
fp64), at most 5 % of the images left out."""

import numpy as np
import pytest
import torch

import styled_ref as SR

pytestmark = pytest.mark.gpu

N, SEED = 128, 20261020
SIX = ["identity", "stripe", "zigzag", "canny_edges", "scale", "brightness"]
SIX_SEV = [1, 1, 1, 1, 5, 5]
R0S = (0, 13, 26)


@pytest.fixture(scope="module")
def imgs():
    x = SR.synth(N, SEED)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def dimgs(imgs):
    return torch.tensor(np.array(imgs), device="cuda")


@pytest.fixture(scope="module")
def zz():
    """(r0, dr) per image: all ten dr, each with r0 in {0, 13, 26}."""
    i = np.arange(N)
    return np.stack([np.asarray(R0S)[(i // 10) % 3], i % 10 - 5], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def canny_ref(imgs):
    outs, margins = zip(*(SR.canny(x) for x in imgs))
    return np.stack(outs), np.asarray(margins)


def run(dimgs, kinds, sevs, style=None, zz=None, table=None, labels=None, cand=None):
    from cvhip.styled import stylize

    n = dimgs.shape[0]
    if labels is None:
        labels = torch.zeros(n, dtype=torch.int64, device="cuda")
    if table is None:
        table = torch.full((1, len(kinds)), 1.0 / len(kinds), device="cuda")
    if style is not None:
        style = torch.as_tensor(style)
    out, st, z = stylize(dimgs, labels, table, kinds, sevs, style=style, zz=None if zz is None else torch.as_tensor(zz),
                         cand=cand)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), z.cpu().numpy()


def single(dimgs, kind, sev=1, zz=None):
    n = dimgs.shape[0]
    out, st, _ = run(dimgs, [kind], [sev], style=np.zeros(n, dtype=np.int32), zz=zz)
    assert not st.any()
    return out


# ------------------------------------------------------------------------------------------------ per style
@pytest.mark.parametrize("kind", ["identity", "stripe"])
def test_exact_styles(imgs, dimgs, kind):
    got = single(dimgs, kind)
    ref = np.stack([getattr(SR, kind)(x) for x in imgs])
    assert got.dtype == np.float32 and np.array_equal(got, ref)


@pytest.mark.parametrize("kind,sev", [("scale", 5), ("scale", 3), ("brightness", 5), ("brightness", 2)])
def test_graded_styles(imgs, dimgs, kind, sev):
    got = single(dimgs, kind, sev)
    ref = np.stack([getattr(SR, kind)(x, sev) for x in imgs])
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{kind}({sev}): max abs err {err:.3e}")
    assert err <= 1e-4
    assert got.min() >= 0.0 and got.max() <= 255.0


def test_zigzag(imgs, dimgs, zz):
    assert {int(d) for d in zz[:, 1]} == set(range(-5, 5))
    assert {(int(r), int(d)) for r, d in zz} >= {(r, d) for r in R0S for d in range(-5, 5)}
    out, _, zo = run(dimgs, ["zigzag"], [1], style=np.zeros(N, dtype=np.int32), zz=zz)
    assert np.array_equal(zo, zz)
    ref = np.stack([SR.zigzag(x, int(r), int(d)) for x, (r, d) in zip(imgs, zz)])
    err = np.abs(out.astype(np.float64) - ref).reshape(N, -1).max(axis=1)
    print(f"zigzag: max abs err {err.max():.3e} (image {int(err.argmax())}, zz {zz[int(err.argmax())]})")
    assert err.max() <= 1e-2
    assert (ref != imgs).reshape(N, -1).any(axis=1).all()  # (every image got a zigzag)


def test_canny(imgs, dimgs, canny_ref):
    ref, margin = canny_ref
    got = single(dimgs, "canny_edges")
    assert set(np.unique(got)) <= {0.0, 255.0}
    sure = margin >= 1e-5
    print(f"canny: {int((~sure).sum())} of {N} images below margin 1e-5, smallest margin {margin.min():.3e}; "
          f"images that differ: {int((got != ref).reshape(N, -1).any(axis=1).sum())}")
    assert (~sure).sum() <= 0.05 * N
    bad = [i for i in np.nonzero(sure)[0] if not np.array_equal(got[i], ref[i])]
    assert not bad, (bad, [int((got[i] != ref[i]).sum()) for i in bad])
    assert (ref.reshape(N, -1).sum(axis=1) > 0).all()


def test_canny_flood_finishes_on_the_longest_chain(dimgs):
    """A one-pixel-wide spiral of weak candidates over the whole plane with one strong pixel at its end: the flood
    has to walk all of it, one way or the other, within its sweep bound."""
    state, length = SR.spiral_candidates()
    assert length > 350
    weak = np.where(state == 2, 1, state)
    outer = weak.copy()
    outer[0, 0] = 2  # the strong pixel at the outer end instead: the flood runs the other way
    cands = np.stack([state, outer, state.T.copy(), state[::-1, ::-1].copy(), weak, np.zeros_like(state)])
    out, _, _ = run(dimgs[:len(cands)], ["canny_edges"], [1], style=np.zeros(len(cands), dtype=np.int32),
                    cand=torch.tensor(cands))
    for k, c in enumerate(cands):
        want = SR.hysteresis(c).astype(np.float32) * 255.0
        assert np.array_equal(out[k], want), (k, int((out[k] > 0).sum()), int((want > 0).sum()))
    assert [(o > 0).sum() for o in out] == [length] * 4 + [0, 0]


# ------------------------------------------------------------------------------------------------ mixed batch
@pytest.fixture(scope="module")
def singles(dimgs, zz):
    return [single(dimgs, k, s, zz=zz) for k, s in zip(SIX, SIX_SEV)]


@pytest.mark.parametrize("n", [N, 127, 7, 1])
def test_mixed_batch_equals_single_styles(dimgs, zz, singles, n):
    style = (np.arange(n) % 6).astype(np.int32)
    if n == 1:
        style[:] = 3
    out, st, zo = run(dimgs[:n], SIX, SIX_SEV, style=style, zz=zz[:n])
    assert np.array_equal(st, style) and st.dtype == np.int64 and np.array_equal(zo, zz[:n])
    for i in range(n):
        assert np.array_equal(out[i], singles[style[i]][i]), (i, SIX[style[i]])
    # the other way round, so that every image meets another style and other neighbours
    style2 = ((np.arange(n) + 3) % 6).astype(np.int32)
    out2, _, _ = run(dimgs[:n], SIX, SIX_SEV, style=style2, zz=zz[:n])
    for i in range(n):
        assert np.array_equal(out2[i], singles[style2[i]][i]), (i, SIX[style2[i]])


def test_several_images_per_workgroup(dimgs, zz, singles):
    """Past 16384 images a workgroup works through several consecutive images (here 3, the last workgroup 1): the
    planes in LDS are reused, and every image must still equal its single-style result."""
    n = 2 * 16384 + 5
    rep = -(-n // N)
    big = dimgs.repeat(rep, 1, 1)[:n].contiguous()
    g = torch.Generator().manual_seed(3)
    style = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
    from cvhip.styled import stylize

    labels = torch.zeros(n, dtype=torch.int64, device="cuda")
    table = torch.full((1, 6), 1 / 6, device="cuda")
    out, st, zo = stylize(big, labels, table, SIX, SIX_SEV, style=style, zz=torch.as_tensor(zz).repeat(rep, 1)[:n])
    sel = style.to("cuda", torch.int64)
    want = torch.tensor(np.stack(singles), device="cuda")[sel, torch.arange(n, device="cuda") % N]
    assert torch.equal(st, sel)
    diff = (out != want).reshape(n, -1).any(dim=1)
    assert not bool(diff.any()), torch.nonzero(diff)[:8].flatten().tolist()
    # a drawn launch of that size moves the counter on by one and leaves its arrival word at zero
    from cvhip import rng

    seeded(16)
    _, off = rng.offset_tensor(big.device)
    _, st2, _ = stylize(big, labels, table, SIX, SIX_SEV)
    assert off.cpu().tolist() == [1, 0]
    assert torch.bincount(st2, minlength=6).min() > n // 8


# ------------------------------------------------------------------------------------------------ draws
ND = 8192
PROBS = [0.15, 0.2, 0.25, 0.1, 0.1, 0.2]


@pytest.fixture(scope="module")
def big(dimgs):
    return dimgs.repeat(ND // N, 1, 1).contiguous()


def seeded(seed):
    from cvhip import rng

    torch.manual_seed(seed)
    rng.reset_counters()


def test_drawn_styles_follow_the_table(big, singles):
    seeded(11)
    labels = (torch.arange(ND, device="cuda") % 10).to(torch.int64)
    table = torch.tensor([PROBS] * 10, device="cuda")
    out, st, z = run(big, SIX, SIX_SEV, table=table, labels=labels)
    for s, p in enumerate(PROBS):
        share, sigma = (st == s).mean(), np.sqrt(p * (1 - p) / ND)
        assert abs(share - p) <= 5 * sigma, (s, share, p)
    assert z[:, 0].min() == 0 and z[:, 0].max() == 26 and set(z[:, 0]) == set(range(27))
    assert z[:, 1].min() == -5 and z[:, 1].max() == 4 and set(z[:, 1]) == set(range(-5, 5))
    # style and (r0, dr) are independent words of the draw: every slope occurs with every style
    assert len({(int(a), int(b)) for a, b in zip(st, z[:, 1])}) == 60
    # the images are what their drawn style makes of them
    for s in (0, 1, 3, 4, 5):
        pick = np.nonzero(st == s)[0][:64]
        for i in pick:
            assert np.array_equal(out[i], singles[s][i % N]), (i, s)


def test_k_style_table_never_yields_a_zero_probability_style(big):
    seeded(12)
    g = np.random.default_rng(2)
    table = np.zeros((10, 6), dtype=np.float32)
    for c in range(10):
        keep = g.choice(6, size=1 + c % 3, replace=False)
        table[c, keep] = 1.0 / len(keep)
    table[9] = [0, 0, 0, 0, 0, 1]
    table[8] = [1, 0, 0, 0, 0, 0]
    table[7] = [0, 0, 0.5, 0.5, 0, 0]
    labels = torch.tensor(g.integers(0, 10, size=ND), device="cuda")
    _, st, _ = run(big, SIX, SIX_SEV, table=torch.tensor(table, device="cuda"), labels=labels)
    lab = labels.cpu().numpy()
    assert (table[lab, st] > 0).all()
    for c in range(10):  # and every allowed style of a class does occur
        assert set(st[lab == c]) == set(np.nonzero(table[c])[0]), c


def test_draws_are_reproducible_and_advance(big):
    table = torch.tensor([PROBS], device="cuda")
    seeded(13)
    a = run(big[:1024], SIX, SIX_SEV, table=table)
    b = run(big[:1024], SIX, SIX_SEV, table=table)  # no reset: the counter moved on
    seeded(13)
    c = run(big[:1024], SIX, SIX_SEV, table=table)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2]) and not np.array_equal(a[0], b[0])
    seeded(14)
    d = run(big[:1024], SIX, SIX_SEV, table=table)
    assert not np.array_equal(a[1], d[1])


def test_labels_must_index_the_table(dimgs):
    labels = torch.zeros(N, dtype=torch.int64, device="cuda")
    labels[5] = 3
    with pytest.raises(IndexError):
        run(dimgs, SIX, SIX_SEV, table=torch.tensor([PROBS] * 3, device="cuda"), labels=labels)
    with pytest.raises(IndexError):
        run(dimgs, SIX, SIX_SEV, style=np.full(N, 6, dtype=np.int32))
    with pytest.raises(ValueError):
        run(dimgs[:, :, :27].contiguous(), SIX, SIX_SEV)


# ------------------------------------------------------------------------------------------------ public path
def test_public_path(imgs):
    from src.utils.data_utils import DeviceLoader, DeviceStyledMNIST, generate_style_dict

    seeded(15)
    labels = np.arange(N) % 10
    styles = {"identity": 0.15, "stripe": 0.2, "zigzag": 0.25, "canny_edges": 0.1, ("scale", 5): 0.1,
              "brightness": 0.2}
    ds = DeviceStyledMNIST(np.array(imgs), labels, styles)
    assert len(ds) == N and ds.images.shape == (N, 1, 28, 28) and ds.images.dtype == torch.float32
    assert ds.images.is_cuda and float(ds.images.min()) >= 0.0 and float(ds.images.max()) <= 1.0
    assert ds.styles.dtype == torch.int64 and int(ds.styles.min()) >= 0 and int(ds.styles.max()) <= 5
    # every image is its style's function of the digit, / 255
    st = ds.styles.cpu().numpy()
    zz = ds.zigzag.cpu().numpy()
    got = ds.images.cpu().numpy()[:, 0] * np.float32(255.0)
    for i in range(N):
        name, sev = ds.style_specs[st[i]]
        if name == "canny_edges":
            continue  # (test_canny)
        ref = (SR.zigzag(imgs[i], *map(int, zz[i])) if name == "zigzag" else
               getattr(SR, name)(imgs[i], sev) if name in ("scale", "brightness") else getattr(SR, name)(imgs[i]))
        assert np.abs(got[i] - ref).max() <= (1e-2 if name == "zigzag" else 1e-3), (i, name)

    x, y, s = ds[-1]
    assert torch.equal(x, ds.images[N - 1]) and int(y) == labels[-1] and int(s) == st[-1]
    assert ds[0][0].shape == (1, 28, 28)
    with pytest.raises(IndexError):
        ds[N]
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([0, N], device="cuda"))

    loader = DeviceLoader(ds, batch_size=50, shuffle=True)
    torch.manual_seed(21)
    batches = list(loader)
    torch.manual_seed(21)
    order = torch.randperm(N, device="cuda")
    assert len(loader) == 3 and [b[0].shape[0] for b in batches] == [50, 50, 28]
    for k, (X, lab, sty) in enumerate(batches):
        idx = order[50 * k:50 * k + 50]
        assert X.dtype == torch.float32 and X.shape[1:] == (1, 28, 28)
        assert 0.0 <= float(X.min()) <= float(X.max()) <= 1.0
        assert torch.equal(X, ds.images[idx]) and torch.equal(lab, ds.labels[idx]) and torch.equal(sty, ds.styles[idx])

    # KStyledMNISTGenerator semantics: the style is one of style_dict[label][split]
    np.random.seed(5)
    names = ["identity", "stripe", "zigzag", "canny_edges"]
    sd = generate_style_dict(range(10), list(range(4)), 2)
    for split in ("train", "test"):
        kds = DeviceStyledMNIST(np.array(imgs), labels, names, style_dict=sd, split=split)
        ks = kds.styles.cpu().numpy()
        assert all(ks[i] in sd[labels[i]][split] for i in range(N))

    # one fused CLEAR-VAE step takes a batch from the loader
    from cvhip.engine import ClearStep
    from src.utils.trainer_utils import get_clearvae_trainer

    dev = torch.device("cuda", 0)
    tr = get_clearvae_trainer(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=16, alpha=100, temperature=0.1, device=dev)
    eng = ClearStep.build(tr, "clear")
    assert eng is not None
    X, lab, _ = batches[0]
    L = eng.step(X, lab).cpu()
    assert torch.isfinite(L).all() and float(L[0]) > 0
