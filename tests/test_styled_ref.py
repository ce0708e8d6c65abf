"""Pins tests/styled_ref.py, the fp64 restatement the device Styled-MNIST generator is tested against, by facts that
can be checked by hand (no GPU)."""

import numpy as np
import pytest

import styled_ref as SR


@pytest.fixture(scope="module")
def imgs():
    return SR.synth(16, 7)


def test_synth_is_stroke_like(imgs):
    assert imgs.dtype == np.uint8 and imgs.shape == (16, 28, 28)
    assert 100 < (imgs > 0).sum(axis=(1, 2)).mean() < 600
    assert (imgs == 255).any() and np.array_equal(imgs, SR.synth(16, 7))


def test_identity_and_stripe_exact(imgs):
    for x in imgs:
        assert np.array_equal(SR.identity(x), x.astype(np.float32))
        s = SR.stripe(x)
        assert s.dtype == np.float32
        assert np.array_equal(s[:, 7:21], x[:, 7:21].astype(np.float32))
        assert np.array_equal(s[:, :7], 255.0 - x[:, :7].astype(np.float32))
        assert np.array_equal(s[:, 21:], 255.0 - x[:, 21:].astype(np.float32))


def test_scale5_is_the_box_mean(imgs):
    for x in imgs:
        v = x.astype(np.float64)
        box = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]) / 4.0
        want = np.zeros((28, 28))
        want[7:21, 7:21] = box
        assert np.allclose(SR.scale(x, 5), want, rtol=0, atol=1e-4)


def test_scale_fixes_the_centre():
    # the map keeps 13.5 fixed: a constant image stays constant wherever all four corners are inside
    x = np.full((28, 28), 200, dtype=np.uint8)
    y = SR.scale(x, 3)
    lo = int(np.ceil(13.5 - 13.5 * 0.7)) + 1
    assert np.allclose(y[lo:28 - lo, lo:28 - lo], 200.0, atol=1e-4)
    assert y[0, 0] == 0.0 and y[27, 27] == 0.0


@pytest.mark.parametrize("sev", [1, 2, 5])
def test_brightness(imgs, sev):
    for x in imgs:
        want = np.minimum(x.astype(np.float64) + 25.5 * sev, 255.0)
        assert np.allclose(SR.brightness(x, sev), want, rtol=0, atol=1e-4)
    assert np.allclose(SR.brightness(imgs[0]), np.minimum(imgs[0] + 127.5, 255.0), rtol=0, atol=1e-4)


@pytest.mark.parametrize("r0", [0, 13, 26])
def test_zigzag_flat_stays_in_its_band(r0):
    x = np.zeros((28, 28), dtype=np.uint8)
    y = SR.zigzag(x, r0, 0)
    touched = y > 0
    assert touched.any() and y.max() == 255.0
    rows, cols = np.nonzero(touched)
    assert cols.min() >= 2 and cols.max() <= 24
    assert rows.min() >= max(r0 - 4, 0) and rows.max() <= min(r0 + 4, 27)
    # the first tooth climbs from (column 2, row r0) to (column 4, row r0 + 2): on the line the term is 1
    if r0 + 2 <= 27:
        assert y[r0, 2] == 255.0 and y[r0 + 1, 3] == 255.0


def test_zigzag_has_seven_segments_for_every_slope():
    for dr in range(-5, 5):
        cs, rs = SR.zigzag_polyline(0, dr)
        assert len(cs) == 8 and np.all(np.diff(cs) > 0), dr
        assert cs[0] == 2.0 and rs[0] == 0.0
        if dr == 0:
            assert np.array_equal(cs, np.round(cs))
        else:  # no endpoint column close enough to an integer for its floor / ceil to be in doubt
            assert np.abs(cs[1:] - np.round(cs[1:])).min() > 0.01, dr


def test_zigzag_only_adds(imgs):
    for i, x in enumerate(imgs):
        y = SR.zigzag(x, i % 27, i % 10 - 5)
        assert (y >= x.astype(np.float32) - 1e-4).all() and y.max() <= 255.0


def test_canny_blank_is_empty():
    out, margin = SR.canny(np.zeros((28, 28), dtype=np.uint8))
    assert not out.any()
    assert margin == pytest.approx(0.1)
    assert not SR.canny(np.full((28, 28), 255, dtype=np.uint8))[0].any()  # (the bleed-over division flattens it)


def test_canny_square_gives_a_closed_ring():
    x = np.zeros((28, 28), dtype=np.uint8)
    x[8:20, 8:20] = 255
    out, _ = SR.canny(x)
    edge = out > 0
    assert set(np.unique(out)) == {0.0, 255.0}
    lab, count = SR.ndi.label(edge, np.ones((3, 3), bool))
    assert count == 1
    # closed: the ring separates the square's centre from the image corner (4-connected background)
    bg, _ = SR.ndi.label(~edge)
    assert bg[14, 14] != bg[0, 0] and not edge[14, 14]
    # it lies on the square's outline
    rows, cols = np.nonzero(edge)
    assert rows.min() >= 6 and rows.max() <= 21 and cols.min() >= 6 and cols.max() <= 21
    assert not edge[10:18, 10:18].any()


def test_canny_values_and_margin(imgs):
    for x in imgs:
        out, margin = SR.canny(x)
        assert out.dtype == np.float32 and set(np.unique(out)) <= {0.0, 255.0}
        assert 0.0 <= margin <= 0.1
        assert out[0].sum() == out[-1].sum() == out[:, 0].sum() == out[:, -1].sum() == 0.0
    assert sum(SR.canny(x)[0].any() for x in imgs) == len(imgs)


def test_hysteresis_and_spiral():
    state, length = SR.spiral_candidates()
    assert length > 350 and (state == 2).sum() == 1 and (state > 0).sum() == length
    kept = SR.hysteresis(state)
    assert kept.sum() == length  # one chain: the strong end keeps all of it
    weak_only = np.where(state == 2, 0, state)
    assert not SR.hysteresis(weak_only).any()
    # every pixel of the chain but its two ends has exactly two chain neighbours on its own row / column
    nb4 = sum(np.roll(np.pad(state > 0, 1), s, a)[1:-1, 1:-1] for s in (-1, 1) for a in (0, 1))
    assert ((nb4[state > 0] == 2).sum(), (nb4[state > 0] == 1).sum()) == (length - 2, 2)
