"""fp64 numpy / scipy.ndimage restatement of the six Styled-MNIST style functions, the yardstick of
tests/test_gpu_styled.py, pinned by hand-checkable facts in tests/test_styled_ref.py.  Not a test module.

Every function takes one uint8 (or integer-valued) 28x28 image and returns the float32 image in [0, 255] that the
style function returns.  canny() also returns the image's decision margin; synth() makes the stroke images the tests
use (no MNIST file is needed)."""

import numpy as np
from scipy import ndimage as ndi

SIDE = 28
SCALE_FACTOR = {1: 1 / 0.9, 2: 1 / 0.8, 3: 1 / 0.7, 4: 1 / 0.6, 5: 1 / 0.5}


def identity(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def stripe(x):
    y = np.asarray(x, dtype=np.float64).copy()
    y[:, :7] = 255.0 - y[:, :7]
    y[:, 21:] = 255.0 - y[:, 21:]
    return y.astype(np.float32)


def brightness(x, severity=5):
    v = np.asarray(x, dtype=np.float64) / 255.0
    return (np.minimum(v + 0.1 * severity, 1.0) * 255.0).astype(np.float32)


def sample_bilinear(img, rows, cols):
    """img at the real coordinates (rows[i], cols[j]); a corner outside the image counts 0."""
    r0 = np.floor(rows).astype(int)
    c0 = np.floor(cols).astype(int)
    tr = (rows - r0)[:, None]
    tc = (cols - c0)[None, :]
    pad = np.zeros((SIDE + 2, SIDE + 2))
    pad[1:-1, 1:-1] = img

    def at(r, c):  # 0 outside [0, 28)
        return pad[np.clip(r + 1, 0, SIDE + 1)[:, None], np.clip(c + 1, 0, SIDE + 1)[None, :]]

    top = (1 - tc) * at(r0, c0) + tc * at(r0, c0 + 1)
    bot = (1 - tc) * at(r0 + 1, c0) + tc * at(r0 + 1, c0 + 1)
    return (1 - tr) * top + tr * bot


def scale(x, severity=3):
    s = SCALE_FACTOR[severity]
    v = np.asarray(x, dtype=np.float64) / 255.0
    coord = s * np.arange(SIDE, dtype=np.float64) + 13.5 * (1.0 - s)
    return (np.clip(sample_bilinear(v, coord, coord), 0.0, 1.0) * 255.0).astype(np.float32)


def zigzag_polyline(r0, dr):
    """(columns, rows) of the zigzag's endpoints: teeth of half-length 2 and height +-2 along the line from
    (column 2, row r0) to (column 25, row r0 + dr), plus the last partial tooth."""
    theta = np.arctan(dr / 23.0)
    d = 23.0 / np.cos(theta)
    u, v = [0.0], [0.0]
    for i in range(int(np.floor((d - 2.0) / 4.0)) + 1):  # the teeth's tips, at odd multiples of 2 along the line
        u.append((2 * i + 1) * 2.0)
        v.append(2.0 if i % 2 == 0 else -2.0)
    whole = 4.0 * np.floor(d / 4.0)
    if d != whole:
        u.append(d)
        v.append(v[-1] / (2.0 * (d - whole)))
    u, v = np.array(u), np.array(v)
    cs = np.cos(theta) * u - np.sin(theta) * v + 2.0
    rs = np.sin(theta) * u + np.cos(theta) * v + r0
    return cs, rs


def zigzag_term(c0, r0, c1, r1):
    """What one segment adds: 1 on the line, log-decaying to 0 at distance 2.3 (1 - 1/e), inside its columns."""
    cc = np.arange(SIDE, dtype=np.float64)[None, :]
    rr = np.arange(SIDE, dtype=np.float64)[:, None]
    m = (r1 - r0) / (c1 - c0)
    dist = np.clip(np.abs(rr - (m * (cc - c0) + r0)), 0.0, 2.3 - 1e-10)
    term = np.clip(np.log(1.0 - dist / 2.3) + 1.0, 0.0, 1.0)
    lo, hi = int(np.floor(c0)), int(np.ceil(c1))
    term[:, :lo] = 0.0
    term[:, hi:] = 0.0
    return term


def zigzag(x, r0, dr):
    v = np.asarray(x, dtype=np.float64) / 255.0
    cs, rs = zigzag_polyline(r0, dr)
    for i in range(1, len(cs)):
        v = np.clip(v + zigzag_term(cs[i - 1], rs[i - 1], cs[i], rs[i]), 0.0, 1.0)
    return (v * 255.0).astype(np.float32)


def hysteresis(state):
    """state 0 / 1 weak / 2 strong -> bool map of the candidates whose 8-connected component holds a strong one."""
    cand = state > 0
    lab, count = ndi.label(cand, np.ones((3, 3), bool))
    if count == 0:
        return cand
    good = np.zeros(count + 1, bool)
    good[np.unique(lab[state == 2])] = True
    good[0] = False
    return good[lab]


def canny_state(x, dtype=np.float64):
    """(state map 0 / 1 / 2, decision margin) of canny's front end on x / 255."""
    v = (np.asarray(x, dtype=np.float64) / 255.0).astype(dtype)
    blur = ndi.gaussian_filter(v, 1.0, mode="constant", cval=0.0)
    ones = ndi.gaussian_filter(np.ones_like(v), 1.0, mode="constant", cval=0.0)
    sm = blur / (ones + dtype(np.finfo(np.float64).eps))
    gi = ndi.sobel(sm, axis=0)
    gj = ndi.sobel(sm, axis=1)
    m = np.sqrt(gi * gi + gj * gj)
    state = np.zeros((SIDE, SIDE), dtype=np.uint8)
    margin = np.inf
    for r in range(1, SIDE - 1):
        for c in range(1, SIDE - 1):
            mv = m[r, c]
            margin = min(margin, abs(mv - 0.1))
            if not mv >= 0.1:
                continue
            a, b = gi[r, c], gj[r, c]
            same = (a >= 0 and b >= 0) or (a <= 0 and b <= 0)
            dd = 1 if same else -1  # the diagonal neighbour of a row step +1 lies dd columns over
            if abs(a) > abs(b):
                w = abs(b) / abs(a)
                n1 = m[r + 1, c + dd] * w + m[r + 1, c] * (1 - w)
                n2 = m[r - 1, c - dd] * w + m[r - 1, c] * (1 - w)
            else:
                w = abs(a) / abs(b)
                n1 = m[r + dd, c + 1] * w + m[r, c + 1] * (1 - w)
                n2 = m[r - dd, c - 1] * w + m[r, c - 1] * (1 - w)
            margin = min(margin, abs(n1 - mv), abs(n2 - mv))
            if n1 <= mv and n2 <= mv:
                margin = min(margin, abs(mv - 0.2))
                state[r, c] = 2 if mv >= 0.2 else 1
    return state, float(margin)


def canny(x, dtype=np.float64):
    """(float32 edge image in {0, 255}, decision margin: the smallest |m - 0.1|, |m - 0.2| and
    |m - interpolated neighbour| over the comparisons made on interior pixels)."""
    state, margin = canny_state(x, dtype)
    return hysteresis(state).astype(np.float32) * 255.0, margin


def synth(n, seed):
    """n uint8 stroke images: 2-4 random segments with endpoints uniform in [4, 24]^2 and width sigma uniform in
    [0.8, 1.6], intensity clip(1.6 exp(-d^2 / 2 sigma^2), 0, 1), the maximum over the segments."""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(SIDE, dtype=np.float64), np.arange(SIDE, dtype=np.float64), indexing="ij")
    out = np.zeros((n, SIDE, SIDE), dtype=np.uint8)
    for i in range(n):
        img = np.zeros((SIDE, SIDE))
        for _ in range(int(rng.integers(2, 5))):
            p, q = rng.uniform(4.0, 24.0, size=2), rng.uniform(4.0, 24.0, size=2)
            sigma = rng.uniform(0.8, 1.6)
            e = q - p
            t = np.clip(((rr - p[0]) * e[0] + (cc - p[1]) * e[1]) / max(float(e @ e), 1e-12), 0.0, 1.0)
            d2 = (rr - p[0] - t * e[0]) ** 2 + (cc - p[1] - t * e[1]) ** 2
            img = np.maximum(img, np.clip(1.6 * np.exp(-d2 / (2 * sigma * sigma)), 0.0, 1.0))
        out[i] = np.rint(img * 255.0).astype(np.uint8)
    return out


def spiral_candidates():
    """A one-pixel-wide rectangular spiral of weak candidates (1) over the whole 28x28 plane, turns two pixels
    apart so that they never touch, with a single strong pixel (2) at its inner end: (state map, chain length)."""
    state = np.zeros((SIDE, SIDE), dtype=np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    path = [(0, 0)]
    state[0, 0] = 1

    def free(rr, cc):  # inside, and no pixel of the path other than the last few next to it
        if not (0 <= rr < SIDE and 0 <= cc < SIDE) or state[rr, cc]:
            return False
        near = {(rr + a, cc + b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - set(path[-2:])
        return not any(0 <= a < SIDE and 0 <= b < SIDE and state[a, b] for a, b in near)

    while True:
        if free(r + dr, c + dc):
            r, c = r + dr, c + dc
        else:
            dr, dc = dc, -dr  # turn right
            if not free(r + dr, c + dc):
                break
            r, c = r + dr, c + dc
        state[r, c] = 1
        path.append((r, c))
    state[r, c] = 2
    return state, len(path)
