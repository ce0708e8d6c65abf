"""A restatement, in numpy on the host, of what cvhip.figures computes: torchvision.utils.make_grid's algorithm
(without normalize / scale_each), the recolouring of the reference's make_colored_grid and the compositions of its
feature_swapping_plot and interpolation_plot.  torchvision is not installed where these tests run, so this restatement
has not been compared with it; it follows make_grid's documented algorithm step by step.

Everything here moves values without arithmetic, so the device results must equal it bit for bit (NaNs compared by
position).  interp_ref is the one numeric piece: the interpolation latents in fp64."""

import math

import numpy as np


def make_grid(images: np.ndarray, nrow=8, padding=2, pad_value=0.0) -> np.ndarray:
    """images [M, C, H, W] float32 -> [3, Hg, Wg] float32."""
    images = np.asarray(images, dtype=np.float32)
    if images.shape[1] == 1:  # single-channel images are repeated over the three channels
        images = np.concatenate([images, images, images], axis=1)
    m, c, h, w = images.shape
    if m == 1:  # one image is returned as it is: no border
        return images[0].copy()
    xmaps = min(nrow, m)
    ymaps = int(math.ceil(float(m) / xmaps))
    height, width = h + padding, w + padding
    grid = np.full((c, height * ymaps + padding, width * xmaps + padding), pad_value, dtype=np.float32)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= m:
                break
            grid[:, y * height + padding:y * height + padding + h, x * width + padding:x * width + padding + w] = \
                images[k]
            k += 1
    return grid


def recolour(grid: np.ndarray, color: str) -> np.ndarray:
    """The reference's three masked assignments, one after the other, each evaluating its mask when it runs."""
    g = grid.copy()
    tested, values = {"red": (0, (1.0, 0.0, 0.0)), "blue": (2, (0.0, 0.0, 1.0))}[color]
    for ch in range(3):
        g[ch][g[tested] == np.float32(0.25)] = values[ch]
    return g


def colored_grid(images, nrow, color):
    return recolour(make_grid(images, nrow=nrow, pad_value=0.25), color)


def swap_figure(X: np.ndarray, decoded: np.ndarray) -> np.ndarray:
    n, _, h, w = X.shape
    hgrid = colored_grid(X, n, "blue")
    vgrid = colored_grid(X, 1, "red")
    main = make_grid(decoded, nrow=n)
    left = np.concatenate([np.ones((3, h + 4, w + 4), np.float32), vgrid], axis=1)
    right = np.concatenate([hgrid, main], axis=1)
    return np.concatenate([left, right], axis=2)


def strip(X_src: np.ndarray, X_tgt: np.ndarray, decoded: np.ndarray, steps: int) -> np.ndarray:
    src, tgt = colored_grid(X_src, 1, "red"), colored_grid(X_tgt, 1, "blue")
    space = np.ones((3, src.shape[1], 8), np.float32)
    return np.concatenate([src, space, make_grid(decoded, nrow=steps), space, tgt], axis=2)


def pairs(z_c: np.ndarray, z_s: np.ndarray) -> np.ndarray:
    n = z_c.shape[0]
    a = np.repeat(z_c[:, None, :], n, axis=1)
    b = np.repeat(z_s[None, :, :], n, axis=0)
    return np.concatenate([a, b], axis=-1).reshape(n * n, -1)


def linspace_1_0(steps: int) -> np.ndarray:
    """linspace(1, 0, steps) in exact arithmetic (fp64)."""
    if steps == 1:
        return np.ones(1)
    return 1.0 - np.arange(steps, dtype=np.float64) / (steps - 1)


def interp_ref(z: np.ndarray, z_dim: int, src, tgt, steps: int):
    """(out, mag): out [2, S, T, D] in fp64; mag [2, S, T, D] = |a| + |b| of the two values every element mixes."""
    z = z.astype(np.float64)
    p = linspace_1_0(steps)[None, :, None]
    z1, z2 = z[np.asarray(src)][:, None, :], z[np.asarray(tgt)][:, None, :]
    mix = p * z1 + (1.0 - p) * z2
    keep = np.broadcast_to(z1, mix.shape)
    style = np.concatenate([keep[..., :z_dim], mix[..., z_dim:]], axis=-1)
    content = np.concatenate([mix[..., :z_dim], keep[..., z_dim:]], axis=-1)
    mag = np.broadcast_to(np.abs(z1) + np.abs(z2), mix.shape)
    return np.stack([style, content]), np.stack([mag, mag])


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
