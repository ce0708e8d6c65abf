"""The paper's two figures on the device: the feature-swapping grid and the style / content interpolation strips of
the reference's ``expr/visual_utils.py`` (``feature_swapping_plot`` :29-58, ``interpolation_plot`` :61-128,
``make_colored_grid`` :13-26), composed by csrc/cv_figure.hip without torchvision.

    pair_latents     cv_latent_pairs: the n x n swap latents, row i n + j = (z_c[i], z_s[j])
    interp_latents   cv_latent_interp: every latent of the interpolation loop, ``[2, S, T, D]``, in one launch
    make_grid        cv_make_grid: ``torchvision.utils.make_grid(images, nrow, padding, pad_value=...)`` (without
                     ``normalize`` / ``scale_each``) with ``make_colored_grid``'s recolouring as ``frame``, optionally
                     written into a sub-rectangle of a larger canvas (``out``, ``origin``)
    swap_figure      the feature-swapping figure from the images and their n x n decodes: four launches
    interp_figure    one interpolation strip from the source / target images and the S x T decodes: five launches

Two things are kept from the reference on purpose.  ``frame="red"`` is not red: ``make_colored_grid`` sets channel 0
to 1 where it is 0.25 and then tests channel 0 again for the other two channels, which no longer matches, so the frame
is (1, 0.25, 0.25).  And the recolouring goes by value: an image pixel that is exactly 0.25 in the tested channel
(channel 0 for red, channel 2 for blue) is recoloured with the padding.  A single image (``M == 1``) comes back
without padding, as torchvision returns it.

Every function raises ``ValueError`` before anything is launched: shapes and dtypes are checked first, then that the
tensors are on the ROCm device.  Inputs are fp32; images are made contiguous."""

from __future__ import annotations

import torch

from . import _lib

MAX_IMAGES = 65536
MAX_SIDE = 4096
SPACER = 8  # white columns between the strips' frames and their grid (visual_utils.py:80)


def _require_gpu(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError("clear-vae_amd: HIP kernels need tensors on the ROCm device ('cuda')")


def _tensors(name: str, *ts):
    for t in ts:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected torch tensors (got {type(t).__name__}); "
                             "clear-vae_amd: HIP kernels need tensors on the ROCm device ('cuda')")


def _rows(name: str, x: torch.Tensor) -> torch.Tensor:
    """A 2-D fp32 ``x`` with unit column stride and a row stride >= its width (a column slice passes as it is)."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{name}: expected a 2-D float32 tensor (got {tuple(x.shape)}, {x.dtype})")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _ld(x: torch.Tensor) -> int:
    return max(int(x.stride(0)), int(x.shape[1]))  # (a single row's stride is arbitrary)


def pair_latents(z_c: torch.Tensor, z_s: torch.Tensor) -> torch.Tensor:
    """``[n * n, dc + ds]``: row ``i * n + j`` is ``(z_c[i], z_s[j])``, bit for bit: the reference's
    ``cat((z_c[:, None].repeat(1, n, 1), z_s[None].repeat(n, 1, 1)), -1).view(-1, dc + ds)`` in one launch with no
    intermediate.  ``z_c`` ``[n, dc]`` and ``z_s`` ``[n, ds]`` may be column slices of one tensor (no copy is made)."""
    _tensors("pair_latents", z_c, z_s)
    z_c, z_s = _rows("pair_latents", z_c.detach()), _rows("pair_latents", z_s.detach())
    n, dc = z_c.shape
    if z_s.shape[0] != n:
        raise ValueError(f"pair_latents: z_c has {n} rows, z_s has {z_s.shape[0]}")
    ds = z_s.shape[1]
    if n < 1 or dc < 1 or ds < 1:
        raise ValueError("pair_latents: z_c and z_s must not be empty")
    if n * n * (dc + ds) >= 2 ** 31:
        raise ValueError("pair_latents: n * n * (dc + ds) must be below 2^31")
    _require_gpu(z_c, z_s)
    out = torch.empty((n * n, dc + ds), dtype=torch.float32, device=z_c.device)
    _lib.call("cv_latent_pairs", z_c.data_ptr(), _ld(z_c), z_s.data_ptr(), _ld(z_s), n, dc, ds, out.data_ptr(),
              _lib.stream_handle())
    return out


def _ids(name: str, ids, s: int | None) -> torch.Tensor:
    t = torch.as_tensor(ids)
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool or t.numel() < 1:
        raise ValueError(f"{name}: the ids must be a non-empty 1-D integer sequence")
    if s is not None and t.numel() != s:
        raise ValueError(f"{name}: src_ids and tgt_ids must have the same length ({s} and {t.numel()})")
    return t


def interp_latents(z: torch.Tensor, z_dim: int, src_ids, tgt_ids, steps: int) -> torch.Tensor:
    """``[2, S, steps, D]``: with ``z1 = z[src_ids[i]]``, ``z2 = z[tgt_ids[i]]`` and ``p = linspace(1, 0, steps)``,
    ``out[0, i, k] = (z1[:z_dim], p_k z1[z_dim:] + (1 - p_k) z2[z_dim:])`` (style interpolation) and
    ``out[1, i, k] = (p_k z1[:z_dim] + (1 - p_k) z2[:z_dim], z1[z_dim:])`` (content interpolation): every
    ``z_combined`` of the reference's loop.  The ids (a tensor on either device, or a sequence) are checked against
    ``[0, N)`` here: on the host when they are there, else with one read-back of their minimum and maximum."""
    _tensors("interp_latents", z)
    z = _rows("interp_latents", z.detach())
    n, d = z.shape
    z_dim, steps = int(z_dim), int(steps)
    if n < 1 or not 1 <= z_dim < d:
        raise ValueError(f"interp_latents: z_dim={z_dim} must be in 1..{d - 1} and z must have rows")
    if steps < 1:
        raise ValueError(f"interp_latents: steps={steps} must be at least 1")
    src = _ids("interp_latents", src_ids, None)
    tgt = _ids("interp_latents", tgt_ids, src.numel())
    s = src.numel()
    if 2 * s * steps * d >= 2 ** 31:
        raise ValueError("interp_latents: 2 * S * steps * D must be below 2^31")
    _require_gpu(z)
    both = torch.cat([src.to(torch.int64).reshape(-1), tgt.to(device=src.device, dtype=torch.int64).reshape(-1)])
    lo, hi = (int(v) for v in torch.stack([both.min(), both.max()]).cpu())  # (the one read-back, if on the device)
    if lo < 0 or hi >= n:
        raise ValueError(f"interp_latents: ids must be in [0, {n}) (got {lo}..{hi})")
    both = both.to(z.device)
    out = torch.empty((2, s, steps, d), dtype=torch.float32, device=z.device)
    _lib.call("cv_latent_interp", z.data_ptr(), _ld(z), n, d, z_dim, both.data_ptr(), both[s:].data_ptr(), s, steps,
              out.data_ptr(), _lib.stream_handle())
    return out


def _images(name: str, images: torch.Tensor) -> torch.Tensor:
    """The shape and dtype checks of an image batch (the device is checked by the caller, after every shape)."""
    _tensors(name, images)
    if images.dim() != 4:
        raise ValueError(f"{name}: images must be [M, C, H, W] (got {tuple(images.shape)})")
    if images.dtype != torch.float32:
        raise ValueError(f"{name}: images must be float32 (got {images.dtype})")
    m, c, h, w = images.shape
    if c not in (1, 3):
        raise ValueError(f"{name}: images must have 1 or 3 channels (C={c})")
    if not 1 <= m <= MAX_IMAGES:
        raise ValueError(f"{name}: the number of images must be in 1..{MAX_IMAGES} (M={m})")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"{name}: H and W must be in 1..{MAX_SIDE} (H={h}, W={w})")
    return images.detach()


def grid_size(m: int, h: int, w: int, nrow: int = 8, padding: int = 2):
    """``(height, width)`` of ``make_grid``'s result for ``m`` images of ``h x w``."""
    if m == 1:
        return h, w
    xmaps = min(nrow, m)
    ymaps = -(-m // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def _canvas(name: str, out: torch.Tensor):
    _tensors(name, out)
    if out.dim() != 3 or out.shape[0] != 3 or out.dtype != torch.float32:
        raise ValueError(f"{name}: out must be a float32 [3, Hd, Wd] tensor (got {tuple(out.shape)}, {out.dtype})")
    _, hd, wd = out.shape
    cp, rp = out.stride(0), out.stride(1)
    if hd < 1 or wd < 1 or out.stride(2) != 1 or rp < wd or cp < hd * rp:
        raise ValueError(f"{name}: out must have unit column stride and non-overlapping rows and channels")
    if 2 * cp + hd * rp >= 2 ** 31:
        raise ValueError(f"{name}: out must span fewer than 2^31 elements")
    return hd, wd, cp, rp


def _place(name, out, origin, gh, gw):
    hd, wd, cp, rp = _canvas(name, out)
    y0, x0 = (int(v) for v in origin)
    if y0 < 0 or x0 < 0 or y0 + gh > hd or x0 + gw > wd:
        raise ValueError(f"{name}: the {gh} x {gw} grid at ({y0}, {x0}) does not fit out ({hd} x {wd})")
    return hd, wd, cp, rp, y0, x0


def _frame(name: str, frame):
    if frame not in _lib.FRAME:
        raise ValueError(f"{name}: frame must be None, 'red' or 'blue' (got {frame!r})")
    return _lib.FRAME[frame]


def make_grid(images: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value: float = 0.0, frame=None,
              out: torch.Tensor | None = None, origin=(0, 0)) -> torch.Tensor:
    """``torchvision.utils.make_grid(images, nrow=nrow, padding=padding, pad_value=pad_value)`` as a ``[3, Hg, Wg]``
    tensor (a single-channel batch is written to all three channels; one image comes back unpadded), recoloured as
    ``make_colored_grid`` does it when ``frame`` is ``"red"`` or ``"blue"`` (module docstring).  With ``out`` (fp32
    ``[3, Hd, Wd]``, unit column stride) the grid is written with its top left corner at ``origin = (y0, x0)``,
    nothing else of ``out`` is touched, and the view of ``out`` that holds the grid is returned."""
    images = _images("make_grid", images)
    nrow, padding = int(nrow), int(padding)
    if nrow < 1:
        raise ValueError(f"make_grid: nrow={nrow} must be at least 1")
    if padding < 0:
        raise ValueError(f"make_grid: padding={padding} must not be negative")
    fr = _frame("make_grid", frame)
    m, c, h, w = images.shape
    gh, gw = grid_size(m, h, w, nrow, padding)
    if out is None:
        if 3 * gh * gw >= 2 ** 31:
            raise ValueError("make_grid: the grid must have fewer than 2^31 elements")
        _require_gpu(images)
        out = torch.empty((3, gh, gw), dtype=torch.float32, device=images.device)
        origin = (0, 0)
    hd, wd, cp, rp, y0, x0 = _place("make_grid", out, origin, gh, gw)
    _require_gpu(images, out)
    images = images.contiguous()
    _lib.call("cv_make_grid", images.data_ptr(), m, c, h, w, nrow, padding, float(pad_value), fr, _lib.GRID_IMAGES,
              out.data_ptr(), hd, wd, cp, rp, y0, x0, _lib.stream_handle())
    return out[:, y0:y0 + gh, x0:x0 + gw]


def fill(out: torch.Tensor, origin, size, value: float, frame=None) -> torch.Tensor:
    """Set the ``size = (h, w)`` rectangle of every channel of ``out`` at ``origin`` to ``value`` (CV_GRID_FILL)."""
    h, w = (int(v) for v in size)
    if h < 1 or w < 1:
        raise ValueError(f"fill: the rectangle must not be empty ({h} x {w})")
    fr = _frame("fill", frame)
    hd, wd, cp, rp, y0, x0 = _place("fill", out, origin, h, w)
    _require_gpu(out)
    _lib.call("cv_make_grid", None, 0, 3, h, w, 1, 0, float(value), fr, _lib.GRID_FILL, out.data_ptr(), hd, wd, cp,
              rp, y0, x0, _lib.stream_handle())
    return out[:, y0:y0 + h, x0:x0 + w]


def _same_images(name, a, b):
    if a.shape[1:] != b.shape[1:]:
        raise ValueError(f"{name}: the image batches must agree in [C, H, W] ({tuple(a.shape)} and "
                         f"{tuple(b.shape)})")


def swap_figure(X: torch.Tensor, decoded: torch.Tensor) -> torch.Tensor:
    """The feature-swapping figure (visual_utils.py:38-52), ``[3, (H+4) + n(H+2) + 2, (W+4) + n(W+2) + 2]``: a white
    ``(H+4) x (W+4)`` corner, the red-framed column of ``X`` below it, the blue-framed row of ``X`` to its right and
    the ``n x n`` grid of ``decoded`` (``[n * n, C, H, W]``, row-major: image ``i n + j`` has the content of ``X[i]``
    and the style of ``X[j]``).  ``n >= 2``: a single image would come unpadded and the parts would not fit."""
    X, decoded = _images("swap_figure", X), _images("swap_figure", decoded)
    _same_images("swap_figure", X, decoded)
    n, _, h, w = X.shape
    if n < 2:
        raise ValueError("swap_figure: needs at least 2 images (n >= 2)")
    if decoded.shape[0] != n * n:
        raise ValueError(f"swap_figure: decoded must hold n * n = {n * n} images (got {decoded.shape[0]})")
    gh, gw = grid_size(n * n, h, w, n)
    if 3 * (h + 4 + gh) * (w + 4 + gw) >= 2 ** 31:
        raise ValueError("swap_figure: the figure must have fewer than 2^31 elements")
    _require_gpu(X, decoded)
    fig = torch.empty((3, h + 4 + gh, w + 4 + gw), dtype=torch.float32, device=X.device)
    fill(fig, (0, 0), (h + 4, w + 4), 1.0)
    make_grid(X, nrow=1, pad_value=0.25, frame="red", out=fig, origin=(h + 4, 0))
    make_grid(X, nrow=n, pad_value=0.25, frame="blue", out=fig, origin=(0, w + 4))
    make_grid(decoded, nrow=n, out=fig, origin=(h + 4, w + 4))
    return fig


def interp_figure(X_src: torch.Tensor, X_tgt: torch.Tensor, decoded: torch.Tensor,
                  like: torch.Tensor | None = None) -> torch.Tensor:
    """One interpolation strip (visual_utils.py:74-82, :112-118),
    ``[3, S(H+2) + 2, (W+4) + 8 + T(W+2) + 2 + 8 + (W+4)]``: the red-framed column of the ``S`` source images, 8 white
    columns, the ``S x T`` grid of ``decoded`` (``[S * T, C, H, W]``, ``T`` images per row), 8 white columns and the
    blue-framed column of the target images.  ``S >= 2``.

    ``like``: a strip this function made from the same ``X_src`` / ``X_tgt`` and as many decodes.  Everything but the
    middle grid is the same in both, so it is copied from ``like`` (one device copy) instead of composed again."""
    X_src, X_tgt, decoded = (_images("interp_figure", t) for t in (X_src, X_tgt, decoded))
    _same_images("interp_figure", X_src, decoded)
    if X_src.shape != X_tgt.shape:
        raise ValueError(f"interp_figure: X_src and X_tgt differ in shape ({tuple(X_src.shape)} and "
                         f"{tuple(X_tgt.shape)})")
    s, _, h, w = X_src.shape
    if s < 2:
        raise ValueError("interp_figure: needs at least 2 source images (S >= 2)")
    if decoded.shape[0] % s:
        raise ValueError(f"interp_figure: decoded must hold S * T images ({decoded.shape[0]} is no multiple of {s})")
    t = decoded.shape[0] // s
    gh, gw = grid_size(s * t, h, w, t)
    side = w + 4
    shape = (3, gh, side + SPACER + gw + SPACER + side)
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError("interp_figure: the figure must have fewer than 2^31 elements")
    _require_gpu(X_src, X_tgt, decoded)
    if like is not None:
        _require_gpu(like)
        if tuple(like.shape) != shape or like.dtype != torch.float32 or like.device != X_src.device:
            raise ValueError(f"interp_figure: like must be a float32 {list(shape)} strip on the images' device")
        fig = like.clone(memory_format=torch.contiguous_format)
    else:
        fig = torch.empty(shape, dtype=torch.float32, device=X_src.device)
        make_grid(X_src, nrow=1, pad_value=0.25, frame="red", out=fig, origin=(0, 0))
        fill(fig, (0, side), (gh, SPACER), 1.0)
        fill(fig, (0, side + SPACER + gw), (gh, SPACER), 1.0)
        make_grid(X_tgt, nrow=1, pad_value=0.25, frame="blue", out=fig, origin=(0, side + SPACER + gw + SPACER))
    make_grid(decoded, nrow=t, out=fig, origin=(0, side + SPACER))
    return fig
