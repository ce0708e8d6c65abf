"""Device Styled-MNIST generation: the binding of cv_style_mnist (csrc/cv_style.hip).

The reference builds Styled-MNIST on the host, one PIL image at a time, through corruption_utils.corruptions
(skimage / wand / cv2; code/src/utils/data_utils.py:29-52, code/expr/expr_utils.py:18-32).  stylize() turns uint8
digits resident in HBM into the float32 corrupted images (the corruption functions' return values, in [0, 255]) and
the per-image style index in one launch; the style and the zigzag's (r0, dr) are drawn per image on the device from
the Philox stream of cvhip.rng (keyed by torch.initial_seed()).

Test hooks, in the spirit of rng.inject_*: style= gives the style of every image, zz= the zigzag (r0, dr), cand= the
canny candidate map (0 none, 1 weak, 2 strong) in place of the canny front end.
"""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, rng

KINDS = _lib.STYLE  # style name -> CV_STYLE_*
GRADED = ("scale", "brightness")  # the styles that take a severity in 1..5
SIDE = 28
ZZ_DR = tuple(range(-5, 5))  # np.random.randint(-5, 5)
ZZ_R0 = 27  # np.random.randint(0, 27): r0 in [0, 27)

_zz_cache: dict = {}


def zigzag_table():
    """The zigzag polylines of corruptions.py:665-704 for the ten slopes dr = -5..4 with r0 = 0, in fp64:
    (pts [10, 8, 2] (column, row) endpoints, cols [10, 7, 2] = every segment's (floor(c0), ceil(c1))).

    The polyline runs along the straight line from column 2 to column 25 that climbs dr rows: teeth of half-length
    2 and height +-2 along a baseline of length d = 23 / cos(theta), a last partial tooth, rotated by theta about the
    start point.  Every slope gives 8 endpoints (7 segments)."""
    pts = np.zeros((len(ZZ_DR), 8, 2))
    cols = np.zeros((len(ZZ_DR), 7, 2), dtype=np.int32)
    half = height = 2.0
    c_start, c_end = 2, 25
    for k, dr in enumerate(ZZ_DR):
        theta = np.arctan(dr / (c_end - c_start))
        d = (c_end - c_start) / np.cos(theta)
        teeth = int((d - half) // (2 * half)) + 1
        along = [0.0] + [(2 * i + 1) * half for i in range(teeth)]
        across = [0.0] + [(-1.0) ** i * height for i in range(teeth)]
        whole = (2 * half) * (d // (2 * half))
        if d != whole:
            along.append(d)
            across.append(across[-1] / (2 * (d - whole)))
        if len(along) != 8:
            raise AssertionError(f"zigzag dr={dr}: {len(along) - 1} segments, expected 7")
        rot = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        c, r = rot.dot(np.array([along, across]))
        pts[k, :, 0] = c + c_start
        pts[k, :, 1] = r
        cols[k, :, 0] = np.floor(pts[k, :-1, 0]).astype(np.int32)
        cols[k, :, 1] = np.ceil(pts[k, 1:, 0]).astype(np.int32)
    return pts, cols


def _zz_device(device):
    key = (device.type, device.index)
    t = _zz_cache.get(key)
    if t is None:
        pts, cols = zigzag_table()
        t = _zz_cache[key] = (torch.from_numpy(pts).to(device).contiguous(),
                              torch.from_numpy(cols).to(device).contiguous())
    return t


def check_kinds(kinds, severities):
    """(kind codes, severities) as int lists; ValueError for an unknown kind or a severity outside 1..5."""
    ks, ss = [], []
    if len(kinds) != len(severities):
        raise ValueError("one severity per kind")
    if not 1 <= len(kinds) <= 16:
        raise ValueError(f"{len(kinds)} styles: 1..16 are supported")
    for k, s in zip(kinds, severities):
        code = KINDS.get(k) if isinstance(k, str) else (int(k) if int(k) in KINDS.values() else None)
        if code is None:
            raise ValueError(f"unknown style {k!r}: one of {sorted(KINDS)}")
        s = int(s)
        if code in (KINDS["scale"], KINDS["brightness"]) and not 1 <= s <= 5:
            raise ValueError(f"severity {s} outside 1..5")
        ks.append(code)
        ss.append(s)
    return ks, ss


def _hook(t, shape, name, device):
    t = torch.as_tensor(t)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def stylize(images, labels, table, kinds, severities, style=None, zz=None, stream=None, *, cand=None):
    """images uint8 [n, 28, 28] and labels int64 [n] on the device, table float32 [n_class, n_style] (rows sum to 1),
    kinds / severities: n_style style names (or CV_STYLE_* codes) and severities -> (out float32 [n, 28, 28] in
    [0, 255], style int64 [n], zz int32 [n, 2] = the (r0, dr) of every image).

    Labels must index the table's rows: IndexError otherwise (one device read, as load_batch).  style (int [n]),
    zz (int [n, 2]) and cand (uint8 [n, 28, 28]) are the test hooks of the module docstring."""
    for name, t, dt in (("images", images, torch.uint8), ("labels", labels, torch.int64),
                        ("table", table, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"clear-vae_amd: stylize needs {name} as a tensor on the ROCm device")
        if t.dtype != dt:
            raise ValueError(f"{name}: dtype {t.dtype}, expected {dt}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if images.dim() != 3 or tuple(images.shape[1:]) != (SIDE, SIDE) or images.shape[0] < 1:
        raise ValueError(f"images: [n, {SIDE}, {SIDE}] with n >= 1, got {tuple(images.shape)}")
    n = images.shape[0]
    ks, ss = check_kinds(kinds, severities)
    if labels.shape != (n,):
        raise ValueError("one label per image")
    if table.dim() != 2 or table.shape[1] != len(ks) or table.shape[0] < 1:
        raise ValueError(f"table: [n_class, {len(ks)}], got {tuple(table.shape)}")
    dev = images.device
    if labels.device != dev or table.device != dev:
        raise ValueError("images, labels and table must be on one device")
    lo, hi = (int(v) for v in torch.aminmax(labels))
    if lo < 0 or hi >= table.shape[0]:
        raise IndexError(f"stylize: labels in [{lo}, {hi}] do not index the table's {table.shape[0]} rows")
    if style is not None:
        style = _hook(style, (n,), "style", dev)
        lo, hi = (int(v) for v in torch.aminmax(style))
        if lo < 0 or hi >= len(ks):
            raise IndexError(f"stylize: style in [{lo}, {hi}] for {len(ks)} styles")
    if zz is not None:
        zz = _hook(zz, (n, 2), "zz", dev)
        z = zz.cpu()
        if int(z[:, 0].min()) < 0 or int(z[:, 0].max()) >= ZZ_R0 or int(z[:, 1].min()) < ZZ_DR[0] \
                or int(z[:, 1].max()) > ZZ_DR[-1]:
            raise IndexError("stylize: zz outside r0 in [0, 26], dr in [-5, 4]")
    if cand is not None:
        cand = torch.as_tensor(cand)
        if tuple(cand.shape) != (n, SIDE, SIDE):
            raise ValueError(f"cand: shape {tuple(cand.shape)}, expected {(n, SIDE, SIDE)}")
        cand = cand.to(device=dev, dtype=torch.uint8).contiguous()
    pts, cols = _zz_device(dev)
    seed, off = rng.offset_tensor(dev)
    out = torch.empty(n, SIDE, SIDE, dtype=torch.float32, device=dev)
    style_out = torch.empty(n, dtype=torch.int64, device=dev)
    zz_out = torch.empty(n, 2, dtype=torch.int32, device=dev)
    karr = (ctypes.c_int * len(ks))(*ks)
    sarr = (ctypes.c_int * len(ss))(*ss)
    with torch.cuda.device(dev):
        _lib.call("cv_style_mnist", images.data_ptr(), n, SIDE, SIDE, labels.data_ptr(), table.data_ptr(),
                  table.shape[0], len(ks), karr, sarr, pts.data_ptr(), cols.data_ptr(), ctypes.c_uint64(seed),
                  off.data_ptr(), _lib.ptr(style), _lib.ptr(zz), _lib.ptr(cand), out.data_ptr(),
                  style_out.data_ptr(), zz_out.data_ptr(), _lib.stream_handle() if stream is None else stream)
    return out, style_out, zz_out
