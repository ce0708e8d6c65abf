"""The MI-bound study of the reference's ``code/mi_experiment.ipynb`` on the device: the bindings of ``cv_blobs`` and
``cv_snn_bounds`` (csrc/cv_bound.hip).

The notebook draws, per trial, 1500 points from three isotropic Gaussian blobs on the host (cell 3), moves them to
the GPU and evaluates its ``SNN`` / ``PSSNN`` modules (cell 2: ``losses.py:98-137`` with the cosine similarity) once
per temperature, 2 x 1100 trials in all.  :func:`gaussian_blobs` draws every trial in one launch and
:func:`snn_bounds` evaluates both bounds at every temperature for every trial in one pass over the pairs:

    u_j = x_j / max(|x_j|, 1e-8),  s_ij = u_i . u_j
    lse_all = log sum_{j != i} exp(s_ij / tau)     lse_pos: j != i with label_j == label_i     lse_neg: the rest
    SNN row term = lse_all - lse_pos               PS-SNN row term = lse_all - lse_neg
    bound = the mean over the rows whose term is finite, count = how many such rows there are

With no finite row the bound is NaN and the count 0 (the reference takes the mean of an empty tensor); a NaN anywhere
in a trial does that to the trial and leaves the others alone.  Forward only.
"""

from __future__ import annotations

import ctypes
import math

import torch

from . import _lib, rng

MAX_N = 65536
MAX_D = 64
MAX_T = 8
MAX_BLOBS = 16
_WORK: dict = {}


def _workspace(B: int, n: int, T: int, device) -> torch.Tensor:
    key = (B, n, T, device)
    w = _WORK.get(key)
    if w is None:
        nbytes = int(_lib.lib().cv_snn_bounds_workspace_bytes(B, n, T))
        w = _WORK[key] = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)
    return w


def _positive_floats(name: str, values) -> list:
    try:
        vals = [float(v) for v in values]
    except TypeError:
        vals = [float(values)]
    for v in vals:
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{name}: every value must be finite and positive (got {v})")
    return vals


def gaussian_blobs(stds, n_samples: int, dim: int = 3, centers=(-1.0, 2.0, 7.0), n_blobs: int = 3, out=None,
                   device=None):
    """``B = len(stds)`` independent draws of the notebook's ``generate_gaussian_blobs`` (cell 3) in one launch:
    ``(x [B, n, dim] fp32, label [n] int64)`` on the device with ``n = (n_samples // n_blobs) * n_blobs`` (the
    reference truncates the same way), ``label = arange(n) // (n // n_blobs)`` and
    ``x[b, i] = centers[label[i]] + stds[b] * eps``, eps standard normal from the library's Philox stream
    (``cvhip.rng``: keyed by ``torch.manual_seed``, the counter advances on the device by one per call).

    ``stds`` is a device fp32 ``[B]`` tensor (one small read checks that it is finite and positive) or a Python
    sequence, checked on the host and uploaded to ``device`` (default: the current ROCm device).  ``x`` is stored as
    ``[n, B, dim]`` and returned permuted, so ``x.permute(1, 0, 2).reshape(n, B * dim)`` is a view that
    :func:`cvhip.metrics.knn_mi` takes as it is.  ``out``: a device fp32 ``[B, n, dim]`` tensor to fill instead, in
    either storage order, with unit stride along ``dim``."""
    n_blobs, n_samples, dim = int(n_blobs), int(n_samples), int(dim)
    if not 1 <= n_blobs <= MAX_BLOBS:
        raise ValueError(f"gaussian_blobs: n_blobs must be in 1..{MAX_BLOBS} (got {n_blobs})")
    if n_samples < n_blobs:
        raise ValueError(f"gaussian_blobs: n_samples={n_samples} is fewer than the {n_blobs} blobs")
    if dim < 1:
        raise ValueError("gaussian_blobs: dim must be positive")
    cs = [float(c) for c in centers]
    if len(cs) < n_blobs or not all(math.isfinite(c) for c in cs):
        raise ValueError(f"gaussian_blobs: need {n_blobs} finite centers (got {cs})")
    on_device = isinstance(stds, torch.Tensor) and stds.device.type == "cuda"
    if isinstance(stds, torch.Tensor) and not on_device:
        raise ValueError("gaussian_blobs: a tensor of stds must be on the ROCm device ('cuda'); pass a sequence "
                         "to have it uploaded")
    if on_device:
        if stds.dim() != 1 or stds.dtype != torch.float32 or stds.numel() < 1:
            raise ValueError("gaussian_blobs: stds must be a non-empty 1-D float32 tensor")
    else:
        host = _positive_floats("gaussian_blobs: stds", stds)
        if not host:
            raise ValueError("gaussian_blobs: stds is empty")
    if out is not None and (not isinstance(out, torch.Tensor) or out.device.type != "cuda"):
        raise ValueError("gaussian_blobs: out must be a tensor on the ROCm device ('cuda')")
    # ---- nothing above touches the device
    if on_device:
        if not bool((torch.isfinite(stds) & (stds > 0)).all()):
            raise ValueError("gaussian_blobs: every std must be finite and positive")
        stds = stds.contiguous()
    else:
        stds = torch.tensor(host, dtype=torch.float32).to(torch.device(device if device is not None else "cuda"))
    dev = stds.device
    B = int(stds.numel())
    per = n_samples // n_blobs
    n = per * n_blobs
    if out is None:
        x = torch.empty((n, B, dim), dtype=torch.float32, device=dev).permute(1, 0, 2)
    else:
        x = out
        if tuple(x.shape) != (B, n, dim) or x.dtype != torch.float32 or x.device != dev:
            raise ValueError(f"gaussian_blobs: out must be float32 {(B, n, dim)} on {dev}")
        st, sr = x.stride(0), x.stride(1)
        if x.stride(2) != 1 or not ((sr >= dim and st >= n * sr) or (st >= dim and sr >= B * st)):
            raise ValueError("gaussian_blobs: out must be stored as [B][n][dim] or [n][B][dim] with unit stride "
                             "along dim")
    label = torch.arange(n, device=dev, dtype=torch.int64) // per
    seed, off = rng.offset_tensor(dev)
    carr = (ctypes.c_float * n_blobs)(*cs[:n_blobs])
    with torch.cuda.device(dev):
        _lib.call("cv_blobs", x.data_ptr(), x.stride(0), x.stride(1), B, n, dim, carr, n_blobs, stds.data_ptr(),
                  ctypes.c_uint64(seed), off.data_ptr(), _lib.stream_handle())
    return x, label


def check_taus(taus) -> list:
    """The temperatures as a list of floats; ``ValueError`` unless there are 1..8 of them, all finite and > 0."""
    if isinstance(taus, torch.Tensor):
        taus = taus.detach().cpu().reshape(-1).tolist()
    vals = _positive_floats("snn_bounds: taus", taus)
    if not 1 <= len(vals) <= MAX_T:
        raise ValueError(f"snn_bounds: need 1..{MAX_T} temperatures (got {len(vals)})")
    for v in vals:  # what the kernel sees is the fp32 value
        f = ctypes.c_float(v).value
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"snn_bounds: temperature {v} is not a positive finite float32")
    return vals


def snn_bounds(x: torch.Tensor, label: torch.Tensor, taus, return_rows: bool = False):
    """Both bounds of the module docstring for every trial and temperature in one pass:
    ``(snn [B, T] fp64, pssnn [B, T] fp64, count [B, T, 2] int32[, rows [B, T, 3, n] fp32])`` on the device, ``count``
    holding the finite rows behind (SNN, PS-SNN) and ``rows`` the row values ``lse_all, lse_pos, lse_neg``.

    ``x`` is fp32 ``[B, n, d]`` or ``[n, d]`` (then B = 1) on the device; any trial and row stride is taken as it is
    when the stride along d is 1 (a permuted ``[n, B, d]`` storage, a ``[..., :d]`` slice), anything else is made
    contiguous.  ``label`` is an integer tensor ``[n]`` (shared by the trials) or ``[B, n]``, compared as int64.
    ``2 <= n <= 65536``, ``1 <= d <= 64``, 1..8 temperatures, ``B n < 2^31``; ``ValueError`` outside that, for CPU
    tensors, a wrong dtype or shape, before anything is launched.  Deterministic: the same inputs give the same bits,
    and trial b of a batch has the bits of the call on ``x[b]`` alone."""
    if not isinstance(x, torch.Tensor) or not isinstance(label, torch.Tensor):
        raise ValueError("snn_bounds: x and label must be tensors")
    if x.dtype != torch.float32 or x.dim() not in (2, 3):
        raise ValueError("snn_bounds: x must be a float32 tensor of shape [B, n, d] or [n, d]")
    if label.is_floating_point() or label.is_complex() or label.dtype == torch.bool:
        raise ValueError("snn_bounds: label must be an integer tensor")
    vals = check_taus(taus)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, n, d = x.shape
    if B < 1 or not 2 <= n <= MAX_N or not 1 <= d <= MAX_D:
        raise ValueError(f"snn_bounds: need B >= 1, 2 <= n <= {MAX_N}, 1 <= d <= {MAX_D} (got B={B} n={n} d={d})")
    if B * n >= 1 << 31:
        raise ValueError(f"snn_bounds: B * n must stay below 2^31 (B={B} n={n})")
    if tuple(label.shape) not in ((n,), (B, n)):
        raise ValueError(f"snn_bounds: label must have shape {(n,)} or {(B, n)} (got {tuple(label.shape)})")
    if x.device.type != "cuda" or label.device != x.device:
        raise ValueError("snn_bounds: x and label must be on the same ROCm device ('cuda')")
    dev = x.device
    if x.stride(2) != 1:
        x = x.contiguous()
    ld_label = n if (label.dim() == 2 and B > 1) else 0
    lab = label.to(torch.int64).contiguous()
    T = len(vals)
    bound = torch.empty((B, T, 2), dtype=torch.float64, device=dev)
    count = torch.empty((B, T, 2), dtype=torch.int32, device=dev)
    rows = torch.empty((B, T, 3, n), dtype=torch.float32, device=dev) if return_rows else None
    work = _workspace(B, n, T, dev)
    tarr = (ctypes.c_float * T)(*vals)
    with torch.cuda.device(dev):
        _lib.call("cv_snn_bounds", x.data_ptr(), x.stride(0), x.stride(1), B, n, d, lab.data_ptr(), ld_label, tarr,
                  T, bound.data_ptr(), count.data_ptr(), _lib.ptr(rows), work.data_ptr(), _lib.stream_handle())
    if return_rows:
        return bound[..., 0], bound[..., 1], count, rows
    return bound[..., 0], bound[..., 1], count
