"""The notebooks' figures (reference code/expr/visual_utils.py; ``swapping_interpolation.ipynb`` starts with
``from expr.visual_utils import feature_swapping_plot, interpolation_plot``): here the import reads
``from src.utils.visual_utils import ...``.  The figures are composed on the device by :mod:`cvhip.figures`; the
latent scatters come from :class:`cvhip.tsne.TSNE`.  Neither torchvision nor sklearn is needed, and matplotlib is only
imported inside the functions that draw, so the module (and with it a notebook's first cell) imports without it.

What differs from the reference: every ``*_plot`` function has a twin that *returns* what is drawn
(:func:`feature_swapping_grid`, :func:`interpolation_grids`, :func:`latent_embeddings`); at least two images
(``n >= 2``, ``sample_size >= 2``) are required, where the reference fails inside its own ``torch.cat`` (torchvision
returns a single image without padding); nothing calls ``.cuda()``: the tensors must already be on the ROCm device;
the swap latents are decoded in one batch, and in eval mode so are all ``2 * sample_size * inter_steps``
interpolation latents.  The recolouring quirks of ``make_colored_grid`` are kept (:mod:`cvhip.figures`)."""

import torch

from cvhip import figures
from cvhip.tsne import TSNE


def make_colored_grid(imgs, nrow, color: str):
    """``make_grid(imgs, nrow=nrow, pad_value=0.25)`` with the padding recoloured (visual_utils.py:13-26); any colour
    but ``"red"`` and ``"blue"`` raises the reference's ``ValueError``."""
    if color not in ("red", "blue"):
        raise ValueError("other color not implemented yet")
    return figures.make_grid(imgs, nrow=nrow, pad_value=0.25, frame=color)


def _show(fig):
    import matplotlib.pyplot as plt

    plt.imshow(fig.permute(1, 2, 0).cpu().numpy())
    plt.axis("off")
    plt.show()


def _latents(name, z, what):
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError(f"{name}: {what} must be a 2-D float32 tensor")


def _batch(name, X, n, what):
    if not isinstance(X, torch.Tensor) or X.dim() != 4 or X.dtype != torch.float32:
        raise ValueError(f"{name}: X must be a float32 [N, C, H, W] tensor")
    if X.shape[0] != n:
        raise ValueError(f"{name}: X has {X.shape[0]} images, {what} has {n} rows")


def feature_swapping_grid(z_c, z_s, X, vae: torch.nn.Module, img_size=28):
    """The feature-swapping figure as a ``[3, (H+4) + n(H+2) + 2, (W+4) + n(W+2) + 2]`` device tensor: row ``i``,
    column ``j`` of the main area is ``vae.decode((z_c[i], z_s[j]))``, the ``n * n`` latents decoded in one call
    (visual_utils.py:29-52).  ``n >= 2``; ``img_size`` must be both H and W of ``X``."""
    name = "feature_swapping_grid"
    _latents(name, z_c, "z_c")
    _latents(name, z_s, "z_s")
    n = z_c.shape[0]
    if z_s.shape[0] != n:
        raise ValueError(f"{name}: z_c has {n} rows, z_s has {z_s.shape[0]}")
    _batch(name, X, n, "z_c")
    if n < 2:
        raise ValueError(f"{name}: needs at least 2 images (n >= 2)")
    if X.shape[1] not in (1, 3):
        raise ValueError(f"{name}: images must have 1 or 3 channels (C={X.shape[1]})")
    if X.shape[2] != img_size or X.shape[3] != img_size:
        raise ValueError(f"{name}: img_size={img_size} must be the height and the width of X "
                         f"({X.shape[2]} x {X.shape[3]})")
    figures._require_gpu(z_c, z_s, X)
    with torch.no_grad():
        return figures.swap_figure(X, vae.decode(figures.pair_latents(z_c, z_s)))


def feature_swapping_plot(z_c, z_s, X, vae: torch.nn.Module, img_size=28):
    """Draw :func:`feature_swapping_grid` (visual_utils.py:29-58); returns ``None`` like the reference."""
    _show(feature_swapping_grid(z_c, z_s, X, vae, img_size))


def interpolation_grids(X, z, vae, z_dim, sample_size=10, inter_steps=11, src_ids=None, tgt_ids=None):
    """``(style_fig, content_fig)``, the two strips of ``interpolation_plot`` (visual_utils.py:61-118) as
    ``[3, S(H+2) + 2, (W+4) + 8 + T(W+2) + 2 + 8 + (W+4)]`` device tensors.  ``src_ids`` / ``tgt_ids``: the rows of
    ``z`` (and images of ``X``) to interpolate between; ``None`` draws them as the reference does, two successive
    ``torch.randperm(z.size(0))[:sample_size]``.  ``sample_size >= 2``.

    With the model in eval mode the ``2 * S * T`` latents are decoded in one call.  In train mode BatchNorm makes a
    decode depend on its batch, so the ``2 * S`` batches of ``T`` latents are decoded one by one in the reference's
    order (style, then content, per sample).  The model's mode is never changed."""
    name = "interpolation_grids"
    _latents(name, z, "z")
    _batch(name, X, z.shape[0], "z")
    sample_size, inter_steps = int(sample_size), int(inter_steps)
    if sample_size < 2:
        raise ValueError(f"{name}: sample_size={sample_size} must be at least 2")
    if inter_steps < 1:
        raise ValueError(f"{name}: inter_steps={inter_steps} must be at least 1")
    if X.shape[1] not in (1, 3):
        raise ValueError(f"{name}: images must have 1 or 3 channels (C={X.shape[1]})")
    if (src_ids is None) != (tgt_ids is None):
        raise ValueError(f"{name}: give both src_ids and tgt_ids, or neither")
    figures._require_gpu(X, z)
    with torch.no_grad():
        if src_ids is None:
            src_ids = torch.randperm(z.size(0))[:sample_size]
            tgt_ids = torch.randperm(z.size(0))[:sample_size]
        src_ids, tgt_ids = torch.as_tensor(src_ids), torch.as_tensor(tgt_ids)
        if src_ids.dim() != 1 or src_ids.shape != tgt_ids.shape or src_ids.numel() != sample_size:
            raise ValueError(f"{name}: src_ids and tgt_ids must each hold sample_size = {sample_size} ids")
        lat = figures.interp_latents(z, z_dim, src_ids, tgt_ids, inter_steps)  # [2, S, T, D]; checks the ids
        src_dev, tgt_dev = src_ids.to(X.device), tgt_ids.to(X.device)
        X_src, X_tgt = X[src_dev], X[tgt_dev]
        s, t, d = sample_size, inter_steps, z.shape[1]
        if vae.training:
            style, content = [], []
            for i in range(s):
                style.append(vae.decode(lat[0, i]))
                content.append(vae.decode(lat[1, i]))
            style, content = torch.cat(style, dim=0), torch.cat(content, dim=0)
        else:
            dec = vae.decode(lat.view(2 * s * t, d))
            style, content = dec[:s * t], dec[s * t:]
        style_fig = figures.interp_figure(X_src, X_tgt, style)
        return style_fig, figures.interp_figure(X_src, X_tgt, content, like=style_fig)


def interpolation_plot(X: torch.Tensor, z: torch.Tensor, vae, z_dim: int, sample_size=10, inter_steps=11):
    """Draw both strips of :func:`interpolation_grids`, style first (visual_utils.py:61-128); returns ``None``."""
    for fig in interpolation_grids(X, z, vae, z_dim, sample_size, inter_steps):
        _show(fig)


def latent_embeddings(dataloader, vae, device, **tsne_kw):
    """``(emb_c, emb_s, labels, styles)``: the 2-D t-SNE embeddings (fp32 ``[N, 2]`` device tensors) of ``mu_c`` and
    ``mu_s`` over ``dataloader`` (batches of ``(X, content label, style label)``), and the labels concatenated in
    loader order (visual_utils.py:151-179).  Each embedding is
    ``cvhip.tsne.TSNE(n_components=2, perplexity=30, learning_rate=200, init="pca", **tsne_kw).fit_transform``."""
    mu_cs, mu_ss, labels, styles = [], [], [], []
    with torch.no_grad():
        for X, c, s in dataloader:
            _, latent_params = vae(X.to(device))
            mu_cs.append(latent_params["mu_c"])
            mu_ss.append(latent_params["mu_s"])
            labels.append(c)
            styles.append(s)
    if not mu_cs:
        raise ValueError("latent_embeddings: the dataloader is empty")
    mu_cs, mu_ss = torch.cat(mu_cs, dim=0), torch.cat(mu_ss, dim=0)
    labels, styles = torch.cat(labels, dim=0), torch.cat(styles, dim=0)
    kw = dict(perplexity=30, learning_rate=200, init="pca")
    kw.update(tsne_kw)
    emb_c = TSNE(n_components=2, **kw).fit_transform(mu_cs.float().contiguous())
    emb_s = TSNE(n_components=2, **kw).fit_transform(mu_ss.float().contiguous())
    return emb_c, emb_s, labels, styles


def _tsne_plot(tsne_2d, class_labels, classes):
    """One scatter of a 2-D embedding coloured by ``class_labels``, ``classes`` as legend (visual_utils.py:131-141)."""
    import matplotlib.pyplot as plt
    import numpy as np

    cmap = plt.get_cmap("viridis")
    colors = [cmap(i) for i in np.linspace(0, 1, len(classes))]
    _, ax = plt.subplots()
    for g in range(len(classes)):
        i = np.where(class_labels == g)[0]
        ax.scatter(tsne_2d[i, 0], tsne_2d[i, 1], alpha=0.2, c=colors[g], label=classes[g])
    ax.legend()
    plt.show()


def tsne_plot(dataloader, vae, device, content_labels=None, style_labels=None):
    """The four latent scatters (visual_utils.py:144-183): the content embedding coloured by content and by style,
    then the style embedding coloured by style and by content.  The argument order is the reference's, including its
    swapped legends in the last two: the style embedding coloured by *style* gets ``content_labels`` as its legend
    and the one coloured by *content* gets ``style_labels`` (:180-181).  Returns ``None``."""
    emb_c, emb_s, labels, styles = latent_embeddings(dataloader, vae, device)
    if content_labels is None:
        content_labels = list(range(labels.max().item() + 1))
    if style_labels is None:
        style_labels = list(range(styles.max().item() + 1))
    emb_c, emb_s = emb_c.cpu().numpy(), emb_s.cpu().numpy()
    labels, styles = labels.cpu().numpy(), styles.cpu().numpy()
    _tsne_plot(emb_c, labels, content_labels)
    _tsne_plot(emb_c, styles, style_labels)
    _tsne_plot(emb_s, styles, content_labels)
    _tsne_plot(emb_s, labels, style_labels)
