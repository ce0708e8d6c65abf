"""Device-resident datasets and loaders: the producer side of the training step.

The reference builds batches on the host: StyledMNIST keeps a materialised list of PIL images and applies
ToTensor per item (code/src/utils/data_utils.py:55-77); PACS and Camelyon17 resize every PIL image with
transforms.Resize((64, 64)) + ToTensor() in the DataLoader (code/run_pacs_downstream_expr.py:88-98,
code/run_camelyon17_downstream_expr.ipynb cell 6).  DeviceImageDataset holds the raw uint8 images in HBM
(Camelyon17's 302k 96x96x3 training patches are 8.3 GB: the whole set fits on one MI355X many times over)
and DeviceLoader yields (X, label[, style]) batches made by one cv_load_batch_u8 launch each — the same
values as the reference's transforms, bit for bit (tests/test_gpu_data.py).

Styled-MNIST itself is generated on the device: DeviceStyledMNIST runs the six style corruptions the reference's
Styled-MNIST scripts use (identity, stripe, zigzag, canny_edges, scale, brightness; corruption_utils.corruptions)
and the per-image style draw of StyledMNISTGenerator (code/src/utils/data_utils.py:29-52) / KStyledMNISTGenerator
(code/expr/expr_utils.py:18-32) as one cv_style_mnist launch over the whole set, and keeps the float32 result: the
reference feeds the corruptions' unquantised float32 values through ToTensor() and img / 255.0
(code/run_mig_expr_mnist.py:63-65), which a uint8 DeviceImageDataset cannot hold.  DeviceImageDataset still takes a
host-made uint8 set (the other corruptions, or any other image data).
"""

from __future__ import annotations

import numpy as np
import torch

from cvhip.data import load_batch

STYLE_NAMES = ("identity", "stripe", "zigzag", "canny_edges", "scale", "brightness")
DEFAULT_SEVERITY = {"scale": 3, "brightness": 5}  # the reference functions' defaults


class DeviceImageDataset:
    """uint8 images [N, H, W] or [N, H, W, C] + int labels (+ style labels) on the device; items come out
    as transforms.Compose([Resize(size), ToTensor()]) would make them (size=None: ToTensor only)."""

    def __init__(self, images, labels, styles=None, size=None, device="cuda") -> None:
        imgs = torch.as_tensor(np.asarray(images) if not isinstance(images, torch.Tensor) else images)
        if imgs.dtype != torch.uint8 or imgs.dim() not in (3, 4):
            raise ValueError("images: uint8 [N, H, W] or [N, H, W, C]")
        self.images = imgs.to(device).contiguous()
        self.labels = torch.as_tensor(labels).reshape(-1).to(device=device, dtype=torch.int64)
        self.styles = None if styles is None else torch.as_tensor(styles).reshape(-1).to(device=device,
                                                                                         dtype=torch.int64)
        if self.labels.numel() != self.images.shape[0]:
            raise ValueError("one label per image")
        if self.styles is not None and self.styles.numel() != self.images.shape[0]:
            raise ValueError("one style label per image")
        H, W = self.images.shape[1:3]
        self.size = tuple(size) if size is not None else (H, W)

    @classmethod
    def from_items(cls, items, size=None, device="cuda"):
        """From (image, label[, style]) items, e.g. a materialised StyledMNIST list (data_utils.py:61-65):
        images are PIL images or uint8 arrays of one size; uploaded once."""
        imgs, labels, styles = [], [], []
        for it in items:
            imgs.append(np.asarray(it[0], dtype=np.uint8))
            labels.append(int(it[1]))
            if len(it) > 2:
                styles.append(int(it[2]))
        return cls(np.stack(imgs), labels, styles if styles else None, size, device)

    def __len__(self) -> int:
        return self.images.shape[0]

    def __getitem__(self, idx) -> tuple:
        k, n = int(idx), len(self)
        if not -n <= k < n:  # (list indexing semantics, like the reference's materialised list)
            raise IndexError(f"index {k} out of range for {n} images")
        i = torch.tensor([k % n], device=self.images.device)
        x, y, s = load_batch(self.images, i, self.size, self.labels, self.styles, checked=False)
        return (x[0], y[0]) if s is None else (x[0], y[0], s[0])

    def batch(self, index: torch.Tensor, out: torch.Tensor | None = None, checked: bool = True) -> tuple:
        x, y, s = load_batch(self.images, index, self.size, self.labels, self.styles, out=out, checked=checked)
        return (x, y) if s is None else (x, y, s)


class DeviceLoader:
    """torch DataLoader semantics over a DeviceImageDataset (batch_size, shuffle, drop_last); the
    permutation is drawn on the device, batches are (X, label[, style]) device tensors."""

    def __init__(self, dataset: DeviceImageDataset, batch_size: int = 1, shuffle: bool = False,
                 drop_last: bool = False, generator: torch.Generator | None = None) -> None:
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.drop_last = drop_last
        self.generator = generator

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        dev = self.dataset.images.device
        if self.shuffle:
            order = torch.randperm(n, device=dev, generator=self.generator)
        else:
            order = torch.arange(n, device=dev)
        for b in range(len(self)):
            yield self.dataset.batch(order[b * self.batch_size:(b + 1) * self.batch_size], checked=False)


# ---------------------------------------------------------------------------------------------- Styled-MNIST
def parse_style(spec) -> tuple:
    """A style spec, a name of STYLE_NAMES or (name, severity), as (name, severity); severities (1..5) belong to
    scale and brightness and default to the reference's (scale 3, brightness 5)."""
    name, sev = (spec, None) if isinstance(spec, str) else (tuple(spec) if len(spec) == 2 else (None, None))
    if name not in STYLE_NAMES:
        raise ValueError(f"unknown style {spec!r}: a name of {STYLE_NAMES} or (name, severity)")
    if name not in DEFAULT_SEVERITY:
        if sev is not None:
            raise ValueError(f"style {name!r} takes no severity")
        return name, 1
    sev = DEFAULT_SEVERITY[name] if sev is None else sev
    if isinstance(sev, bool) or not isinstance(sev, (int, np.integer)) or not 1 <= sev <= 5:
        raise ValueError(f"severity {sev!r} of {name!r} outside 1..5")
    return name, int(sev)


def random_style_distribution(styles=STYLE_NAMES[:4]) -> dict:
    """{style: p} with p ~ Dirichlet([10] * len(styles)) from numpy's global generator, on the host (the
    reference's random_style_distribution, code/src/utils/data_utils.py:14-26)."""
    styles = list(styles)
    probs = np.random.dirichlet([10] * len(styles))
    return {st: probs[i] for i, st in enumerate(styles)}


def generate_style_dict(classes, styles, k: int) -> dict:
    """{class: {"train": k styles drawn without replacement, "test": the others, sorted}} (the reference's
    generate_style_dict, code/expr/expr_utils.py:7-15); styles are usually indices into a style list."""
    styles = list(styles)
    if k < 1 or k >= len(styles):
        raise ValueError("k must be in [1, len(styles) - 1]")
    out = {}
    for c in classes:
        train = np.random.choice(styles, k, replace=False)
        out[c] = {"train": train, "test": np.setdiff1d(styles, train)}
    return out


class DeviceStyledMNIST:
    """Styled-MNIST generated on the device in one launch and held there as float32.

    images: uint8 [N, 28, 28] (numpy array, tensor, or a dataset with .data / .targets like torchvision's MNIST,
    in which case labels may be None).  styles: a {spec: p} dict (StyledMNISTGenerator: every class draws from the
    same distribution) or a list of specs with style_dict and split (KStyledMNISTGenerator: the style of an image
    is uniform over style_dict[label][split], indices into the list).  A spec is a name of STYLE_NAMES or
    (name, severity).

    .images float32 [N, 1, 28, 28] in [0, 1] (the corruption's float32 value / 255: ToTensor() then img / 255.0),
    .labels and .styles int64 [N].  Items and batches are (X, label, style); DeviceLoader works over it."""

    def __init__(self, images, labels, styles, style_dict=None, split=None, device="cuda") -> None:
        if labels is None and hasattr(images, "targets"):
            labels = images.targets
        if hasattr(images, "data") and hasattr(images, "targets"):
            images = images.data
        imgs = torch.as_tensor(np.asarray(images) if not isinstance(images, torch.Tensor) else images)
        if imgs.dtype != torch.uint8 or imgs.dim() != 3 or tuple(imgs.shape[1:]) != (28, 28) or imgs.shape[0] < 1:
            raise ValueError("images: uint8 [N, 28, 28]")
        if labels is None:
            raise ValueError("labels are required")
        labs = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).reshape(-1)
        if labs.numel() != imgs.shape[0]:
            raise ValueError("one label per image")
        labs = labs.to(torch.int64)
        if isinstance(styles, dict):
            if style_dict is not None or split is not None:
                raise ValueError("a {style: p} dict takes no style_dict / split")
            specs = [parse_style(s) for s in styles]
            p = np.asarray([float(v) for v in styles.values()], dtype=np.float64)
            if not specs or (p < 0).any() or abs(p.sum() - 1.0) > 1e-6:
                raise ValueError("style probabilities must be non-negative and sum to 1")
            n_class = int(labs.max()) + 1 if labs.numel() else 1
            table = np.tile(p, (max(n_class, 1), 1))
        else:
            specs = [parse_style(s) for s in styles]
            if style_dict is None or split is None:
                raise ValueError("a style list needs style_dict and split (or pass a {style: p} dict)")
            n_class = max(int(c) for c in style_dict) + 1
            table = np.zeros((n_class, len(specs)), dtype=np.float64)
            for c, d in style_dict.items():
                if split not in d:
                    raise ValueError(f"style_dict[{c!r}] has no split {split!r}")
                idx = np.asarray(d[split]).reshape(-1).astype(np.int64)
                if idx.size == 0 or idx.min() < 0 or idx.max() >= len(specs):
                    raise ValueError(f"style_dict[{c!r}][{split!r}] must hold indices into the {len(specs)} styles")
                np.add.at(table[int(c)], idx, 1.0 / idx.size)  # (np.random.choice over the list: uniform)
            missing = sorted(set(labs.unique().tolist()) - {int(c) for c in style_dict})
            if missing:
                raise ValueError(f"labels {missing} have no entry in style_dict")
        if not 1 <= len(specs) <= 16:
            raise ValueError(f"{len(specs)} styles: 1..16 are supported")
        if int(labs.min()) < 0:
            raise ValueError("labels must be non-negative")
        self.style_specs = specs
        self.table = table
        # (everything above ran on the host; the device is touched from here on)
        from cvhip.styled import stylize

        raw = imgs.to(device).contiguous()
        self.labels = labs.to(device)
        out, style, zz = stylize(raw, self.labels, torch.as_tensor(table, dtype=torch.float32).to(device),
                                 [s[0] for s in specs], [s[1] for s in specs])
        self.images = (out / 255.0).unsqueeze(1)
        self.styles = style
        self.zigzag = zz

    def __len__(self) -> int:
        return self.images.shape[0]

    def __getitem__(self, idx) -> tuple:
        k, n = int(idx), len(self)
        if not -n <= k < n:  # (list indexing semantics, like the reference's materialised list)
            raise IndexError(f"index {k} out of range for {n} images")
        k %= n
        return self.images[k], self.labels[k], self.styles[k]

    def batch(self, index: torch.Tensor, out: torch.Tensor | None = None, checked: bool = True) -> tuple:
        idx = index.to(device=self.images.device, dtype=torch.int64)
        n = len(self)
        if checked and idx.numel():
            lo, hi = (int(v) for v in torch.aminmax(idx))
            if lo < 0 or hi >= n:
                raise IndexError(f"batch: index out of range [{lo}, {hi}] for {n} images")
        x = torch.index_select(self.images, 0, idx, out=out)
        return x, self.labels.index_select(0, idx), self.styles.index_select(0, idx)
