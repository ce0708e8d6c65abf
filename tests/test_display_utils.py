"""src.utils.display_utils: the module every demo notebook imports in its first cell."""

import importlib
import sys

import torch


def test_module_imports_without_torchvision_and_matplotlib(monkeypatch):
    for name in ("torchvision", "torchvision.utils", "torchvision.transforms", "matplotlib", "matplotlib.pyplot"):
        monkeypatch.setitem(sys.modules, name, None)  # `import name` now raises ImportError
    sys.modules.pop("src.utils.display_utils", None)
    mod = importlib.import_module("src.utils.display_utils")
    assert callable(mod.interpolate_latent) and callable(mod.display_util)
    # the package imports of a demo notebook's first cell (demo_clearvae), in its order
    from src.models.vae import VAE  # noqa: F401
    from src.trainer import CLEARVAETrainer  # noqa: F401
    from src.utils.display_utils import interpolate_latent  # noqa: F401


def _formula(a, b, steps):
    p = torch.linspace(1, 0, steps)[:, None].repeat(1, a.shape[-1])
    return p * a[None, :].repeat(steps, 1) + (1 - p) * b[None, :].repeat(steps, 1)


def test_interpolate_latent_equals_the_formula():
    from src.utils.display_utils import interpolate_latent

    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(8, generator=g), torch.randn(8, generator=g)
    out = interpolate_latent(a, b, 11)
    assert out.shape == (11, 8) and out.dtype == torch.float32 and out.device == a.device
    assert torch.equal(out, _formula(a, b, 11))
    assert torch.equal(out[0], a) and torch.equal(out[-1], b)
    one = interpolate_latent(a, b, 1)
    assert one.shape == (1, 8) and torch.equal(one[0], a)
    assert torch.equal(interpolate_latent(latent1=a, latent2=b, num_steps=5), _formula(a, b, 5))
