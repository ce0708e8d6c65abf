"""Latent interpolation for the demo notebooks (reference code/src/utils/display_utils.py:11-51; every demo notebook
and expr/visual_utils.py start with ``from src.utils.display_utils import interpolate_latent``).

torchvision and matplotlib are only needed to draw: they are imported inside :func:`display_util`, so the module (and
with it a notebook's first cell) imports without them."""

import torch


def interpolate_latent(latent1, latent2, num_steps):
    """``[num_steps, dim]``: row k is ``p_k * latent1 + (1 - p_k) * latent2`` with ``p = linspace(1, 0, num_steps)``,
    on the inputs' device (display_utils.py:11-21)."""
    p = torch.linspace(1, 0, num_steps, device=latent1.device).unsqueeze(1)
    return p * latent1.unsqueeze(0) + (1 - p) * latent2.unsqueeze(0)


def display_util(idx1, idx2, z, model, z_dim, device):
    """Show the style and the content interpolation between the latents ``z[idx1]`` and ``z[idx2]`` (each the
    concatenation of ``z_dim`` content and the style dimensions) as two rows of 11 decoded images, and return the two
    end points decoded as PIL images (display_utils.py:24-51).  ``model.decode`` is this package's HIP decoder: the
    latents are moved to ``device`` (the ROCm device) as contiguous fp32 before every call."""
    import matplotlib.pyplot as plt
    from torchvision.transforms import ToPILImage
    from torchvision.utils import make_grid

    steps = 11

    def decode(v):
        return model.decode(v.to(device=device, dtype=torch.float32).contiguous())

    def show(title, grid_z):
        print(title)
        plt.imshow(make_grid(decode(grid_z), nrow=steps).permute(1, 2, 0).cpu())
        plt.axis("off")
        plt.show()

    with torch.no_grad():
        z1, z2 = z[idx1], z[idx2]
        c1, s1, c2, s2 = z1[:z_dim], z1[z_dim:], z2[:z_dim], z2[z_dim:]
        img1, img2 = (ToPILImage()(decode(v.reshape(1, -1))[0].cpu()) for v in (z1, z2))
        show("interpolate style:", torch.cat([c1.expand(steps, -1), interpolate_latent(s1, s2, steps)], dim=1))
        show("interpolate content:", torch.cat([interpolate_latent(c1, c2, steps), s1.expand(steps, -1)], dim=1))
        return img1, img2
