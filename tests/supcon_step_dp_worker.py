"""Worker of tests/test_supcon_step_api.py (importable by spawned processes): in a gloo group of `world` ranks, what
constructing a CLEARVAETrainer with a SupCon loss_name and loss_step = "fused" does."""

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "clear-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(rank, world, port, q):
    try:
        import torch
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from src.utils.trainer_utils import get_clearvae_trainer

        kw = dict(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=16, alpha=100, temperature=0.1, device="cpu")
        out = {}
        for step in ("fused", "module"):
            try:
                get_clearvae_trainer(loss_name="supcon_in_loss", loss_step=step, **kw)
                out[step] = "constructed"
            except NotImplementedError as e:
                out[step] = f"NotImplementedError: {e}"
        # (snn_loss is data parallel: the key is accepted and ignored there)
        tr = get_clearvae_trainer(loss_step="fused", **kw)
        out["snn"] = (tr.loss_name, tr._loss_kw)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out, None))
    except Exception:  # pragma: no cover
        q.put((rank, None, traceback.format_exc()))
