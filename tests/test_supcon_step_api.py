"""The public switch of the fused SupCon step without a GPU: hyperparameter["loss_step"] ("module" | "fused") of
CLEARVAETrainer, the environment's CVHIP_SUPCON_STEP behind it, the factory keyword, and what a CPU device or a
process group of two ranks does with "fused"."""

import multiprocessing as mp
import socket

import pytest
import torch

SUPCON = ("supcon_in_loss", "supcon_out_loss")
KW = dict(beta=1 / 8, ps=True, vae_lr=5e-4, z_dim=16, alpha=100, temperature=0.1, device="cpu")
DEFAULT_HP = {"temperature": 0.1, "alpha": 100, "beta": 1 / 8, "ps": True, "loc": 0, "scale": 1}


def _trainer(**hp):
    from src.models.vae import VAE
    from src.trainer import CLEARVAETrainer

    vae = VAE(total_z_dim=16, in_channel=1)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    return CLEARVAETrainer(vae, opt, "cosine", dict(DEFAULT_HP, **hp), 1, torch.device("cpu"))


def test_loss_step_resolution_key_then_environment_then_module(monkeypatch):
    monkeypatch.delenv("CVHIP_SUPCON_STEP", raising=False)
    assert _trainer(loss_name="supcon_in_loss").loss_step() == "module"
    assert _trainer(loss_name="supcon_in_loss", loss_step="fused").loss_step() == "fused"
    monkeypatch.setenv("CVHIP_SUPCON_STEP", "fused")
    tr = _trainer(loss_name="supcon_out_loss")
    assert tr.loss_step() == "fused"
    assert _trainer(loss_name="supcon_out_loss", loss_step="module").loss_step() == "module"  # the key wins
    monkeypatch.setenv("CVHIP_SUPCON_STEP", "module")  # read when asked, not at construction
    assert tr.loss_step() == "module"
    assert _trainer(loss_name="supcon_out_loss", loss_step="fused").loss_step() == "fused"


@pytest.mark.parametrize("bad", ["graph", "", "Fused", 1, True])
def test_bad_loss_step_raises_at_construction(bad):
    with pytest.raises(ValueError, match="loss_step"):
        _trainer(loss_name="supcon_in_loss", loss_step=bad)
    with pytest.raises(ValueError, match="loss_step"):  # whatever the loss name is
        _trainer(loss_step=bad)


def test_bad_environment_value_raises_when_asked(monkeypatch):
    monkeypatch.setenv("CVHIP_SUPCON_STEP", "graph")
    tr = _trainer(loss_name="supcon_in_loss")
    with pytest.raises(ValueError, match="CVHIP_SUPCON_STEP"):
        tr._fused()
    assert _trainer(loss_name="supcon_in_loss", loss_step="module")._fused() is None  # the key wins: never read


@pytest.mark.parametrize("loss", SUPCON)
def test_factory_keyword_enters_the_dict_only_when_given(loss):
    from src.utils.trainer_utils import get_clearvae_trainer

    assert get_clearvae_trainer(loss_name=loss, **KW).hyperparameter == dict(DEFAULT_HP, loss_name=loss)
    assert get_clearvae_trainer(loss_name=loss, loss_step=None, **KW).hyperparameter == dict(DEFAULT_HP, loss_name=loss)
    for step in ("module", "fused"):
        tr = get_clearvae_trainer(loss_name=loss, loss_step=step, **KW)
        assert tr.hyperparameter == dict(DEFAULT_HP, loss_name=loss, loss_step=step)
        assert list(tr.hyperparameter) == list(DEFAULT_HP) + ["loss_name", "loss_step"]
        assert tr.loss_step() == step
    assert get_clearvae_trainer(**KW).hyperparameter == DEFAULT_HP
    with pytest.raises(ValueError, match="loss_step"):
        get_clearvae_trainer(loss_name=loss, loss_step="graph", **KW)


def test_snn_loss_accepts_and_ignores_the_key(monkeypatch):
    from src.utils.trainer_utils import get_clearvae_trainer

    monkeypatch.setenv("CVHIP_SUPCON_STEP", "module")
    for step in ("module", "fused"):
        tr = get_clearvae_trainer(loss_step=step, **KW)
        assert tr.hyperparameter == dict(DEFAULT_HP, loss_step=step)
        assert tr.loss_name == "snn_loss" and tr._loss_kw == {}
        # (its step is the fused one whatever the key says; on a CPU device the engine declines)
        assert tr._fused() is None and tr._engine is None


@pytest.mark.parametrize("loss", SUPCON)
def test_fused_on_a_cpu_device_declines_without_raising(loss, monkeypatch):
    """_fused() asks the engine, which declines a CPU device: the trainer trains on the module path, as an snn_loss
    trainer on the CPU does."""
    from cvhip.engine import ClearStep

    asked = []
    real = ClearStep.build.__func__

    def build(cls, trainer, mode):
        asked.append(mode)
        return real(cls, trainer, mode)

    monkeypatch.setattr(ClearStep, "build", classmethod(build))
    tr = _trainer(loss_name=loss, loss_step="fused")
    assert tr._fused() is None and tr._engine is None
    assert asked == ["clear"]
    asked.clear()
    assert _trainer(loss_name=loss)._fused() is None and asked == []  # the module path never asks


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_process_group_of_two_ranks_raises_not_implemented():
    """As tests/test_dist_gloo.py starts its group: two spawned gloo ranks, each constructing the trainers."""
    import supcon_step_dp_worker

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=supcon_step_dp_worker.run, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, out, err = q.get(timeout=240)
            assert err is None, err
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(world):
        for step in ("fused", "module"):
            assert res[r][step].startswith("NotImplementedError") and "not data parallel" in res[r][step], res[r]
        assert res[r]["snn"] == ("snn_loss", {})
