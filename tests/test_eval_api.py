"""evaluate(backend=...) of the VAE trainers without a GPU: the switch is validated before anything else happens, and
its default is today's module path."""

import inspect

import pytest
import torch


def trainers():
    from src.utils import trainer_utils as U

    dev = torch.device("cpu")
    kw = dict(vae_lr=5e-4, z_dim=16, device=dev)
    return [
        U.get_clearvae_trainer(beta=1 / 8, ps=True, alpha=100, temperature=0.1, **kw),
        U.get_clearmimvae_trainer(beta=1 / 8, mi_estimator="CLUBSample", la=2.0, mi_estimator_lr=2e-3, alpha=100,
                                  temperature=0.1, **kw),
        U.get_cleartcvae_trainer(beta=1 / 8, la=2.0, factor_cls_lr=1e-3, alpha=100, temperature=0.1, **kw),
        U.get_hierarchical_vae_trainer(beta=1 / 8, group_mode="GVAE", **kw),
    ]


class Untouchable:
    """A loader that fails the test if evaluate() gets as far as looking at it."""

    def __iter__(self):
        raise AssertionError("evaluate() iterated the loader before validating its backend")

    def __len__(self):
        raise AssertionError("evaluate() measured the loader before validating its backend")


@pytest.mark.parametrize("i", range(4))
def test_a_bogus_backend_raises_before_anything_else(i, monkeypatch):
    monkeypatch.delenv("CVHIP_EVAL", raising=False)
    tr = trainers()[i]
    tr.model.train()
    with pytest.raises(ValueError, match="bogus"):
        tr.evaluate(Untouchable(), False, 0, backend="bogus")
    monkeypatch.setenv("CVHIP_EVAL", "bogus")
    with pytest.raises(ValueError, match="bogus"):
        tr.evaluate(Untouchable(), False, 0)
    assert tr.model.training  # (not even vae.eval() ran)
    assert tr._eval_pass is None


def test_the_default_backend_is_module(monkeypatch):
    import src.trainer as T

    monkeypatch.delenv("CVHIP_EVAL", raising=False)
    assert T.EVAL_BACKENDS == ("module", "fused")
    assert T._eval_backend(None) == "module"
    monkeypatch.setenv("CVHIP_EVAL", "fused")  # read at the call
    assert T._eval_backend(None) == "fused"
    assert T._eval_backend("module") == "module"  # the argument wins over the environment
    monkeypatch.setenv("CVHIP_EVAL", "")
    assert T._eval_backend(None) == "module"


def test_signatures():
    import src.trainer as T

    for cls in (T.CLEARVAETrainer, T.ClearMIMVAETrainer, T.ClearTCVAETrainer):
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "dataloader", "verbose", "epoch_id",
                                                                    "backend"]
        assert inspect.signature(cls.evaluate).parameters["backend"].default is None
    p = inspect.signature(T.HierarchicalVAETrainer.evaluate).parameters
    assert list(p) == ["self", "dataloader", "verbose", "epoch_id", "with_evidence_acc", "backend"]
    assert p["with_evidence_acc"].default is False and p["backend"].default is None


def test_eval_pass_refuses_a_cpu_model():
    from cvhip.evaluate import EvalPass

    tr = trainers()[0]
    assert "not on the ROCm device" in EvalPass.unsupported_reason(tr, "clear")
    assert EvalPass.build(tr, "clear") is None
    with pytest.raises(ValueError):
        EvalPass.unsupported_reason(tr, "nope")
