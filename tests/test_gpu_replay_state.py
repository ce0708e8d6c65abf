"""State the replayed step keeps on the host (cvhip/engine.py) against changes made outside the engine.  Reference
step: trainer.py:452-484 (CLEAR-VAE).

Packed weights: with ADAM_PACK the replayed step packs the conv weights only when the parameters' version counters
moved (_pack_and_load, _param_sig).  Two steps (the second a replay), the parameters changed from outside, one more
replayed step: its losses and the parameters after it match an engine given the same sequence under ADAM_PACK = 0,
which packs at every step start, within 1e-6 relative (test_gpu_wgrad_lane.py's bar for this pair of Adam kernels).
Every change moves the third step's reconstruction loss by more than 1e-3 relative against the undisturbed sequence
(asserted: 14 % on the fp64 oracle for the in-place change, 11 % for the other state), so a step on stale packed
weights cannot pass.  The in-place change is w <- 1.25 w + 0.02 on every Conv2d / ConvTranspose2d weight: a plain
scale is absorbed by the BatchNorm that follows every convolution (1e-6 on the oracle).

Batch shape: the raw batch copies (_load_batch, the copy folded into the packing launch) take a batch of the static
input's own shape only; an NHWC batch, a batch of smaller images and a two-column label raise before anything of the
step is enqueued, and the engine goes on as if the call had not been made."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HP = {"temperature": 0.1, "beta": 1 / 32, "loc": 0, "scale": 1, "alpha": 100.0, "lambda": 3.0, "ps": True}
ARCHS = {"VAE": ("VAE", 16, 1, 28, 32), "VAE64": ("VAE64", 64, 3, 64, 16)}  # arch, z, C, image side, n


def _torch_state(sd):
    return {k: torch.as_tensor(np.asarray(v)).float() if np.asarray(v).dtype != np.int64
            else torch.as_tensor(np.asarray(v)) for k, v in sd.items()}


def _build(key, adam_pack=None):
    """(trainer, engine, X, label) from the deterministic state; adam_pack None: the engine's default."""
    from oracle import cpu_ref as R
    from cvhip import engine, rng
    from cvhip.engine import ClearStep
    from test_gpu_parity import _fused_trainer

    arch, zt, C, hw, n = ARCHS[key]
    torch.manual_seed(4321)
    rng.clear_injections()
    rng.reset_counters()
    tr = _fused_trainer(arch, zt, C, R.det_state(arch, zt, C), HP)
    prev = engine.ADAM_PACK
    if adam_pack is not None:
        engine.ADAM_PACK = adam_pack
    try:
        eng = ClearStep.build(tr, "clear")
    finally:
        engine.ADAM_PACK = prev
    assert eng is not None
    assert adam_pack is None or eng.adam_pack == adam_pack
    x, label, _, _, _ = R.det_inputs(n, C, hw, zt, 4)
    return tr, eng, torch.tensor(x, dtype=torch.float32, device="cuda"), torch.tensor(label, device="cuda")


def _result(eng, out):
    torch.cuda.synchronize()
    return out[:6].cpu().double().numpy(), eng.arena.flat.double().cpu().numpy()


def _conv_weights(tr):
    return [m.weight for m in tr.model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]


def _change_state(tr, eng, key):
    from oracle import cpu_ref as R

    arch, zt, C, _, _ = ARCHS[key]
    tr.model.load_state_dict(_torch_state(R.det_state(arch, zt, C, seed=1)))


def _change_inplace(tr, eng, key):
    with torch.no_grad():
        for p in _conv_weights(tr):
            p.mul_(1.25).add_(0.02)


def _change_data(tr, eng, key):
    for p in _conv_weights(tr):  # (`.data` aliases escape the version counters: the caller says so)
        p.data.mul_(1.25).add_(0.02)
    eng.invalidate_packed()


CHANGES = {"load_state_dict": _change_state, "inplace": _change_inplace, "data_invalidate": _change_data}


def _sequence(key, adam_pack, change):
    """Two steps, the change, a third step: (losses[:6], arena.flat) after it."""
    tr, eng, X, L = _build(key, adam_pack)
    n = X.shape[0]
    for _ in range(2):
        eng.step(X, L)
    torch.cuda.synchronize()
    assert "graphs" in eng.graphs[n], "the second step was not a replay"
    if change is not None:
        CHANGES[change](tr, eng, key)
    res = _result(eng, eng.step(X, L))
    assert eng.graphs[n]["count"] == 3
    return res


@functools.lru_cache(maxsize=None)
def _undisturbed(key):
    return _sequence(key, True, None)


@functools.lru_cache(maxsize=None)
def _control(key, values):
    """The engine that packs at every step start, given the same sequence (`inplace` and `data_invalidate` write the
    same values)."""
    return _sequence(key, False, "load_state_dict" if values == "state" else "inplace")


@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("key", list(ARCHS))
def test_replay_repacks_after_outside_parameter_change(key, change):
    loss, flat = _sequence(key, True, change)
    ref_loss, ref_flat = _control(key, "state" if change == "load_state_dict" else "values")
    base_loss, _ = _undisturbed(key)
    teeth = abs(ref_loss[0] - base_loss[0]) / abs(base_loss[0])
    print("teeth (rec, changed against undisturbed)", key, change, teeth)
    assert teeth > 1e-3, teeth
    for name, a, b in (("loss", loss, ref_loss), ("flat", flat, ref_flat)):
        err = float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)
        print(name, "against the repacking engine", err)
        assert err <= 1e-6, (name, err)
    assert abs(loss[0] - base_loss[0]) / abs(base_loss[0]) > 1e-3


def _bad_batch(kind, X, L):
    n, C, hw = X.shape[0], X.shape[1], X.shape[2]
    if kind == "nhwc":
        return X.permute(0, 2, 3, 1).contiguous(), L
    if kind == "small":
        return X[:, :, :hw // 2, :hw // 2].contiguous(), L
    assert kind == "label2"
    return X, torch.stack([L, L], 1).contiguous()


@functools.lru_cache(maxsize=None)
def _three_steps(key):
    tr, eng, X, L = _build(key)
    for _ in range(3):
        out = eng.step(X, L)
    return _result(eng, out)


@pytest.mark.parametrize("key,kind,when", [
    ("VAE64", "nhwc", "replay"), ("VAE64", "small", "replay"), ("VAE64", "label2", "replay"),
    ("VAE", "small", "replay"), ("VAE", "label2", "replay"),
    ("VAE", "small", "first"), ("VAE", "label2", "first"),  # (the eager step's copy: _load_batch)
])
def test_batch_of_another_shape_is_refused(key, kind, when):
    from cvhip import _lib

    tr, eng, X, L = _build(key)
    n = X.shape[0]
    done = 0 if when == "first" else 2
    for _ in range(done):
        eng.step(X, L)
    if done:
        assert "graphs" in eng.graphs[n]
    with pytest.raises((RuntimeError, ValueError)):
        eng.step(*_bad_batch(kind, X, L))
    assert eng.graphs[n]["count"] == done
    for _ in range(3 - done):
        out = eng.step(X, L)
    loss, flat = _result(eng, out)
    assert _lib.lib().cv_ntxent_aux_pending() == 0
    ref_loss, ref_flat = _three_steps(key)
    assert np.array_equal(loss, ref_loss), (loss, ref_loss)
    assert np.array_equal(flat, ref_flat), float(np.abs(flat - ref_flat).max())
