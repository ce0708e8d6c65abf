"""The fused CLEAR-MIM step with the CLUB estimator under the engine's schedules (cvhip/engine.py): the graph replay
against eager execution (as tests/test_gpu_determinism.py holds replays to each other), and the estimator updates
on side lanes against the sequential form (as tests/test_gpu_mim_branches.py does for CLUB-S and L1OutUB).  Same
weights, same batch, the device Philox counters reset before each run: everything the step produces is
bit-identical, because the CLUB kernels fold their per-workgroup partials in block order and the step has no
order-dependent sum."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HP = {"temperature": 0.1, "beta": 1 / 32, "loc": 0, "scale": 1, "alpha": 100.0, "lambda": 3.0}


def _trainer(arch, zt, C, kind, lr=3e-5):
    from oracle import cpu_ref as R
    from src.models import mi_estimator as MI
    from src.trainer import ClearMIMVAETrainer
    from test_gpu_parity import _model

    vae = _model(arch, zt, C, R.det_state(arch, zt, C))
    opt = torch.optim.Adam(vae.parameters(), lr=lr)
    est = getattr(MI, kind)(zt // 2, zt // 2, zt).cuda()
    est.load_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in R.det_mlp(zt // 2, zt).items()})
    eopt = torch.optim.Adam(est.parameters(), lr=2e-3)
    return ClearMIMVAETrainer(vae, est, {"vae_optim": opt, "mi_estimator_optim": eopt}, "cosine", dict(HP), 1,
                              torch.device("cuda"))


def _two_steps(arch, zt, C, hw, n, kind, graphs=True, branches=None):
    from oracle import cpu_ref as R
    from cvhip import engine, rng
    from cvhip.engine import ClearStep

    prev = engine.MIM_BRANCHES
    if branches is not None:
        engine.MIM_BRANCHES = branches
    try:
        torch.manual_seed(4321)
        rng.clear_injections()
        rng.reset_counters()
        tr = _trainer(arch, zt, C, kind)
        eng = ClearStep.build(tr, "mim")
        assert eng is not None
        eng.graphs_enabled = graphs
        x, label, _, _, _ = R.det_inputs(n, C, hw, zt, 4)
        X = torch.tensor(x, dtype=torch.float32, device="cuda")
        L = torch.tensor(label, device="cuda")
        res = []
        for _ in range(2):  # (the first step runs eagerly; the second from the graph when graphs are enabled)
            lo, learn = eng.step(X, L)
            torch.cuda.synchronize()
            res.append(dict(loss=lo[:6].cpu().double().numpy(), learn=learn.cpu().double().numpy(),
                            bufs={k: b.detach().double().cpu().numpy() for k, b in tr.model.named_buffers()},
                            flat=eng.arena.flat.double().cpu().numpy(), grad=eng.arena.grad.double().cpu().numpy(),
                            est=eng.est_arena.flat.double().cpu().numpy()))
        G = eng.graphs[n]
        return dict(res=res, lanes={c[3] for c in G["learn"].calls}, replayed="graphs" in G, kind=eng.kind)
    finally:
        engine.MIM_BRANCHES = prev


def test_club_graph_replay_matches_eager():
    """VAE, n = 64: two steps with the second replayed from the captured graph, against two eager steps."""
    from cvhip import _lib

    a = _two_steps("VAE", 16, 1, 28, 64, "CLUB", graphs=True)
    b = _two_steps("VAE", 16, 1, 28, 64, "CLUB", graphs=False)
    assert a["kind"] == b["kind"] == _lib.MI_CLUB
    assert a["replayed"] and not b["replayed"]
    for step, (ra, rb) in enumerate(zip(a["res"], b["res"])):
        for k in ("loss", "learn", "flat", "grad", "est"):
            assert np.array_equal(ra[k], rb[k]), (step, k, float(np.abs(ra[k] - rb[k]).max()))
        for k in rb["bufs"]:
            assert np.array_equal(ra["bufs"][k], rb["bufs"][k]), (step, k)
    assert np.isfinite(a["res"][1]["loss"]).all() and a["res"][1]["loss"][5] != 0.0


def test_club_branched_lanes_match_sequential():
    """VAE64, n = 16: the five estimator forwards on side lanes (MIM_BRANCHES = 2) against the sequential
    schedule (MIM_BRANCHES = 0), at the bars of tests/test_gpu_mim_branches.py."""
    a = _two_steps("VAE64", 64, 3, 64, 16, "CLUB", branches=2)
    b = _two_steps("VAE64", 64, 3, 64, 16, "CLUB", branches=0)
    assert any(isinstance(v, int) and v >= 1 for v in a["lanes"]), a["lanes"]
    assert not any(isinstance(v, int) and v >= 1 for v in b["lanes"]), b["lanes"]
    assert a["replayed"] and b["replayed"]
    for step, (ra, rb) in enumerate(zip(a["res"], b["res"])):
        assert np.array_equal(ra["loss"], rb["loss"]), (step, ra["loss"], rb["loss"])
        assert np.array_equal(ra["learn"], rb["learn"]), (step, ra["learn"], rb["learn"])
        for k in rb["bufs"]:
            if k.endswith("num_batches_tracked"):
                assert np.array_equal(ra["bufs"][k], rb["bufs"][k]), (step, k)
            else:  # (one launch instead of five: an fma contracted differently, an ulp apart)
                d = np.abs(ra["bufs"][k] - rb["bufs"][k]).max() / max(np.abs(rb["bufs"][k]).max(), 1e-3)
                assert d <= 1e-6, (step, k, d)
        assert np.array_equal(ra["flat"], rb["flat"]), step
        assert np.array_equal(ra["est"], rb["est"]), step
