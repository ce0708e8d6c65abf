"""The device LAM baseline on the GPU, engine and trainer: cvhip.lam.LamStep and LAMCNNTrainer(backend="device")
against the literal three-forward step of tests/lam_ref.py (this repository's src/ modules run by PyTorch on the CPU
in fp64 with torch.optim.Adam), with the pairing injected or replayed from the engine's pair_log.

Inputs and the seed rule: tests/lam_ref.py (the batches of tests/cnn_ref.py; in the single-step cases no BatchNorm
output of the fp64 reference is within 1e-5 of zero; tests/test_lam_ref.py asserts the rule on the same seeds).

Bounds.  One step at lam_coef 1.0: per tensor (both losses, every p.grad, every running_mean / running_var), relative
L2 against fp64 <= 30 x the error of the same literal step run by PyTorch in fp32 on the CPU, computed in the test;
where that product exceeds 1e-4 the case counts as ill-conditioned (another qualifying seed is due, never a looser
bound): the rule of tests/test_gpu_cnn_trainer.py.  num_batches_tracked is exactly +3.  The conv biases (they feed a
train-mode BatchNorm) have p.grad exactly 0 and stay bit-unchanged.  The Adam part: tests/adam_ref.py fed the gradients
the step itself wrote.  Trainer: TOL = 1e-4 relative on parameters and running statistics, with the allowance of
tests/test_gpu_cnn_trainer.py after a step PyTorch took (the refused batch), which starts from non-zero BatchNorm
biases for the reason given there.

Measured on an MI355X (the tests print LAMERR lines):
  one step at lam_coef 1, relative L2 against fp64, device / bound (30 x the fp32 CPU run):
    LAMCNNClassifier(10, 1) n=16 seed 2:    ce 6.2e-08 / 1.9e-06, lam 6.9e-08 / 1.4e-06; grads <= 7.1e-07 (net.0.weight,
      bound 2.7e-05; tightest cls_head.bias 1.5e-07 / 3.0e-06); running statistics <= 1.3e-07 against >= 1.5e-06
    LAMCNNClassifier(7, 3) n=50 seed 12:    ce 5.6e-08 / 3.5e-06, lam 2.5e-08 / 7.4e-07; grads <= 1.1e-06 (net.0.weight,
      bound 3.9e-05; tightest net.7.bias 1.0e-07 / 3.3e-06); running statistics <= 1.1e-07 against >= 1.5e-06
    LAMCNN64Classifier(4, 3) n=8 seed 18:   ce 2.0e-07 / 6.7e-07, lam 5.6e-08 / 4.6e-07; grads <= 1.2e-06 (net.0.weight,
      bound 4.8e-05; tightest net.13.bias 1.7e-07 / 7.5e-06); running statistics <= 2.5e-07 / 7.3e-06
    Adam part (p in lr, m in |g|, v in g^2; kernel | e32): 5.88e-05 5.68e-09 1.16e-10 | the same
  fit(2) over 16, 16, 5 at lam_coef 0.1 against the fp64 loop on pair_log: <= 6.7e-06 (net.6.weight; running statistics
    <= 5.7e-06) in one run, <= 8.1e-07 in another (the drawn pairings differ with the seed the process is at); eval
    logits <= 2.8e-07 (n=16 and n=1)
  16, 1040 (refused, PyTorch), 16, 16 from non-zero BatchNorm biases: <= 2.4e-06 (net.6.weight)
"""

import copy
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import adam_ref as AR
import cnn_ref as CR
import lam_ref as LR

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_cnn_trainer.py
LR1 = 1e-3  # the single-step cases (lam_ref.model_case)
LRT = 1e-4  # the trainer cases (the scripts' value)
CASES = list(LR.MODEL_SEEDS)
IDS = [f"{c[0]}-c{c[1]}-ch{c[2]}-n{c[3]}" for c in CASES]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy().copy()


def _trainer(model0, lr, lam, backend="device"):
    from src.trainer import LAMCNNTrainer

    model = copy.deepcopy(model0).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    return LAMCNNTrainer(model, opt, nn.CrossEntropyLoss(), {"lam_coef": lam}, 10, torch.device("cuda"),
                         backend=backend)


def _engine(tr):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng = tr._cnn_engine()
    assert eng is not None, "the device backend was refused"
    return eng


def _bn_buffers(model):
    return {k: v for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}


# ------------------------------------------------------------------------------------------------ 1. one step
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_step_against_fp64(case):
    arch, n_class, in_ch, n = case
    seed = LR.MODEL_SEEDS[case]
    model0, (X, y), pair, margin, r64, r32 = LR.model_case(arch, n_class, in_ch, n, seed, 1.0, LR1)
    assert margin >= LR.MASK_MARGIN
    tr = _trainer(model0, LR1, 1.0)
    model, eng = tr.model, _engine(tr)
    model.train()
    host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    before = (host(eng.arena.flat), host(eng.adam.m), host(eng.adam.v))
    p_before = {k: _bits(p) for k, p in model.named_parameters()}
    losses = eng.step(X.cuda(), y.cuda(), pair=pair).tolist()
    torch.cuda.synchronize()
    m64, _, l64, g64 = r64
    m32, _, l32, g32 = r32
    rows, res = [], []

    def check(name, err, bound):
        rows.append(f"{name} {err:.1e}/{bound:.1e}")
        res.append((name, err, bound))

    for i, name in enumerate(("ce", "lam")):
        check(name, abs(losses[i] - l64[0][i]) / abs(l64[0][i]), 30.0 * abs(l32[0][i] - l64[0][i]) / abs(l64[0][i]))
    zero = LR.ZERO_GRAD_BIASES[arch]
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == eng.arena.gptr(p), k
        if k in zero:
            assert not _bits(p.grad).any(), f"{k}.grad must be exact zeros"
            assert np.array_equal(_bits(p), p_before[k]), f"{k} moved under an exact-zero gradient"
        else:
            check(k, CR.rel_l2(p.grad, g64[k]), 30.0 * CR.rel_l2(g32[k], g64[k]))
    b64, b32, b0 = _bn_buffers(m64), _bn_buffers(m32), _bn_buffers(model0)
    for k, v in _bn_buffers(model).items():
        if "num_batches" in k:
            assert int(v) == int(b64[k]) == int(b0[k]) + 3, k
        else:
            check(k, CR.rel_l2(v, b64[k]), 30.0 * CR.rel_l2(b32[k], b64[k]))
    print(f"LAMERR step {IDS[CASES.index(case)]} seed {seed} (device/bound): " + " ".join(rows))
    for name, err, bound in res:
        assert bound <= TOL, ("ill-conditioned case: pick another qualifying seed", name, bound)
        assert err <= bound, (name, err, bound)
    # the Adam part: adam_ref fed the gradients the step itself wrote
    g = host(eng.arena.grad)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    case_a = AR.Case(*before, g[None], (LR1, 0.9, 0.999, 1e-8, 0.0), 0)
    err, ok = case_a.errors(0, host(eng.arena.flat), host(eng.adam.m), host(eng.adam.v))
    print(f"ADAMERR lam step: kernel p {err[0]:.3g} m {err[1]:.3g} v {err[2]:.3g} | e32 p {case_a.e32_p[0]:.3g} "
          f"m {case_a.e32_m[0]:.3g} v {case_a.e32_v[0]:.3g}")
    assert ok, err
    assert eng.adam.step.tolist() == [1, 0]


def test_a_given_pair_must_be_a_permutation():
    case = CASES[0]
    model0 = LR.make_model(case[0], case[1], case[2], LR.MODEL_SEEDS[case])
    X, y = LR.make_batch(case[0], case[1], case[2], 16, 30)
    tr = _trainer(model0, LR1, 0.1)
    eng = _engine(tr)
    tr.model.train()
    for bad in (torch.zeros(16, dtype=torch.int64), torch.arange(15), torch.arange(1, 17)):
        with pytest.raises(ValueError):
            eng.step(X.cuda(), y.cuda(), pair=bad)
    assert eng.steps_taken == 0


# ------------------------------------------------------------------------------------------------ 2. eager vs replay
def _state_bits(tr, eng):
    out = [_bits(eng.loss), _bits(eng.arena.flat), _bits(eng.arena.grad), _bits(eng.adam.m), _bits(eng.adam.v),
           np.array(eng.adam.step.tolist())]
    return out + [_bits(v) for v in _bn_buffers(tr.model).values()]


def test_eager_and_replayed_steps_are_bit_identical():
    """Drawn pairings: both runs restart the device Philox stream, so they draw the same pairs."""
    from cvhip import rng

    case = CASES[0]
    model0 = LR.make_model(case[0], case[1], case[2], LR.MODEL_SEEDS[case])
    batches = [LR.make_batch(case[0], case[1], case[2], case[3], 40 + s) for s in range(4)]
    runs, logs = [], []
    for graphs in (True, False):
        rng.reset_counters()
        tr = _trainer(model0, LR1, 0.1)
        eng = _engine(tr)
        eng.graphs_enabled, eng.record_pairs = graphs, True
        tr.model.train()
        states = []
        for X, y in batches:
            eng.step(X.cuda(), y.cuda())
            torch.cuda.synchronize()
            states.append(_state_bits(tr, eng))
        assert ("graph" in eng.sizes[case[3]]) == graphs and eng.sizes[case[3]]["count"] == 4
        runs.append(states)
        logs.append([p.cpu() for p in eng.pair_log])
    for k in range(4):
        assert torch.equal(logs[0][k], logs[1][k]), k
        y = batches[k][1]
        assert sorted(logs[0][k].tolist()) == list(range(case[3])) and bool((y[logs[0][k]] == y).all())
        for i, (a, b) in enumerate(zip(runs[0][k], runs[1][k])):
            assert np.array_equal(a, b), (k, i)
    assert not torch.equal(logs[0][0], logs[0][1]) or not torch.equal(logs[0][1], logs[0][2])  # (fresh draws)
    assert not np.array_equal(runs[0][0][1], runs[0][3][1])  # (the parameters did move)


# ------------------------------------------------------------------------------------------------ 3. trainer
def _drift(T):
    """|b_t - b_0| <= t lr for a bias under Adam, and running_mean is a sub-convex combination of batch means."""
    return T * LRT * 1.01


def _compare(model, m64, model0, torch_steps, tag):
    """Parameters and running statistics against the fp64 loop (tests/test_gpu_cnn_trainer.py::_compare)."""
    zero = LR.ZERO_GRAD_BIASES[type(model).__name__]
    sd0, worst = model0.state_dict(), {}
    for (k, a), (_, b) in zip(model.state_dict().items(), m64.state_dict().items()):
        if "num_batches" in k:
            assert int(a) == int(b), k
        elif k in zero:
            if torch_steps == 0:
                assert torch.equal(a.cpu(), sd0[k]), f"{k} moved under exact-zero gradients"
            else:
                assert float((a.cpu().double() - sd0[k].double()).abs().max()) <= _drift(torch_steps), k
        elif "running_mean" in k and torch_steps:
            diff = float((a.cpu().double() - b).abs().max())
            assert diff <= _drift(torch_steps) + TOL * float(b.abs().max()), (k, diff)
        else:
            worst[k] = CR.rel_l2(a, b)
    print(f"LAMERR trainer {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < TOL, (k, v)


def _batches(case, sizes, seed0=60):
    return [LR.make_batch(case[0], case[1], case[2], n, seed0 + i) for i, n in enumerate(sizes)]


def _fresh_fp64(model):
    m = type(model)(n_class=model.cls_head.out_features, in_channel=model.net[0].in_channels).double()
    m.load_state_dict({k: (v.cpu().double() if v.dtype.is_floating_point else v.cpu())
                       for k, v in model.state_dict().items()})
    return m.eval()


def test_trainer_fit_matches_the_fp64_loop():
    case = CASES[0]
    model0 = LR.make_model(case[0], case[1], case[2], LR.MODEL_SEEDS[case])
    batches = _batches(case, (16, 16, 5))
    tr = _trainer(model0, LRT, 0.1)
    _engine(tr).record_pairs = True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr.fit(2, batches)
    assert not [w for w in rec if "LAMCNNTrainer" in str(w.message)], "the device backend was refused"
    eng, model, opt = tr._engine, tr.model, tr.optimizer
    assert eng is not None and eng.steps_taken == 6 and len(eng.pair_log) == 6
    assert all("graph" in eng.sizes[m] and eng.sizes[m]["count"] == cnt for m, cnt in ((16, 4), (5, 2)))
    for p in model.parameters():
        st = opt.state[p]
        assert float(st["step"]) == 6.0
        o, _ = eng.arena.offset[id(p)]
        assert st["exp_avg"].data_ptr() == eng.adam.m.data_ptr() + 4 * o  # (a live view of the engine's moments)
        assert p.grad is not None and p.grad.data_ptr() == eng.arena.grad.data_ptr() + 4 * o
    for pair, (_, y) in zip(eng.pair_log, batches + batches):
        pair = pair.cpu()
        assert sorted(pair.tolist()) == list(range(len(y))) and bool((y[pair] == y).all())
    m64 = LR.literal_steps(model0, batches, eng.pair_log, 0.1, LRT, torch.float64, epochs=2)[0]
    _compare(model, m64, model0, 0, "fit")

    # evaluate(): the reference's structure, through cv_lam_forward; logits against fp64 on the same parameters
    (aupr, auroc), acc = tr.evaluate(batches, verbose=False, epoch_id=0)
    ys = torch.cat([y for _, y in batches])
    assert set(aupr) == set(auroc) == set(range(int(ys.max()) + 1)) and 0.0 <= float(acc) <= 1.0
    assert eng.steps_taken == 6 and not model.training
    ref = _fresh_fp64(model)
    for X in (batches[0][0], batches[2][0][:1]):
        assert eng.accepts_eval(X.cuda())
        with torch.no_grad():
            err = CR.rel_l2(eng.logits(X.cuda()), ref(X.double()))
        print(f"LAMERR eval n{X.shape[0]}: logits {err:.1e}")
        assert err <= 1e-5, (X.shape[0], err)


def test_refused_batch_takes_the_torch_path_and_the_engine_continues():
    """Non-zero BatchNorm biases from the start, for the reason tests/test_gpu_cnn_trainer.py gives.  The refused
    batch is stepped by PyTorch with ss_pairing's own torch.randperm pairing; the reference replays it from the same
    CPU generator state."""
    case = CASES[0]
    model0 = LR.make_model(case[0], case[1], case[2], LR.MODEL_SEEDS[case])
    g = torch.Generator().manual_seed(71)
    with torch.no_grad():
        for mod in model0.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    batches = _batches(case, (16, 1040, 16, 16), seed0=70)
    tr = _trainer(model0, LRT, 0.1)
    _engine(tr).record_pairs = True
    torch.manual_seed(123)
    cpu_state = torch.get_rng_state()
    tr.fit(1, batches)
    eng = tr._engine
    assert eng is not None and eng.steps_taken == 3 and 1040 not in eng.sizes
    assert not eng.accepts(batches[1][0].cuda())
    assert all(float(tr.optimizer.state[p]["step"]) == 4.0 for p in tr.model.parameters())
    assert eng.adam.step.tolist() == [4, 0]
    for p in tr.model.parameters():
        assert p.grad.data_ptr() == eng.arena.gptr(p)
    # the pairing ss_pairing drew for the refused batch: the same torch.randperm calls from the same generator state
    torch.set_rng_state(cpu_state)
    y1 = batches[1][1]
    big = torch.arange(1040)
    for c in torch.unique(y1):
        idx = (y1 == c).nonzero(as_tuple=True)[0]
        big[idx] = idx[torch.randperm(idx.shape[0])]
    log = [p.cpu() for p in eng.pair_log]
    pairs = [log[0], big, log[1], log[2]]
    m64 = LR.literal_steps(model0, batches, pairs, 0.1, LRT, torch.float64)[0]
    _compare(tr.model, m64, model0, 3, "refused-batch")


def test_lam_coef_change_between_replays_takes_effect():
    case = CASES[0]
    model0 = LR.make_model(case[0], case[1], case[2], LR.MODEL_SEEDS[case])
    (X, y), = _batches(case, (16,), seed0=80)
    pair = LR.model_pair(y, 80)
    out = {}
    runs = (("change", (0.1, 0.1, 0.1, 4.0)), ("keep", (0.1, 0.1, 0.1, 0.1)), ("fresh", (0.1, 0.1, 0.1, 4.0)))
    for tag, lams in runs:
        tr = _trainer(model0, LR1, lams[0])
        eng = _engine(tr)
        eng.graphs_enabled = tag != "fresh"  # ("fresh": the same sequence without any replay)
        tr.model.train()
        for lam in lams:
            tr.hyperparameter["lam_coef"] = lam
            eng.step(X.cuda(), y.cuda(), pair=pair)
        torch.cuda.synchronize()
        assert ("graph_given" in eng.sizes[16]) == (tag != "fresh")
        out[tag] = _state_bits(tr, eng)
    assert not np.array_equal(out["change"][1], out["keep"][1]), "the new lam_coef had no effect on a replayed step"
    for i, (a, b) in enumerate(zip(out["change"], out["fresh"])):
        assert np.array_equal(a, b), i


def test_simple_model_warns_once_and_trains_in_torch():
    case = CASES[0]
    batches = _batches(case, (16, 16), seed0=90)
    out = []
    for backend in ("device", "torch"):
        model0 = CR.make_model("SimpleCNNClassifier", case[1], case[2], 3)
        # (lam_loss reads cls_head.weight: give the Simple model a one-layer head so the torch loop runs)
        torch.manual_seed(4)
        model0.cls_head = nn.Linear(2048, case[1])
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            tr = _trainer(model0, LRT, 0.1, backend=backend)
            torch.manual_seed(5)  # (ss_pairing's torch.randperm stream)
            tr.fit(2, batches)
        out.append((tr, model0, [w for w in rec if "backend='device'" in str(w.message)]))
    (dev, model0, dev_w), (ref, _, ref_w) = out
    assert len(dev_w) == 1 and "LAMCNNTrainer" in str(dev_w[0].message), [str(w.message) for w in dev_w]
    assert not ref_w
    assert dev._engine is None and ref._engine is None
    # the same PyTorch loop twice.  Not bit for bit: the backward of cls_head.weight[y] adds with atomics.  So TOL,
    # and the conv biases, whose gradients are rounding noise under PyTorch, by the Adam drift bound of _compare
    zero, sd0 = LR.ZERO_GRAD_BIASES["LAMCNNClassifier"], model0.state_dict()
    for (k, a), (_, b) in zip(dev.model.state_dict().items(), ref.model.state_dict().items()):
        if "num_batches" in k:
            assert int(a) == int(b) == 12, k  # (three forwards a step)
        elif k in zero:
            for t in (a, b):
                assert float((t.cpu().double() - sd0[k].double()).abs().max()) <= _drift(4), k
        elif "running_mean" in k:  # (a sub-convex combination of batch means that carry those biases, twice)
            assert float((a - b).abs().max()) <= 2 * _drift(4) + TOL * float(b.abs().max()), k
        else:
            assert CR.rel_l2(a, b) < TOL, (k, CR.rel_l2(a, b))
    assert not torch.equal(dev.model.cls_head.weight.cpu(), model0.cls_head.weight)
