"""The device CNN baseline on the GPU, engine and trainer: cvhip.cnn.CnnStep and SimpleCNNTrainer(backend="device")
against the fp64 CPU model of tests/cnn_ref.py (this repository's src/models/cnn.py run by PyTorch in fp64 with
torch.optim.Adam).

Inputs and the seed rule: tests/cnn_ref.py (uniform images, random labels; in the single-step cases no BatchNorm output
of the fp64 reference is within 1e-5 of zero, so fp32 rounding flips no ReLU mask; tests/test_cnn_ref.py asserts the
rule on the same seeds).

Bounds.  One step: per tensor (loss, every p.grad, every BatchNorm's running_mean / running_var), relative L2 against
fp64 <= 30 x the error of the same step run by PyTorch in fp32 on the CPU, computed in the test; where that product
exceeds 1e-4 the case counts as ill-conditioned (another qualifying seed is due, never a looser bound).
num_batches_tracked is exact.  The biases that feed a train-mode BatchNorm (conv biases, cls_head.0.bias) have p.grad
exactly 0 and stay bit-unchanged.  The Adam part: tests/adam_ref.py fed the gradients the step itself wrote, as
tests/test_gpu_adam_engine.py.  Trainer: TOL = 1e-4 relative on parameters and running statistics
(tests/test_gpu_downstream.py).  After a step PyTorch took (a refused batch) the zero-gradient biases carry Adam steps
on rounding noise, at most lr each, and the running mean behind them carries the same drift (the allowance of
tests/test_gpu_probe.py, restated in _drift).  That sequence starts from non-zero BatchNorm biases, so that TOL
measures the tensors and not the rounding of PyTorch's own n = 1040 step against biases of a few lr.

Measured on an MI355X (the tests print CNNERR lines):
  one step, relative L2 against fp64, device / bound (30 x the fp32 CPU run), the worst tensor of each kind:
    SimpleCNNClassifier(10, 1) n=16 seed 2:    loss 7.6e-08 / 9.1e-07; grads <= 8.7e-07 (net.7.weight) against bounds
      >= 3.2e-06; running statistics <= 1.6e-07 / 4.6e-06 (cls_head.1.running_mean); largest bound 3.1e-05
    SimpleCNNClassifier(7, 3) n=50 seed 12:    loss 1.1e-07 / 3.4e-06; grads <= 1.0e-06 (net.0.weight, bound 4.1e-05);
      running statistics <= 1.5e-07 / 3.1e-06
    SimpleCNN64Classifier(4, 3) n=8 seed 18:   loss 1.2e-07 / 1.2e-06; grads <= 1.7e-06 (net.1.bias, bound 4.2e-05;
      tightest cls_head.3.bias 1.1e-07 / 9.8e-07); running statistics <= 4.6e-07 / 1.2e-05; largest bound 5.6e-05
    Adam part (p in lr, m in |g|, v in g^2; kernel | e32): 5.94e-05 5.68e-09 1.17e-10 | the same
  fit(2) over 16, 16, 5 against the fp64 loop: <= 1.2e-05 (net.4.bias); weights <= 3.5e-06; eval logits 2.8e-07 (n=16),
    1.6e-07 (n=1)
  16, 1040 (refused, PyTorch), 16, 16 from non-zero BatchNorm biases: <= 7.2e-07 (cls_head.0.weight); the BatchNorm
    biases 4.2e-08 - 5.6e-08.  (From zero-initialised biases the same sequence gave net.1 / 4 / 7.bias 1.5e-04,
    2.6e-04, 6.7e-04, and backend="torch" alone 1.7e-04, 2.7e-04, 6.7e-04: the ill-conditioned input this test avoids.)
"""

import copy
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import adam_ref as AR
import cnn_ref as CR
from test_cnn_ref import MODEL_SEEDS

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_downstream.py
LR1 = 1e-3  # the single-step cases (cnn_ref.model_case)
LR = 1e-4   # the trainer cases (the scripts' value)
CASES = list(MODEL_SEEDS)
IDS = [f"{c[0]}-c{c[1]}-ch{c[2]}-n{c[3]}" for c in CASES]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy().copy()


def _trainer(model0, lr, backend="device", criterion=None, optimizer=None, transform=None, state=None):
    from src.trainer import SimpleCNNTrainer

    model = copy.deepcopy(model0)
    if state is not None:
        model.load_state_dict(state)
    model = model.cuda()
    opt = (optimizer or (lambda ps: torch.optim.Adam(ps, lr=lr)))(model.parameters())
    return SimpleCNNTrainer(model, opt, criterion or nn.CrossEntropyLoss(), 10, torch.device("cuda"),
                            transform=transform, backend=backend)


def _engine(tr):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng = tr._cnn_engine()
    assert eng is not None, "the device backend was refused"
    return eng


def _bn_buffers(model):
    return {k: v for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}


# ------------------------------------------------------------------------------------------------ 4. one step
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_step_against_fp64(case):
    arch, n_class, in_ch, n = case
    seed = MODEL_SEEDS[case]
    model0, (X, y), margin, r64, r32 = CR.model_case(arch, n_class, in_ch, n, seed, LR1)
    assert margin >= CR.MASK_MARGIN
    tr = _trainer(model0, LR1)
    model, eng = tr.model, _engine(tr)
    model.train()
    host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    before = (host(eng.arena.flat), host(eng.adam.m), host(eng.adam.v))
    p_before = {k: _bits(p) for k, p in model.named_parameters()}
    loss = float(eng.step(X.cuda(), y.cuda()))
    torch.cuda.synchronize()
    m64, _, l64, g64 = r64
    m32, _, l32, g32 = r32
    rows = []

    def check(name, got, want, base):
        err, bound = CR.rel_l2(got, want), 30.0 * CR.rel_l2(base, want)
        rows.append(f"{name} {err:.1e}/{bound:.1e}")
        return name, err, bound

    res = [("loss", abs(loss - l64[0]) / abs(l64[0]), 30.0 * abs(l32[0] - l64[0]) / abs(l64[0]))]
    rows.append(f"loss {res[0][1]:.1e}/{res[0][2]:.1e}")
    zero = CR.ZERO_GRAD_BIASES[arch]
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == eng.arena.gptr(p), k
        if k in zero:
            assert not _bits(p.grad).any(), f"{k}.grad must be exact zeros"
            assert np.array_equal(_bits(p), p_before[k]), f"{k} moved under an exact-zero gradient"
        else:
            res.append(check(k, p.grad, g64[k], g32[k]))
    b64, b32 = _bn_buffers(m64), _bn_buffers(m32)
    for k, v in _bn_buffers(model).items():
        if "num_batches" in k:
            assert int(v) == int(b64[k]) == 1, k
        else:
            res.append(check(k, v, b64[k], b32[k]))
    print(f"CNNERR step {IDS[CASES.index(case)]} seed {seed} (device/bound): " + " ".join(rows))
    for name, err, bound in res:
        assert bound <= TOL, ("ill-conditioned case: pick another qualifying seed", name, bound)
        assert err <= bound, (name, err, bound)
    # the Adam part: adam_ref fed the gradients the step itself wrote
    g = host(eng.arena.grad)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    case_a = AR.Case(*before, g[None], (LR1, 0.9, 0.999, 1e-8, 0.0), 0)
    err, ok = case_a.errors(0, host(eng.arena.flat), host(eng.adam.m), host(eng.adam.v))
    print(f"ADAMERR cnn step: kernel p {err[0]:.3g} m {err[1]:.3g} v {err[2]:.3g} | e32 p {case_a.e32_p[0]:.3g} "
          f"m {case_a.e32_m[0]:.3g} v {case_a.e32_v[0]:.3g}")
    assert ok, err
    assert eng.adam.step.tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ 5. eager vs replay
def _state_bits(tr, eng):
    out = [_bits(eng.loss), _bits(eng.arena.flat), _bits(eng.arena.grad), _bits(eng.adam.m), _bits(eng.adam.v),
           np.array(eng.adam.step.tolist())]
    return out + [_bits(v) for v in _bn_buffers(tr.model).values()]


def test_eager_and_replayed_steps_are_bit_identical():
    case = CASES[0]
    model0 = CR.make_model(case[0], case[1], case[2], MODEL_SEEDS[case])
    batches = [CR.make_batch(case[0], case[1], case[2], case[3], 40 + s) for s in range(4)]
    runs = []
    for graphs in (True, False):
        tr = _trainer(model0, LR1)
        eng = _engine(tr)
        eng.graphs_enabled = graphs
        tr.model.train()
        states = []
        for X, y in batches:
            eng.step(X.cuda(), y.cuda())
            torch.cuda.synchronize()
            states.append(_state_bits(tr, eng))
        assert ("graph" in eng.sizes[case[3]]) == graphs and eng.sizes[case[3]]["count"] == 4
        runs.append(states)
    for k in range(4):
        for i, (a, b) in enumerate(zip(runs[0][k], runs[1][k])):
            assert np.array_equal(a, b), (k, i)
    assert not np.array_equal(runs[0][0][1], runs[0][3][1])  # (the parameters did move)


# ------------------------------------------------------------------------------------------------ 6. trainer
def _rel(a, b):
    return CR.rel_l2(a, b)


def _drift(T):
    """|b_t - b_0| <= t lr for a bias under Adam, and running_mean is a sub-convex combination of batch means."""
    return T * LR * 1.01


def _compare(model, m64, model0, torch_steps, tag):
    """Parameters and running statistics against the fp64 loop; torch_steps: Adam updates of the zero-gradient biases
    that carried rounding noise (steps PyTorch took on the device, and every later step while their moment decays)."""
    zero = CR.ZERO_GRAD_BIASES[type(model).__name__]
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
            worst[k] = _rel(a, b)
    print(f"CNNERR trainer {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < TOL, (k, v)


def _batches(case, sizes, seed0=60):
    return [CR.make_batch(case[0], case[1], case[2], n, seed0 + i) for i, n in enumerate(sizes)]


def _fresh_fp64(model):
    m = type(model)(n_class=model.cls_head[3].out_features, in_channel=model.net[0].in_channels).double()
    m.load_state_dict({k: (v.cpu().double() if v.dtype.is_floating_point else v.cpu())
                       for k, v in model.state_dict().items()})
    return m.eval()


def test_trainer_fit_matches_the_fp64_loop():
    case = CASES[0]
    model0 = CR.make_model(case[0], case[1], case[2], MODEL_SEEDS[case])
    batches = _batches(case, (16, 16, 5))
    tr = _trainer(model0, LR)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr.fit(2, batches)
    assert not [w for w in rec if "SimpleCNNTrainer" in str(w.message)], "the device backend was refused"
    eng, model, opt = tr._engine, tr.model, tr.optimizer
    assert eng is not None and eng.steps_taken == 6
    assert all("graph" in eng.sizes[m] and eng.sizes[m]["count"] == cnt for m, cnt in ((16, 4), (5, 2)))
    for p in model.parameters():
        st = opt.state[p]
        assert float(st["step"]) == 6.0
        o, _ = eng.arena.offset[id(p)]
        assert st["exp_avg"].data_ptr() == eng.adam.m.data_ptr() + 4 * o  # (a live view of the engine's moments)
        assert p.grad is not None and p.grad.data_ptr() == eng.arena.grad.data_ptr() + 4 * o
    assert float(opt.state[model.cls_head[3].weight]["exp_avg"].abs().max()) > 0
    m64 = CR.train_steps(model0, batches, LR, torch.float64, epochs=2)[0]
    _compare(model, m64, model0, 0, "fit")

    # evaluate(): the reference's structure, through cv_cls_forward; logits against fp64 on the same parameters
    (aupr, auroc), acc = tr.evaluate(batches, verbose=False, epoch_id=0)
    ys = torch.cat([y for _, y in batches])
    assert set(aupr) == set(auroc) == set(range(int(ys.max()) + 1)) and 0.0 <= float(acc) <= 1.0
    assert eng.steps_taken == 6 and not model.training
    ref = _fresh_fp64(model)
    for X in (batches[0][0], batches[2][0][:1]):
        assert eng.accepts_eval(X.cuda())
        with torch.no_grad():
            err = _rel(eng.logits(X.cuda()), ref(X.double()))
        print(f"CNNERR eval n{X.shape[0]}: logits {err:.1e}")
        assert err <= 1e-5, (X.shape[0], err)


def test_refused_batch_takes_the_torch_path_and_the_engine_continues():
    """The model starts from non-zero BatchNorm biases (0.3 N(0,1), as the tail inputs of cnn_ref): from PyTorch's
    zero initialisation the biases are a few lr after four steps, and the relative error of such a tensor measures the
    rounding of PyTorch's own n = 1040 step (cancelling sums of 1040 x H x W terms behind Adam) against a norm of
    4e-4, not the engine: an ill-conditioned input, replaced rather than given a wider bound."""
    case = CASES[0]
    model0 = CR.make_model(case[0], case[1], case[2], MODEL_SEEDS[case])
    g = torch.Generator().manual_seed(71)
    with torch.no_grad():
        for mod in model0.modules():
            if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    batches = _batches(case, (16, 1040, 16, 16), seed0=70)
    tr = _trainer(model0, LR)
    tr.fit(1, batches)
    eng = tr._engine
    assert eng is not None and eng.steps_taken == 3 and 1040 not in eng.sizes
    assert not eng.accepts(batches[1][0].cuda())
    assert all(float(tr.optimizer.state[p]["step"]) == 4.0 for p in tr.model.parameters())
    assert eng.adam.step.tolist() == [4, 0]
    for p in tr.model.parameters():
        assert p.grad.data_ptr() == eng.arena.gptr(p)
    m64 = CR.train_steps(model0, batches, LR, torch.float64)[0]
    _compare(tr.model, m64, model0, 3, "refused-batch")


# ------------------------------------------------------------------------------------------------ 7. state changes
@pytest.mark.parametrize("how", ["load_state_dict", "data"])
def test_state_change_between_replays_is_picked_up(how):
    case = CASES[0]
    seed = MODEL_SEEDS[case]
    model0 = CR.make_model(case[0], case[1], case[2], seed)
    other = CR.make_model(case[0], case[1], case[2], seed + 1).state_dict()
    other["net.1.running_mean"] = other["net.1.running_mean"] + 0.25
    (X, y), (X2, y2) = _batches(case, (16, 16), seed0=80)
    tr = _trainer(model0, LR1)
    eng = _engine(tr)
    tr.model.train()
    for _ in range(3):
        eng.step(X.cuda(), y.cuda())
    assert "graph" in eng.sizes[16]
    eng.sync_host_state()
    opt_state = copy.deepcopy(tr.optimizer.state_dict())  # (what a checkpoint taken here would hold)
    if how == "load_state_dict":
        tr.model.load_state_dict(other)
    else:
        with torch.no_grad():
            for k, p in tr.model.named_parameters():
                p.data.copy_(other[k])
            for k, b in tr.model.named_buffers():
                b.copy_(other[k])
        tr.invalidate_packed()
    eng.step(X2.cuda(), y2.cuda())
    torch.cuda.synchronize()
    eng.sync_host_state()
    got = _state_bits(tr, eng)

    # a fresh engine on `other`, adopting the optimizer state the first one had before its last step
    tr_b = _trainer(model0, LR1, state=other)
    tr_b.optimizer.load_state_dict(opt_state)
    eng_b = _engine(tr_b)
    assert eng_b.adam.step.tolist() == [3, 0]
    tr_b.model.train()
    eng_b.step(X2.cuda(), y2.cuda())
    torch.cuda.synchronize()
    want = _state_bits(tr_b, eng_b)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (how, i)


# ------------------------------------------------------------------------------------------------ 8. refusals
def _fit_pair(build):
    """(device-backend trainer, its warnings, torch-backend trainer) after the same two epochs."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # (both runs: bit-identity of two PyTorch runs is what is compared)
    try:
        out = []
        for backend in ("device", "torch"):
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                tr, batches = build(backend)
                tr.fit(2, batches)
            out.append((tr, [w for w in rec if "backend='device'" in str(w.message)]))
        return out
    finally:
        torch.backends.cudnn.deterministic = prev


@pytest.mark.parametrize("what", ["lam_model", "label_smoothing", "sgd", "transform"])
def test_outside_contract_warns_once_and_runs_as_torch(what):
    from src.models.cnn import LAMCNNClassifier

    case = CASES[0]
    batches = _batches(case, (16, 16), seed0=90)

    def build(backend):
        if what == "lam_model":
            torch.manual_seed(3)
            model0 = LAMCNNClassifier(case[1], case[2])
        else:
            model0 = CR.make_model(case[0], case[1], case[2], MODEL_SEEDS[case])
        kw = {}
        if what == "label_smoothing":
            kw["criterion"] = nn.CrossEntropyLoss(label_smoothing=0.1)
        if what == "sgd":
            kw["optimizer"] = lambda ps: torch.optim.SGD(ps, lr=1e-2)
        if what == "transform":
            kw["transform"] = lambda x: x * 1.0
        return _trainer(model0, LR, backend=backend, **kw), batches

    (dev, dev_w), (ref, ref_w) = _fit_pair(build)
    assert len(dev_w) == 1, [str(w.message) for w in dev_w]
    assert not ref_w
    assert dev._engine is None and ref._engine is None  # (backend="torch" never builds an engine)
    for (k, a), (_, b) in zip(dev.model.state_dict().items(), ref.model.state_dict().items()):
        assert torch.equal(a, b), k
