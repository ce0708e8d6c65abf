"""Test helper (no tests here): the CNN baseline's classifier tail restated in numpy, the fp64 CPU copy of a whole
classifier, the input generators and the seed rule of tests/test_cnn_ref.py, tests/test_gpu_cnn.py and
tests/test_gpu_cnn_trainer.py.

The tail is BatchNorm1d(h) -> ReLU -> Linear(h,c) with nn.CrossEntropyLoss() defaults on a [n][h], the output of
cls_head[0] (src/models/cnn.py).  tail_step writes the forward, the running-statistics update and the analytic
gradients out by hand (fp64 by default; dtype=np.float32 is the fp32 restatement whose own error against fp64 sizes
the one exceptional bound of the GPU test); tests/test_cnn_ref.py checks it against torch fp64 autograd to 1e-12.

Tail inputs (make_tail): a ~ N(0,1) rounded to fp32; gamma ~ U(0.5, 1.5); beta ~ 0.3 N(0,1); W2, b2 ~ U(+-1/sqrt(h));
labels uniform in [0, c); running_mean ~ 0.2 N(0,1), running_var ~ U(0.5, 2), num_batches_tracked = 5.

Whole-model inputs (model_case): torch.manual_seed(seed), the classifier with PyTorch's default initialisation, images
~ U[0, 1) and labels uniform in [0, n_class) from a generator seeded with seed + 1000.

Seed rule: a seed is accepted only if, in the fp64 reference, no pre-ReLU value (the output of any BatchNorm2d /
BatchNorm1d; for the tail, gamma xhat + beta) is within 1e-5 of zero, so no ReLU mask can flip on fp32 rounding.  A
condition on the inputs, not a tolerance."""

import copy
import functools

import numpy as np
import torch
from torch import nn

EPS, MOMENTUM, NBT0 = 1e-5, 0.1, 5
MASK_MARGIN = 1e-5
TAIL_NAMES = ("gamma", "beta", "w2", "b2")


def shape_id(shape):
    return "n{}-h{}-c{}".format(*shape)


def rel_l2(got, want):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64).reshape(-1)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-300))


# ------------------------------------------------------------------------------------------------ the tail
def make_tail(shape, seed):
    """fp32 numpy arrays: a [n][h], gamma, beta, w2 [c][h], b2, label, rm, rv."""
    n, h, c = shape
    g = np.random.default_rng([seed, n, h, c])
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
    kh = 1.0 / np.sqrt(h)
    return dict(
        shape=shape, seed=seed,
        a=f32(g.standard_normal((n, h))),
        gamma=f32(g.uniform(0.5, 1.5, h)), beta=f32(0.3 * g.standard_normal(h)),
        w2=f32(g.uniform(-kh, kh, (c, h))), b2=f32(g.uniform(-kh, kh, c)),
        label=g.integers(0, c, n).astype(np.int64),
        rm=f32(0.2 * g.standard_normal(h)), rv=f32(g.uniform(0.5, 2.0, h)),
    )


def tail_step(inp, dtype=np.float64, eps=EPS, momentum=MOMENTUM):
    """One train-mode step of the tail: loss, dW2, db2, dgamma, dbeta, da, the new running statistics, the logits and
    min |gamma xhat + beta| (the ReLU margin of these inputs)."""
    T = {k: inp[k].astype(dtype) for k in TAIL_NAMES + ("a", "rm", "rv")}
    a, y = T["a"], inp["label"]
    n = a.shape[0]
    one = dtype(1.0)
    mean = a.sum(0) / dtype(n)
    var = ((a - mean) ** 2).sum(0) / dtype(n)
    istd = one / np.sqrt(var + dtype(eps))
    xhat = (a - mean) * istd
    pre = T["gamma"] * xhat + T["beta"]
    yy = np.maximum(pre, dtype(0.0))
    logits = yy @ T["w2"].T + T["b2"]
    mx = logits.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))[:, 0]
    rows = np.arange(n)
    loss = (lse - logits[rows, y]).sum() / dtype(n)
    dlog = np.exp(logits - lse[:, None])
    dlog[rows, y] -= one
    dlog = dlog / dtype(n)
    dpre = (dlog @ T["w2"]) * (pre > 0).astype(dtype)
    dbeta = dpre.sum(0)
    dgamma = (dpre * xhat).sum(0)
    da = T["gamma"] * istd * (dpre - dbeta / dtype(n) - xhat * (dgamma / dtype(n)))
    return dict(
        loss=loss, logits=logits, w2=dlog.T @ yy, b2=dlog.sum(0), gamma=dgamma, beta=dbeta, da=da,
        rm=(one - dtype(momentum)) * T["rm"] + dtype(momentum) * mean,
        rv=(one - dtype(momentum)) * T["rv"] + dtype(momentum) * var * dtype(n) / dtype(n - 1),
        margin=float(np.abs(pre).min()),
    )


def tail_eval(inp, dtype=np.float64, eps=EPS, a=None):
    """Eval-mode logits (running statistics) of `a` (default: the case's own a)."""
    T = {k: inp[k].astype(dtype) for k in TAIL_NAMES + ("rm", "rv")}
    a = (inp["a"] if a is None else a).astype(dtype)
    pre = T["gamma"] * (a - T["rm"]) / np.sqrt(T["rv"] + dtype(eps)) + T["beta"]
    return np.maximum(pre, dtype(0.0)) @ T["w2"].T + T["b2"]


def tail_torch(inp, eps=EPS, momentum=MOMENTUM):
    """The same step by nn modules and autograd in fp64 on the CPU (what tail_step is checked against)."""
    n, h, c = inp["shape"]
    bn, lin = nn.BatchNorm1d(h, eps=eps, momentum=momentum).double(), nn.Linear(h, c).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(inp["gamma"]))
        bn.bias.copy_(torch.from_numpy(inp["beta"]))
        bn.running_mean.copy_(torch.from_numpy(inp["rm"]))
        bn.running_var.copy_(torch.from_numpy(inp["rv"]))
        bn.num_batches_tracked.fill_(NBT0)
        lin.weight.copy_(torch.from_numpy(inp["w2"]))
        lin.bias.copy_(torch.from_numpy(inp["b2"]))
    a = torch.from_numpy(inp["a"]).double().requires_grad_(True)
    bn.train()
    logits = lin(torch.relu(bn(a)))
    loss = nn.CrossEntropyLoss()(logits, torch.from_numpy(inp["label"]))
    loss.backward()
    out = dict(loss=loss.detach(), logits=logits.detach(), w2=lin.weight.grad, b2=lin.bias.grad, gamma=bn.weight.grad,
               beta=bn.bias.grad, da=a.grad, rm=bn.running_mean.clone(), rv=bn.running_var.clone(),
               nbt=int(bn.num_batches_tracked))
    with torch.no_grad():  # eval-mode logits on the running statistics the step started from
        xn = nn.functional.batch_norm(a.detach(), torch.from_numpy(inp["rm"]).double(),
                                      torch.from_numpy(inp["rv"]).double(), bn.weight, bn.bias, False, momentum, eps)
        out["eval"] = lin(torch.relu(xn))
    return out


@functools.lru_cache(maxsize=None)
def find_tail_seed(shape):
    """The first seed in 0..63 with a ReLU margin of at least MASK_MARGIN in the fp64 reference, or None."""
    for seed in range(64):
        if tail_step(make_tail(shape, seed))["margin"] >= MASK_MARGIN:
            return seed
    return None


@functools.lru_cache(maxsize=None)
def tail_case(shape):
    """(inputs, fp64 step reference) of a shape at its seed (shared by the tests; do not modify)."""
    seed = find_tail_seed(shape)
    assert seed is not None, f"no seed in 0..63 keeps |gamma xhat + beta| >= {MASK_MARGIN} for {shape}"
    inp = make_tail(shape, seed)
    return inp, tail_step(inp)


# ------------------------------------------------------------------------------------------------ the whole classifier
ARCH_HW = {"SimpleCNNClassifier": 28, "SimpleCNN64Classifier": 64}


def make_model(arch, n_class, in_ch, seed):
    """The fp32 CPU classifier with PyTorch's default initialisation under torch.manual_seed(seed)."""
    from src.models import cnn as M

    torch.manual_seed(seed)
    return getattr(M, arch)(n_class=n_class, in_channel=in_ch)


def make_batch(arch, n_class, in_ch, n, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    hw = ARCH_HW[arch]
    X = torch.rand(n, in_ch, hw, hw, generator=g, dtype=torch.float32)
    y = torch.randint(0, n_class, (n,), generator=g, dtype=torch.int64)
    return X, y


def relu_margin(model64, X):
    """min |output of any BatchNorm| of a train-mode forward of X through a copy of `model64`."""
    m = copy.deepcopy(model64).train()
    lo = [float("inf")]

    def hook(_mod, _inp, out):
        lo[0] = min(lo[0], float(out.detach().abs().min()))

    for mod in m.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        m(X.to(next(m.parameters()).dtype))
    return lo[0]


def train_steps(model0, batches, lr, dtype, epochs=1):
    """A copy of `model0` in `dtype` trained on the CPU by torch.optim.Adam over `batches` (epochs times); returns
    (model, optimizer, [loss per step], {name: grad of the last step})."""
    m = copy.deepcopy(model0).to(dtype).train()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    losses = []
    for _ in range(epochs):
        for X, y in batches:
            opt.zero_grad()
            loss = nn.CrossEntropyLoss()(m(X.to(dtype)), y.reshape(-1).long())
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return m, opt, losses, grads


@functools.lru_cache(maxsize=None)
def model_case(arch, n_class, in_ch, n, seed, lr=1e-3):
    """One step at a seed: (fp32 initial model, (X, y), margin, fp64 result, fp32 CPU result); each result is (model,
    optimizer, losses, grads) of train_steps.  Shared by the tests; do not modify."""
    model0 = make_model(arch, n_class, in_ch, seed)
    X, y = make_batch(arch, n_class, in_ch, n, seed)
    margin = relu_margin(copy.deepcopy(model0).double(), X)
    r64 = train_steps(model0, [(X, y)], lr, torch.float64)
    r32 = train_steps(model0, [(X, y)], lr, torch.float32)
    return model0, (X, y), margin, r64, r32


def qualifying_seeds(arch, n_class, in_ch, n, seeds=range(12)):
    out = []
    for s in seeds:
        m0 = make_model(arch, n_class, in_ch, s)
        X, _ = make_batch(arch, n_class, in_ch, n, s)
        if relu_margin(copy.deepcopy(m0).double(), X) >= MASK_MARGIN:
            out.append(s)
    return out


ZERO_GRAD_BIASES = {
    "SimpleCNNClassifier": ("net.0.bias", "net.3.bias", "net.6.bias", "cls_head.0.bias"),
    "SimpleCNN64Classifier": ("net.0.bias", "net.3.bias", "net.6.bias", "net.9.bias", "net.12.bias",
                              "cls_head.0.bias"),
}
