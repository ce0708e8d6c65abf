"""Test helper (no tests here): the downstream probe's training step and eval forward restated in torch on the CPU, the
input generator and the seed rule of tests/test_probe_ref.py and tests/test_gpu_probe.py.

The probe is Linear(d,h) -> BatchNorm1d(h) -> ReLU -> Linear(h,c) with nn.CrossEntropyLoss() defaults
(run_styledmnist_downstream_expr.py:110-117).  step_ref writes the forward, the running-statistics update and the
analytic gradients out by hand (fp64 by default; dtype=torch.float32 is the fp32 restatement whose own error against
fp64 sizes the one exceptional bound of the GPU test); tests/test_probe_ref.py checks it against nn.Sequential +
autograd to 1e-12.

Inputs (make_inputs): x ~ N(0,1) rounded to fp32 in rows of stride ldx; W1, b1 ~ U(+-1/sqrt(d)); gamma ~ U(0.5, 1.5);
beta ~ 0.3 N(0,1); W2, b2 ~ U(+-1/sqrt(h)); labels uniform in [0, c); running_mean ~ 0.2 N(0,1), running_var ~
U(0.5, 2) (non-trivial starts), num_batches_tracked = 5.

Seed rule (find_seed): for a shape, the first seed in 0..63 whose fp64 reference has min |gamma xhat + beta| >= 1e-5,
so no ReLU mask can flip on fp32 rounding.  A condition on the inputs, not a tolerance."""

import functools

import numpy as np
import torch

EPS, MOMENTUM, NBT0 = 1e-5, 0.1, 5
MASK_MARGIN = 1e-5

# (n, d, h, c, ldx)
SHAPES = [
    (128, 8, 256, 10, 32),    # the scripts' MNIST shape
    (32, 32, 256, 10, 128),   # the scripts' VAE64 shape
    (5, 3, 20, 3, 3),         # unaligned rows
    (3, 4, 16, 2, 4),
    (2, 4, 16, 3, 16),        # the minimum batch
    (1000, 8, 256, 10, 8),
    (37, 17, 130, 7, 40),     # nothing divides anything
    (1024, 64, 64, 4, 256),   # contract corner
    (64, 8, 512, 32, 32),     # contract corner
]
NAMES = ("w1", "b1", "gamma", "beta", "w2", "b2")


def shape_id(shape):
    return "n{}-d{}-h{}-c{}-ld{}".format(*shape)


def make_inputs(shape, seed):
    """fp32 numpy arrays: xfull [n][ldx] (x = its first d columns), the six parameters, label, rm, rv."""
    n, d, h, c, ldx = shape
    g = np.random.default_rng([seed, n, d, h, c, ldx])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    kd, kh = 1.0 / np.sqrt(d), 1.0 / np.sqrt(h)
    return dict(
        shape=shape, seed=seed,
        xfull=f32(g.standard_normal((n, ldx))),
        w1=f32(g.uniform(-kd, kd, (h, d))), b1=f32(g.uniform(-kd, kd, h)),
        gamma=f32(g.uniform(0.5, 1.5, h)), beta=f32(0.3 * g.standard_normal(h)),
        w2=f32(g.uniform(-kh, kh, (c, h))), b2=f32(g.uniform(-kh, kh, c)),
        label=g.integers(0, c, n).astype(np.int64),
        rm=f32(0.2 * g.standard_normal(h)), rv=f32(g.uniform(0.5, 2.0, h)),
    )


def _t(inp, dtype):
    d = inp["shape"][1]
    out = {k: torch.from_numpy(inp[k]).to(dtype) for k in NAMES + ("rm", "rv")}
    out["x"] = torch.from_numpy(inp["xfull"][:, :d].copy()).to(dtype)
    out["label"] = torch.from_numpy(inp["label"])
    return out


def step_ref(inp, dtype=torch.float64, eps=EPS, momentum=MOMENTUM):
    """One train-mode step: loss, the analytic gradients (d b1 as the formula gives it: rounding noise around 0),
    the new running statistics, and min |gamma xhat + beta| (the ReLU margin of these inputs)."""
    T = _t(inp, dtype)
    x, y = T["x"], T["label"]
    n = x.shape[0]
    a = x @ T["w1"].T + T["b1"]
    mean = a.sum(0) / n
    var = ((a - mean) ** 2).sum(0) / n
    istd = 1.0 / torch.sqrt(var + eps)
    xhat = (a - mean) * istd
    pre = T["gamma"] * xhat + T["beta"]
    hh = torch.relu(pre)
    logits = hh @ T["w2"].T + T["b2"]
    lse = torch.logsumexp(logits, 1)
    rows = torch.arange(n)
    loss = (lse - logits[rows, y]).sum() / n
    dlog = torch.softmax(logits, 1)
    dlog[rows, y] -= 1.0
    dlog = dlog / n
    dpre = (dlog @ T["w2"]) * (pre > 0).to(dtype)
    dbeta = dpre.sum(0)
    dgamma = (dpre * xhat).sum(0)
    dxhat = dpre * T["gamma"]
    da = istd * (dxhat - dxhat.sum(0) / n - xhat * ((dxhat * xhat).sum(0) / n))
    out = dict(
        loss=loss, logits=logits,
        w1=da.T @ x, b1=da.sum(0), gamma=dgamma, beta=dbeta, w2=dlog.T @ hh, b2=dlog.sum(0),
        rm=(1 - momentum) * T["rm"] + momentum * mean,
        rv=(1 - momentum) * T["rv"] + momentum * var * n / (n - 1),
        margin=float(pre.abs().min()),
    )
    return out


def eval_ref(inp, dtype=torch.float64, eps=EPS):
    """Eval-mode logits (running statistics)."""
    T = _t(inp, dtype)
    a = T["x"] @ T["w1"].T + T["b1"]
    pre = T["gamma"] * (a - T["rm"]) / torch.sqrt(T["rv"] + eps) + T["beta"]
    return torch.relu(pre) @ T["w2"].T + T["b2"]


@functools.lru_cache(maxsize=None)
def find_seed(shape):
    """The first seed in 0..63 with a ReLU margin of at least MASK_MARGIN in the fp64 reference, or None."""
    for seed in range(64):
        if step_ref(make_inputs(shape, seed))["margin"] >= MASK_MARGIN:
            return seed
    return None


@functools.lru_cache(maxsize=None)
def case(shape):
    """(inputs, fp64 step reference) of a shape at its seed (shared by the tests; do not modify)."""
    seed = find_seed(shape)
    assert seed is not None, f"no seed in 0..63 keeps |gamma xhat + beta| >= {MASK_MARGIN} for {shape}"
    inp = make_inputs(shape, seed)
    return inp, step_ref(inp)


def rel_l2(got, want):
    if not torch.is_tensor(got):
        got = torch.as_tensor(np.asarray(got))
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return float((got - want).norm() / (want.norm() + 1e-300))
