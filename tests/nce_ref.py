"""fp64 references for InfoNCE and CLUBMean (reference mi_estimator.py:245-273 and 65-105), shared by
tests/test_gpu_mi_nce_clubmean.py and tests/test_gpu_mim_nce_step.py.

The literal forms are the reference's own tensor code: InfoNCE tiles x and y into [N, N, dx+dy] and runs the critic
on every pair; CLUBMean broadcasts [N, N, d].  Above LITERAL_MAX rows the same sums are taken over blocks of rows
(the literal InfoNCE at n = 1025 would hold 1025 * 1025 * (2d + H) doubles), differentiated block by block; autograd
accumulates the leaves' gradients across the blocks.  Every reference is computed once (lru_cache) on deterministic
fp32 weights and inputs, in fp64, and nothing modifies what it returns."""

import functools
import math

import torch
import torch.nn.functional as F

LITERAL_MAX = 257


def det_weights(kind, d, hidden, scale=1.0):
    """Deterministic fp32 state_dict of InfoNCE(d, d, hidden).F_func / CLUBMean(d, d, hidden).p_mu: nn.Linear's
    uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)); `scale` multiplies the critic's output layer."""
    g = torch.Generator().manual_seed(77 * d + hidden + (0 if kind == "InfoNCE" else 5000))

    def lin(o, i):
        b = 1.0 / math.sqrt(i)
        return ((torch.rand(o, i, generator=g) * 2 - 1) * b, (torch.rand(o, generator=g) * 2 - 1) * b)

    if kind == "InfoNCE":
        w1, b1 = lin(hidden, 2 * d)
        w2, b2 = lin(1, hidden)
        return {"F_func.0.weight": w1, "F_func.0.bias": b1, "F_func.2.weight": w2 * scale, "F_func.2.bias": b2 * scale}
    w1, b1 = lin(hidden, d)
    w2, b2 = lin(d, hidden)
    return {"p_mu.0.weight": w1, "p_mu.0.bias": b1, "p_mu.2.weight": w2, "p_mu.2.bias": b2}


def critic(P, xy):
    """F_func (mi_estimator.py:250-253): Linear -> ReLU -> Linear -> Softplus."""
    hid = torch.relu(xy @ P["F_func.0.weight"].T + P["F_func.0.bias"])
    return F.softplus(hid @ P["F_func.2.weight"].T + P["F_func.2.bias"])


def log_n(n):
    """log n as the reference takes it, torch.tensor(sample_size).log() (mi_estimator.py:268): an integer tensor's
    log is fp32, whatever the dtype of the samples."""
    return float(torch.tensor(n).log())


def infonce_literal(P, x, y):
    """InfoNCE.forward as the reference writes it (mi_estimator.py:259-270)."""
    n = y.shape[0]
    x_tile = x.unsqueeze(0).repeat((n, 1, 1))
    y_tile = y.unsqueeze(1).repeat((1, n, 1))
    t0 = critic(P, torch.cat([x, y], dim=-1))
    t1 = critic(P, torch.cat([x_tile, y_tile], dim=-1))
    return t0.mean() - (t1.logsumexp(dim=1).mean() - torch.tensor(n).log())


def infonce_blockwise_backward(P, x, y, block=32):
    """The same value over blocks of rows i; calls backward block by block (P, x, y: leaves) and returns the value."""
    n = y.shape[0]
    total = log_n(n)
    for r0 in range(0, n, block):
        yy = y[r0:r0 + block]
        b = yy.shape[0]
        t0 = critic(P, torch.cat([x[r0:r0 + block], yy], dim=-1))
        t1 = critic(P, torch.cat([x.unsqueeze(0).expand(b, n, -1), yy.unsqueeze(1).expand(b, n, -1)], dim=-1))
        part = (t0.sum() - t1.logsumexp(dim=1).sum()) / n
        part.backward()
        total += float(part.detach())
    return total


def p_mu(P, x):
    return torch.relu(x @ P["p_mu.0.weight"].T + P["p_mu.0.bias"]) @ P["p_mu.2.weight"].T + P["p_mu.2.bias"]


def clubmean_literal(mu, y):
    """CLUBMean.forward (mi_estimator.py:84-97)."""
    positive = -((mu - y) ** 2) / 2.0
    negative = -((y.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0
    return (positive.sum(dim=-1) - negative.sum(dim=-1)).mean()


def clubmean_blockwise_backward(P, x, y, block=32):
    n = y.shape[0]
    total = 0.0
    for r0 in range(0, n, block):
        mu, yy = p_mu(P, x[r0:r0 + block]), y[r0:r0 + block]
        positive = -((mu - yy) ** 2) / 2.0
        negative = -((y.unsqueeze(0) - mu.unsqueeze(1)) ** 2).mean(dim=1) / 2.0
        part = (positive.sum(dim=-1) - negative.sum(dim=-1)).sum() / n
        part.backward()
        total += float(part.detach())
    return total


def clubmean_loglikeli(P, x, y):
    """CLUBMean.loglikeli (mi_estimator.py:99-101): no division by two."""
    return (-((p_mu(P, x) - y) ** 2)).sum(dim=1).mean(dim=0)


def inputs(n, d):
    """fp32 x and y; y with a non-zero mean and a non-unit scale."""
    g = torch.Generator().manual_seed(1000 * n + d)
    x32 = torch.randn(n, d, generator=g, dtype=torch.float32)
    y32 = 1.5 * torch.randn(n, d, generator=g, dtype=torch.float32) + 0.7
    return x32, y32


def forward_backward(kind, W, x32, y32, dtype=torch.float64):
    """value, d/dx, d/dy and the parameter gradients of est.forward in `dtype` on the CPU."""
    P = {k: v.to(dtype).requires_grad_(True) for k, v in W.items()}
    x, y = x32.to(dtype).requires_grad_(True), y32.to(dtype).requires_grad_(True)
    n = x.shape[0]
    if n <= LITERAL_MAX:
        val = infonce_literal(P, x, y) if kind == "InfoNCE" else clubmean_literal(p_mu(P, x), y)
        val.backward()
        value = float(val.detach())
    elif kind == "InfoNCE":
        value = infonce_blockwise_backward(P, x, y)
    else:
        value = clubmean_blockwise_backward(P, x, y)
    return dict(value=value, gx=x.grad.clone(), gy=y.grad.clone(), gp={k: v.grad.clone() for k, v in P.items()})


@functools.lru_cache(maxsize=None)
def reference(kind, n, d, hidden, scale=1.0):
    """fp64 reference of est.forward (value, gx, gy, gp) and of est.learning_loss (loss, lgp) on deterministic
    weights W and inputs x, y (fp32 values: the device sees exactly what the reference differentiates)."""
    W = det_weights(kind, d, hidden, scale)
    x32, y32 = inputs(n, d)
    out = forward_backward(kind, W, x32, y32)
    if kind == "InfoNCE":  # learning_loss = -forward (mi_estimator.py:272-273)
        loss, lgp = -out["value"], {k: -v for k, v in out["gp"].items()}
    else:  # learning_loss = -loglikeli (mi_estimator.py:103-105)
        P = {k: v.double().requires_grad_(True) for k, v in W.items()}
        ll = -clubmean_loglikeli(P, x32.double(), y32.double())
        ll.backward()
        loss, lgp = float(ll.detach()), {k: v.grad.clone() for k, v in P.items()}
    scale = {}
    if kind == "CLUBMean":
        # d forward / d p_mu.2.bias = mean_i (y_i - mean y) is zero identically (mu_i enters the positive and the
        # negative term with opposite signs), so its fp64 "reference" is rounding noise and a ratio against it says
        # nothing; the error of that one tensor is measured against the positive term's gradient instead, the
        # magnitude of each of the two parts that cancel
        P = {k: v.double().requires_grad_(True) for k, v in W.items()}
        (-((p_mu(P, x32.double()) - y32.double()) ** 2) / 2.0).sum(dim=-1).mean().backward()
        scale["p_mu.2.bias"] = float(P["p_mu.2.bias"].grad.norm())
    return dict(out, W=W, x=x32, y=y32, loss=loss, lgp=lgp, scale=scale)


def grad_error(ref, k, got):
    """rel-L2 of a forward parameter gradient against the fp64 one (see `scale` in reference())."""
    if k in ref["scale"]:
        return float((torch.as_tensor(got).double().cpu() - ref["gp"][k]).norm() / ref["scale"][k])
    return rel(got, ref["gp"][k])


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1).cpu(), torch.as_tensor(b).double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
