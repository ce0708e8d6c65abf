"""Test helper (no tests here): the LAM baseline's tail restated in numpy, the literal three-forward LAM step run by
PyTorch on the CPU with this repository's src/ modules, the input generators and the seed rule of
tests/test_lam_ref.py, tests/test_gpu_lam.py and tests/test_gpu_lam_trainer.py.

The tail works on y [n][pix][ch], the last conv block's pre-BN output in storage order: h = ReLU(BN(y)) flattened in
PyTorch feature order f = ch * pix + p, cls_head = Linear(F, c), nn.CrossEntropyLoss() defaults and lam_loss
(src/losses.py) between h and h[pair].  tail_step writes the forward and the analytic gradients out by hand (fp64 by
default; dtype=np.float32 is the fp32 restatement whose own error against fp64 sizes the exceptional bound of the GPU
test); tests/test_lam_ref.py checks it against torch fp64 autograd to 1e-12.

Tail inputs (make_tail): y ~ N(0.3, 1) rounded to fp32; gamma ~ U(0.5, 1.5); beta ~ 0.3 N(0,1); W, b ~ U(+-1/sqrt(F));
labels uniform in [0, c) ("absent": in [0, c - 1)); running_mean ~ 0.2 N(0,1), running_var ~ U(0.5, 2).  Pair kinds:
"shuffle" permutes inside each label, "cross" permutes the whole batch, "fixed" permutes inside each label and then
puts every third row back onto itself (swapping values, so it stays a permutation), "absent" is "shuffle" on labels
that leave the last class out.

Whole-model inputs: torch.manual_seed(seed), the LAM classifier with PyTorch's default initialisation, the batch of
cnn_ref.make_batch for the matching Simple architecture, the pair from np.random.default_rng([seed, 2000]) permuting
inside each label.

Seed rule (cnn_ref's): a seed is accepted only if, in the fp64 reference, no BatchNorm output is within 1e-5 of zero,
so no ReLU mask can flip on fp32 rounding.  A condition on the inputs, not a tolerance."""

import copy
import functools

import numpy as np
import torch
from torch import nn

import cnn_ref as CR

EPS, MOMENTUM = CR.EPS, CR.MOMENTUM
MASK_MARGIN = CR.MASK_MARGIN
PAIR_KINDS = ("shuffle", "cross", "fixed", "absent")
rel_l2 = CR.rel_l2


def shape_id(shape):
    return "n{}-ch{}-pix{}-c{}".format(*shape)


# ------------------------------------------------------------------------------------------------ pairs
def stratified_pair(label, g):
    """A permutation inside each label stratum: pair[idx[j]] = idx[perm[j]] (ss_pairing of src/trainer.py)."""
    label = np.asarray(label)
    pair = np.arange(label.size, dtype=np.int64)
    for c in np.unique(label):
        idx = np.nonzero(label == c)[0]
        pair[idx] = idx[g.permutation(idx.size)]
    return pair


def make_pair(label, kind, g):
    n = len(label)
    if kind == "cross":
        return g.permutation(n).astype(np.int64)
    pair = stratified_pair(label, g)
    if kind == "fixed":
        for i in range(0, n, 3):  # i <- i, and whoever pointed at i takes i's old partner
            j = int(np.nonzero(pair == i)[0][0])
            pair[j], pair[i] = pair[i], i
    return pair


# ------------------------------------------------------------------------------------------------ the tail
def make_tail(shape, kind, seed):
    """fp32 numpy arrays: y [n][pix][ch], gamma, beta [ch], w [c][F], b [c], rm, rv [ch]; int64 label, pair."""
    n, ch, pix, c = shape
    g = np.random.default_rng([seed, n, ch, pix, c, PAIR_KINDS.index(kind)])
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
    F = ch * pix
    kf = 1.0 / np.sqrt(F)
    label = g.integers(0, c - 1 if kind == "absent" else c, n).astype(np.int64)
    return dict(
        shape=shape, kind=kind, seed=seed,
        y=f32(g.standard_normal((n, pix, ch)) + 0.3),
        gamma=f32(g.uniform(0.5, 1.5, ch)), beta=f32(0.3 * g.standard_normal(ch)),
        w=f32(g.uniform(-kf, kf, (c, F))), b=f32(g.uniform(-kf, kf, c)),
        label=label, pair=make_pair(label, kind, g),
        rm=f32(0.2 * g.standard_normal(ch) + 0.3), rv=f32(g.uniform(0.5, 2.0, ch)),
    )


def _flat(a):
    """[n][pix][ch] storage order -> [n][F] PyTorch feature order f = ch * pix + p."""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(a.shape[0], -1)


def _storage(a, pix, ch):
    """[n][F] PyTorch feature order -> [n][pix][ch] storage order."""
    return np.ascontiguousarray(a.reshape(a.shape[0], ch, pix).transpose(0, 2, 1))


def tail_step(inp, lam, dtype=np.float64, eps=EPS, pair=None):
    """One train-mode step of the tail: ce, lam (unscaled), gw, gb, gin [n][pix][ch], the BatchNorm backward sums
    gs1 = sum dz, gs2 = sum dz xhat per channel, the logits, pre (the BatchNorm output) and its margin min |pre|."""
    n, ch, pix, c = inp["shape"]
    T = {k: inp[k].astype(dtype) for k in ("y", "gamma", "beta", "w", "b")}
    y, label = T["y"], inp["label"]
    p = inp["pair"] if pair is None else np.asarray(pair)
    q = np.empty_like(p)
    q[p] = np.arange(n)
    one, cnt = dtype(1.0), dtype(n * pix)
    lam = dtype(lam)
    mean = y.sum((0, 1)) / cnt
    var = ((y - mean) ** 2).sum((0, 1)) / cnt
    istd = one / np.sqrt(var + dtype(eps))
    xhat = (y - mean) * istd
    pre = T["gamma"] * xhat + T["beta"]
    h = _flat(np.maximum(pre, dtype(0.0)))
    W = T["w"]
    logits = h @ W.T + T["b"]
    mx = logits.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))[:, 0]
    rows = np.arange(n)
    ce = (lse - logits[rows, label]).sum() / dtype(n)
    dlog = np.exp(logits - lse[:, None])
    dlog[rows, label] -= one
    dlog = dlog / dtype(n)
    d = h - h[p]           # h[i] - h[p_i]
    e = h[q] - h           # h[q_i] - h[i]
    Wy = W[label]
    lam_loss = ((d * Wy) ** 2).sum() / dtype(n)
    two_n = dtype(2.0) / dtype(n)
    gw = dlog.T @ h
    for k in range(c):
        gw[k] += lam * two_n * W[k] * (d[label == k] ** 2).sum(0)
    dh = dlog @ W + lam * two_n * (Wy ** 2 * d - W[label[q]] ** 2 * e)
    gin = _storage(dh, pix, ch) * (pre > 0).astype(dtype)
    return dict(ce=ce, lam=lam_loss, gw=gw, gb=dlog.sum(0), gin=gin, gs1=gin.sum((0, 1)), gs2=(gin * xhat).sum((0, 1)),
                logits=logits, pre=pre, margin=float(np.abs(pre).min()))


def tail_eval(inp, dtype=np.float64, eps=EPS, y=None):
    """Eval-mode logits (running statistics) of `y` (default: the case's own y)."""
    T = {k: inp[k].astype(dtype) for k in ("gamma", "beta", "w", "b", "rm", "rv")}
    y = (inp["y"] if y is None else y).astype(dtype)
    pre = T["gamma"] * (y - T["rm"]) / np.sqrt(T["rv"] + dtype(eps)) + T["beta"]
    return _flat(np.maximum(pre, dtype(0.0))) @ T["w"].T + T["b"]


def tail_torch(inp, lam, eps=EPS):
    """The same step (one-forward form) by nn modules, src.losses.lam_loss and autograd in fp64 on the CPU."""
    from src.losses import lam_loss

    n, ch, pix, c = inp["shape"]
    bn, lin = nn.BatchNorm2d(ch, eps=eps).double(), nn.Linear(ch * pix, c).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(inp["gamma"]))
        bn.bias.copy_(torch.from_numpy(inp["beta"]))
        lin.weight.copy_(torch.from_numpy(inp["w"]))
        lin.bias.copy_(torch.from_numpy(inp["b"]))
    x = torch.from_numpy(inp["y"]).double().permute(0, 2, 1).reshape(n, ch, pix, 1)  # NCHW, H = pix, W = 1
    label, pair = torch.from_numpy(inp["label"]), torch.from_numpy(inp["pair"])
    bn.train()
    pre = bn(x)
    pre.retain_grad()
    h = torch.relu(pre).flatten(1)
    logits = lin(h)
    ce = nn.CrossEntropyLoss()(logits, label)
    ll = lam_loss(h, h[pair], label, lin.weight)
    (ce + lam * ll).backward()
    gin = pre.grad.reshape(n, ch, pix).permute(0, 2, 1)
    return dict(ce=ce.detach(), lam=ll.detach(), gw=lin.weight.grad, gb=lin.bias.grad, gin=gin, gs1=bn.bias.grad,
                gs2=bn.weight.grad, logits=logits.detach())


@functools.lru_cache(maxsize=None)
def find_tail_seed(shape, kind):
    """The first seed in 0..63 with a ReLU margin of at least MASK_MARGIN in the fp64 reference, or None."""
    for seed in range(64):
        if tail_step(make_tail(shape, kind, seed), 0.0)["margin"] >= MASK_MARGIN:
            return seed
    return None


@functools.lru_cache(maxsize=None)
def tail_case(shape, kind):
    """The inputs of a shape and pair kind at its seed (shared by the tests; do not modify)."""
    seed = find_tail_seed(shape, kind)
    assert seed is not None, f"no seed in 0..63 keeps |BN output| >= {MASK_MARGIN} for {shape}"
    return make_tail(shape, kind, seed)


@functools.lru_cache(maxsize=None)
def tail_ref(shape, kind, lam):
    """The fp64 step reference of tail_case(shape, kind) at lam (shared; do not modify)."""
    return tail_step(tail_case(shape, kind), lam)


# ------------------------------------------------------------------------------------------------ the whole classifier
SIMPLE_OF = {"LAMCNNClassifier": "SimpleCNNClassifier", "LAMCNN64Classifier": "SimpleCNN64Classifier"}
MODEL_SEEDS = {  # (arch, n_class, in_ch, n) -> seed
    ("LAMCNNClassifier", 10, 1, 16): 2,
    ("LAMCNNClassifier", 7, 3, 50): 12,
    ("LAMCNN64Classifier", 4, 3, 8): 18,
}
ZERO_GRAD_BIASES = {k: tuple(b for b in CR.ZERO_GRAD_BIASES[v] if b.startswith("net."))
                    for k, v in SIMPLE_OF.items()}


def make_model(arch, n_class, in_ch, seed):
    return CR.make_model(arch, n_class, in_ch, seed)


def make_batch(arch, n_class, in_ch, n, seed):
    return CR.make_batch(SIMPLE_OF[arch], n_class, in_ch, n, seed)


def model_pair(y, seed):
    return torch.from_numpy(stratified_pair(y.numpy(), np.random.default_rng([seed, 2000])))


def literal_steps(model0, batches, pairs, lam, lr, dtype, epochs=1):
    """A copy of `model0` in `dtype` trained on the CPU as LAMCNNTrainer._train does (three train-mode trunk forwards,
    lam_loss, torch.optim.Adam), with X_tilde = X[pair] for the given pairs (one per step, epochs x batches of them).
    Returns (model, optimizer, [(ce, lam) per step], {name: grad of the last step})."""
    from src.losses import lam_loss

    m = copy.deepcopy(model0).to(dtype).train()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    losses, pairs = [], iter(pairs)
    for _ in range(epochs):
        for X, y in batches:
            X, y = X.to(dtype), y.reshape(-1).long()
            X_tilde = X[next(pairs).cpu().long()]
            opt.zero_grad()
            ce = nn.CrossEntropyLoss()(m(X), y)
            ll = lam_loss(m.net(X), m.net(X_tilde), y, m.cls_head.weight)
            (ce + lam * ll).backward()
            opt.step()
            losses.append((float(ce.detach()), float(ll.detach())))
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return m, opt, losses, grads


def one_forward_step(model0, X, y, pair, lam, dtype=torch.float64):
    """The one-forward form of a LAM step on a copy of `model0` (no optimizer): one train-mode trunk pass,
    h[pair] for the second operand of lam_loss, and the running statistics advanced as three forwards of the same
    batch advance them.  Returns (model, (ce, lam), grads)."""
    from src.losses import lam_loss

    m = copy.deepcopy(model0).to(dtype).train()
    before = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k}
    X, y = X.to(dtype), y.reshape(-1).long()
    h = m.net(X)
    ce = nn.CrossEntropyLoss()(m.cls_head(h), y)
    ll = lam_loss(h, h[pair.long()], y, m.cls_head.weight)
    (ce + lam * ll).backward()
    with torch.no_grad():
        for prefix, mod in m.named_modules():
            if isinstance(mod, nn.BatchNorm2d):
                mo = mod.momentum
                for name in ("running_mean", "running_var"):
                    r1, r0 = getattr(mod, name), before[f"{prefix}.{name}"]
                    stat = (r1 - (1 - mo) * r0) / mo  # this batch's statistic
                    r = r1.clone()
                    for _ in range(2):
                        r = (1 - mo) * r + mo * stat
                    r1.copy_(r)
                mod.num_batches_tracked += 2
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return m, (float(ce.detach()), float(ll.detach())), grads


@functools.lru_cache(maxsize=None)
def model_case(arch, n_class, in_ch, n, seed, lam=1.0, lr=1e-3):
    """One step at a seed: (fp32 initial model, (X, y), pair, margin, fp64 result, fp32 CPU result); each result is
    literal_steps' (model, optimizer, losses, grads).  Shared by the tests; do not modify."""
    model0 = make_model(arch, n_class, in_ch, seed)
    X, y = make_batch(arch, n_class, in_ch, n, seed)
    pair = model_pair(y, seed)
    margin = CR.relu_margin(copy.deepcopy(model0).double(), X)
    r64 = literal_steps(model0, [(X, y)], [pair], lam, lr, torch.float64)
    r32 = literal_steps(model0, [(X, y)], [pair], lam, lr, torch.float32)
    return model0, (X, y), pair, margin, r64, r32
