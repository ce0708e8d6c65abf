"""Test helper (no tests here): torch.optim.Adam (foreach semantics) restated in numpy, the inputs and the tolerance
rule of the Adam kernel tests (tests/test_adam_ref.py, tests/test_gpu_adam.py, tests/test_gpu_adam_engine.py).

adam_ref is the reference: fp32 inputs widened to fp64, one update per row of `grads_per_step`

    g   = g * grad_scale (+ weight_decay * p)
    m  += (1 - beta1) * (g - m)
    v   = beta2 * v + (1 - beta2) * g * g
    den = sqrt(v) / sqrt(1 - beta2^t) + eps
    p  -= lr / (1 - beta1^t) * m / den            t = t0 + k + 1

The same function with dtype=np.float32 is the fp32 restatement: the arithmetic a correct fp32 kernel performs, up to
the order of a few roundings.  Its error against the fp64 reference (e32) is the yardstick of the tolerance rule
(`Case`): a kernel may differ from the reference by 8 x e32 (contraction of a*b+c, the kernels' pre-divided constants
-lr/bc1 and sqrt(bc2) rounded to fp32), never less than one fp32 ulp of the value.  The errors are normalised: p by lr,
m by the element's gradient magnitude, v by its square, so one figure per step covers elements whose gradients span
24 decades.  The gradient magnitude of an element is the largest |g * grad_scale + weight_decay * p| the reference saw
for it (for a warm start also |m0| and sqrt(v0), which are bounded by the magnitudes of the earlier steps).

MUTANTS are deliberately wrong restatements (tests/test_adam_ref.py pins that none of them fits under the rule)."""

import numpy as np

# (lr, beta1, beta2, eps, weight_decay), grad_scale
HYPER_A, SCALE_A = (5e-4, 0.9, 0.999, 1e-8, 0.0), 1.0
HYPER_B, SCALE_B = (2e-3, 0.8, 0.95, 1e-6, 0.01), 0.25
SETS = {"A": (HYPER_A, SCALE_A), "B": (HYPER_B, SCALE_B)}
STEPS = 12
WARM = 7  # steps of the reference that produce the moments of a warm start
SEED = 20240607
TOL_FACTOR = 8.0

MUTANTS = ("bc_one_step_behind", "no_bc2", "eps_inside_sqrt", "eps_before_bc2", "beta1_in_v_decay",
           "weight_decay_ignored", "grad_scale_ignored")


def _hyper_rows(hyper, steps, dtype):
    h = np.asarray(hyper, dtype=np.float32)
    if h.ndim == 1:
        h = np.broadcast_to(h[:5], (steps, 5))
    assert h.shape == (steps, 5), h.shape
    return h.astype(dtype)


def adam_ref(p, m, v, grads_per_step, hyper, t0, grad_scale=1.0, dtype=np.float64, mutant=None):
    """(P, M, V), each [steps][numel]: parameters and moments after every step.  hyper: (lr, beta1, beta2, eps,
    weight_decay), or one such row per step (a learning rate changed between steps)."""
    assert mutant is None or mutant in MUTANTS, mutant
    G = np.asarray(grads_per_step, dtype=np.float32)
    steps = G.shape[0]
    H = _hyper_rows(hyper, steps, dtype)
    p, m, v = (np.asarray(a, dtype=np.float32).astype(dtype).reshape(-1) for a in (p, m, v))
    gs = np.float32(grad_scale).astype(dtype)
    one = dtype(1)
    P, M, V = (np.empty((steps, p.size), dtype=dtype) for _ in range(3))
    with np.errstate(all="raise", under="ignore"):
        for k in range(steps):
            lr, b1, b2, eps, wd = H[k]
            t = t0 + k + 1
            if mutant == "bc_one_step_behind":
                t = max(t - 1, 1)
            g = G[k].astype(dtype).reshape(-1)
            if mutant != "grad_scale_ignored":
                g = g * gs
            if wd != 0 and mutant != "weight_decay_ignored":
                g = g + wd * p
            m = m + (one - b1) * (g - m)
            v = (b1 if mutant == "beta1_in_v_decay" else b2) * v + (one - b2) * g * g
            bc1 = one - b1 ** dtype(t)
            bc2 = one - b2 ** dtype(t)
            if mutant == "no_bc2":
                den = np.sqrt(v) + eps
            elif mutant == "eps_inside_sqrt":
                den = np.sqrt(v / bc2 + eps)
            elif mutant == "eps_before_bc2":
                den = (np.sqrt(v) + eps) / np.sqrt(bc2)
            else:
                den = np.sqrt(v) / np.sqrt(bc2) + eps
            p = p - (lr / bc1) * (m / den)
            P[k], M[k], V[k] = p, m, v
    return P, M, V


def make_grads(numel, steps, seed=SEED):
    """[steps][numel] fp32 gradients: per-element magnitudes log-uniform over 1e-9 .. 10 with fresh signs every
    step; a block whose gradient is exactly 0 at every step (`zero_block`); a few elements of magnitude ~1e15 (their
    squares stay far below the fp32 maximum)."""
    rng = np.random.default_rng([seed, numel])
    mag = 10.0 ** rng.uniform(-9.0, 1.0, numel)
    mag[huge_elements(numel)] = 1e15 * rng.uniform(0.5, 2.0, len(huge_elements(numel)))
    z0, z1 = zero_block(numel)
    mag[z0:z1] = 0.0
    sign = rng.integers(0, 2, (steps, numel)) * 2.0 - 1.0
    return (sign * mag).astype(np.float32)


def zero_block(numel):
    z0 = numel // 3
    return z0, z0 + max(1, numel // 8)


def huge_elements(numel):
    idx = [numel - 1] + ([numel // 2, 5] if numel >= 64 else [])
    z0, z1 = zero_block(numel)
    return [i for i in idx if not z0 <= i < z1]


class Case:
    """Inputs, fp64 reference and tolerances of one trajectory.  p0 / m0 / v0 [numel] and g [steps][numel] are the
    fp32 inputs the kernel under test gets; P / M / V the reference after every step; tol_p / tol_m / tol_v
    [steps][numel] what the kernel may differ by; e32_p / e32_m / e32_v [steps] the normalised errors of the fp32
    restatement they come from."""

    def __init__(self, p0, m0, v0, g, hyper, t0, grad_scale=1.0):
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))  # noqa: E731
        self.p0, self.m0, self.v0 = f32(p0), f32(m0), f32(v0)
        self.g = np.ascontiguousarray(np.asarray(g, dtype=np.float32))
        self.hyper, self.t0, self.grad_scale = hyper, t0, grad_scale
        self.steps, self.numel = self.g.shape
        args = (self.p0, self.m0, self.v0, self.g, hyper, t0, grad_scale)
        self.P, self.M, self.V = adam_ref(*args)
        r32 = adam_ref(*args, dtype=np.float32)
        H = _hyper_rows(hyper, self.steps, np.float64)
        self.lr = H[:, 0]
        # the gradients the reference consumed, after grad_scale and weight decay
        prev = np.concatenate([self.p0[None].astype(np.float64), self.P[:-1]])
        geff = self.g.astype(np.float64) * float(np.float32(grad_scale)) + H[:, 4:5] * prev
        self.gmag = np.maximum(np.abs(geff).max(0),
                               np.maximum(np.abs(self.m0.astype(np.float64)), np.sqrt(self.v0.astype(np.float64))))
        live = self.gmag > 0
        gm = np.where(live, self.gmag, 1.0)
        self.e32_p = np.abs(r32[0] - self.P).max(1) / self.lr
        self.e32_m = (np.abs(r32[1] - self.M) / gm).max(1)
        self.e32_v = (np.abs(r32[2] - self.V) / (gm * gm)).max(1)
        ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)  # noqa: E731
        self.tol_p = np.maximum(TOL_FACTOR * (self.e32_p * self.lr)[:, None], ulp(self.P))
        self.tol_m = np.maximum(TOL_FACTOR * self.e32_m[:, None] * self.gmag[None], ulp(self.M))
        self.tol_v = np.maximum(TOL_FACTOR * self.e32_v[:, None] * (self.gmag * self.gmag)[None], ulp(self.V))

    def errors(self, k, p, m, v):
        """The normalised errors (p / lr, m / |g|, v / g^2) of a kernel's fp32 results after step k and whether each
        element is inside its tolerance: ((err_p, err_m, err_v), ok)."""
        gm = np.where(self.gmag > 0, self.gmag, 1.0)
        d = [np.abs(np.asarray(a, dtype=np.float32).astype(np.float64).reshape(-1) - r[k])
             for a, r in ((p, self.P), (m, self.M), (v, self.V))]
        ok = bool((d[0] <= self.tol_p[k]).all() and (d[1] <= self.tol_m[k]).all() and (d[2] <= self.tol_v[k]).all())
        return (float(d[0].max() / self.lr[k]), float((d[1] / gm).max()), float((d[2] / (gm * gm)).max())), ok


def make_case(numel, hyper_set, t0, steps=STEPS, seed=SEED):
    """The synthetic trajectory of the kernel tests: parameters ~N(0, 0.1^2), make_grads gradients, hyper set "A" or
    "B", zero moments for t0 = 0 and otherwise the moments (and parameters) the reference reaches after WARM steps
    on gradients of the same magnitudes."""
    hyper, scale = SETS[hyper_set]
    rng = np.random.default_rng([seed, numel, 1])
    p0 = (0.1 * rng.standard_normal(numel)).astype(np.float32)
    g = make_grads(numel, steps + WARM, seed)
    m0 = v0 = np.zeros(numel, dtype=np.float32)
    if t0 != 0:
        P, M, V = adam_ref(p0, m0, v0, g[steps:], hyper, 0, scale)
        p0, m0, v0 = (a[-1].astype(np.float32) for a in (P, M, V))
    return Case(p0, m0, v0, g[:steps], hyper, t0, scale)
