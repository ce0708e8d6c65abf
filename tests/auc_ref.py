"""NumPy fp64 oracle for the rank statistics behind losses.auc (average precision and AUROC, one class against the
rest), by the definitions of cvhip/metrics.py, and the seeded inputs the CPU and GPU tests share.

For class k with scores s_j = score[j, k], P positives (y == k) and N = n - P negatives, every positive i gets

    ge_pos_i = #{j positive : s_j >= s_i}     (itself included)
    ge_neg_i = #{j negative : s_j >= s_i}
    gt_neg_i = #{j negative : s_j >  s_i}

    ap_sum = sum_i ge_pos_i / (ge_pos_i + ge_neg_i)            AP    = ap_sum / P
    U2     = sum_i [2 (N - ge_neg_i) + (ge_neg_i - gt_neg_i)]  AUROC = U2 / (2 P N)

The counts come from sorted arrays and binary searches, which is a different route from the kernel's pair loop."""

import numpy as np
import torch


def class_stats(score_k, pos):
    """One class: scores [n] (fp32 or fp64, compared exactly) and the boolean positives mask.  Returns a dict with the
    int64 counts of the positives in sample order, P, N, ap_sum, U2, and AP / AUROC with the degenerate classes as
    sklearn has them (P = 0: AP 0.0; N = 0: AP 1.0; AUROC nan for both)."""
    s = np.asarray(score_k, dtype=np.float64)
    pos = np.asarray(pos, dtype=bool)
    P, N = int(pos.sum()), int((~pos).sum())
    sp, sn = np.sort(s[pos]), np.sort(s[~pos])
    si = s[pos]
    ge_pos = P - np.searchsorted(sp, si, side="left")
    ge_neg = N - np.searchsorted(sn, si, side="left")
    gt_neg = N - np.searchsorted(sn, si, side="right")
    ap_sum = float(np.sum(ge_pos.astype(np.float64) / (ge_pos + ge_neg).astype(np.float64))) if P else 0.0
    u2 = int(np.sum(2 * (N - ge_neg) + (ge_neg - gt_neg)))
    if P == 0:
        ap, auroc = 0.0, float("nan")
    elif N == 0:
        ap, auroc = 1.0, float("nan")
    else:
        ap, auroc = ap_sum / P, float(np.float64(u2) / np.float64(2 * P * N))
    return dict(ge_pos=ge_pos.astype(np.int64), ge_neg=ge_neg.astype(np.int64), gt_neg=gt_neg.astype(np.int64), P=P, N=N,
                ap_sum=ap_sum, u2=u2, ap=ap, auroc=auroc)


def rank_oracle(score, y, c=None):
    """All classes 0..c-1 (c defaults to y.max() + 1) of score [n, >= c]: a dict with counts int64 [n, 3] (each
    sample's counts for its own class), P, ap_sum, u2, ap, auroc as arrays of length c."""
    score, y = np.asarray(score), np.asarray(y).reshape(-1)
    c = int(y.max()) + 1 if c is None else c
    n = len(y)
    counts = np.zeros((n, 3), dtype=np.int64)
    out = dict(P=[], ap_sum=[], u2=[], ap=[], auroc=[])
    for k in range(c):
        pos = y == k
        st = class_stats(score[:, k], pos)
        counts[pos, 0], counts[pos, 1], counts[pos, 2] = st["ge_pos"], st["ge_neg"], st["gt_neg"]
        for key in out:
            out[key].append(st[key])
    res = {key: np.array(v) for key, v in out.items()}
    res["counts"] = counts
    return res


def softmax32(logit):
    """torch's fp32 softmax on the CPU (what the sklearn backend scores)."""
    return torch.as_tensor(logit, dtype=torch.float32).softmax(dim=1).numpy()


def make_logits(n, c, seed, width=None):
    """Seeded fp32 logits [n, width or c] that carry the label (so the metrics are away from 0.5) and labels in
    [0, c) with every class present."""
    g = np.random.default_rng(seed)
    y = g.integers(0, c, n)
    y[:c] = np.arange(c) if n >= c else y[:c]
    w = c if width is None else width
    x = g.standard_normal((n, w))
    x[np.arange(n), y] += 1.5
    return x.astype(np.float32), y.astype(np.int64)


def cases():
    """name -> (logits fp32 [n, c], labels int64 [n]): the shapes at which each mechanism of the kernel can break,
    and the value patterns (ties, saturation, rare and absent classes) at which the statistic can."""
    out = {}
    out["n2_c2"] = (np.array([[0.25, -0.5], [-1.0, 0.75]], dtype=np.float32), np.array([0, 1]))
    x, _ = make_logits(5, 1, 1)
    out["n5_c1"] = (x, np.zeros(5, dtype=np.int64))  # N = 0
    out["n257_c3"] = make_logits(257, 3, 2)  # one thread past a tile
    out["n1025_c2"] = make_logits(1025, 2, 3)  # one sample past an LDS stage
    x, y = make_logits(777, 32, 4)
    y[y == 7] = 8  # class 7 absent
    y[y == 19] = 20
    y[400] = 19  # class 19 has a single positive
    out["n777_c32"] = (x, y)
    _, y = make_logits(512, 4, 5)
    out["n512_c4_tied"] = (np.full((512, 4), 0.375, dtype=np.float32), y)  # every score tied
    x, y = make_logits(600, 10, 6)
    out["n600_c10_saturated"] = ((x * 40).astype(np.float32), y)  # exact 0 and 1 probabilities
    x, y = make_logits(1000, 10, 7)
    out["n1000_c10_halves"] = ((np.round(x * 2) / 2).astype(np.float32), y)  # some ties (ten columns mix)
    x, y = make_logits(500, 2, 9)
    out["n500_c2_halves"] = ((np.round(x * 2) / 2).astype(np.float32), y)  # heavy ties: a few dozen distinct scores
    return out


def rare_case():
    """n = 2000, c = 2 with a 1 % positive class 1."""
    g = np.random.default_rng(8)
    y = (g.random(2000) < 0.01).astype(np.int64)
    y[:2] = [0, 1]
    x = g.standard_normal((2000, 2))
    x[np.arange(2000), y] += 1.0
    return x.astype(np.float32), y


def midpoint_distance(v):
    """Distance of v from the nearest 3-decimal rounding midpoint (x.xxx5)."""
    t = v * 1000.0 - 0.5
    return abs(t - round(t)) / 1000.0
