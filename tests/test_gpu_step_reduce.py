"""cv_step_reduce (csrc/cv_bn.hip, include/clearvae.h) called directly, one launch per case, against fp64 NumPy.

Deferred weight gradients (cv_wgrad_defer: partial tiles [split][M][ntot], element (m, col = tap*cb + c) added into
gweight[m][c][tap], column N into gbias[m]): cb = 4, kk = 9 (N = 36), ntot = N and N + 1, M = 5 — M*ntot = 180 /
185 is no multiple of the 64-element segment, so each record's last block is partial — and split in {1, 5, 37}: with
four thread groups per element these run the tail loop only, the tail only, and one 8-deep unrolled trip plus the
tail.  Every launch carries two live records around one split = 0 record (skipped: its gradient stays as it is), and
gweight / gbias start from non-zero values (the result is +=).  The kernel sums each element's partials in fp32 in a
fixed order, so against the exact sum the error is at most (split - 1) roundings of partial sums plus the final
add's: split * 2^-24 * sum|partials| + 2^-24 * |result|.

BatchNorm half (not reached by the other direct calls, which pass nbn = 0): one layer of C = 32 (the block-
cooperative bn_fold path) and one of C = 320 (one channel per thread, two blocks, the second partial), train = 1,
forward and backward sums spread over all CV_STAT_REPL(C) fp64 replicas, the cv_bn built by plan.BNView.cv.  dgamma /
dbeta are float32(fp64 sum): within one fp32 ulp (the replica fold order can move the fp64 sum's last bits across a
rounding boundary).  running = 1: running_mean / running_var take m * float(stat) + (1 - m) * old in fp32 — float(),
the product and the sum round term one, (1 - m), the product and the sum round term two: three roundings each — and
num_batches_tracked += 1 once per layer; running = 0 leaves all three buffers alone."""

import ctypes
import functools

import numpy as np
import pytest

U = 2.0 ** -24  # fp32 unit roundoff
CB, KK, M = 4, 9, 5
N = CB * KK
MOMENTUM = 0.1
BN_LAYERS = ((32, 16 * 7 * 7), (320, 16))  # (C, count)
DEFER_CASES = [(ntot, splits) for ntot in (N, N + 1) for splits in ((1, 37), (5, 1), (37, 5))]


def _stat_repl(C):
    from cvhip import _lib

    return _lib.stat_repl(C)


@functools.lru_cache(maxsize=None)
def defer_case(ntot, splits):
    """Inputs, exact result and bound of one launch: records (splits[0], 0, splits[1])."""
    gen = np.random.default_rng(1000 * ntot + 37 * splits[0] + splits[1])
    recs = []
    for split in (splits[0], 0, splits[1]):
        part = gen.standard_normal((split, M, ntot)).astype(np.float32)
        gw0 = gen.standard_normal((M, CB, KK)).astype(np.float32)
        gb0 = gen.standard_normal(M).astype(np.float32)
        p64 = part.astype(np.float64)
        # column tap*cb + c of row m -> gweight[m][c][tap]
        w_sum = p64[:, :, :N].sum(0).reshape(M, KK, CB).transpose(0, 2, 1)
        w_abs = np.abs(p64[:, :, :N]).sum(0).reshape(M, KK, CB).transpose(0, 2, 1)
        gw = gw0.astype(np.float64) + w_sum
        gw_tol = split * U * w_abs + U * np.abs(gw)
        gb, gb_tol = gb0.astype(np.float64), np.zeros(M)
        if ntot > N:
            gb = gb + p64[:, :, N].sum(0)
            gb_tol = split * U * np.abs(p64[:, :, N]).sum(0) + U * np.abs(gb)
        recs.append(dict(split=split, part=part, gw0=gw0, gb0=gb0, gw=gw, gw_tol=gw_tol, gb=gb, gb_tol=gb_tol))
    return recs


@functools.lru_cache(maxsize=None)
def bn_case():
    """Per layer: the replica sums, the old running buffers and the exact fp64 results with their bounds."""
    gen = np.random.default_rng(77)
    out = []
    for C, count in BN_LAYERS:
        R = _stat_repl(C)
        mu, var = gen.standard_normal(C), gen.uniform(0.5, 2.0, C)
        w = gen.uniform(0.5, 1.5, (R, 1, C))
        w /= w.sum(0)
        stat = w * np.stack([count * mu, count * (var + mu * mu)])[None]  # [R][2][C]: sum x, sum x^2
        gstat = gen.standard_normal((R, 2, C)) * np.sqrt(count)  # sum dz, sum dz*xhat
        rm0 = gen.standard_normal(C).astype(np.float32)
        rv0 = gen.uniform(0.5, 2.0, C).astype(np.float32)
        s = stat.astype(np.longdouble).sum(0).astype(np.float64)
        g = gstat.astype(np.longdouble).sum(0).astype(np.float64)
        mean = s[0] / count
        v = np.maximum(s[1] / count - mean * mean, 0.0) * count / (count - 1.0)
        m1 = float(np.float32(MOMENTUM)), float(np.float32(1.0) - np.float32(MOMENTUM))
        rm = m1[0] * mean + m1[1] * rm0.astype(np.float64)
        rv = m1[0] * v + m1[1] * rv0.astype(np.float64)
        three = (1 + U) ** 3 - 1  # three roundings, each (1 + delta), |delta| <= U
        rm_tol = three * (np.abs(m1[0] * mean) + np.abs(m1[1] * rm0))
        rv_tol = three * (np.abs(m1[0] * v) + np.abs(m1[1] * rv0))
        out.append(dict(C=C, count=count, stat=stat, gstat=gstat, rm0=rm0, rv0=rv0, db=g[0], dg=g[1], rm=rm, rv=rv,
                        rm_tol=rm_tol, rv_tol=rv_tol))
    return out


def test_references_are_finite_and_bounds_bind():
    """CPU: the fp64 references are finite, every bound is positive and far below the values it guards (a result
    off in its fifth digit fails), and the BatchNorm counts allow the unbiased variance."""
    for ntot, splits in DEFER_CASES:
        for r in defer_case(ntot, splits):
            for ref, tol, moved in ((r["gw"], r["gw_tol"], r["split"] > 0), (r["gb"], r["gb_tol"], r["split"] > 0
                                                                             and ntot > N)):
                assert np.isfinite(ref).all() and np.isfinite(tol).all()
                if moved:
                    assert (tol > 0).all() and tol.max() < 1e-4 * np.abs(ref).max()
    for L in bn_case():
        assert L["count"] >= 2
        for k in ("db", "dg", "rm", "rv"):
            assert np.isfinite(L[k]).all()
        for k in ("rm", "rv"):
            assert (L[k + "_tol"] > 0).all() and L[k + "_tol"].max() < 1e-5 * np.abs(L[k]).max()
        assert np.abs(np.float32(L["rm"]) - L["rm0"]).min() > 0  # (the update moves every element)


def _records(recs, dev):
    """The cv_wgrad_defer array of a launch and the device tensors behind it."""
    import torch

    from cvhip import _lib

    arr = (_lib.cv_wgrad_defer * len(recs))()
    bufs = []
    for i, r in enumerate(recs):
        part = torch.tensor(r["part"], device=dev) if r["split"] else None
        gw, gb = torch.tensor(r["gw0"], device=dev), torch.tensor(r["gb0"], device=dev)
        ntot = r["part"].shape[2]
        arr[i] = _lib.cv_wgrad_defer(part.data_ptr() if part is not None else None, r["split"], M, N, ntot, CB, KK,
                                     gw.data_ptr(), gb.data_ptr() if ntot > N else None)
        bufs.append((part, gw, gb))
    return arr, bufs


def _check_records(recs, bufs):
    for r, (_, gw, gb) in zip(recs, bufs):
        gw, gb = gw.cpu().numpy(), gb.cpu().numpy()
        if r["split"] == 0:  # skipped: nothing of it is touched
            assert np.array_equal(gw, r["gw0"]) and np.array_equal(gb, r["gb0"])
            continue
        err = np.abs(gw.astype(np.float64) - r["gw"])
        print("split", r["split"], "gweight max err / bound", float((err / r["gw_tol"]).max()))
        assert (err <= r["gw_tol"]).all(), (r["split"], float((err / r["gw_tol"]).max()))
        if r["part"].shape[2] > N:
            err = np.abs(gb.astype(np.float64) - r["gb"])
            assert (err <= r["gb_tol"]).all(), (r["split"], float((err / r["gb_tol"]).max()))
        else:
            assert np.array_equal(gb, r["gb0"])


@pytest.mark.gpu
@pytest.mark.parametrize("ntot,splits", DEFER_CASES)
def test_deferred_weight_gradients(ntot, splits):
    import torch

    from cvhip import _lib

    recs = defer_case(ntot, splits)
    arr, bufs = _records(recs, "cuda")
    _lib.call("cv_step_reduce", arr, len(recs), None, 0, None, None, 0, ctypes.c_float(MOMENTUM), None,
              _lib.stream_handle())
    torch.cuda.synchronize()
    _check_records(recs, bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("running,grads", [(1, True), (0, True), (1, False)])
def test_batchnorm_gradients_and_running_statistics(running, grads):
    """Both layers in one launch behind two deferred records (the BatchNorm blocks follow the records' blocks).
    grads=False: dgamma = dbeta = NULL, the running statistics only."""
    import torch

    from cvhip import _lib
    from cvhip.plan import BNView, ptr_array, struct_array

    layers = bn_case()
    recs = defer_case(N + 1, (5, 1))
    arr, bufs = _records(recs, "cuda")
    views, dgs, dbs, nbts = [], [], [], []
    for L in layers:
        mod = torch.nn.BatchNorm1d(L["C"], momentum=MOMENTUM).cuda()
        with torch.no_grad():
            mod.running_mean.copy_(torch.tensor(L["rm0"]))
            mod.running_var.copy_(torch.tensor(L["rv0"]))
            mod.num_batches_tracked.fill_(7)
        views.append(BNView(mod, torch.tensor(L["stat"], device="cuda"), torch.tensor(L["gstat"], device="cuda"),
                            L["count"]))
        dgs.append(torch.full((L["C"],), -3.0, device="cuda"))  # (written, not accumulated)
        dbs.append(torch.full((L["C"],), -3.0, device="cuda"))
        nbts.append(mod.num_batches_tracked)
    bns = struct_array(_lib.cv_bn, [v.cv(True) for v in views])
    _lib.call("cv_step_reduce", arr, len(recs), bns, len(views),
              ptr_array([t.data_ptr() for t in dgs]) if grads else None,
              ptr_array([t.data_ptr() for t in dbs]) if grads else None, running, ctypes.c_float(MOMENTUM),
              ptr_array([t.data_ptr() for t in nbts]) if running else None, _lib.stream_handle())
    torch.cuda.synchronize()
    _check_records(recs, bufs)
    for L, v, dg, db in zip(layers, views, dgs, dbs):
        dg, db = dg.cpu().numpy(), db.cpu().numpy()
        if grads:
            for got, ref in ((dg, L["dg"]), (db, L["db"])):
                r32 = ref.astype(np.float32)
                assert (np.abs(got.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32))).all()
        else:
            assert (dg == -3.0).all() and (db == -3.0).all()
        rm, rv = v.mod.running_mean.cpu().numpy(), v.mod.running_var.cpu().numpy()
        if running:
            for got, ref, tol in ((rm, L["rm"], L["rm_tol"]), (rv, L["rv"], L["rv_tol"])):
                err = np.abs(got.astype(np.float64) - ref)
                print("C", L["C"], "running max err / bound", float((err / tol).max()))
                assert (err <= tol).all(), (L["C"], float((err / tol).max()))
            assert int(v.mod.num_batches_tracked.item()) == 8
        else:
            assert np.array_equal(rm, L["rm0"]) and np.array_equal(rv, L["rv0"])
            assert int(v.mod.num_batches_tracked.item()) == 7
