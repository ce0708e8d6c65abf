"""bench.py's output dump and its plain / --full split.

CPU: dump_outputs writes one flat float32 / float64 .npy per output, cuts an array above its share of the byte
budget to the same seeded sample on every call, and --kernel-table (a product of the in-step pass) is refused
without --full.  GPU: one plain run of the command line with --dump-outputs keeps the headline keys, times exactly
--steps steps, leaves the --full legs out, and writes finite arrays of the step's losses and parameters."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench  # (the repository root is on sys.path: tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_shapes(tmp_path):
    outs = {"losses": torch.arange(6, dtype=torch.float32) / 7,
            "model.bn.num_batches_tracked": torch.tensor(12345678901, dtype=torch.int64),
            "model.w": torch.arange(24, dtype=torch.float64).reshape(2, 3, 4) / 3,
            "half": torch.arange(4, dtype=torch.bfloat16)}
    bench.dump_outputs(outs, str(tmp_path / "d"))
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == sorted(outs)
    assert got["losses"].dtype == np.float32 and np.array_equal(got["losses"], outs["losses"].numpy())
    assert got["model.bn.num_batches_tracked"].dtype == np.float64
    assert got["model.bn.num_batches_tracked"].tolist() == [12345678901.0]
    assert got["model.w"].dtype == np.float64 and np.array_equal(got["model.w"], outs["model.w"].reshape(-1).numpy())
    assert got["half"].dtype == np.float32 and got["half"].tolist() == [0.0, 1.0, 2.0, 3.0]


def test_dump_outputs_samples_large_arrays_identically(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 400)  # 2 outputs: 400 bytes = 100 float32 each
    g = torch.Generator().manual_seed(3)
    big, small = torch.rand(1000, generator=g), torch.rand(100, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs({"big": big, "small": small}, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and np.array_equal(a, b)
    # a sorted sample without repeats of the array's own elements
    idx = np.sort(np.random.default_rng(0).choice(1000, size=100, replace=False))
    assert len(set(idx.tolist())) == 100 and np.array_equal(a, big.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())  # (within its share: whole)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 400 + 2 * 128  # (data + the two .npy headers)


def test_kernel_table_needs_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--kernel-table", "t.txt", "--dry-run"],
                       capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert p.returncode == 2 and "--full" in p.stderr


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(recs) == 1
    r = recs[0]
    assert r["metric"] == "training images/sec at bs=512; ELBO rel-err vs CPU ref" and r["unit"] == "images/s"
    assert r["higher_is_better"] is True and r["dtype"] == "fp32" and r["steps"] == 3 and r["warmup"] == 2
    assert r["ms_per_step"] > 0 and r["losses_finite"] is True
    # value and ms_per_step describe the same 3 steps of 512 images (each rounded for the line)
    assert r["value"] == pytest.approx(512 / (r["ms_per_step"] * 1e-3), rel=1e-3)
    for key in ("c3", "celeba", "pacs", "camelyon_bf16", "cpu_baseline", "input_pipeline", "elbo_rel_err"):
        assert key not in r, key  # (--full only)
    assert r["roofline"] is None and r["instep_sum_ms"] is None
    names = sorted(f[:-4] for f in os.listdir(d))
    assert "losses" in names and any(n.startswith("model.") and n.endswith(".weight") for n in names)
    size = 0
    for n in names:
        a = np.load(d / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.ndim == 1 and a.size > 0 and np.isfinite(a).all(), n
        size += os.path.getsize(d / (n + ".npy"))
    assert size <= 64 << 20
    assert np.abs(np.load(d / "losses.npy")).max() > 0
