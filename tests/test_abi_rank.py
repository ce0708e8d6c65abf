"""cv_rank_auc at the C-ABI boundary without a GPU: the workspace query through the binding, and every refusal path of
the host validation under AddressSanitizer (tests/abi_asan_rank.c, a stand-alone program run as a child process)."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_query_through_the_binding():
    from cvhip import _lib

    L = _lib.lib()
    assert "cv_rank_auc" in _lib.EXPORTED and "cv_rank_auc_workspace_bytes" in _lib.EXPORTED
    # one fp64 and one 64-bit integer partial per workgroup, cdiv(n, 256) + c workgroups
    assert L.cv_rank_auc_workspace_bytes(10000, 10) == (40 + 10) * 16
    assert L.cv_rank_auc_workspace_bytes(34000, 2) == (133 + 2) * 16
    assert L.cv_rank_auc_workspace_bytes(0, 2) == 0
    assert L.cv_rank_auc_workspace_bytes((1 << 22) + 1, 2) == 0
    assert L.cv_rank_auc_workspace_bytes(100, 0) == 0


def test_refusal_without_launch_through_the_binding():
    from cvhip import _lib

    L = _lib.lib()
    fake = 0x1000  # never dereferenced: the call is refused on the host
    rc = L.cv_rank_auc(fake, 4, 100, 5, fake, fake, fake, None, fake, fake, fake, None)
    assert rc != 0
    assert b"rank_auc: row stride 4" in L.cv_last_error()


def test_rank_auc_host_validation_under_asan():
    """`make asan` builds abi_asan_rank next to abi_asan against the host-only sanitised library; the driver walks
    every refusal path of cv_rank_auc.  A failed check or any ASan report fails the run."""
    csrc = os.path.join(ROOT, "clear-vae_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "asan", "-j8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "abi_asan_rank")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr
    assert "all rank_auc host validation checks passed" in r.stdout
