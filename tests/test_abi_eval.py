"""cv_eval_batch at the C-ABI boundary without a GPU: the workspace query and a refusal through the binding, the
cv_eval_sink layout against the header (a gcc probe, as tests/test_abi.py does for the other structs), and every
refusal path of the host validation under AddressSanitizer (tests/abi_asan_eval.c, a stand-alone program run as a child
process)."""

import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clearvae.h")


def test_workspace_query_through_the_binding():
    from cvhip import _lib

    L = _lib.lib()
    assert "cv_eval_batch" in _lib.EXPORTED and "cv_eval_workspace_bytes" in _lib.EXPORTED
    # three fp64 partials per workgroup of the element pass, cdiv(n c hw, 1024) workgroups, at most 1024
    assert L.cv_eval_workspace_bytes(1, 1, 784) == 24
    assert L.cv_eval_workspace_bytes(37, 1, 784) == 29 * 24
    assert L.cv_eval_workspace_bytes(16, 3, 4096) == 192 * 24
    assert L.cv_eval_workspace_bytes(512, 3, 4096) == 1024 * 24
    assert L.cv_eval_workspace_bytes(0, 1, 784) == 0
    assert L.cv_eval_workspace_bytes(4, 5, 784) == 0
    assert L.cv_eval_workspace_bytes(4, 1, 0) == 0


def _fake_call(L, _lib, n=4, c=1, hw=784, d=8, nterm=0, cap=16, work=0x7000, totals=0x6000):
    fake = 0x1000  # never dereferenced: the call is refused on the host
    bn = _lib.cv_bn(fake, fake, None, None, fake, fake, 1, 1, 0, 1e-5, None, None, None)
    sink = _lib.cv_eval_sink(fake, fake, fake, cap, fake, totals)
    terms = (ctypes.c_void_p * 2)(fake, fake)
    scale = (ctypes.c_float * 2)(1.0, -1.0)
    return L.cv_eval_batch(ctypes.byref(bn), fake, fake, n, c, hw, fake, fake, d, fake, terms, scale, nterm,
                           ctypes.byref(sink), work, None)


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), b"n=0"), (dict(d=0), b"d=0"), (dict(c=5), b"c=5"), (dict(c=0), b"c=0"), (dict(hw=0), b"hw=0"),
    (dict(nterm=3), b"nterm=3"), (dict(nterm=-1), b"nterm=-1"), (dict(cap=-1), b"cap=-1"), (dict(work=None), b"null work"),
    (dict(totals=None), b"totals"),
])
def test_refusal_without_launch_through_the_binding(kw, word):
    from cvhip import _lib

    L = _lib.lib()
    assert _fake_call(L, _lib, **kw) != 0
    err = L.cv_last_error()
    assert b"eval_batch" in err and word in err and b"launch" not in err, err


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "clearvae.h"
#define S(T) printf(#T " size %zu\n", sizeof(T));
#define O(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  S(cv_eval_sink) O(cv_eval_sink, lat_c) O(cv_eval_sink, lat_s) O(cv_eval_sink, label) O(cv_eval_sink, cap)
  O(cv_eval_sink, cursor) O(cv_eval_sink, totals)
  return 0;
}
"""


def test_sink_layout_matches_header(tmp_path):
    from cvhip import _lib

    c = tmp_path / "probe.c"
    c.write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        parts = line.split()
        T = getattr(_lib, parts[0])
        if parts[1] == "size":
            assert ctypes.sizeof(T) == int(parts[2]), line
        else:
            assert getattr(T, parts[1]).offset == int(parts[2]), line
        seen += 1
    assert seen == 7


def test_eval_batch_host_validation_under_asan():
    """`make asan` builds abi_asan_eval next to the other two drivers against the host-only sanitised library; the
    driver walks every refusal path of cv_eval_batch and the workspace query.  A failed check or any ASan report
    fails the run."""
    csrc = os.path.join(ROOT, "clear-vae_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "asan", "-j8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "abi_asan_eval")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr
    assert "all eval_batch host validation checks passed" in r.stdout
