/* Host-side validation of cv_eval_batch / cv_eval_workspace_bytes (include/clearvae.h) under AddressSanitizer,
 * without a GPU.
 *
 * Built by `make -C clear-vae_amd/csrc asan` next to abi_asan and abi_asan_rank, against the same host-only,
 * ASan-instrumented build of the library (the kernels are stubs), and run by tests/test_abi_eval.py.  Every call
 * below must be refused on the host with a non-zero status and a cv_last_error() message before anything is
 * enqueued; a call that got as far as a launch would fail differently (there is no device code), which the message
 * checks tell apart. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "clearvae.h"

static int failures = 0;

/* the call is refused, and the message names the function and holds `word` */
#define EXPECT_REFUSED(call, word, what)                                                           \
  do {                                                                                            \
    int rc_ = (call);                                                                             \
    const char* e_ = cv_last_error();                                                             \
    if (rc_ == 0 || !e_ || !strstr(e_, "eval_batch") || !strstr(e_, word) || strstr(e_, "launch")) { \
      fprintf(stderr, "FAIL %s: rc=%d err='%s'\n", what, rc_, e_ ? e_ : "(null)");               \
      ++failures;                                                                                 \
    } else {                                                                                      \
      printf("ok   %-36s -> %s\n", what, e_);                                                     \
    }                                                                                             \
  } while (0)

#define EXPECT(cond, what)                \
  do {                                    \
    if (!(cond)) {                        \
      fprintf(stderr, "FAIL %s\n", what); \
      ++failures;                         \
    } else {                              \
      printf("ok   %s\n", what);          \
    }                                     \
  } while (0)

int main(void) {
  /* fake, never dereferenced device pointers: every call below must fail before any launch */
  float* fp = (float*)(uintptr_t)0x1000;
  int64_t* ip = (int64_t*)(uintptr_t)0x2000;
  double* dp = (double*)(uintptr_t)0x3000;
  cv_stream_t st = NULL;
  cv_bn bn;
  memset(&bn, 0, sizeof bn);
  bn.gamma = fp;
  bn.beta = fp;
  bn.running_mean = fp;
  bn.running_var = fp;
  bn.C = 1;
  bn.count = 1;
  bn.eps = 1e-5f;
  const cv_eval_sink good = {fp, fp, ip, 16, ip, dp};
  cv_eval_sink s = good;
  const float* terms[2] = {fp, fp};
  const float scale[2] = {1.f, -1.f};

  /* ---- workspace sizes: three fp64 partials per workgroup, cdiv(n c hw, 1024) workgroups, at most 1024 */
  EXPECT(cv_eval_workspace_bytes(1, 1, 784) == 1 * 24, "workspace(1, 1, 784)");
  EXPECT(cv_eval_workspace_bytes(2, 1, 784) == 2 * 24, "workspace(2, 1, 784)");
  EXPECT(cv_eval_workspace_bytes(37, 1, 784) == 29 * 24, "workspace(37, 1, 784)");
  EXPECT(cv_eval_workspace_bytes(3, 4, 49) == 1 * 24, "workspace(3, 4, 49)");
  EXPECT(cv_eval_workspace_bytes(16, 3, 4096) == 192 * 24, "workspace(16, 3, 4096)");
  EXPECT(cv_eval_workspace_bytes(128, 3, 4096) == 1024 * 24, "workspace(128, 3, 4096): the grid's cap");
  EXPECT(cv_eval_workspace_bytes(0, 1, 784) == 0, "workspace: n < 1");
  EXPECT(cv_eval_workspace_bytes(-4, 1, 784) == 0, "workspace: n < 0");
  EXPECT(cv_eval_workspace_bytes(4, 0, 784) == 0, "workspace: c < 1");
  EXPECT(cv_eval_workspace_bytes(4, 5, 784) == 0, "workspace: c > 4");
  EXPECT(cv_eval_workspace_bytes(4, 1, 0) == 0, "workspace: hw < 1");
  EXPECT(cv_eval_workspace_bytes(1 << 20, 4, 1 << 10) == 0, "workspace: n c hw > 2^31");

#define CALL(bn_, y_, x_, n_, c_, hw_, h_, z_, d_, l_, t_, ts_, nt_, s_, w_) \
  cv_eval_batch(bn_, y_, x_, n_, c_, hw_, h_, z_, d_, l_, t_, ts_, nt_, s_, w_, st)

  /* ---- null arguments */
  EXPECT_REFUSED(CALL(NULL, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "null bn", "null bn");
  EXPECT_REFUSED(CALL(&bn, NULL, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "null y", "null y");
  EXPECT_REFUSED(CALL(&bn, fp, NULL, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "null x", "null x");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, NULL, fp, 8, ip, terms, scale, 2, &s, dp), "null heads", "null heads");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, NULL, 8, ip, terms, scale, 2, &s, dp), "null z", "null z");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, NULL, terms, scale, 2, &s, dp), "null label", "null label");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, NULL, dp), "null sink", "null sink");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, NULL), "null work", "null work");
  s = good; s.lat_c = NULL;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "lat_c", "null sink lat_c");
  s = good; s.lat_s = NULL;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "lat_s", "null sink lat_s");
  s = good; s.label = NULL;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "sink label", "null sink label");
  s = good; s.cursor = NULL;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "cursor", "null sink cursor");
  s = good; s.totals = NULL;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "totals", "null sink totals");
  s = good;
  {
    const float* t1[2] = {fp, NULL};
    EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, t1, scale, 2, &s, dp), "null term 1", "null terms[1]");
    EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, NULL, scale, 1, &s, dp), "null term 0", "null terms");
    EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, NULL, 1, &s, dp), "null term 0", "null term_scale");
  }

  /* ---- sizes */
  EXPECT_REFUSED(CALL(&bn, fp, fp, 0, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "n=0", "n < 1");
  EXPECT_REFUSED(CALL(&bn, fp, fp, -2, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "n=-2", "n < 0");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 0, ip, terms, scale, 2, &s, dp), "d=0", "d < 1");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 0, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "c=0", "c < 1");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 5, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "c=5", "c > 4");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 0, fp, fp, 8, ip, terms, scale, 2, &s, dp), "hw=0", "hw < 1");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, -1, &s, dp), "nterm=-1", "nterm < 0");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 3, &s, dp), "nterm=3", "nterm > 2");
  s = good; s.cap = -1;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "cap=-1", "cap < 0");
  s = good;
  EXPECT_REFUSED(CALL(&bn, fp, fp, 1 << 20, 4, 1 << 10, fp, fp, 8, ip, terms, scale, 2, &s, dp), "n*c*hw",
                 "n c hw > 2^31");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 3, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "bn has 1 channels",
                 "bn.C != c");
  {
    cv_bn b2 = bn;
    b2.running_var = NULL;
    EXPECT_REFUSED(CALL(&b2, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "running statistics",
                   "eval bn without running_var");
  }

  /* ---- a refusal leaves its own message, not the previous one's */
  EXPECT_REFUSED(CALL(&bn, fp, fp, 0, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, dp), "n=0", "n < 1 again");
  EXPECT_REFUSED(CALL(&bn, fp, fp, 4, 1, 784, fp, fp, 8, ip, terms, scale, 2, &s, NULL), "null work", "null work again");

  if (failures) {
    fprintf(stderr, "%d eval_batch host validation check(s) failed\n", failures);
    return 1;
  }
  printf("all eval_batch host validation checks passed\n");
  return 0;
}
