/* Host-side validation of cv_rank_auc / cv_rank_auc_workspace_bytes (include/clearvae.h) under AddressSanitizer,
 * without a GPU.
 *
 * Built by `make -C clear-vae_amd/csrc asan` next to abi_asan, against the same host-only, ASan-instrumented build
 * of the library (the kernels are stubs), and run by tests/test_abi_rank.py.  Every call below must be refused on
 * the host with a non-zero status and a cv_last_error() message before anything is enqueued; a call that got as far
 * as a launch would fail differently (there is no device code), which the message checks tell apart. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "clearvae.h"

static int failures = 0;

/* the call is refused, and the message names the function and holds `word` */
#define EXPECT_REFUSED(call, word, what)                                                         \
  do {                                                                                          \
    int rc_ = (call);                                                                           \
    const char* e_ = cv_last_error();                                                           \
    if (rc_ == 0 || !e_ || !strstr(e_, "rank_auc") || !strstr(e_, word) || strstr(e_, "launch")) { \
      fprintf(stderr, "FAIL %s: rc=%d err='%s'\n", what, rc_, e_ ? e_ : "(null)");             \
      ++failures;                                                                               \
    } else {                                                                                    \
      printf("ok   %-36s -> %s\n", what, e_);                                                   \
    }                                                                                           \
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
  float* sc = (float*)(uintptr_t)0x1000;
  int32_t* ip = (int32_t*)(uintptr_t)0x2000;
  uint32_t* cnt = (uint32_t*)(uintptr_t)0x3000;
  double* ap = (double*)(uintptr_t)0x4000;
  unsigned long long* u2 = (unsigned long long*)(uintptr_t)0x5000;
  void* work = (void*)(uintptr_t)0x6000;
  cv_stream_t st = NULL;
  const int big = (1 << 22) + 1;

  /* ---- workspace sizes: one fp64 and one 64-bit integer partial per workgroup, cdiv(n, 256) + c of them */
  EXPECT(cv_rank_auc_workspace_bytes(1, 1) == 2 * 16, "workspace(1, 1)");
  EXPECT(cv_rank_auc_workspace_bytes(256, 3) == 4 * 16, "workspace(256, 3)");
  EXPECT(cv_rank_auc_workspace_bytes(257, 3) == 5 * 16, "workspace(257, 3)");
  EXPECT(cv_rank_auc_workspace_bytes(10000, 10) == 50 * 16, "workspace(10000, 10)");
  EXPECT(cv_rank_auc_workspace_bytes(1 << 22, 2) == (size_t)(16384 + 2) * 16, "workspace(2^22, 2)");
  EXPECT(cv_rank_auc_workspace_bytes(0, 2) == 0, "workspace: n < 1");
  EXPECT(cv_rank_auc_workspace_bytes(-5, 2) == 0, "workspace: n < 0");
  EXPECT(cv_rank_auc_workspace_bytes(big, 2) == 0, "workspace: n > 2^22");
  EXPECT(cv_rank_auc_workspace_bytes(100, 0) == 0, "workspace: c < 1");
  EXPECT(cv_rank_auc_workspace_bytes(100, -1) == 0, "workspace: c < 0");

  /* ---- null arguments (counts_out alone may be NULL) */
  EXPECT_REFUSED(cv_rank_auc(NULL, 10, 100, 10, ip, ip, ip, cnt, ap, u2, work, st), "score", "null score");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, NULL, ip, ip, cnt, ap, u2, work, st), "label", "null label");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, NULL, ip, cnt, ap, u2, work, st), "order", "null order");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, NULL, cnt, ap, u2, work, st), "start", "null start");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, ip, cnt, NULL, u2, work, st), "ap_sum_out", "null ap_sum_out");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, ip, cnt, ap, NULL, work, st), "u2_out", "null u2_out");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, ip, NULL, NULL, NULL, work, st), "ap_sum_out",
                 "null outputs");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, ip, cnt, ap, u2, NULL, st), "work", "null work");

  /* ---- sizes */
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 0, 10, ip, ip, ip, cnt, ap, u2, work, st), "n=0", "n < 1");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, -3, 10, ip, ip, ip, cnt, ap, u2, work, st), "n=-3", "n < 0");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, big, 10, ip, ip, ip, cnt, ap, u2, work, st), "n=4194305", "n > 2^22");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 0, ip, ip, ip, cnt, ap, u2, work, st), "c=0", "c < 1");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, -2, ip, ip, ip, cnt, ap, u2, work, st), "c=-2", "c < 0");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, big, ip, ip, ip, cnt, ap, u2, work, st), "c=4194305", "c > 2^22");
  EXPECT_REFUSED(cv_rank_auc(sc, 9, 100, 10, ip, ip, ip, cnt, ap, u2, work, st), "stride 9", "lds < c");
  EXPECT_REFUSED(cv_rank_auc(sc, 0, 100, 1, ip, ip, ip, cnt, ap, u2, work, st), "stride 0", "lds = 0");

  /* ---- a refusal leaves its own message, not the previous one's */
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 0, 10, ip, ip, ip, cnt, ap, u2, work, st), "n=0", "n < 1 again");
  EXPECT_REFUSED(cv_rank_auc(sc, 10, 100, 10, ip, ip, ip, cnt, ap, u2, NULL, st), "work", "null work again");

  if (failures) {
    fprintf(stderr, "%d rank_auc host validation check(s) failed\n", failures);
    return 1;
  }
  printf("all rank_auc host validation checks passed\n");
  return 0;
}
