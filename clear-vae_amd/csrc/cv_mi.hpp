// Shared between cv_mi.hip and cv_nce.hip: the estimator workspace header and the learning step's last launch
// (per-workgroup gradient partials folded in block order, with the estimator's Adam update).
#pragma once
#include "cv_common.hpp"

namespace cv {

// ---------------------------------------------------------------- workspace
constexpr int MI_MAXN = 4096;      // largest batch of the one-workgroup device permutation (bitonic sort in LDS)
constexpr int MI_MAXBIG = 1 << 20;  // largest batch at all (above MI_MAXN: mi_perm_big_kernel)
#ifndef CV_MI_NB
#define CV_MI_NB 64  // (64 row workgroups for the learning step measured +0.2 % on C3 over 32)
#endif
constexpr int MI_NB = CV_MI_NB;            // max row workgroups whose partials are folded
constexpr int MI_FP = 2 + 128;             // per-workgroup forward partial: acc0, acc1, E[64], M[64]
constexpr int MI_GSZ = 4 * 64 * 64 + 256;  // per-workgroup learning-gradient partial (lane-major)
struct MiWork {
  double* sums;       // Sy[64], Sy2[64], E[64], M[64]
  double* fpart;      // [MI_NB][MI_FP]
  double* lpart;      // [MI_NB]
  unsigned* ticket;   // [0] rows arrivals, [1] learn-reduce arrivals (self-resetting)
  float* gpart;       // [MI_NB][MI_GSZ]
  int* perm;
  int* invperm;
};
static inline size_t mi_work_bytes(int n) {
  return 4 * 64 * 8 + MI_NB * MI_FP * 8 + MI_NB * 8 + 64 + (size_t)MI_NB * MI_GSZ * 4 + (size_t)2 * n * 4 + 64;
}
__host__ __device__ inline MiWork mi_work(void* base, int n) {
  MiWork w;
  char* p = (char*)base;
  w.sums = (double*)p;
  p += 4 * 64 * 8;
  w.fpart = (double*)p;
  p += MI_NB * MI_FP * 8;
  w.lpart = (double*)p;
  p += MI_NB * 8;
  w.ticket = (unsigned*)p;
  p += 64;
  w.gpart = (float*)p;
  p += (size_t)MI_NB * MI_GSZ * 4;
  w.perm = (int*)p;
  p += (size_t)n * 4;
  w.invperm = (int*)p;
  return w;
}

// ---------------------------------------------------------------- learning step
struct LearnArgs {
  cv_mlp P;
  const float* x; int ldx;
  const float* y; int ldy;
  int n;
  void* work;
  float* loss_out;
  // Adam (optional): flat arena
  float* params; const float* grads; float* m; float* v; long numel;
  const float* hyper; int64_t* step;
};

// parameter segments of the estimator: canonical element j of segment s is partial word
// poff + (trans ? (j % inner)*64 + j / inner : (j / inner)*64 + j % inner)  (inner == 0: poff + j)
struct LearnSegs {
  float* g[8];
  int len[8], inner[8], poff[8], trans[8];
};

// the learning step's last launch (cv_mi.hip): the nb workgroup partials of `work`'s gpart / lpart folded in block
// order into the segments' gradients and loss_out = -(sum lpart) / a.n, with the Adam update when a.params is set;
// reads a.work, a.n, a.loss_out and the Adam fields of `a` only
int mi_learn_reduce_launch(const LearnArgs& a, const LearnSegs& sg, int nb, int total, hipStream_t st);

}  // namespace cv
