// Evaluation metrics on the device: the kNN mutual-information estimator behind gMIG (losses.py:10-16, which calls
// sklearn's mutual_info_classif: Ross 2014, continuous feature against a discrete label).
//
// For one feature column x and class ids cls (-1 = the point takes part in nothing), per kept point i:
//   key of a neighbour j     (D_ij, j),  D_ij = |(double)x_j - (double)x_i|, ordered by distance, then index
//   radius neighbour j*      the min(k, cnt_i - 1)-th smallest key among kept j != i of i's class
//   m_i                      1 + #{kept j != i : key_j < key_j*}
// and the launch returns the integers m_i and sum_i psi(m_i).  Everything is a compare of exact fp64 differences of
// fp32 values, so m_i is an exact integer; the only floating-point reduction is the psi sum, which is added in a
// fixed order: a fixed shuffle tree inside a tile of KNN_NT points, one fp64 partial per (feature, tile) in `work`,
// and a second launch that adds a feature's partials in tile order.  No atomics, no cross-workgroup hand-off.
//
// knn_mi_kernel: one thread per point of a tile, workgroups stride over (tile of i) x (feature).  The column and the
// class ids are streamed through LDS in tiles of KNN_TJ points; every lane reads the same LDS address per step (a
// broadcast).  Pass 1 keeps the K smallest same-class keys in registers by insertion; pass 2 re-streams the column
// and counts the keys below the radius key.  A point that is not kept is staged as NaN, whose distance compares
// false everywhere, so the inner loops need no "kept" test.
#include <limits.h>
#include <math.h>

#include "cv_common.hpp"

namespace cv {

constexpr int KNN_NT = 256;        // points per tile of i = threads per workgroup
constexpr int KNN_TJ = 1024;       // points per LDS tile of j
constexpr int KNN_MAXWG = 2048;    // workgroups per launch: one resident round (256 CUs x 8 of 256 threads)
constexpr int KNN_MAXK = 8;
constexpr int KNN_U = 8;  // LDS reads issued together in the inner loops (KNN_TJ is a multiple)

struct KnnArgs {
  const float* x;
  const int32_t* cls;
  const double* psi;
  int32_t* m_out;
  double* part;  // [d][ntiles]
  double* psi_sum;
  int ldx, n, d, ntiles;
};

__device__ __forceinline__ void knn_stage(const KnnArgs& A, int f, int j0, double* xs, int* cs) {
  for (int t = threadIdx.x; t < KNN_TJ; t += KNN_NT) {
    const int j = j0 + t;
    int c = -1;
    double v = __builtin_nan("");
    if (j < A.n) {
      c = A.cls[j];
      if (c >= 0) v = (double)A.x[(size_t)j * (size_t)A.ldx + f];
    }
    xs[t] = v;
    cs[t] = c;
  }
}

// steps of the inner loops over a staged tile with `left` points still to come: whole chunks of KNN_U (the tile is
// padded with points that are not kept, which compare false)
__device__ __forceinline__ int knn_chunks(int left) {
  const int lim = left < KNN_TJ ? left : KNN_TJ;
  return (lim + KNN_U - 1) / KNN_U * KNN_U;
}

template <int K>
__global__ __launch_bounds__(KNN_NT) void knn_mi_kernel(const KnnArgs A) {
  __shared__ double xs[KNN_TJ];
  __shared__ int cs[KNN_TJ];
  __shared__ double red[KNN_NT / 64];
  const double inf = __builtin_inf();
  for (int f = blockIdx.y; f < A.d; f += gridDim.y) {
    for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
      const int i = tile * KNN_NT + (int)threadIdx.x;
      const int ci = i < A.n ? A.cls[i] : -1;
      const bool kept = ci >= 0;
      const double xi = kept ? (double)A.x[(size_t)i * (size_t)A.ldx + f] : 0.0;

      // pass 1: the K smallest (D, j) of i's class, ascending.  j rises through the stream, so a key whose
      // distance ties one already held sorts after it: a strict compare on D alone is the (D, j) order.
      double kd[K];
      int kj[K];
#pragma unroll
      for (int p = 0; p < K; ++p) {
        kd[p] = inf;
        kj[p] = INT_MAX;
      }
      for (int j0 = 0; j0 < A.n; j0 += KNN_TJ) {
        __syncthreads();
        knn_stage(A, f, j0, xs, cs);
        __syncthreads();
        if (!kept) continue;
        const int lim = knn_chunks(A.n - j0);
        for (int t = 0; t < lim; t += KNN_U) {
          double v[KNN_U];
          int c[KNN_U];
#pragma unroll
          for (int u = 0; u < KNN_U; ++u) {
            v[u] = xs[t + u];
            c[u] = cs[t + u];
          }
#pragma unroll
          for (int u = 0; u < KNN_U; ++u) {
            const double D = fabs(v[u] - xi);
            const int j = j0 + t + u;
            if (c[u] == ci && j != i && D < kd[K - 1]) {
#pragma unroll
              for (int p = K - 1; p > 0; --p) {
                if (D < kd[p - 1]) {
                  kd[p] = kd[p - 1];
                  kj[p] = kj[p - 1];
                } else if (D < kd[p]) {
                  kd[p] = D;
                  kj[p] = j;
                }
              }
              if (D < kd[0]) {
                kd[0] = D;
                kj[0] = j;
              }
            }
          }
        }
      }
      // radius key: the last slot that was filled (the class has min(K, cnt_i - 1) other members or more)
      double Ds = -1.0;
      int js = -1;
#pragma unroll
      for (int p = 0; p < K; ++p) {
        if (kj[p] != INT_MAX) {
          Ds = kd[p];
          js = kj[p];
        }
      }

      // pass 2: keys below the radius key among every kept j; the point itself (D = 0) is counted by the loop
      // exactly when (0, i) < (Ds, js), which is taken off again below
      int cnt = 0;
      for (int j0 = 0; j0 < A.n; j0 += KNN_TJ) {
        __syncthreads();
        knn_stage(A, f, j0, xs, cs);
        __syncthreads();
        if (!kept) continue;
        const int lim = knn_chunks(A.n - j0);
        for (int t = 0; t < lim; t += KNN_U) {
          double v[KNN_U];
#pragma unroll
          for (int u = 0; u < KNN_U; ++u) v[u] = xs[t + u];
#pragma unroll
          for (int u = 0; u < KNN_U; ++u) {
            const double D = fabs(v[u] - xi);
            cnt += (D < Ds) | ((D == Ds) & (j0 + t + u < js)) ? 1 : 0;
          }
        }
      }
      int m = 0;
      double ps = 0.0;
      if (kept) {
        const int self = (0.0 < Ds) | ((0.0 == Ds) & (i < js)) ? 1 : 0;
        m = 1 + cnt - self;
        ps = A.psi[m];
      }
      if (A.m_out && i < A.n) A.m_out[(size_t)f * (size_t)A.n + i] = m;
      const double tot = block_sum<KNN_NT>(ps, red);
      if (threadIdx.x == 0) A.part[(size_t)f * (size_t)A.ntiles + tile] = tot;
    }
  }
}

// psi_sum[f] = the feature's tile partials added in tile order (fixed per-thread strides, then a fixed tree)
__global__ __launch_bounds__(KNN_NT) void knn_mi_sum_kernel(const KnnArgs A) {
  __shared__ double red[KNN_NT / 64];
  for (int f = blockIdx.x; f < A.d; f += gridDim.x) {
    double s = 0.0;
    for (int t = threadIdx.x; t < A.ntiles; t += KNN_NT) s += A.part[(size_t)f * (size_t)A.ntiles + t];
    const double tot = block_sum<KNN_NT>(s, red);
    if (threadIdx.x == 0) A.psi_sum[f] = tot;
  }
}

}  // namespace cv

using namespace cv;

extern "C" size_t cv_knn_mi_workspace_bytes(int n, int d) {
  if (n < 1 || d < 1) return 0;
  return (size_t)d * (size_t)cdiv(n, KNN_NT) * sizeof(double);
}

extern "C" int cv_knn_mi(const float* x, int ldx, int n, int d, const int32_t* cls, int k, const double* psi,
                         int32_t* m_out, double* psi_sum_out, void* work, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(n >= 2 && d >= 1, "knn_mi: need n >= 2 points and d >= 1 features (n=%d d=%d)", n, d);
  CV_REQUIRE(ldx >= d, "knn_mi: row stride %d is shorter than the %d features", ldx, d);
  CV_REQUIRE(k >= 1 && k <= KNN_MAXK, "knn_mi: k must be in 1..%d (k=%d)", KNN_MAXK, k);
  CV_REQUIRE(x && cls && psi && psi_sum_out && work, "knn_mi: x, cls, psi, psi_sum_out and work must be given");
  KnnArgs a;
  a.x = x;
  a.cls = cls;
  a.psi = psi;
  a.m_out = m_out;
  a.part = static_cast<double*>(work);
  a.psi_sum = psi_sum_out;
  a.ldx = ldx;
  a.n = n;
  a.d = d;
  a.ntiles = cdiv(n, KNN_NT);
  const int gy = d < KNN_MAXWG ? d : KNN_MAXWG;
  const int room = KNN_MAXWG / gy;
  const int gx = a.ntiles < room ? a.ntiles : room;
  const dim3 grid(gx, gy), block(KNN_NT);
  switch (k) {
    case 1: hipLaunchKernelGGL(knn_mi_kernel<1>, grid, block, 0, S(stream), a); break;
    case 2: hipLaunchKernelGGL(knn_mi_kernel<2>, grid, block, 0, S(stream), a); break;
    case 3: hipLaunchKernelGGL(knn_mi_kernel<3>, grid, block, 0, S(stream), a); break;
    case 4: hipLaunchKernelGGL(knn_mi_kernel<4>, grid, block, 0, S(stream), a); break;
    case 5: hipLaunchKernelGGL(knn_mi_kernel<5>, grid, block, 0, S(stream), a); break;
    case 6: hipLaunchKernelGGL(knn_mi_kernel<6>, grid, block, 0, S(stream), a); break;
    case 7: hipLaunchKernelGGL(knn_mi_kernel<7>, grid, block, 0, S(stream), a); break;
    default: hipLaunchKernelGGL(knn_mi_kernel<8>, grid, block, 0, S(stream), a); break;
  }
  CV_LAUNCH_CHECK("knn_mi.count");
  hipLaunchKernelGGL(knn_mi_sum_kernel, dim3(d < 1024 ? d : 1024), block, 0, S(stream), a);
  CV_LAUNCH_CHECK("knn_mi.sum");
  return 0;
}
