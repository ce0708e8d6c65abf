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
//
// The rank statistics behind losses.py:24-33 (sklearn's average_precision_score and roc_auc_score, one class against
// the rest).  For class k with scores s_j = score[j][k], P positives (label == k) and N = n - P negatives, every
// positive i gets three exact integers
//   ge_pos_i = #{j positive : s_j >= s_i} (itself included),  ge_neg_i = #{j negative : s_j >= s_i},
//   gt_neg_i = #{j negative : s_j > s_i}
// and the launch returns ap_sum_k = sum_i ge_pos_i / (ge_pos_i + ge_neg_i) (fp64 quotients; AP_k = ap_sum_k / P) and
// the integer U2_k = sum_i [2 (N - ge_neg_i) + (ge_neg_i - gt_neg_i)] (AUROC_k = U2_k / (2 P N), ties one half).
//
// rank_auc_kernel: one thread per positive.  The caller passes the samples ordered by label (order, start), so a
// workgroup of RANK_NT threads owns one tile of one class's segment and every lane wants the same column.  The grid
// is sized from n and c alone (cdiv(n, RANK_NT) + c workgroups bound the number of tiles); a workgroup finds its
// (class, tile) by walking `start`, a surplus one leaves.  Column k and the "is negative" flag of all n samples
// stream through LDS RANK_TJ at a time and are read back RANK_U at a time from one address (a broadcast); padding
// is staged as (-inf, negative), which compares false against every finite score.  The only floating-point
// reduction is the AP sum: a fixed shuffle tree per tile, one partial per workgroup in `work`, and
// rank_auc_sum_kernel adds a class's partials in tile order (U2 goes the same way).  No atomics.
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

// ---------------------------------------------------------------- rank statistics (AP / AUROC)
constexpr int RANK_NT = 256;    // positives per tile = threads per workgroup
constexpr int RANK_TJ = 1024;   // samples per LDS stage
constexpr int RANK_U = 8;       // LDS reads issued together (RANK_TJ is a multiple)
constexpr int RANK_MAXN = 1 << 22;

struct RankArgs {
  const float* score;
  const int32_t* label;
  const int32_t* order;
  const int32_t* start;
  uint32_t* counts;              // [n][3] or null
  double* ap_part;               // [nwg]
  unsigned long long* u2_part;   // [nwg]
  double* ap_sum;                // [c]
  unsigned long long* u2;        // [c]
  int lds, n, c, nwg;
};

template <class T>
__device__ __forceinline__ T rank_block_add(T v, T* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[w] = v;
  __syncthreads();
  T r = 0;
#pragma unroll
  for (int i = 0; i < RANK_NT / 64; ++i) r += scratch[i];
  return r;
}

// class k's segment [s0, s1) of `order` (clamped to [0, n]) and its number of tiles
__device__ __forceinline__ int rank_tiles(const RankArgs& A, int k, int& s0, int& s1) {
  s0 = A.start[k];
  s1 = A.start[k + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > A.n ? A.n : s1;
  return s1 > s0 ? (s1 - s0 + RANK_NT - 1) / RANK_NT : 0;
}

__global__ __launch_bounds__(RANK_NT) void rank_auc_kernel(const RankArgs A) {
  __shared__ __attribute__((aligned(16))) float xs[RANK_TJ];
  __shared__ __attribute__((aligned(16))) int ns[RANK_TJ];
  __shared__ double redd[RANK_NT / 64];
  __shared__ unsigned long long redu[RANK_NT / 64];
  // this workgroup's (class, tile): the tiles of class 0, then of class 1, ...
  int k = 0, tile = (int)blockIdx.x, s0 = 0, s1 = 0;
  for (; k < A.c; ++k) {
    const int nt = rank_tiles(A, k, s0, s1);
    if (tile < nt) break;
    tile -= nt;
  }
  if (k == A.c) return;  // surplus workgroup (uniform: before any barrier)
  const int P = s1 - s0, N = A.n - P;
  const int p = s0 + tile * RANK_NT + (int)threadIdx.x;
  int i = p < s1 ? A.order[p] : -1;
  const bool valid = (unsigned)i < (unsigned)A.n;
  // a lane without a positive compares against +inf: nothing is counted, nothing is written
  const float si = valid ? A.score[(size_t)i * (size_t)A.lds + k] : __builtin_inff();

  uint32_t ge_all = 0, ge_neg = 0, gt_neg = 0;
  for (int j0 = 0; j0 < A.n; j0 += RANK_TJ) {
    __syncthreads();
    for (int t = threadIdx.x; t < RANK_TJ; t += RANK_NT) {
      const int j = j0 + t;
      float v = -__builtin_inff();
      int neg = 1;
      if (j < A.n) {
        v = A.score[(size_t)j * (size_t)A.lds + k];
        neg = A.label[j] != k ? 1 : 0;
      }
      xs[t] = v;
      ns[t] = neg;
    }
    __syncthreads();
    const int left = A.n - j0;
    const int lim = ((left < RANK_TJ ? left : RANK_TJ) + RANK_U - 1) / RANK_U * RANK_U;
    for (int t = 0; t < lim; t += RANK_U) {
      float v[RANK_U];
      int g[RANK_U];
#pragma unroll
      for (int u = 0; u < RANK_U; ++u) {
        v[u] = xs[t + u];
        g[u] = ns[t + u];
      }
#pragma unroll
      for (int u = 0; u < RANK_U; ++u) {
        const bool ge = v[u] >= si, gt = v[u] > si;
        ge_all += ge ? 1u : 0u;
        ge_neg += ge ? (uint32_t)g[u] : 0u;
        gt_neg += gt ? (uint32_t)g[u] : 0u;
      }
    }
  }
  double term = 0.0;
  unsigned long long u2 = 0;
  if (valid) {
    const uint32_t ge_pos = ge_all - ge_neg;
    term = (double)ge_pos / (double)ge_all;
    u2 = 2ull * (unsigned long long)((uint32_t)N - ge_neg) + (unsigned long long)(ge_neg - gt_neg);
    if (A.counts) {
      uint32_t* o = A.counts + (size_t)i * 3;
      o[0] = ge_pos;
      o[1] = ge_neg;
      o[2] = gt_neg;
    }
  }
  const double tsum = rank_block_add(term, redd);
  const unsigned long long usum = rank_block_add(u2, redu);
  if (threadIdx.x == 0) {
    A.ap_part[blockIdx.x] = tsum;
    A.u2_part[blockIdx.x] = usum;
  }
}

// ap_sum[k], u2[k] = class k's tile partials added in tile order (fixed per-thread strides, then a fixed tree);
// a class without positives gets 0
__global__ __launch_bounds__(RANK_NT) void rank_auc_sum_kernel(const RankArgs A) {
  __shared__ int redi[RANK_NT / 64];
  __shared__ double redd[RANK_NT / 64];
  __shared__ unsigned long long redu[RANK_NT / 64];
  for (int k = blockIdx.x; k < A.c; k += gridDim.x) {
    int s0, s1, before = 0;
    for (int q = threadIdx.x; q < k; q += RANK_NT) before += rank_tiles(A, q, s0, s1);
    const int first = rank_block_add(before, redi);
    const int nt = rank_tiles(A, k, s0, s1);
    double s = 0.0;
    unsigned long long u = 0;
    for (int t = threadIdx.x; t < nt && first + t < A.nwg; t += RANK_NT) {  // (the bound: a malformed `start`)
      s += A.ap_part[first + t];
      u += A.u2_part[first + t];
    }
    const double tsum = rank_block_add(s, redd);
    const unsigned long long usum = rank_block_add(u, redu);
    if (threadIdx.x == 0) {
      A.ap_sum[k] = tsum;
      A.u2[k] = usum;
    }
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

static long rank_workgroups(int n, int c) { return (long)cdiv(n, RANK_NT) + (long)c; }

extern "C" size_t cv_rank_auc_workspace_bytes(int n, int c) {
  if (n < 1 || n > RANK_MAXN || c < 1 || c > RANK_MAXN) return 0;
  return (size_t)rank_workgroups(n, c) * (sizeof(double) + sizeof(unsigned long long));
}

extern "C" int cv_rank_auc(const float* score, int lds, int n, int c, const int32_t* label, const int32_t* order,
                           const int32_t* start, uint32_t* counts_out, double* ap_sum_out, unsigned long long* u2_out,
                           void* work, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(n >= 1 && n <= RANK_MAXN, "rank_auc: n must be in 1..%d (n=%d)", RANK_MAXN, n);
  CV_REQUIRE(c >= 1 && c <= RANK_MAXN, "rank_auc: c must be in 1..%d (c=%d)", RANK_MAXN, c);
  CV_REQUIRE(lds >= c, "rank_auc: row stride %d is shorter than the %d classes", lds, c);
  CV_REQUIRE(score && label && order && start, "rank_auc: score, label, order and start must be given");
  CV_REQUIRE(ap_sum_out && u2_out, "rank_auc: ap_sum_out and u2_out must be given");
  CV_REQUIRE(work, "rank_auc: work must be given (cv_rank_auc_workspace_bytes)");
  const long nwg = rank_workgroups(n, c);
  RankArgs a;
  a.score = score;
  a.label = label;
  a.order = order;
  a.start = start;
  a.counts = counts_out;
  a.ap_part = static_cast<double*>(work);
  a.u2_part = reinterpret_cast<unsigned long long*>(a.ap_part + nwg);
  a.ap_sum = ap_sum_out;
  a.u2 = u2_out;
  a.lds = lds;
  a.n = n;
  a.c = c;
  a.nwg = (int)nwg;
  const dim3 block(RANK_NT);
  hipLaunchKernelGGL(rank_auc_kernel, dim3((unsigned)nwg), block, 0, S(stream), a);
  CV_LAUNCH_CHECK("rank_auc.count");
  hipLaunchKernelGGL(rank_auc_sum_kernel, dim3(c < 1024 ? c : 1024), block, 0, S(stream), a);
  CV_LAUNCH_CHECK("rank_auc.sum");
  return 0;
}
