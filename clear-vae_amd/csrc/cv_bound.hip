// The MI-bound study of code/mi_experiment.ipynb on the device: the Gaussian blobs of its cell 3
// (generate_gaussian_blobs) for B trials in one launch, and the SNN / PS-SNN bounds of its cell 2 (which is
// losses.py:98-137 with the cosine similarity) for B trials and T temperatures in one pass over the pairs.
//
// blobs_kernel: one thread per Philox call, i.e. per two consecutive elements in STORAGE order (the larger of the two
// strides is the outer dimension), so a wave writes one contiguous run whichever of [B][n][d] and [n][B][d] the
// caller chose.  The counter is advanced by the last workgroup to finish (style_mnist_kernel's pattern).
//
// snn_bounds_kernel: one workgroup of 256 threads per (trial, tile of 256 rows), one row i per thread.  The trial's
// unit vectors u_j = x_j / max(|x_j|, 1e-8) (ntr_unit's quotients, cv_ntxent.hpp) and its int64 labels stream through
// LDS in tiles of BD_TJ<DM> points (<= 20 KiB for every d class); every lane reads the same LDS address per step (a
// broadcast).  Per pair the similarity s = u_i . u_j is evaluated once and feeds every temperature.  The positives
// (same label, j != i) and the negatives partition j != i, so only those two sets are accumulated, each as
//   running maximum m of the SIMILARITY (one per set: it does not depend on tau) and, per temperature,
//   S_t = sum_j exp((s_j - m) / tau_t)
// with one exp per pair and temperature, e = exp(-|s - m| / tau_t): a new maximum rescales, S_t <- S_t e + 1, anything
// else adds, S_t <- S_t + e.  There is no fixed shift, so a set whose similarities all sit near -1 keeps its row at
// tau = 0.01.  Then, in fp64, lse_set = m / tau + log S (-inf for an empty set), lse_all = logaddexp of the two, and
// the row terms lse_all - lse_pos (SNN) and lse_all - lse_neg (PS-SNN).  A NaN similarity makes both sums of its set
// NaN, hence every row of the trial (each row meets every other row), hence count 0 and a NaN bound for that trial
// and no other.
//
// The mean over the finite rows: a fixed shuffle tree inside the tile gives one fp64 (sum, count) pair per (trial,
// tile, temperature, bound) in `work`, and snn_bounds_mean_kernel adds a trial's pairs in tile order (knn_mi_kernel /
// knn_mi_sum_kernel's scheme, cv_metric.hip).  No atomics; a row's sum runs over j in index order; a (trial, tile)
// never depends on B or on which workgroup ran it, so a trial of a batch has the bits of a B = 1 call on it.
#include <math.h>

#include "cv_common.hpp"

namespace cv {

constexpr int BD_NT = 256;          // threads per workgroup = rows per tile of i
constexpr int BD_MAXT = 8;          // temperatures at most
constexpr int BD_MAXN = 65536;      // rows per trial at most (256 tiles: one per thread of the mean kernel)
constexpr int BD_MAXWG = 1 << 20;   // workgroups per launch at most; the rest is looped over
constexpr int BL_MAXBLOBS = 16;
constexpr uint64_t BL_TAG = 0x626c6f6273ull;

// points per streamed LDS tile for a d class: DM floats + one int64 label each, 16.5 .. 20 KiB
template <int DM>
__host__ __device__ constexpr int bd_tj() {
  return DM <= 8 ? 512 : DM <= 16 ? 256 : DM <= 32 ? 128 : 64;
}

// ---------------------------------------------------------------- blobs
struct BlobArgs {
  float* x;
  const float* stds;
  uint64_t* offset;
  uint64_t seed;
  long long ld_trial, ld_row, total;  // total = B n d elements
  int B, n, d, per;                   // per = n / n_blobs rows per blob
  int trial_outer;                    // 1: storage [B][n][d], 0: storage [n][B][d]
  float centers[BL_MAXBLOBS];
};

__global__ __launch_bounds__(BD_NT) void blobs_kernel(const BlobArgs A) {
  const uint64_t off = A.offset ? A.offset[0] : 0;
  const long long npair = (A.total + 1) / 2;
  for (long long p = (long long)blockIdx.x * BD_NT + threadIdx.x; p < npair; p += (long long)gridDim.x * BD_NT) {
    float e[2];
    normal2(A.seed, off ^ BL_TAG, (uint64_t)p, e[0], e[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long q = 2 * p + h;  // the element's position in storage order
      if (q < A.total) {
        const long long r = q / A.d;
        const int k = (int)(q - r * A.d);
        long long b, i;
        if (A.trial_outer) {
          b = r / A.n;
          i = r - b * A.n;
        } else {
          i = r / A.B;
          b = r - i * A.B;
        }
        A.x[b * A.ld_trial + i * A.ld_row + k] = A.centers[(int)(i / A.per)] + A.stds[b] * e[h];
      }
    }
  }
  if (A.offset) {  // the last workgroup to finish advances the counter
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long prev = atomicAdd((unsigned long long*)(A.offset + 1), 1ull);
      if (prev == (unsigned long long)(gridDim.x - 1)) {
        A.offset[0] = off + 1;
        A.offset[1] = 0;
      }
    }
  }
}

// ---------------------------------------------------------------- bounds
struct BoundArgs {
  const float* x;
  const int64_t* label;
  double* part;  // [B][ntiles][T][2 bounds][sum, count]
  float* rows;   // null or [B][T][3][n]
  long long ld_trial, ld_row, ld_label;
  int B, n, d, T, ntiles;
  float inv_tau[BD_MAXT];
  double inv_tau_d[BD_MAXT];
};

// u <- the unit vector of the d floats at p, zero-padded to DM (reg_norm's sum order, ntr_unit's quotients)
template <int DM>
__device__ __forceinline__ void bd_unit(const float* p, int d, float* u) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    u[k] = k < d ? p[k] : 0.f;
    if (k < d) s += u[k] * u[k];
  }
  const float nr = fmaxf(sqrtf(s), 1e-8f);
#pragma unroll
  for (int k = 0; k < DM; ++k)
    if (k < d) u[k] = u[k] / nr;
}

// lse of a set from its running maximum and its shifted sum; an empty set (the maximum never moved) is -inf
__device__ __forceinline__ double bd_lse(float m, float S, double inv_tau) {
  return m == -__builtin_inff() ? -__builtin_inf() : (double)m * inv_tau + log((double)S);
}

template <int DM, int T>
__global__ __launch_bounds__(BD_NT) void snn_bounds_kernel(const BoundArgs A) {
  constexpr int TJ = bd_tj<DM>();
  __shared__ __attribute__((aligned(16))) float us[TJ * DM];
  __shared__ int64_t ls[TJ];
  __shared__ double red[BD_NT / 64];
  const float ninf = -__builtin_inff();
  const long long total = (long long)A.B * A.ntiles;
  for (long long wg = blockIdx.x; wg < total; wg += gridDim.x) {  // (uniform)
    const int b = (int)(wg / A.ntiles), tile = (int)(wg - (long long)b * A.ntiles);
    const float* xb = A.x + (long long)b * A.ld_trial;
    const int64_t* lb = A.label + (long long)b * A.ld_label;
    const int i = tile * BD_NT + (int)threadIdx.x;
    const bool active = i < A.n;
    float ui[DM];
    int64_t li = 0;
    if (active) {
      bd_unit<DM>(xb + (long long)i * A.ld_row, A.d, ui);
      li = lb[i];
    } else {
#pragma unroll
      for (int k = 0; k < DM; ++k) ui[k] = 0.f;
    }
    float mp = ninf, mn = ninf, P[T], N[T];
#pragma unroll
    for (int t = 0; t < T; ++t) P[t] = N[t] = 0.f;

    for (int j0 = 0; j0 < A.n; j0 += TJ) {
      __syncthreads();
      for (int t = threadIdx.x; t < TJ; t += BD_NT) {
        const int j = j0 + t;
        float u[DM];
        int64_t lab = 0;
        if (j < A.n) {
          bd_unit<DM>(xb + (long long)j * A.ld_row, A.d, u);
          lab = lb[j];
        } else {
#pragma unroll
          for (int k = 0; k < DM; ++k) u[k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < DM; ++k) us[t * DM + k] = u[k];
        ls[t] = lab;
      }
      __syncthreads();
      if (!active) continue;
      const int lim = A.n - j0 < TJ ? A.n - j0 : TJ;  // only staged points that exist are visited
#pragma unroll 4
      for (int t = 0; t < lim; ++t) {
        const float* uj = us + t * DM;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) s = fmaf(ui[k], uj[k], s);
        const bool same = ls[t] == li;
        const bool up = same && (j0 + t != i), un = !same;
        const float m = same ? mp : mn;
        const bool gt = s > m;
        const float dl = -fabsf(s - m);  // -inf against an empty set: e = 0 and the sum becomes 0 * 0 + 1
#pragma unroll
        for (int q = 0; q < T; ++q) {
          const float e = __expf(dl * A.inv_tau[q]);
          const float cur = same ? P[q] : N[q];
          const float nv = gt ? fmaf(cur, e, 1.f) : cur + e;
          P[q] = up ? nv : P[q];
          N[q] = un ? nv : N[q];
        }
        mp = (up && gt) ? s : mp;
        mn = (un && gt) ? s : mn;
      }
    }

    double* part = A.part + (size_t)wg * T * 4;
#pragma unroll
    for (int q = 0; q < T; ++q) {
      double term[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0};
      if (active) {
        const double lp = bd_lse(mp, P[q], A.inv_tau_d[q]), lnn = bd_lse(mn, N[q], A.inv_tau_d[q]);
        double la;
        if (lp == -__builtin_inf()) la = lnn;
        else if (lnn == -__builtin_inf()) la = lp;
        else {
          const double M = lp > lnn ? lp : lnn;
          la = M + log(exp(lp - M) + exp(lnn - M));
        }
        const double v[2] = {la - lp, la - lnn};
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (isfinite(v[c])) {
            term[c] = v[c];
            cnt[c] = 1.0;
          }
        if (A.rows) {
          float* o = A.rows + ((size_t)b * T + q) * 3 * (size_t)A.n + i;
          o[0] = (float)la;
          o[A.n] = (float)lp;
          o[2 * (size_t)A.n] = (float)lnn;
        }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const double ts = block_sum<BD_NT>(term[c], red);
        const double tc = block_sum<BD_NT>(cnt[c], red);
        if (threadIdx.x == 0) {
          part[(q * 2 + c) * 2] = ts;
          part[(q * 2 + c) * 2 + 1] = tc;
        }
      }
    }
  }
}

// bound[b][t][c] = the trial's tile sums added in tile order over its tile counts (NaN over 0, the mean of nothing)
__global__ __launch_bounds__(BD_NT) void snn_bounds_mean_kernel(const BoundArgs A, double* bound, int32_t* count) {
  __shared__ double red[BD_NT / 64];
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
    for (int q = 0; q < 2 * A.T; ++q) {
      double s = 0.0, c = 0.0;
      for (int t = threadIdx.x; t < A.ntiles; t += BD_NT) {
        const double* p = A.part + (((size_t)b * A.ntiles + t) * 2 * A.T + q) * 2;
        s += p[0];
        c += p[1];
      }
      const double ts = block_sum<BD_NT>(s, red);
      const double tc = block_sum<BD_NT>(c, red);
      if (threadIdx.x == 0) {
        bound[(size_t)b * 2 * A.T + q] = tc > 0.0 ? ts / tc : __builtin_nan("");
        count[(size_t)b * 2 * A.T + q] = (int32_t)tc;
      }
    }
  }
}

template <int DM>
static const void* bound_kernel_for(int T) {
  switch (T) {
    case 1: return (const void*)snn_bounds_kernel<DM, 1>;
    case 2: return (const void*)snn_bounds_kernel<DM, 2>;
    case 3: return (const void*)snn_bounds_kernel<DM, 3>;
    case 4: return (const void*)snn_bounds_kernel<DM, 4>;
    case 5: return (const void*)snn_bounds_kernel<DM, 5>;
    case 6: return (const void*)snn_bounds_kernel<DM, 6>;
    case 7: return (const void*)snn_bounds_kernel<DM, 7>;
    default: return (const void*)snn_bounds_kernel<DM, 8>;
  }
}

}  // namespace cv

using namespace cv;

extern "C" int cv_blobs(float* x, long long ld_trial, long long ld_row, int B, int n, int d, const float* centers,
                        int n_blobs, const float* stds, uint64_t seed, uint64_t* offset, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(B >= 1 && n >= 1 && d >= 1, "blobs: need B >= 1, n >= 1, d >= 1 (B=%d n=%d d=%d)", B, n, d);
  CV_REQUIRE(n_blobs >= 1 && n_blobs <= BL_MAXBLOBS, "blobs: n_blobs=%d outside 1..%d", n_blobs, BL_MAXBLOBS);
  CV_REQUIRE(n % n_blobs == 0, "blobs: n=%d is not a multiple of n_blobs=%d", n, n_blobs);
  CV_REQUIRE(x && centers && stds, "blobs: x, centers and stds must be given");
  const bool trial_outer = ld_row >= d && ld_trial >= (long long)n * ld_row;
  const bool row_outer = ld_trial >= d && ld_row >= (long long)B * ld_trial;
  CV_REQUIRE(trial_outer || row_outer,
             "blobs: strides (trial %lld, row %lld) describe neither [B][n][d] nor [n][B][d] storage", ld_trial,
             ld_row);
  BlobArgs A;
  memset(&A, 0, sizeof(A));
  A.x = x;
  A.stds = stds;
  A.offset = offset;
  A.seed = seed;
  A.ld_trial = ld_trial;
  A.ld_row = ld_row;
  A.total = (long long)B * n * d;
  A.B = B;
  A.n = n;
  A.d = d;
  A.per = n / n_blobs;
  A.trial_outer = trial_outer ? 1 : 0;
  for (int c = 0; c < n_blobs; ++c) A.centers[c] = centers[c];
  const long long wgs = ((A.total + 1) / 2 + BD_NT - 1) / BD_NT;
  hipLaunchKernelGGL(blobs_kernel, dim3((unsigned)(wgs < BD_MAXWG ? wgs : BD_MAXWG)), dim3(BD_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("blobs");
  return 0;
}

static bool bound_shape_ok(int B, int n, int T) {
  return B >= 1 && n >= 2 && n <= BD_MAXN && T >= 1 && T <= BD_MAXT && (long long)B * n < (1ll << 31);
}

extern "C" size_t cv_snn_bounds_workspace_bytes(int B, int n, int T) {
  if (!bound_shape_ok(B, n, T)) return 0;
  return (size_t)B * (size_t)cdiv(n, BD_NT) * (size_t)T * 4 * sizeof(double);
}

extern "C" int cv_snn_bounds(const float* x, long long ld_trial, long long ld_row, int B, int n, int d,
                             const int64_t* label, long long ld_label, const float* taus, int T, double* bound,
                             int32_t* count, float* rows, void* work, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(B >= 1, "snn_bounds: B=%d must be positive", B);
  CV_REQUIRE(n >= 2 && n <= BD_MAXN, "snn_bounds: n must be in 2..%d (n=%d)", BD_MAXN, n);
  CV_REQUIRE(d >= 1 && d <= 64, "snn_bounds: d must be in 1..64 (d=%d)", d);
  CV_REQUIRE(T >= 1 && T <= BD_MAXT, "snn_bounds: the number of temperatures must be in 1..%d (T=%d)", BD_MAXT, T);
  CV_REQUIRE((long long)B * n < (1ll << 31), "snn_bounds: B * n must stay below 2^31 (B=%d n=%d)", B, n);
  CV_REQUIRE(x && label && taus && bound && count && work,
             "snn_bounds: x, label, taus, bound, count and work must be given");
  BoundArgs A;
  memset(&A, 0, sizeof(A));
  for (int t = 0; t < T; ++t) {
    CV_REQUIRE(isfinite(taus[t]) && taus[t] > 0.f, "snn_bounds: taus[%d]=%g must be finite and positive", t,
               (double)taus[t]);
    A.inv_tau_d[t] = 1.0 / (double)taus[t];
    A.inv_tau[t] = (float)A.inv_tau_d[t];
  }
  A.x = x;
  A.label = label;
  A.part = static_cast<double*>(work);
  A.rows = rows;
  A.ld_trial = ld_trial;
  A.ld_row = ld_row;
  A.ld_label = ld_label;
  A.B = B;
  A.n = n;
  A.d = d;
  A.T = T;
  A.ntiles = cdiv(n, BD_NT);
  const long long wgs = (long long)B * A.ntiles;
  const void* kern = d <= 8    ? bound_kernel_for<8>(T)
                     : d <= 16 ? bound_kernel_for<16>(T)
                     : d <= 32 ? bound_kernel_for<32>(T)
                               : bound_kernel_for<64>(T);
  void* args[] = {&A};
  hipError_t e = hipLaunchKernel(kern, dim3((unsigned)(wgs < BD_MAXWG ? wgs : BD_MAXWG)), dim3(BD_NT), args, 0,
                                 S(stream));
  if (e != hipSuccess) {
    set_error("snn_bounds.rows: launch failed: %s", hipGetErrorString(e));
    return 2;
  }
  CV_LAUNCH_CHECK("snn_bounds.rows");
  hipLaunchKernelGGL(snn_bounds_mean_kernel, dim3(B < 4096 ? B : 4096), dim3(BD_NT), 0, S(stream), A, bound, count);
  CV_LAUNCH_CHECK("snn_bounds.mean");
  return 0;
}
