// Exact t-SNE on the device, matrix-free: the computation behind the notebooks' latent plots (demo_clearvae,
// demo_clearmimvae, demo_cleartcvae and expr/visual_utils.py:144-183, which call sklearn's TSNE on host copies of
// mu_c and mu_s).  The algorithm is sklearn's method="exact" (manifold/_t_sne.py and _utils.pyx); memory is O(N D):
// no N x N array of distances, P or Q is ever built, every pair is recomputed from x, beta, logz and y where it is
// needed.  Embedding dimension 2, squared Euclidean distances d_ij, 1 <= D <= 64, 2 <= N <= 65536.
//
// tsne_affinity_kernel: sklearn's _binary_search_perplexity, one thread per row i, workgroups of one wave.  The
// points stream through LDS in tiles of TS_TILE / DP rows (DP = D padded with zero columns to 4, 8, 16, 32 or 64;
// row i's own coordinates sit in registers) and every lane reads the same LDS address per step (a broadcast).  The
// distances are recomputed at every step of the search.  A first sweep finds m_i = min_{j != i} d_ij and every
// exponent is shifted by it, so at least one term of S'_i = sum_{j != i} exp(-beta (d_ij - m_i)) is 1 and a large
// beta d cannot flush the row to zero:
//   H_i = ln S'_i + beta sum_{j != i} (d_ij - m_i) exp(-beta (d_ij - m_i)) / S'_i,   ln S_i = ln S'_i - beta m_i.
// beta, the bracket and the two sums are fp64 (the exponential is fp32); the search is sklearn's: beta = 1, double /
// halve while the bracket is open, else the midpoint, stop at |H - ln perplexity| <= 1e-5 or after 100 evaluations
// (the beta evaluated last is kept, as in sklearn).  The workgroup sweeps until its last row has stopped.  beta is
// then rounded to fp32 and one more sweep evaluates logz = ln S at the rounded value, so the pair (beta, logz) that
// is stored is consistent.
//
// tsne_pair_kernel: one thread per row i of a tile of TS_NT rows, grid = (row tiles) x (slabs of j).  x_j and
// (beta_j, logz_j, y_j) stream through LDS the same way.  Per pair j != i:
//   s_ij = max(exp(-beta_i d - logz_i) + exp(-beta_j d - logz_j), 2N eps),   p_ij = s_ij / 2N  (eps = 2.220446e-16:
//          sklearn's symmetrised, normalised, clamped joint P),   q_ij = 1 / (1 + |y_i - y_j|^2)
// and the sums  A_i = sum e p q (y_i - y_j),  R_i = sum q^2 (y_i - y_j),  z_i = sum q,
// kl_i = sum e p (ln(e p) - ln q),  sp_i = sum e p.  The factor e / 2N is applied once, in fp64, when the partial is
// written.  A thread adds TS_CHUNK pairs in fp32, then adds that into its fp64 accumulators; one fp64 partial per
// (sum, slab, row) goes to the workspace.  The slab length depends on N alone.
//
// tsne_total_kernel + tsne_step_kernel: the slab partials of a row are added in slab order; Z = sum_i z_i, sum kl_i
// and sum sp_i go through a fixed shuffle tree per tile of rows, one partial per tile, and every workgroup of the
// step kernel adds the (at most 256) tile partials through the same tree, so every workgroup holds the same bits.
// KL = sum kl_i + ln Z sum sp_i (sklearn's 2 dot(P, log(P / Q)) with the exaggerated P; Q is not clamped: q_ij / Z
// reaches 2.2e-16 only for embeddings wider than 1e4), grad_i = 4 (A_i - R_i / Z), then sklearn's _gradient_descent
// step in fp32.  No atomics and no order-dependent sum anywhere: the same inputs give the same bits.
#include <math.h>

#include "cv_common.hpp"

namespace cv {

constexpr int TS_TILE = 4096;      // floats of x per LDS tile: TS_TILE / DP points
constexpr int TS_AFF_NT = 64;      // rows per workgroup of the affinity search (one wave)
constexpr int TS_NT = 256;         // rows per tile of the pair / update kernels = threads per workgroup
constexpr int TS_CHUNK = 32;       // pairs added in fp32 before the fp64 accumulators take them (divides every tile)
constexpr int TS_MAXN = 65536;     // at most TS_NT tiles of rows: one tile partial per thread in the step kernel
constexpr int TS_MAXD = 64;
constexpr int TS_TARGET_WG = 1024; // workgroups the pair grid aims at (256 CUs x 4)
constexpr int TS_MIN_SLAB = 64;
constexpr int TS_NSUM = 7;         // A0 A1 R0 R1 z kl sp
constexpr int TS_STEPS = 100;      // sklearn's n_steps
constexpr double TS_PTOL = 1e-5;   // sklearn's PERPLEXITY_TOLERANCE
constexpr double TS_EPS = 2.220446049250313e-16;  // sklearn's MACHINE_EPSILON

struct TsneGeom {
  int rowtiles, slab_len, nslab;
};

// the split of the j range: a function of n alone, so that cv_tsne_pair and cv_tsne_update agree without d
static TsneGeom tsne_geom(int n) {
  TsneGeom g;
  g.rowtiles = cdiv(n, TS_NT);
  const int target = cdiv(TS_TARGET_WG, g.rowtiles);
  int len = cdiv(cdiv(n, target), TS_CHUNK) * TS_CHUNK;
  if (len < TS_MIN_SLAB) len = TS_MIN_SLAB;
  g.slab_len = len;
  g.nslab = cdiv(n, len);
  return g;
}

static int tsne_dp(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }

// squared distance between the row in registers and a staged row (both padded with zero columns)
template <int DP>
__device__ __forceinline__ float tsne_dist(const float (&xi)[DP], const float* xr) {
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
    const float a0 = xi[c] - v[0], a1 = xi[c + 1] - v[1], a2 = xi[c + 2] - v[2], a3 = xi[c + 3] - v[3];
    d = fmaf(a0, a0, d);
    d = fmaf(a1, a1, d);
    d = fmaf(a2, a2, d);
    d = fmaf(a3, a3, d);
  }
  return d;
}

// points j0 .. j0 + cnt - 1 into xs as rows of DP floats; rows cnt .. cntp - 1 and columns d .. DP - 1 are zero
template <int DP, int NT>
__device__ __forceinline__ void tsne_stage_x(const float* x, int ldx, int d, int j0, int cnt, int cntp, float* xs) {
  for (int e = threadIdx.x; e < cntp * DP; e += NT) {
    const int t = e / DP, c = e % DP;
    xs[e] = (t < cnt && c < d) ? x[(size_t)(j0 + t) * (size_t)ldx + c] : 0.f;
  }
}

template <int DP>
__device__ __forceinline__ void tsne_load_row(const float* x, int ldx, int d, int i, bool live, float (&xi)[DP]) {
#pragma unroll
  for (int c = 0; c < DP; ++c) xi[c] = (live && c < d) ? x[(size_t)i * (size_t)ldx + c] : 0.f;
}

// ---------------------------------------------------------------- affinities
struct TsneAffArgs {
  const float* x;
  float* beta;
  float* logz;
  double target;  // ln(perplexity)
  int ldx, n, d;
};

template <int DP>
__global__ __launch_bounds__(TS_AFF_NT) void tsne_affinity_kernel(const TsneAffArgs A) {
  constexpr int TJ = TS_TILE / DP;
  __shared__ __attribute__((aligned(16))) float xs[TS_TILE];
  const int i = blockIdx.x * TS_AFF_NT + (int)threadIdx.x;
  const bool live = i < A.n;
  float xi[DP];
  tsne_load_row<DP>(A.x, A.ldx, A.d, i, live, xi);

  // one pass over every point: body(j, d_ij), the row itself included
  auto sweep = [&](auto&& body) {
    for (int j0 = 0; j0 < A.n; j0 += TJ) {
      const int left = A.n - j0, cnt = left < TJ ? left : TJ;
      __syncthreads();
      tsne_stage_x<DP, TS_AFF_NT>(A.x, A.ldx, A.d, j0, cnt, cnt, xs);
      __syncthreads();
#pragma unroll 4
      for (int t = 0; t < cnt; ++t) body(j0 + t, tsne_dist<DP>(xi, xs + t * DP));
    }
  };

  float dmin = __builtin_inff();
  sweep([&](int j, float d) {
    if (j != i) dmin = fminf(dmin, d);
  });

  const double inf = __builtin_inf();
  double beta = 1.0, lo = -inf, hi = inf;
  bool open = live;
  for (int step = 0; step < TS_STEPS; ++step) {
    if (!__syncthreads_or(open ? 1 : 0)) break;  // uniform: every row of the workgroup has stopped
    const double nb = -beta;
    double S = 0.0, T = 0.0;
    sweep([&](int j, float d) {
      const float r = d - dmin;
      const float e = j != i ? expf((float)(nb * (double)r)) : 0.f;
      S += (double)e;
      T += (double)(r * e);
    });
    if (open) {
      const double diff = log(S) + beta * T / S - A.target;
      if (fabs(diff) <= TS_PTOL || step + 1 == TS_STEPS) {
        open = false;
      } else if (diff > 0.0) {
        lo = beta;
        beta = hi == inf ? beta * 2.0 : 0.5 * (beta + hi);
      } else {
        hi = beta;
        beta = lo == -inf ? beta * 0.5 : 0.5 * (beta + lo);
      }
    }
  }

  const float bf = (float)beta;
  const double nb = -(double)bf;
  double S = 0.0;
  sweep([&](int j, float d) {
    const float e = j != i ? expf((float)(nb * (double)(d - dmin))) : 0.f;
    S += (double)e;
  });
  if (live) {
    A.beta[i] = bf;
    A.logz[i] = (float)(log(S) + nb * (double)dmin);
  }
}

// ---------------------------------------------------------------- pair sums
struct TsnePairArgs {
  const float *x, *beta, *logz, *y;
  double* part;  // [TS_NSUM][nslab][n]
  double scale;  // exaggeration / 2N
  float clamp;   // 2N eps
  int ldx, n, d, slab_len, nslab;
};

template <int DP, bool KL>
__global__ __launch_bounds__(TS_NT) void tsne_pair_kernel(const TsnePairArgs A) {
  constexpr int TJ = TS_TILE / DP;
  __shared__ __attribute__((aligned(16))) float xs[TS_TILE];
  __shared__ __attribute__((aligned(16))) f32x4 aux[TJ];  // beta_j, logz_j, y_j
  const int i = blockIdx.x * TS_NT + (int)threadIdx.x;
  const bool live = i < A.n;
  float xi[DP];
  tsne_load_row<DP>(A.x, A.ldx, A.d, i, live, xi);
  const float nbi = live ? -A.beta[i] : 0.f, nli = live ? -A.logz[i] : 0.f;
  const float yi0 = live ? A.y[2 * (size_t)i] : 0.f, yi1 = live ? A.y[2 * (size_t)i + 1] : 0.f;
  const int jb = (int)blockIdx.y * A.slab_len;
  const int je = jb + A.slab_len < A.n ? jb + A.slab_len : A.n;

  double acc[TS_NSUM];
#pragma unroll
  for (int k = 0; k < TS_NSUM; ++k) acc[k] = 0.0;

  for (int j0 = jb; j0 < je; j0 += TJ) {
    const int left = je - j0, cnt = left < TJ ? left : TJ;
    const int cntp = (cnt + TS_CHUNK - 1) / TS_CHUNK * TS_CHUNK;  // <= TJ: TS_CHUNK divides TJ
    __syncthreads();
    tsne_stage_x<DP, TS_NT>(A.x, A.ldx, A.d, j0, cnt, cntp, xs);
    for (int t = threadIdx.x; t < cntp; t += TS_NT) {
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (t < cnt) {
        const size_t j = (size_t)(j0 + t);
        g[0] = A.beta[j];
        g[1] = A.logz[j];
        g[2] = A.y[2 * j];
        g[3] = A.y[2 * j + 1];
      }
      aux[t] = g;
    }
    __syncthreads();
    for (int t0 = 0; t0 < cntp; t0 += TS_CHUNK) {
      float a0 = 0.f, a1 = 0.f, r0 = 0.f, r1 = 0.f, z = 0.f, kl = 0.f, sp = 0.f;
#pragma unroll 4
      for (int u = 0; u < TS_CHUNK; ++u) {
        const int t = t0 + u;
        // a padded slot and the row itself add nothing (selects, not products: exp(-logz_i) may be infinite)
        const bool ok = (t < cnt) & (j0 + t != i);
        const float d = tsne_dist<DP>(xi, xs + t * DP);
        const f32x4 g = aux[t];
        const float cij = expf(fmaf(nbi, d, nli)), cji = expf(fmaf(-g[0], d, -g[1]));
        const float dy0 = yi0 - g[2], dy1 = yi1 - g[3];
        const float den = 1.f + fmaf(dy0, dy0, dy1 * dy1);
        const float s = ok ? fmaxf(cij + cji, A.clamp) : 0.f;
        const float q = ok ? 1.f / den : 0.f;
        const float w = s * q, q2 = q * q;
        a0 = fmaf(w, dy0, a0);
        a1 = fmaf(w, dy1, a1);
        r0 = fmaf(q2, dy0, r0);
        r1 = fmaf(q2, dy1, r1);
        z += q;
        if (KL) {
          kl += ok ? s * (logf(s) + logf(den)) : 0.f;
          sp += s;
        }
      }
      acc[0] += (double)a0;
      acc[1] += (double)a1;
      acc[2] += (double)r0;
      acc[3] += (double)r1;
      acc[4] += (double)z;
      acc[5] += (double)kl;
      acc[6] += (double)sp;
    }
  }
  if (!live) return;
  // e p = s * scale: sum e p (ln(e p) - ln q) = scale (sum s (ln s - ln q) + ln(scale) sum s)
  const double out[TS_NSUM] = {A.scale * acc[0], A.scale * acc[1], acc[2], acc[3], acc[4],
                               KL ? A.scale * (acc[5] + log(A.scale) * acc[6]) : 0.0, KL ? A.scale * acc[6] : 0.0};
#pragma unroll
  for (int k = 0; k < TS_NSUM; ++k)
    A.part[((size_t)k * (size_t)A.nslab + blockIdx.y) * (size_t)A.n + (size_t)i] = out[k];
}

// ---------------------------------------------------------------- totals and the descent step
struct TsneUpdArgs {
  const double* part;  // [TS_NSUM][nslab][n]
  double* tile;        // [ntile][3]: z, kl, sp of a tile of rows
  float *y, *upd, *gains;  // [n][2], or y null: no step
  float* grad;         // [n][2] or null
  double* kl;          // one value or null
  float momentum, lr;
  int n, nslab, ntile, reset;
};

__device__ __forceinline__ double tsne_slab_sum(const TsneUpdArgs& A, int k, int i) {
  const double* p = A.part + (size_t)k * (size_t)A.nslab * (size_t)A.n + (size_t)i;
  double s = 0.0;
  for (int b = 0; b < A.nslab; ++b) s += p[(size_t)b * (size_t)A.n];
  return s;
}

__global__ __launch_bounds__(TS_NT) void tsne_total_kernel(const TsneUpdArgs A) {
  __shared__ double red[TS_NT / 64];
  const int i = blockIdx.x * TS_NT + (int)threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (i < A.n) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = tsne_slab_sum(A, 4 + k, i);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double tot = block_sum<TS_NT>(v[k], red);
    if (threadIdx.x == 0) A.tile[(size_t)blockIdx.x * 3 + k] = tot;
  }
}

__global__ __launch_bounds__(TS_NT) void tsne_step_kernel(const TsneUpdArgs A) {
  __shared__ double red[TS_NT / 64];
  double tot[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = (int)threadIdx.x < A.ntile ? A.tile[(size_t)threadIdx.x * 3 + k] : 0.0;  // ntile <= TS_NT
    tot[k] = block_sum<TS_NT>(v, red);
  }
  const double Z = tot[0];
  if (A.kl && blockIdx.x == 0 && threadIdx.x == 0) *A.kl = tot[1] + log(Z) * tot[2];
  const int i = blockIdx.x * TS_NT + (int)threadIdx.x;
  if (i >= A.n) return;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double a = tsne_slab_sum(A, c, i), r = tsne_slab_sum(A, 2 + c, i);
    const float g = (float)(4.0 * (a - r / Z));
    const size_t o = 2 * (size_t)i + c;
    if (A.grad) A.grad[o] = g;
    if (A.y) {
      const float u = A.reset ? 0.f : A.upd[o];
      float gn = A.reset ? 1.f : A.gains[o];
      gn = u * g < 0.f ? gn + 0.2f : gn * 0.8f;
      gn = fmaxf(gn, 0.01f);
      const float un = A.momentum * u - A.lr * (g * gn);
      A.gains[o] = gn;
      A.upd[o] = un;
      A.y[o] += un;
    }
  }
}

static int tsne_check_shape(const char* who, int ldx, int n, int d) {
  CV_REQUIRE(n >= 2 && n <= TS_MAXN, "%s: n must be in 2..%d (n=%d)", who, TS_MAXN, n);
  CV_REQUIRE(d >= 1 && d <= TS_MAXD, "%s: d must be in 1..%d (d=%d)", who, TS_MAXD, d);
  CV_REQUIRE(ldx >= d, "%s: row stride %d is shorter than the %d features", who, ldx, d);
  return 0;
}

template <int DP>
static void tsne_launch_pair(const TsnePairArgs& a, const TsneGeom& g, bool kl, hipStream_t st) {
  const dim3 grid(g.rowtiles, g.nslab), block(TS_NT);
  if (kl) hipLaunchKernelGGL((tsne_pair_kernel<DP, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((tsne_pair_kernel<DP, false>), grid, block, 0, st, a);
}

}  // namespace cv

using namespace cv;

extern "C" size_t cv_tsne_workspace_bytes(int n) {
  if (n < 2 || n > TS_MAXN) return 0;
  const TsneGeom g = tsne_geom(n);
  return ((size_t)TS_NSUM * (size_t)g.nslab * (size_t)n + (size_t)g.rowtiles * 3) * sizeof(double);
}

extern "C" int cv_tsne_affinity(const float* x, int ldx, int n, int d, double perplexity, float* beta_out,
                                float* logz_out, cv_stream_t stream) {
  clear_error();
  if (tsne_check_shape("tsne_affinity", ldx, n, d)) return 1;
  CV_REQUIRE(perplexity > 0.0 && perplexity < (double)n, "tsne_affinity: perplexity must be in (0, n) (%g, n=%d)",
             perplexity, n);
  CV_REQUIRE(x && beta_out && logz_out, "tsne_affinity: x, beta_out and logz_out must be given");
  TsneAffArgs a;
  a.x = x;
  a.beta = beta_out;
  a.logz = logz_out;
  a.target = log(perplexity);
  a.ldx = ldx;
  a.n = n;
  a.d = d;
  const dim3 grid(cdiv(n, TS_AFF_NT)), block(TS_AFF_NT);
  switch (tsne_dp(d)) {
    case 4: hipLaunchKernelGGL(tsne_affinity_kernel<4>, grid, block, 0, S(stream), a); break;
    case 8: hipLaunchKernelGGL(tsne_affinity_kernel<8>, grid, block, 0, S(stream), a); break;
    case 16: hipLaunchKernelGGL(tsne_affinity_kernel<16>, grid, block, 0, S(stream), a); break;
    case 32: hipLaunchKernelGGL(tsne_affinity_kernel<32>, grid, block, 0, S(stream), a); break;
    default: hipLaunchKernelGGL(tsne_affinity_kernel<64>, grid, block, 0, S(stream), a); break;
  }
  CV_LAUNCH_CHECK("tsne_affinity");
  return 0;
}

extern "C" int cv_tsne_pair(const float* x, int ldx, int n, int d, const float* beta, const float* logz,
                            const float* y, float exaggeration, int with_kl, void* work, cv_stream_t stream) {
  clear_error();
  if (tsne_check_shape("tsne_pair", ldx, n, d)) return 1;
  CV_REQUIRE(exaggeration > 0.f, "tsne_pair: the exaggeration must be positive (%g)", (double)exaggeration);
  CV_REQUIRE(x && beta && logz && y && work, "tsne_pair: x, beta, logz, y and work must be given");
  const TsneGeom g = tsne_geom(n);
  TsnePairArgs a;
  a.x = x;
  a.beta = beta;
  a.logz = logz;
  a.y = y;
  a.part = static_cast<double*>(work);
  a.scale = (double)exaggeration / (2.0 * (double)n);
  a.clamp = (float)(2.0 * (double)n * TS_EPS);
  a.ldx = ldx;
  a.n = n;
  a.d = d;
  a.slab_len = g.slab_len;
  a.nslab = g.nslab;
  switch (tsne_dp(d)) {
    case 4: tsne_launch_pair<4>(a, g, with_kl != 0, S(stream)); break;
    case 8: tsne_launch_pair<8>(a, g, with_kl != 0, S(stream)); break;
    case 16: tsne_launch_pair<16>(a, g, with_kl != 0, S(stream)); break;
    case 32: tsne_launch_pair<32>(a, g, with_kl != 0, S(stream)); break;
    default: tsne_launch_pair<64>(a, g, with_kl != 0, S(stream)); break;
  }
  CV_LAUNCH_CHECK("tsne_pair");
  return 0;
}

extern "C" int cv_tsne_update(int n, void* work, float* y, float* update, float* gains, float momentum,
                              float learning_rate, int reset, float* grad_out, double* kl_out, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(n >= 2 && n <= TS_MAXN, "tsne_update: n must be in 2..%d (n=%d)", TS_MAXN, n);
  CV_REQUIRE(work, "tsne_update: work must be given (the partials cv_tsne_pair wrote)");
  CV_REQUIRE(!y || (update && gains), "tsne_update: a step needs update and gains");
  CV_REQUIRE(y || grad_out || kl_out, "tsne_update: nothing to do (y, grad_out and kl_out are all null)");
  const TsneGeom g = tsne_geom(n);
  TsneUpdArgs a;
  a.part = static_cast<const double*>(work);
  a.tile = static_cast<double*>(work) + (size_t)TS_NSUM * (size_t)g.nslab * (size_t)n;
  a.y = y;
  a.upd = update;
  a.gains = gains;
  a.grad = grad_out;
  a.kl = kl_out;
  a.momentum = momentum;
  a.lr = learning_rate;
  a.n = n;
  a.nslab = g.nslab;
  a.ntile = g.rowtiles;
  a.reset = reset;
  const dim3 grid(g.rowtiles), block(TS_NT);
  hipLaunchKernelGGL(tsne_total_kernel, grid, block, 0, S(stream), a);
  CV_LAUNCH_CHECK("tsne_update.total");
  hipLaunchKernelGGL(tsne_step_kernel, grid, block, 0, S(stream), a);
  CV_LAUNCH_CHECK("tsne_update.step");
  return 0;
}

extern "C" int cv_tsne_run(const float* x, int ldx, int n, int d, const float* beta, const float* logz, float* y,
                           float* update, float* gains, int n_iter, int exploration_iter, float early_exaggeration,
                           float learning_rate, void* work, double* kl_out, cv_stream_t stream) {
  clear_error();
  if (tsne_check_shape("tsne_run", ldx, n, d)) return 1;
  CV_REQUIRE(n_iter >= 0 && exploration_iter >= 0, "tsne_run: n_iter and exploration_iter must not be negative");
  CV_REQUIRE(early_exaggeration > 0.f, "tsne_run: early_exaggeration must be positive");
  CV_REQUIRE(x && beta && logz && y && update && gains && work,
             "tsne_run: x, beta, logz, y, update, gains and work must be given");
  for (int it = 0; it < n_iter; ++it) {
    const bool early = it < exploration_iter;
    int rc = cv_tsne_pair(x, ldx, n, d, beta, logz, y, early ? early_exaggeration : 1.f, 0, work, stream);
    if (rc) return rc;
    // sklearn runs two _gradient_descent calls: update and gains start afresh at the switch
    rc = cv_tsne_update(n, work, y, update, gains, early ? 0.5f : 0.8f, learning_rate,
                        it == 0 || it == exploration_iter, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  if (kl_out) {
    int rc = cv_tsne_pair(x, ldx, n, d, beta, logz, y, 1.f, 1, work, stream);
    if (rc) return rc;
    rc = cv_tsne_update(n, work, nullptr, nullptr, nullptr, 0.f, 0.f, 0, nullptr, kl_out, stream);
    if (rc) return rc;
  }
  return 0;
}
