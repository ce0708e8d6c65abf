// The tail of one evaluation batch (include/clearvae.h, cv_eval_batch): the reconstruction term from the last
// ConvTranspose2d's pre-BN output without writing xhat, the two KL terms from the heads, the batch's latents and
// labels appended to the epoch's device buffers, and the epoch's fp64 totals advanced — two launches on the stream,
// nothing read back by the host.
//
// Deterministic: every thread visits a fixed set of elements (the grid depends on the shape only), every workgroup
// writes its three fp64 partials into its own slots of `work`, and the second launch (one workgroup) adds the slots in
// a fixed order.  No atomics, no arrival ticket, no grid-wide wait: the launch boundary orders the two passes.
#include "cv_common.hpp"

#include <limits.h>

using namespace cv;

namespace {

constexpr int EV_MAXC = 4;     // OUT_MAXC of cv_bn.hip: the output BatchNorm's channels
constexpr int EV_NT = 256;     // threads per workgroup
constexpr int EV_U = 4;        // elements per thread per batch: all loads of a batch are issued first
constexpr int EV_MAXG = 1024;  // workgroups of the element pass (the rest is grid-strided)
constexpr int EV_SLOTS = 3;    // fp64 partials per workgroup: rec, kl_c, kl_s
// the largest element count: the grid-strided int index stays below 2^31 one stride past the end
constexpr long EV_MAX_TOTAL = (long)INT_MAX - 2L * EV_MAXG * EV_NT * EV_U;

struct EvalArgs {
  cv_bn b;
  const float* y;
  const float* x;
  int n, c, hw, d;
  FDiv fc, fhw, f2d;
  const float* heads;
  const float* z;
  const int64_t* label;
  cv_eval_sink sink;
  double* work;
};

struct EvalTerms {
  const float* term[2];
  float scale[2];
  int nterm;
};

// the batch's first row in the sink, or -1 when the batch is refused (the sticky flag is set, or its rows do not all
// fit under cap): then nothing is appended and the finish pass leaves the totals alone
__device__ __forceinline__ long long eval_row0(const cv_eval_sink& s, int n) {
  const long long cur = s.cursor[0], flag = s.cursor[1];
  if (flag != 0 || cur < 0 || cur > (long long)s.cap - (long long)n) return -1;
  return cur;
}

// Element pass.  Elements of y are visited in NHWC order (y coalesced; x is NCHW), in batches of EV_NT * EV_U per
// workgroup, grid-strided.  The same grid strides over the n x 4d heads (KL) and the n x 2d latents (append).
__global__ __launch_bounds__(EV_NT) void eval_elem_kernel(const EvalArgs A) {
  const cv_bn& b = A.b;
  const float* __restrict__ y = A.y;
  const float* __restrict__ x = A.x;
  const int n = A.n, c = A.c, hw = A.hw, d = A.d;
  __shared__ BnFwdC k[EV_MAXC];
  __shared__ double red[EV_NT / 64][EV_SLOTS];
  __shared__ double scratch[4 * EV_NT];
  const int total = n * c * hw;
  const int bx = blockIdx.x, gx = gridDim.x;
  const int base0 = bx * EV_NT * EV_U;
  float yv[EV_U], xv[EV_U];
  int chs[EV_U];
  bool live[EV_U];
  auto load = [&](int base) {
#pragma unroll
    for (int u = 0; u < EV_U; ++u) {
      const int i = base + u * EV_NT + threadIdx.x;
      yv[u] = 0.f;
      xv[u] = 0.f;
      chs[u] = 0;
      live[u] = i < total;
      if (live[u]) {
        const int pix = A.fc.div(i);  // img*hw + p
        const int ch = i - pix * c;
        const int img = A.fhw.div(pix);
        const int p = pix - img * hw;
        chs[u] = ch;
        yv[u] = y[i];
        xv[u] = x[(img * c + ch) * hw + p];
      }
    }
  };
  if (base0 < total) load(base0);  // (requested before the BN fold: its latency overlaps the constants' reads)
  bn_fold<EV_NT>(b, false, scratch, [&](int f, double s, double q, double, double) { k[f] = bn_fwd_const_s(b, f, s, q); });
  float rec = 0.f;
  for (int base = base0; base < total; base += gx * EV_NT * EV_U) {
    if (base != base0) load(base);
#pragma unroll
    for (int u = 0; u < EV_U; ++u) {
      if (!live[u]) continue;
      const float v = bn_out(yv[u], k[chs[u]]);
      const float xh = 1.0f / (1.0f + expf(-v));
      const float diff = xh - xv[u];
      rec = fmaf(diff, diff, rec);
    }
  }
  // KL sums over the heads rows (mu_c | lv_c | mu_s | lv_s): thread e owns the (row, column) pair of one mu
  float klc = 0.f, kls = 0.f;
  const int nkl = n * 2 * d;
  for (int e = bx * EV_NT + threadIdx.x; e < nkl; e += gx * EV_NT) {
    const int r = A.f2d.div(e), j = e - r * 2 * d;  // j < d: content, else style
    const int col = j < d ? j : j + d;              // mu_c at [0, d), mu_s at [2d, 3d)
    const float* row = A.heads + (size_t)r * 4 * d;
    const float m = row[col], l = row[col + d];
    const float t = 1.0f + l - m * m - expf(l);
    if (j < d) klc += t;
    else kls += t;
  }
  // append: z[:, :d] -> lat_c, z[:, d:] -> lat_s, label -> label at rows row0 .. row0 + n (all below cap)
  const long long row0 = eval_row0(A.sink, n);
  if (row0 >= 0) {
    for (int e = bx * EV_NT + threadIdx.x; e < nkl; e += gx * EV_NT) {
      const int r = A.f2d.div(e), j = e - r * 2 * d;
      const float v = A.z[e];
      if (j < d) A.sink.lat_c[(size_t)(row0 + r) * d + j] = v;
      else A.sink.lat_s[(size_t)(row0 + r) * d + (j - d)] = v;
    }
    for (int e = bx * EV_NT + threadIdx.x; e < n; e += gx * EV_NT) A.sink.label[row0 + e] = A.label[e];
  }
  // workgroup partials, fp64, into this workgroup's slots
  double vals[EV_SLOTS] = {(double)rec, (double)klc, (double)kls};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < EV_SLOTS; ++q) {
    const double v = wave_sum(vals[q]);
    if (lane == 0) red[w][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < EV_SLOTS) {
    const int q = threadIdx.x;
    A.work[(size_t)bx * EV_SLOTS + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// Finish pass, one workgroup: the `g` workgroups' partials added in a fixed order (thread t takes slots t, t + 256,
// ... in index order, then the wave and workgroup folds), the totals and the cursor advanced by thread 0.
__global__ __launch_bounds__(EV_NT) void eval_finish_kernel(const double* __restrict__ work, int g, int n,
                                                            const cv_eval_sink sink, const EvalTerms T) {
  __shared__ double red[EV_NT / 64][EV_SLOTS];
  double vals[EV_SLOTS] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < g; i += EV_NT) {
#pragma unroll
    for (int q = 0; q < EV_SLOTS; ++q) vals[q] += work[(size_t)i * EV_SLOTS + q];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < EV_SLOTS; ++q) {
    const double v = wave_sum(vals[q]);
    if (lane == 0) red[w][q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long row0 = eval_row0(sink, n);
  if (row0 < 0) {
    sink.cursor[1] = 1;
    return;
  }
  double s[EV_SLOTS];
#pragma unroll
  for (int q = 0; q < EV_SLOTS; ++q) s[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  const double inv_n = 1.0 / (double)n;
  sink.totals[0] += s[0] * inv_n;
  sink.totals[1] += -0.5 * s[1] * inv_n;
  sink.totals[2] += -0.5 * s[2] * inv_n;
  for (int q = 0; q < T.nterm; ++q) sink.totals[3 + q] += (double)T.scale[q] * (double)T.term[q][0];
  sink.totals[7] += 1.0;
  sink.cursor[0] = row0 + n;
}

int host_grid(long total) {
  const long g = (total + EV_NT * EV_U - 1) / (EV_NT * EV_U);
  return (int)(g < 1 ? 1 : (g > EV_MAXG ? EV_MAXG : g));
}

}  // namespace

extern "C" size_t cv_eval_workspace_bytes(int n, int c, int hw) {
  if (n < 1 || c < 1 || c > EV_MAXC || hw < 1) return 0;
  const long total = (long)n * c * hw;
  if (total > EV_MAX_TOTAL) return 0;
  return (size_t)host_grid(total) * EV_SLOTS * sizeof(double);
}

extern "C" int cv_eval_batch(const cv_bn* bn, const float* y, const float* x, int n, int c, int hw, const float* heads,
                             const float* z, int d, const int64_t* label, const float* const* terms,
                             const float* term_scale, int nterm, const cv_eval_sink* sink, double* work,
                             cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(bn != nullptr, "eval_batch: null bn");
  CV_REQUIRE(y != nullptr, "eval_batch: null y");
  CV_REQUIRE(x != nullptr, "eval_batch: null x");
  CV_REQUIRE(heads != nullptr, "eval_batch: null heads");
  CV_REQUIRE(z != nullptr, "eval_batch: null z");
  CV_REQUIRE(label != nullptr, "eval_batch: null label");
  CV_REQUIRE(sink != nullptr, "eval_batch: null sink");
  CV_REQUIRE(work != nullptr, "eval_batch: null work");
  CV_REQUIRE(n >= 1, "eval_batch: n=%d < 1", n);
  CV_REQUIRE(d >= 1, "eval_batch: d=%d < 1", d);
  CV_REQUIRE(c >= 1 && c <= EV_MAXC, "eval_batch: c=%d outside 1..%d", c, EV_MAXC);
  CV_REQUIRE(hw >= 1, "eval_batch: hw=%d < 1", hw);
  CV_REQUIRE(nterm >= 0 && nterm <= 2, "eval_batch: nterm=%d outside 0..2", nterm);
  CV_REQUIRE(sink->cap >= 0, "eval_batch: cap=%lld < 0", (long long)sink->cap);
  CV_REQUIRE(sink->lat_c != nullptr, "eval_batch: null sink lat_c");
  CV_REQUIRE(sink->lat_s != nullptr, "eval_batch: null sink lat_s");
  CV_REQUIRE(sink->label != nullptr, "eval_batch: null sink label");
  CV_REQUIRE(sink->cursor != nullptr, "eval_batch: null sink cursor");
  CV_REQUIRE(sink->totals != nullptr, "eval_batch: null sink totals");
  CV_REQUIRE((long)n * c * hw <= EV_MAX_TOTAL, "eval_batch: n*c*hw=%ld elements > %ld", (long)n * c * hw, EV_MAX_TOTAL);
  CV_REQUIRE((long)n * 4 * d <= EV_MAX_TOTAL, "eval_batch: n*4d=%ld elements > %ld", (long)n * 4 * d, EV_MAX_TOTAL);
  CV_REQUIRE(bn->C == c, "eval_batch: bn has %d channels, c=%d", bn->C, c);
  CV_REQUIRE(bn->train || (bn->running_mean && bn->running_var), "eval_batch: eval-mode bn without running statistics");
  EvalTerms T{};
  T.nterm = nterm;
  for (int q = 0; q < nterm; ++q) {
    CV_REQUIRE(terms != nullptr && term_scale != nullptr && terms[q] != nullptr, "eval_batch: null term %d", q);
    T.term[q] = terms[q];
    T.scale[q] = term_scale[q];
  }
  EvalArgs A{};
  A.b = *bn;
  A.y = y;
  A.x = x;
  A.n = n;
  A.c = c;
  A.hw = hw;
  A.d = d;
  A.fc = FDiv::make((uint32_t)c);
  A.fhw = FDiv::make((uint32_t)hw);
  A.f2d = FDiv::make((uint32_t)(2 * d));
  A.heads = heads;
  A.z = z;
  A.label = label;
  A.sink = *sink;
  A.work = work;
  const int g = host_grid((long)n * c * hw);
  hipLaunchKernelGGL(eval_elem_kernel, dim3(g), dim3(EV_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("eval_batch (element pass)");
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(EV_NT), 0, S(stream), (const double*)work, g, n, *sink, T);
  CV_LAUNCH_CHECK("eval_batch (finish pass)");
  return 0;
}
