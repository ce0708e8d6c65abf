// InfoNCE (mi_estimator.py:245-273) for gfx950 in O(N h) memory.
//
// The critic F = Linear(dx+dy, h) -> ReLU -> Linear(h, 1) -> Softplus is evaluated on all N^2 pairs [x_j, y_i]
// (mi_estimator.py:262-268).  Its first Linear is a sum of an x part and a y part, so with
//   a_j = W1[:, :dx] x_j,   c_i = W1[:, dx:] y_i + b1,   pre_ij = w2 . relu(a_j + c_i) + b2,   s_ij = softplus(pre_ij)
// a pair costs h adds / max / fma on two cached rows and nothing of size N^2 is stored:
//   value = mean_i s_ii - (mean_i logsumexp_j s_ij - log n),     learning_loss = -value.
// With p_ij = softmax_j s_ij and G_ij = g (delta_ij - p_ij) / n * sigmoid(pre_ij):
//   d c_i = w2 (.) sum_j G_ij 1[a_j + c_i > 0],   d a_j = w2 (.) sum_i G_ij 1[a_j + c_i > 0],
//   d w2 = sum_ij G_ij relu(a_j + c_i),   d b2 = sum_ij G_ij = g/n sum_ij p_ij (sigmoid(pre_ii) - sigmoid(pre_ij)),
//   dx_j = W1x^T d a_j,   dy_i = W1y^T d c_i,
//   dW1x = sum_j d a_j x_j^T,   dW1y = sum_i d c_i y_i^T,   db1 = sum_i d c_i.
// Launches (each a kernel boundary; no workgroup reads another's stores inside a launch, except through the
// shared last launch of the learning step, cv_mi.hpp):
//   pro   (one wave per row)  a, c and the diagonal terms s_ii;
//   pass  (one wave = 64 owners x one chunk of the streamed index, tiles through LDS).  Forward: owners are rows i,
//         an online log-sum-exp over the chunk's j.  Backward: the row-owned role recomputes s_ij from a, c and the
//         saved row log-sum-exps and sums G_ij 1[.] (and G_ij relu(.), G_ij) over its chunk in registers; the
//         column-owned role (blockIdx.z = 1) owns a_j, streams c_i and lse_i, and sums over i.  Every (chunk, owner)
//         partial is a slot of its own;
//   fin   (one workgroup) merges the chunks' (max, sum) per row in chunk order into lse_i and reduces the value;
//   epi   (one wave per row) folds the chunk partials in chunk order into d a, d c, applies W1^T (written,
//         accumulated, or chained through z = mu + eps*exp(lv/2) into d(heads), vae.py:56-60) and reduces the
//         parameter gradients in registers, across the waves in LDS, into per-workgroup partials;
//   mi_learn_reduce_launch folds those in block order (and takes the Adam step, trainer.py:885-887).
// Every reduction has a fixed order and no float atomic writes an output: replays are bit-identical.
#include "cv_mi.hpp"

namespace cv {

constexpr int NCE_MAXN = 16384;  // largest batch
constexpr int NCE_WAVES = 512;   // waves a pass aims for (owner groups x chunks)
constexpr int NCE_MINCH = 16;    // smallest chunk of the streamed index
constexpr int NCE_TJ = 32;       // streamed rows per LDS tile

static inline int bucket64(int v) { return v <= 8 ? 8 : v <= 16 ? 16 : v <= 32 ? 32 : 64; }

// chunk length of the streamed index for batch n (its count is cdiv(n, chunk))
static inline int nce_chunk(int n) {
  const int rg = cdiv(n, 64);
  int js = NCE_WAVES / rg;
  if (js < 1) js = 1;
  const int mx = cdiv(n, NCE_MINCH);
  if (js > mx) js = mx;
  return cdiv(n, js);
}

// the estimator workspace: the shared header (cv_mi.hpp: gpart / lpart / ticket of the learning step's last launch),
// then a[n][hm], c[n][hm], the diagonal terms s_ii and sigmoid(pre_ii), the row log-sum-exps and the
// per-(chunk, owner) partials
struct NceWork {
  float *a, *c, *sd, *sgd, *lse, *pm, *pl, *pc, *pa, *pw, *pb;
};
__host__ __device__ inline size_t nce_pad16(size_t words) { return (words + 15) / 16 * 16; }
__host__ __device__ inline NceWork nce_work(void* base, size_t hdr, int n, int hm, int js) {
  NceWork w;
  float* p = (float*)((char*)base + hdr);
  const size_t row = nce_pad16((size_t)n * hm), vec = nce_pad16((size_t)n);
  const size_t prow = nce_pad16((size_t)js * n * hm), pvec = nce_pad16((size_t)js * n);
  w.a = p; p += row;
  w.c = p; p += row;
  w.sd = p; p += vec;
  w.sgd = p; p += vec;
  w.lse = p; p += vec;
  w.pm = p; p += pvec;
  w.pl = p; p += pvec;
  w.pc = p; p += prow;
  w.pa = p; p += prow;
  w.pw = p; p += prow;
  w.pb = p;
  return w;
}
static inline size_t nce_work_bytes(int n, int h) {
  const int hm = bucket64(h < 1 ? 1 : h);
  if (n < 1) n = 1;
  const int js = cdiv(n, nce_chunk(n));
  const size_t words = 2 * nce_pad16((size_t)n * hm) + 3 * nce_pad16((size_t)n) + 3 * nce_pad16((size_t)js * n) +
                       3 * nce_pad16((size_t)js * n * hm);
  return mi_work_bytes(0) + words * 4 + 64;
}

struct NceArgs {
  cv_critic P;
  const float* x; int ldx;
  const float* y; int ldy;
  int n;
  void* work; size_t hdr;
  int hm, js, ch;
  float* out;
  // backward
  const float* gscale; float gmul; int learn;  // learn: the seed is -1 (learning_loss = -value)
  float* dx; float* dy; int gld; int accumulate;
  const float* heads; const float* z; float* dheads; int d;  // chain mode (fused step)
};

__device__ __forceinline__ float bcastf(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// nn.Softplus(beta = 1, threshold = 20) and its derivative
__device__ __forceinline__ float softplus20(float p) { return p > 20.f ? p : log1pf(expf(p)); }
__device__ __forceinline__ float dsoftplus20(float p) { return p > 20.f ? 1.f : 1.f / (1.f + expf(-p)); }

// W1 [u][k] in LDS with an odd row pitch (row walks by lane = u and column walks by lane = k conflict free);
// 64 rows allocated, rows >= h are never used unmasked
template <int DM>
__device__ __forceinline__ void stage_critic(const cv_critic& P, float* sw, float* sb1, float* sw2) {
  constexpr int PW = 2 * DM + 1;
  const int t = threadIdx.x, nt = blockDim.x;
  const int din = P.dx + P.dy, tot = P.h * din;
  for (int i = t; i < tot; i += nt) {
    const int u = i / din, k = i - u * din;
    sw[u * PW + k] = P.w1[i];
  }
  for (int i = t; i < 64; i += nt) {
    sb1[i] = (i < P.h) ? P.b1[i] : 0.f;
    sw2[i] = (i < P.h) ? P.w2[i] : 0.f;
  }
  __syncthreads();
}

// ---------------------------------------------------------------- prologue: a, c, s_ii (one wave per row)
template <int DM>
__global__ __launch_bounds__(256) void nce_pro_kernel(const NceArgs A) {
  constexpr int PW = 2 * DM + 1;
  __shared__ float sw[64 * PW];
  __shared__ float sb1[64], sw2[64];
  stage_critic<DM>(A.P, sw, sb1, sw2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = A.n, dx = A.P.dx, dy = A.P.dy, h = A.P.h, hm = A.hm;
  NceWork W = nce_work(A.work, A.hdr, n, hm, A.js);
  const float b2 = A.P.b2[0];
  const float* r1 = sw + lane * PW;
  for (int r = blockIdx.x * 4 + w; r < n; r += gridDim.x * 4) {
    const float xv = (lane < dx) ? A.x[(size_t)r * A.ldx + lane] : 0.f;
    const float yv = (lane < dy) ? A.y[(size_t)r * A.ldy + lane] : 0.f;
    float a = 0.f, c = sb1[lane];
#pragma unroll
    for (int k = 0; k < DM; ++k) {
      if (k < dx) a = fmaf(r1[k], bcastf(xv, k), a);
      if (k < dy) c = fmaf(r1[dx + k], bcastf(yv, k), c);
    }
    if (lane >= h) { a = 0.f; c = 0.f; }
    if (lane < hm) {
      W.a[(size_t)r * hm + lane] = a;
      W.c[(size_t)r * hm + lane] = c;
    }
    const float pre = b2 + wave_sum(sw2[lane] * fmaxf(a + c, 0.f));
    if (lane == 0) {
      W.sd[r] = softplus20(pre);
      W.sgd[r] = dsoftplus20(pre);
    }
  }
}

// ---------------------------------------------------------------- pass: 64 owners x one chunk per wave
// MODE 0: forward (online log-sum-exp); 1: backward, inputs only; 2: backward with the w2 / b2 sums
template <int HM, int MODE>
__global__ __launch_bounds__(64) void nce_pass_kernel(const NceArgs A) {
  __shared__ float4 tile[NCE_TJ * HM / 4];
  __shared__ float4 sw2v[HM / 4];
  __shared__ float tl[NCE_TJ];
  const int lane = threadIdx.x, n = A.n, h = A.P.h;
  const bool col = blockIdx.z == 1;  // column-owned role: owners are the columns j (a_j), the rows i are streamed
  NceWork W = nce_work(A.work, A.hdr, n, HM, A.js);
  const float* own_src = col ? W.a : W.c;
  const float* st_src = col ? W.c : W.a;
  const int o = blockIdx.x * 64 + lane;
  const bool live = o < n;
  const int oc = live ? o : n - 1;
  float own[HM];
#pragma unroll
  for (int q = 0; q < HM / 4; ++q) {
    const float4 v = reinterpret_cast<const float4*>(own_src + (size_t)oc * HM)[q];
    own[4 * q] = v.x; own[4 * q + 1] = v.y; own[4 * q + 2] = v.z; own[4 * q + 3] = v.w;
  }
  if (lane < HM) reinterpret_cast<float*>(sw2v)[lane] = (lane < h) ? A.P.w2[lane] : 0.f;
  const float b2 = A.P.b2[0];
  const int s = blockIdx.y, j0 = s * A.ch, j1 = (j0 + A.ch < n) ? j0 + A.ch : n;
  const float own_lse = (MODE > 0 && !col) ? W.lse[oc] : 0.f;
  const float own_sgd = (MODE == 2 && !col) ? W.sgd[oc] : 0.f;
  const float gsc = (A.learn ? -1.f : A.gmul * (A.gscale ? A.gscale[0] : 1.f)) / (float)n;
  float m = -INFINITY, l = 0.f;
  float dacc[MODE > 0 ? HM : 1], wacc[MODE == 2 ? HM : 1], bacc = 0.f;
#pragma unroll
  for (int u = 0; u < (MODE > 0 ? HM : 1); ++u) dacc[u] = 0.f;
#pragma unroll
  for (int u = 0; u < (MODE == 2 ? HM : 1); ++u) wacc[u] = 0.f;
  for (int jt = j0; jt < j1; jt += NCE_TJ) {
    const int cnt = (j1 - jt < NCE_TJ) ? j1 - jt : NCE_TJ;
    __syncthreads();
    for (int q = lane; q < cnt * (HM / 4); q += 64)
      tile[q] = reinterpret_cast<const float4*>(st_src + (size_t)jt * HM)[q];
    if (MODE > 0 && lane < cnt) tl[lane] = W.lse[jt + lane];
    __syncthreads();
    for (int jj = 0; jj < cnt; ++jj) {
      const float4* tr = tile + jj * (HM / 4);
      // (the same ascending fma chain in every mode and role: s_ij is recomputed to the bit)
      float pre = b2;
#pragma unroll
      for (int q = 0; q < HM / 4; ++q) {
        const float4 v = tr[q], wv = sw2v[q];
        pre = fmaf(wv.x, fmaxf(own[4 * q] + v.x, 0.f), pre);
        pre = fmaf(wv.y, fmaxf(own[4 * q + 1] + v.y, 0.f), pre);
        pre = fmaf(wv.z, fmaxf(own[4 * q + 2] + v.z, 0.f), pre);
        pre = fmaf(wv.w, fmaxf(own[4 * q + 3] + v.w, 0.f), pre);
      }
      const float sij = softplus20(pre);
      if (MODE == 0) {
        // online log-sum-exp with the running maximum subtracted
        if (sij > m) {
          l = l * expf(m - sij) + 1.f;
          m = sij;
        } else {
          l += expf(sij - m);
        }
      } else {
        const float lse = col ? tl[jj] : own_lse;
        const float p = expf(sij - lse);
        const float sg = dsoftplus20(pre);
        const float G = gsc * (((jt + jj) == o ? 1.f : 0.f) - p) * sg;
#pragma unroll
        for (int q = 0; q < HM / 4; ++q) {
          const float4 v = tr[q];
          const float t0 = own[4 * q] + v.x, t1 = own[4 * q + 1] + v.y, t2 = own[4 * q + 2] + v.z,
                      t3 = own[4 * q + 3] + v.w;
          dacc[4 * q] += (t0 > 0.f) ? G : 0.f;
          dacc[4 * q + 1] += (t1 > 0.f) ? G : 0.f;
          dacc[4 * q + 2] += (t2 > 0.f) ? G : 0.f;
          dacc[4 * q + 3] += (t3 > 0.f) ? G : 0.f;
          if (MODE == 2) {
            wacc[4 * q] = fmaf(G, fmaxf(t0, 0.f), wacc[4 * q]);
            wacc[4 * q + 1] = fmaf(G, fmaxf(t1, 0.f), wacc[4 * q + 1]);
            wacc[4 * q + 2] = fmaf(G, fmaxf(t2, 0.f), wacc[4 * q + 2]);
            wacc[4 * q + 3] = fmaf(G, fmaxf(t3, 0.f), wacc[4 * q + 3]);
          }
        }
        // d b2 = sum_ij G_ij = g/n sum_ij p_ij (sigmoid(pre_ii) - sigmoid(pre_ij)), as sum_j p_ij = 1: the two
        // means that cancel in sum_ij G_ij are subtracted pair by pair, where the operands are close
        if (MODE == 2) bacc = fmaf(gsc * p, own_sgd - sg, bacc);
      }
    }
  }
  if (!live) return;
  const size_t slot = (size_t)s * n + o;
  if (MODE == 0) {
    W.pm[slot] = m;
    W.pl[slot] = l;
  } else {
    float4* dst = reinterpret_cast<float4*>((col ? W.pa : W.pc) + slot * HM);
#pragma unroll
    for (int q = 0; q < HM / 4; ++q)
      dst[q] = make_float4(dacc[4 * q], dacc[4 * q + 1], dacc[4 * q + 2], dacc[4 * q + 3]);
    if (MODE == 2 && !col) {  // (the w2 / b2 sums run over all pairs once: the row-owned role keeps them)
      float4* dw = reinterpret_cast<float4*>(W.pw + slot * HM);
#pragma unroll
      for (int q = 0; q < HM / 4; ++q)
        dw[q] = make_float4(wacc[4 * q], wacc[4 * q + 1], wacc[4 * q + 2], wacc[4 * q + 3]);
      W.pb[slot] = bacc;
    }
  }
}

// ---------------------------------------------------------------- fin: lse_i and the value (1 x 1024)
__global__ __launch_bounds__(1024) void nce_fin_kernel(const NceArgs A) {
  __shared__ double scratch[16];
  const int n = A.n, js = A.js, t = threadIdx.x;
  NceWork W = nce_work(A.work, A.hdr, n, A.hm, js);
  double acc = 0.0;
  for (int i = t; i < n; i += 1024) {
    float M = -INFINITY;
    for (int s = 0; s < js; ++s) M = fmaxf(M, W.pm[(size_t)s * n + i]);
    float L = 0.f;
    for (int s = 0; s < js; ++s) L += W.pl[(size_t)s * n + i] * expf(W.pm[(size_t)s * n + i] - M);
    const float lse = M + logf(L);
    W.lse[i] = lse;
    acc += (double)W.sd[i] - (double)lse;
  }
  const double tot = block_sum<1024, double>(acc, scratch);
  const double value = tot / (double)n + log((double)n);
  if (t == 0 && A.out) A.out[0] = (float)value;
  // the learning step's last launch reports -(sum lpart) / n
  MiWork H = mi_work(A.work, 0);
  if (t < MI_NB) H.lpart[t] = (t == 0) ? value * (double)n : 0.0;
}

// ---------------------------------------------------------------- epilogue (one wave per row)
// per-workgroup parameter partial, lane-major with pitch 64: [dW1: k*64 + u] (k < dx+dy; 2*DM*64 words reserved),
// then db1[64] dw2[64] db2[64] (lane 0)
template <int DM, bool PG>
__global__ __launch_bounds__(256) void nce_epi_kernel(const NceArgs A) {
  constexpr int PW = 2 * DM + 1;
  constexpr int SGW = 2 * DM * 64 + 256;
  static_assert(64 * PW <= SGW, "the W1 image fits the reduction buffer");
  __shared__ __attribute__((aligned(16))) float buf[SGW];  // the W1 image, then the cross-wave reduction
  __shared__ float sb1[64], sw2[64];
  stage_critic<DM>(A.P, buf, sb1, sw2);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int n = A.n, dx = A.P.dx, dy = A.P.dy, h = A.P.h, hm = A.hm, js = A.js;
  NceWork W = nce_work(A.work, A.hdr, n, hm, js);
  float g1[PG ? 2 * DM : 1];
#pragma unroll
  for (int k = 0; k < (PG ? 2 * DM : 1); ++k) g1[k] = 0.f;
  float gb1 = 0.f, gw2 = 0.f, gb2 = 0.f;
  for (int r = blockIdx.x * 4 + w; r < n; r += gridDim.x * 4) {
    // the chunk partials in chunk order
    float da = 0.f, dc = 0.f, dw = 0.f, db = 0.f;
    if (lane < h) {
      for (int s = 0; s < js; ++s) {
        const size_t o = ((size_t)s * n + r) * hm + lane;
        dc += W.pc[o];
        da += W.pa[o];
        if (PG) dw += W.pw[o];
      }
      dc *= sw2[lane];
      da *= sw2[lane];
    }
    if (PG && lane == 0)
      for (int s = 0; s < js; ++s) db += W.pb[(size_t)s * n + r];
    if (!A.learn) {
      float dxv = 0.f, dyv = 0.f;
      for (int u = 0; u < h; ++u) {
        dxv = fmaf(buf[u * PW + lane], bcastf(da, u), dxv);
        dyv = fmaf(buf[u * PW + dx + lane], bcastf(dc, u), dyv);
      }
      if (lane >= dx) dxv = 0.f;
      if (lane >= dy) dyv = 0.f;
      if (A.dheads) {
        // x = z_c, y = z_s ; chain through z = mu + eps*exp(lv/2): dmu += dz, dlv += dz*(z-mu)/2
        const int d = A.d;
        if (lane < d) {
          const size_t hr = (size_t)r * 4 * d, zr = (size_t)r * 2 * d;
          const float muc = A.heads[hr + lane], mus = A.heads[hr + 2 * d + lane];
          A.dheads[hr + lane] += dxv;
          A.dheads[hr + d + lane] += dxv * (A.z[zr + lane] - muc) * 0.5f;
          A.dheads[hr + 2 * d + lane] += dyv;
          A.dheads[hr + 3 * d + lane] += dyv * (A.z[zr + d + lane] - mus) * 0.5f;
        }
      } else {
        if (A.dx && lane < dx) {
          float* p = A.dx + (size_t)r * A.gld + lane;
          *p = A.accumulate ? *p + dxv : dxv;
        }
        if (A.dy && lane < dy) {
          float* p = A.dy + (size_t)r * A.gld + lane;
          *p = A.accumulate ? *p + dyv : dyv;
        }
      }
    }
    if (PG) {
      const float xv = (lane < dx) ? A.x[(size_t)r * A.ldx + lane] : 0.f;
      const float yv = (lane < dy) ? A.y[(size_t)r * A.ldy + lane] : 0.f;
#pragma unroll
      for (int k = 0; k < DM; ++k) {
        if (k < dx) g1[k] = fmaf(da, bcastf(xv, k), g1[k]);
        if (k < dy) g1[DM + k] = fmaf(dc, bcastf(yv, k), g1[DM + k]);
      }
      gb1 += dc;
      gw2 += dw;
      gb2 += db;
    }
  }
  if (!PG) return;
  // cross-wave reduction in LDS, waves in sequence (deterministic), lane-major (conflict free)
  __syncthreads();  // (every wave is done with the W1 image)
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
      const bool first = ww == 0;
#pragma unroll
      for (int k = 0; k < DM; ++k) {
        if (k < dx) {
          float* s1 = buf + k * 64 + lane;
          *s1 = first ? g1[k] : *s1 + g1[k];
        }
        if (k < dy) {
          float* s1 = buf + (dx + k) * 64 + lane;
          *s1 = first ? g1[DM + k] : *s1 + g1[DM + k];
        }
      }
      float* sb = buf + 2 * DM * 64;
      sb[lane] = first ? gb1 : sb[lane] + gb1;
      sb[64 + lane] = first ? gw2 : sb[64 + lane] + gw2;
      sb[128 + lane] = first ? gb2 : sb[128 + lane] + gb2;
      sb[192 + lane] = 0.f;
    }
    __syncthreads();
  }
  MiWork H = mi_work(A.work, 0);
  float* dst = H.gpart + (size_t)blockIdx.x * MI_GSZ;
  const int din = dx + dy;
  for (int i = t; i < din * 64; i += 256) dst[i] = buf[i];
  dst[2 * DM * 64 + t] = buf[2 * DM * 64 + t];
}

}  // namespace cv

using namespace cv;

extern "C" int cv_infonce_supported(int n, int dx, int dy, int h) {
  return n >= 2 && n <= NCE_MAXN && dx >= 1 && dx <= 64 && dy >= 1 && dy <= 64 && h >= 1 && h <= 64;
}

extern "C" size_t cv_infonce_workspace_bytes(int n, int h) { return nce_work_bytes(n, h); }

static int check_critic(const cv_critic* P, const float* x, const float* y, int n, const void* work,
                        const char* who) {
  CV_REQUIRE(P && P->w1 && P->b1 && P->w2 && P->b2, "%s: critic weights missing", who);
  CV_REQUIRE(P->dx >= 1 && P->dx <= 64 && P->dy >= 1 && P->dy <= 64 && P->h >= 1 && P->h <= 64,
             "%s: critic widths must be in 1..64 (dx=%d dy=%d h=%d)", who, P->dx, P->dy, P->h);
  CV_REQUIRE(x && y && work, "%s: bad args", who);
  CV_REQUIRE(n >= 2 && n <= NCE_MAXN, "%s: batch must be in 2..%d (n=%d)", who, NCE_MAXN, n);
  CV_REQUIRE((uintptr_t)work % 16 == 0, "%s: workspace must be 16-byte aligned", who);
  return 0;
}

static NceArgs nce_args(const cv_critic* P, const float* x, int ldx, const float* y, int ldy, int n, void* work) {
  NceArgs a;
  memset(&a, 0, sizeof(a));
  a.P = *P;
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.n = n;
  a.work = work;
  a.hdr = mi_work_bytes(0);
  a.hm = bucket64(P->h);
  a.ch = nce_chunk(n);
  a.js = cdiv(n, a.ch);
  return a;
}

static int nce_row_blocks(int n) {
  const int b = cdiv(n, 4);
  return b < MI_NB ? b : MI_NB;
}

#define CV_NCE_DM(dm, KERNEL, grid, block, st, arg)                               \
  do {                                                                            \
    if ((dm) == 8) hipLaunchKernelGGL(KERNEL<8>, grid, block, 0, st, arg);        \
    else if ((dm) == 16) hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, st, arg); \
    else if ((dm) == 32) hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, st, arg); \
    else hipLaunchKernelGGL(KERNEL<64>, grid, block, 0, st, arg);                 \
  } while (0)
#define CV_NCE_DM2(dm, KERNEL, PG, grid, block, st, arg)                              \
  do {                                                                                \
    if ((dm) == 8) hipLaunchKernelGGL((KERNEL<8, PG>), grid, block, 0, st, arg);      \
    else if ((dm) == 16) hipLaunchKernelGGL((KERNEL<16, PG>), grid, block, 0, st, arg); \
    else if ((dm) == 32) hipLaunchKernelGGL((KERNEL<32, PG>), grid, block, 0, st, arg); \
    else hipLaunchKernelGGL((KERNEL<64, PG>), grid, block, 0, st, arg);               \
  } while (0)

// a, c, s_ii; the forward pass; lse and the value
static int nce_forward_launches(const NceArgs& a, hipStream_t st) {
  const int dm = bucket64(a.P.dx > a.P.dy ? a.P.dx : a.P.dy);
  CV_NCE_DM(dm, nce_pro_kernel, dim3(nce_row_blocks(a.n)), dim3(256), st, a);
  CV_LAUNCH_CHECK("infonce.pro");
  CV_NCE_DM2(a.hm, nce_pass_kernel, 0, dim3(cdiv(a.n, 64), a.js, 1), dim3(64), st, a);
  CV_LAUNCH_CHECK("infonce.pass");
  hipLaunchKernelGGL(nce_fin_kernel, dim3(1), dim3(1024), 0, st, a);
  CV_LAUNCH_CHECK("infonce.fin");
  return 0;
}

// both backward roles in one grid, then the epilogue (pg: with the parameter-gradient partials)
static int nce_backward_launches(const NceArgs& a, bool pg, hipStream_t st) {
  const int dm = bucket64(a.P.dx > a.P.dy ? a.P.dx : a.P.dy);
  const dim3 grid(cdiv(a.n, 64), a.js, 2);
  if (pg) CV_NCE_DM2(a.hm, nce_pass_kernel, 2, grid, dim3(64), st, a);
  else CV_NCE_DM2(a.hm, nce_pass_kernel, 1, grid, dim3(64), st, a);
  CV_LAUNCH_CHECK("infonce.pass_bwd");
  if (pg) CV_NCE_DM2(dm, nce_epi_kernel, true, dim3(nce_row_blocks(a.n)), dim3(256), st, a);
  else CV_NCE_DM2(dm, nce_epi_kernel, false, dim3(nce_row_blocks(a.n)), dim3(256), st, a);
  CV_LAUNCH_CHECK("infonce.epi");
  return 0;
}

// the last launch of cv_mi_learning_step over the critic's four segments
static int nce_param_reduce(const NceArgs& a, const cv_critic_grad* g, float* loss_out, float* params,
                            const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel, const float* hyper,
                            int64_t* step, hipStream_t st) {
  const int dm = bucket64(a.P.dx > a.P.dy ? a.P.dx : a.P.dy);
  const int din = a.P.dx + a.P.dy, h = a.P.h;
  LearnArgs la;
  memset(&la, 0, sizeof(la));
  la.n = a.n;
  la.work = a.work;
  la.loss_out = loss_out;
  la.params = params; la.grads = grads; la.m = exp_avg; la.v = exp_avg_sq; la.numel = numel;
  la.hyper = hyper; la.step = step;
  LearnSegs sg;
  memset(&sg, 0, sizeof(sg));
  float* const gp[4] = {g->w1, g->b1, g->w2, g->b2};
  const int ln[4] = {h * din, h, h, 1};
  const int in[4] = {din, 0, 0, 0};
  const int po[4] = {0, 2 * dm * 64, 2 * dm * 64 + 64, 2 * dm * 64 + 128};
  const int tr[4] = {1, 0, 0, 0};
  int total = 0;
  for (int s = 0; s < 4; ++s) {
    sg.g[s] = gp[s]; sg.len[s] = ln[s]; sg.inner[s] = in[s]; sg.poff[s] = po[s]; sg.trans[s] = tr[s];
    total += ln[s];
  }
  return mi_learn_reduce_launch(la, sg, nce_row_blocks(a.n), total, st);
}

extern "C" int cv_infonce_forward(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy, int n,
                                  void* work, float* out, cv_stream_t stream) {
  clear_error();
  if (check_critic(critic, x, y, n, work, "infonce_forward")) return 1;
  NceArgs a = nce_args(critic, x, ldx, y, ldy, n, work);
  a.out = out;
  return nce_forward_launches(a, S(stream));
}

extern "C" int cv_infonce_backward(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy, int n,
                                   void* work, const float* gscale, float gmul, float* dx, float* dy, int gld,
                                   int accumulate, const cv_critic_grad* g, const float* heads, const float* z,
                                   float* dheads, int d, cv_stream_t stream) {
  clear_error();
  if (check_critic(critic, x, y, n, work, "infonce_backward")) return 1;
  CV_REQUIRE(!dheads || (heads && z && d == critic->dx && d == critic->dy),
             "infonce_backward: chain mode needs heads, z, d");
  CV_REQUIRE(!g || (g->w1 && g->b1 && g->w2 && g->b2), "infonce_backward: critic gradient buffers missing");
  NceArgs a = nce_args(critic, x, ldx, y, ldy, n, work);
  a.gscale = gscale; a.gmul = gmul;
  a.dx = dx; a.dy = dy; a.gld = gld; a.accumulate = accumulate;
  a.heads = heads; a.z = z; a.dheads = dheads; a.d = d;
  if (int rc = nce_backward_launches(a, g != nullptr, S(stream))) return rc;
  if (g) return nce_param_reduce(a, g, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, S(stream));
  return 0;
}

extern "C" int cv_infonce_learning_step(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy,
                                        int n, void* work, float* loss_out, const cv_critic_grad* g, float* params,
                                        const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                        const float* hyper, int64_t* step, cv_stream_t stream) {
  clear_error();
  if (check_critic(critic, x, y, n, work, "infonce_learning_step")) return 1;
  CV_REQUIRE(g && g->w1 && g->b1 && g->w2 && g->b2, "infonce_learning_step: bad args");
  CV_REQUIRE(!params || (grads && exp_avg && exp_avg_sq && hyper && step && numel > 0),
             "infonce_learning_step: Adam arena incomplete");
  const int din = critic->dx + critic->dy, h = critic->h;
  float* const gp[4] = {g->w1, g->b1, g->w2, g->b2};
  const int ln[4] = {h * din, h, h, 1};
  if (params)
    for (int s = 0; s < 4; ++s)
      CV_REQUIRE(gp[s] >= grads && gp[s] + ln[s] <= grads + numel,
                 "infonce_learning_step: with Adam the gradients must live in the grads arena");
  NceArgs a = nce_args(critic, x, ldx, y, ldy, n, work);
  a.learn = 1;
  if (int rc = nce_forward_launches(a, S(stream))) return rc;
  if (int rc = nce_backward_launches(a, true, S(stream))) return rc;
  return nce_param_reduce(a, g, loss_out, params, grads, exp_avg, exp_avg_sq, numel, hyper, step, S(stream));
}
