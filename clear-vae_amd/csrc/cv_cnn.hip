// Classifier tail of the CNN baselines (code/src/models/cnn.py:22-27, trainer.py:196-199, :228): BatchNorm1d(h) ->
// ReLU -> Linear(h,c) -> nn.CrossEntropyLoss() defaults on a [n][h], the output of the head's first Linear.  One
// training step of the tail (loss, the four tail gradients, d(a), running statistics; no optimizer) in two launches;
// the eval forward in one.
//
// The slab decomposition of cv_probe.hip: the hidden columns are independent through the BatchNorm, so a workgroup
// owns a slab of CL_S columns for all n rows: its statistics, xhat, y[:,slab], dgamma / dbeta[slab], dW2[:,slab],
// dy[:,slab] = dlogits W2[:,slab] and da[:,slab] are slab-local.  The only cross-workgroup quantity is logits (and
// dlogits):
//   launch 1 (cls_fwd_kernel)  per slab: fp64 column sums of a, xhat (kept in the workspace), running statistics,
//                              the slab's partial logits; the last-arriving workgroup folds the partials in slab
//                              order, adds b2 and computes the loss, dlogits = (softmax - onehot)/n and db2
//   launch 2 (cls_bwd_kernel)  per slab: dy, the ReLU mask, dbeta / dgamma (fp64 sums), dW2[:,slab], da[:,slab]
// No workgroup waits for another; every sum has a fixed order (no floating-point atomics): the same state and batch
// give the same bits, eager or replayed.
#include "cv_common.hpp"

namespace cv {

constexpr int CL_S = 16;    // hidden columns per workgroup
constexpr int CL_TR = 64;   // rows per tile
constexpr int CL_NT = 256;  // threads per workgroup
constexpr int CL_MAXH = 512, CL_MAXC = 32, CL_MAXN = 1024;
constexpr int CL_SP = CL_S + 1;     // pitch of a slab-wide LDS row
constexpr int CL_CP = CL_MAXC + 1;  // pitch of a staged dlogits row
constexpr int CL_ER = 8;            // rows per workgroup of the eval forward

struct ClsWork {
  unsigned* ticket;  // [0] launch 1 (self-resetting); the first 64 bytes of the workspace
  float* istd;       // [hp]
  float* xhat;       // [n][hp]
  float* dym;        // [n][hp]  masked dy
  float* part;       // [slabs][n*c] partial logits
  float* dl;         // [n*c] logits, then dlogits
};
__host__ __device__ inline size_t cl_r16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline int cl_slabs(int h) { return (h + CL_S - 1) / CL_S; }
__host__ __device__ inline size_t cls_work_bytes(int n, int h, int c) {
  const size_t hp = (size_t)cl_slabs(h) * CL_S;
  return 64 + cl_r16(hp * 4) + 2 * cl_r16((size_t)n * hp * 4) + cl_r16((size_t)cl_slabs(h) * n * c * 4) +
         cl_r16((size_t)n * c * 4);
}
__host__ __device__ inline ClsWork cls_work(void* base, int n, int h, int c) {
  const size_t hp = (size_t)cl_slabs(h) * CL_S;
  char* p = (char*)base;
  ClsWork w;
  w.ticket = (unsigned*)p;
  p += 64;
  w.istd = (float*)p;
  p += cl_r16(hp * 4);
  w.xhat = (float*)p;
  p += cl_r16((size_t)n * hp * 4);
  w.dym = (float*)p;
  p += cl_r16((size_t)n * hp * 4);
  w.part = (float*)p;
  p += cl_r16((size_t)cl_slabs(h) * n * c * 4);
  w.dl = (float*)p;
  return w;
}

struct ClsArgs {
  cv_cls P;
  const float* a;
  const int64_t* label;
  int n;
  void* work;
  float* loss_out;
  float* da;
  cv_cls_grad G;
};

// last-arriving workgroup detection: every thread drains and releases its own global stores at agent scope (the
// partial logits of a slab are written by all threads, and workgroups of one launch sit on different XCDs), thread 0
// takes a ticket; the last workgroup acquires before it reads the others' partials and resets the ticket for the
// next call
__device__ __forceinline__ bool cl_last_block(unsigned* ticket, int* flag) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = prev == gridDim.x - 1;
    *flag = last ? 1 : 0;
    if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const bool last = *flag != 0;
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return last;
}

// the BatchNorm output before the ReLU; the backward's mask is the sign of the same expression on the same bits
__device__ __forceinline__ float cl_pre(float gamma, float xhat, float beta) { return fmaf(gamma, xhat, beta); }

// ---------------------------------------------------------------- launch 1: forward of each slab, loss by the last
__global__ __launch_bounds__(CL_NT) void cls_fwd_kernel(const ClsArgs A) {
  __shared__ float hs[CL_TR * CL_SP];
  __shared__ float w2s[CL_MAXC * CL_SP];
  __shared__ double red[2 * CL_NT];
  __shared__ double cmean[CL_S], cistd[CL_S];
  __shared__ float cgam[CL_S], cbet[CL_S];
  __shared__ float b2r[(CL_NT / CL_MAXC) * CL_MAXC];
  __shared__ int flag;
  const cv_cls& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x, j0 = slab * CL_S;
  const int n = A.n, h = P.h, c = P.c;
  const int hp = gridDim.x * CL_S;
  const ClsWork W = cls_work(A.work, n, h, c);

  for (int idx = t; idx < c * CL_S; idx += CL_NT) {
    const int k = idx / CL_S, j = idx % CL_S;
    w2s[k * CL_SP + j] = j0 + j < h ? P.w2[(size_t)k * h + j0 + j] : 0.f;
  }
  if (t < CL_S) {
    const bool ok = j0 + t < h;
    cgam[t] = ok ? P.gamma[j0 + t] : 0.f;
    cbet[t] = ok ? P.beta[j0 + t] : 0.f;
  }

  // pass 1: fp64 column sums of a[:,slab] (thread = every 16th row x 1 column)
  const int col = t % CL_S, rl = t / CL_S;
  const bool cok = j0 + col < h;
  double s = 0.0, q = 0.0;
  if (cok)
    for (int i = rl; i < n; i += CL_NT / CL_S) {
      const double v = (double)A.a[(size_t)i * h + j0 + col];
      s += v;
      q += v * v;
    }
  red[t] = s;
  red[CL_NT + t] = q;
  __syncthreads();
  if (t < CL_S) {
    double ss = 0.0, qq = 0.0;
    for (int r = 0; r < CL_NT / CL_S; ++r) {  // row lanes in order
      ss += red[r * CL_S + t];
      qq += red[CL_NT + r * CL_S + t];
    }
    const double mean = ss / (double)n;
    double var = qq / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    const double istd = 1.0 / sqrt(var + (double)P.eps);
    cmean[t] = mean;
    cistd[t] = istd;
    W.istd[j0 + t] = (float)istd;
    if (j0 + t < h) {
      const double mo = (double)P.momentum;
      P.running_mean[j0 + t] = (float)((1.0 - mo) * (double)P.running_mean[j0 + t] + mo * mean);
      P.running_var[j0 + t] =
          (float)((1.0 - mo) * (double)P.running_var[j0 + t] + mo * var * ((double)n / (double)(n - 1)));
    }
  }
  if (slab == 0 && t == 0 && P.nbt) P.nbt[0] += 1;
  __syncthreads();

  // pass 2: xhat, y = relu(gamma xhat + beta), the slab's partial logits (thread = 1 row x every 4th class)
  {
    const double mean = cmean[col], istd = cistd[col];
    const float gam = cgam[col], bet = cbet[col];
    for (int i0 = 0; i0 < n; i0 += CL_TR) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rl + 16 * u, i = i0 + r;
        float hv = 0.f;
        if (i < n) {
          const float av = cok ? A.a[(size_t)i * h + j0 + col] : 0.f;
          const float xh = (float)(((double)av - mean) * istd);
          W.xhat[(size_t)i * hp + j0 + col] = xh;
          hv = fmaxf(cl_pre(gam, xh, bet), 0.f);
        }
        hs[r * CL_SP + col] = hv;
      }
      __syncthreads();
      const int r = t >> 2, i = i0 + r;
      if (i < n) {
        float* dst = W.part + (size_t)slab * n * c + (size_t)i * c;
        for (int k = t & 3; k < c; k += 4) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < CL_S; ++j) acc = fmaf(hs[r * CL_SP + j], w2s[k * CL_SP + j], acc);
          dst[k] = acc;
        }
      }
      __syncthreads();
    }
  }

  if (!cl_last_block(W.ticket, &flag)) return;
  // the last arriver: logits = b2 + partials in slab order
  const int nslab = gridDim.x, nc = n * c;
  for (int e = t; e < nc; e += CL_NT) {
    float v = P.b2[e % c];
    const float* pp = W.part + e;
#pragma unroll 8
    for (int sidx = 0; sidx < nslab; ++sidx) v += pp[(size_t)sidx * nc];
    W.dl[e] = v;
  }
  __syncthreads();
  // loss and dlogits = (softmax - onehot) / n, one row per thread; a label outside [0, c) indexes nothing and makes
  // the loss and its dlogits row NaN
  const float inv_n = 1.0f / (float)n;
  const float nanv = __builtin_nanf("");
  double lsum = 0.0;
  for (int i = t; i < n; i += CL_NT) {
    float* row = W.dl + (size_t)i * c;
    const int64_t lab = A.label[i];
    const bool valid = lab >= 0 && lab < (int64_t)c;
    float mx = row[0];
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, row[k]);
    float se = 0.f;
    for (int k = 0; k < c; ++k) se += expf(row[k] - mx);
    const float lse = mx + logf(se);
    lsum += valid ? (double)(lse - row[(int)(valid ? lab : 0)]) : (double)nanv;
    for (int k = 0; k < c; ++k) {
      const float p = expf(row[k] - mx) / se;
      row[k] = valid ? (p - ((int64_t)k == lab ? 1.f : 0.f)) * inv_n : nanv;
    }
  }
  red[t] = lsum;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int r = 0; r < CL_NT; ++r) tot += red[r];  // thread order
    A.loss_out[0] = (float)(tot / (double)n);
  }
  // db2[k] = sum_i dlogits[i][k]: 8 row classes per k, folded in order
  {
    const int k = t % CL_MAXC, pr = t / CL_MAXC;
    float acc = 0.f;
    if (k < c)
      for (int i = pr; i < n; i += CL_NT / CL_MAXC) acc += W.dl[(size_t)i * c + k];
    b2r[pr * CL_MAXC + k] = acc;
    __syncthreads();
    if (t < c) {
      float g = 0.f;
      for (int r = 0; r < CL_NT / CL_MAXC; ++r) g += b2r[r * CL_MAXC + t];
      A.G.b2[t] = g;
    }
  }
}

// ---------------------------------------------------------------- launch 2: backward of each slab
__global__ __launch_bounds__(CL_NT) void cls_bwd_kernel(const ClsArgs A) {
  __shared__ float dls[CL_TR * CL_CP];
  __shared__ float hs[CL_TR * CL_SP];
  __shared__ float w2s[CL_MAXC * CL_SP];
  __shared__ double red[2 * CL_TR * CL_S];
  __shared__ double cdb[CL_S], cdg[CL_S];
  __shared__ float cgam[CL_S], cbet[CL_S], cistd[CL_S];
  const cv_cls& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x, j0 = slab * CL_S;
  const int n = A.n, h = P.h, c = P.c;
  const int hp = gridDim.x * CL_S;
  const ClsWork W = cls_work(A.work, n, h, c);
  for (int idx = t; idx < c * CL_S; idx += CL_NT) {
    const int k = idx / CL_S, j = idx % CL_S;
    w2s[k * CL_SP + j] = j0 + j < h ? P.w2[(size_t)k * h + j0 + j] : 0.f;
  }
  if (t < CL_S) {
    const bool ok = j0 + t < h;
    cgam[t] = ok ? P.gamma[j0 + t] : 0.f;
    cbet[t] = ok ? P.beta[j0 + t] : 0.f;
    cistd[t] = W.istd[j0 + t];
  }
  __syncthreads();

  // pass A: dy = dlogits W2[:,slab], the mask, dbeta / dgamma (fp64), dW2[:,slab]  (thread = 1 row x 4 columns)
  const int r = t >> 2, cq = (t & 3) * 4;
  double dbs[4] = {0.0, 0.0, 0.0, 0.0}, dgs[4] = {0.0, 0.0, 0.0, 0.0};
  float acc2[2] = {0.f, 0.f};
  for (int i0 = 0; i0 < n; i0 += CL_TR) {
    for (int idx = t; idx < CL_TR * c; idx += CL_NT) {
      const int rr = idx / c, k = idx - rr * c, i = i0 + rr;
      dls[rr * CL_CP + k] = i < n ? W.dl[(size_t)i * c + k] : 0.f;
    }
    __syncthreads();
    const int i = i0 + r;
    float4 hv4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
      const float4 xh4 = *reinterpret_cast<const float4*>(W.xhat + (size_t)i * hp + j0 + cq);
      const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w};
      float dy[4] = {0.f, 0.f, 0.f, 0.f}, hv[4];
      for (int k = 0; k < c; ++k) {
        const float g = dls[r * CL_CP + k];
#pragma unroll
        for (int u = 0; u < 4; ++u) dy[u] = fmaf(g, w2s[k * CL_SP + cq + u], dy[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float pre = cl_pre(cgam[cq + u], xh[u], cbet[cq + u]);
        hv[u] = fmaxf(pre, 0.f);
        dy[u] = pre > 0.f ? dy[u] : 0.f;
        dbs[u] += (double)dy[u];
        dgs[u] += (double)dy[u] * (double)xh[u];
      }
      *reinterpret_cast<float4*>(W.dym + (size_t)i * hp + j0 + cq) = make_float4(dy[0], dy[1], dy[2], dy[3]);
      hv4 = make_float4(hv[0], hv[1], hv[2], hv[3]);
    }
    hs[r * CL_SP + cq + 0] = hv4.x;
    hs[r * CL_SP + cq + 1] = hv4.y;
    hs[r * CL_SP + cq + 2] = hv4.z;
    hs[r * CL_SP + cq + 3] = hv4.w;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = t + CL_NT * u;
      if (o < c * CL_S) {
        const int k = o / CL_S, j = o % CL_S;
        float a2 = acc2[u];
#pragma unroll 8  // (rows in order)
        for (int rr = 0; rr < CL_TR; ++rr) a2 = fmaf(dls[rr * CL_CP + k], hs[rr * CL_SP + j], a2);
        acc2[u] = a2;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    red[r * CL_S + cq + u] = dbs[u];
    red[CL_TR * CL_S + r * CL_S + cq + u] = dgs[u];
  }
  __syncthreads();
  if (t < CL_S) {
    double sb = 0.0, sg = 0.0;
    for (int rr = 0; rr < CL_TR; ++rr) {  // row lanes in order
      sb += red[rr * CL_S + t];
      sg += red[CL_TR * CL_S + rr * CL_S + t];
    }
    cdb[t] = sb / (double)n;
    cdg[t] = sg / (double)n;
    if (j0 + t < h) {
      A.G.beta[j0 + t] = (float)sb;
      A.G.gamma[j0 + t] = (float)sg;
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int o = t + CL_NT * u;
    if (o < c * CL_S) {
      const int k = o / CL_S, j = o % CL_S;
      if (j0 + j < h) A.G.w2[(size_t)k * h + j0 + j] = acc2[u];
    }
  }
  __syncthreads();

  // pass B: da = gamma istd (dy - mean(dy) - xhat mean(dy xhat))
  for (int i = r; i < n; i += CL_TR) {
    const float4 xh4 = *reinterpret_cast<const float4*>(W.xhat + (size_t)i * hp + j0 + cq);
    const float4 dy4 = *reinterpret_cast<const float4*>(W.dym + (size_t)i * hp + j0 + cq);
    const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w}, dy[4] = {dy4.x, dy4.y, dy4.z, dy4.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float v = (float)((double)(cgam[cq + u] * cistd[cq + u]) *
                              ((double)dy[u] - cdb[cq + u] - (double)xh[u] * cdg[cq + u]));
      if (j0 + cq + u < h) A.da[(size_t)i * h + j0 + cq + u] = v;
    }
  }
}

// ---------------------------------------------------------------- eval forward (running statistics), one launch
__global__ __launch_bounds__(CL_NT) void cls_eval_kernel(const cv_cls P, const float* a, int n, float* logits) {
  __shared__ float hs[CL_ER * CL_MAXH];
  const int t = threadIdx.x, i0 = blockIdx.x * CL_ER;
  const int h = P.h, c = P.c;
  for (int j = t; j < h; j += CL_NT) {
    const float mu = P.running_mean[j];
    const float istd = (float)(1.0 / sqrt((double)P.running_var[j] + (double)P.eps));
    const float sc = P.gamma[j] * istd, be = P.beta[j];
#pragma unroll
    for (int r = 0; r < CL_ER; ++r) {
      const int i = i0 + r;
      const float av = i < n ? a[(size_t)i * h + j] : 0.f;
      hs[r * CL_MAXH + j] = fmaxf(fmaf(av - mu, sc, be), 0.f);
    }
  }
  __syncthreads();
  const int r = t / CL_MAXC, k = t % CL_MAXC, i = i0 + r;
  if (k < c && i < n) {
    const float* wr = P.w2 + (size_t)k * h;
    float acc = P.b2[k];
    for (int j = 0; j < h; ++j) acc = fmaf(hs[r * CL_MAXH + j], wr[j], acc);
    logits[(size_t)i * c + k] = acc;
  }
}

}  // namespace cv

using namespace cv;

extern "C" int cv_cls_supported(int n, int h, int c) {
  return n >= 2 && n <= CL_MAXN && h >= 1 && h <= CL_MAXH && c >= 2 && c <= CL_MAXC;
}

extern "C" size_t cv_cls_workspace_bytes(int n, int h, int c) {
  if (n < 1 || h < 1 || c < 1) return 0;
  return cls_work_bytes(n, h, c);
}

static int check_cls(const cv_cls* P, const char* who) {
  CV_REQUIRE(P && P->gamma && P->beta && P->w2 && P->b2 && P->running_mean && P->running_var,
             "%s: classifier weights or running statistics missing", who);
  return 0;
}

extern "C" int cv_cls_step(const cv_cls* P, const float* a, const int64_t* label, int n, void* work, float* loss_out,
                           float* da, const cv_cls_grad* g, cv_stream_t stream) {
  clear_error();
  if (check_cls(P, "cls_step")) return 1;
  CV_REQUIRE(cv_cls_supported(n, P->h, P->c),
             "cls_step: unsupported shape n=%d h=%d c=%d (2 <= n <= %d, 1 <= h <= %d, 2 <= c <= %d)", n, P->h, P->c,
             CL_MAXN, CL_MAXH, CL_MAXC);
  CV_REQUIRE(a && label && work && loss_out && da, "cls_step: a, label, work, loss_out or da missing");
  CV_REQUIRE((uintptr_t)work % 16 == 0, "cls_step: work must be 16-byte aligned");
  CV_REQUIRE(g && g->gamma && g->beta && g->w2 && g->b2, "cls_step: gradient buffers missing");
  ClsArgs A;
  memset(&A, 0, sizeof(A));
  A.P = *P;
  A.a = a; A.label = label; A.n = n;
  A.work = work;
  A.loss_out = loss_out;
  A.da = da;
  A.G = *g;
  const int nslab = cl_slabs(P->h);
  hipLaunchKernelGGL(cls_fwd_kernel, dim3(nslab), dim3(CL_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("cls_step.forward");
  hipLaunchKernelGGL(cls_bwd_kernel, dim3(nslab), dim3(CL_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("cls_step.backward");
  return 0;
}

extern "C" int cv_cls_forward(const cv_cls* P, const float* a, int n, float* logits, cv_stream_t stream) {
  clear_error();
  if (check_cls(P, "cls_forward")) return 1;
  CV_REQUIRE(n >= 1 && cv_cls_supported(2, P->h, P->c),
             "cls_forward: unsupported shape n=%d h=%d c=%d (n >= 1, 1 <= h <= %d, 2 <= c <= %d)", n, P->h, P->c, CL_MAXH,
             CL_MAXC);
  CV_REQUIRE(a && logits, "cls_forward: a or logits missing");
  hipLaunchKernelGGL(cls_eval_kernel, dim3(cdiv(n, CL_ER)), dim3(CL_NT), 0, S(stream), *P, a, n, logits);
  CV_LAUNCH_CHECK("cls_forward");
  return 0;
}
