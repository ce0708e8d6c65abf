// Downstream probe (run_styledmnist_downstream_expr.py:110-117, trainer.py:125-131): Linear(d,h) -> BatchNorm1d(h)
// -> ReLU -> Linear(h,c) with nn.CrossEntropyLoss() defaults, on mu_c of the frozen VAE.  One training step (loss,
// gradients, running statistics, Adam) in two launches; the eval forward in one.
//
// The hidden features are independent through the BatchNorm (its statistics are per column), so a workgroup owns a
// slab of PB_S hidden columns for all n rows: a[:,slab], its statistics, h[:,slab], dgamma / dbeta[slab],
// dW1[slab,:], dW2[:,slab] and dh[:,slab] = dlogits W2[:,slab] are slab-local.  The only cross-workgroup quantity is
// logits (and dlogits):
//   launch 1 (probe_fwd_kernel)  per slab: a = x W1^T + b1, fp64 column sums, xhat (kept in the workspace), running
//                                statistics, the slab's partial logits; the last-arriving workgroup folds the partials
//                                in slab order, adds b2 and computes the loss, dlogits = (softmax - onehot)/n and db2
//   launch 2 (probe_bwd_kernel)  per slab: dh, the ReLU mask, dbeta / dgamma (fp64 sums), dW2[:,slab], da, dW1[slab,:],
//                                db1 = 0, and Adam on the parameters the slab owns (slab 0 also b2; the arena's padding
//                                words are shared out by index); the last arriver advances step[0]
// No workgroup waits for another; every sum has a fixed order (no floating-point atomics): the same state and batch
// give the same bits, eager or replayed.
#include "cv_common.hpp"

namespace cv {

constexpr int PB_S = 16;    // hidden columns per workgroup
constexpr int PB_TR = 64;   // rows per tile
constexpr int PB_NT = 256;  // threads per workgroup
constexpr int PB_MAXD = 64, PB_MAXH = 512, PB_MAXC = 32, PB_MAXN = 1024;
constexpr int PB_XP = PB_MAXD + 1;  // largest pitch of a staged x / W1 row (d | 1: odd, so columns spread over banks)
constexpr int PB_SP = PB_S + 1;     // pitch of a slab-wide LDS row
constexpr int PB_CP = PB_MAXC + 1;  // pitch of a staged dlogits row
constexpr int PB_ER = 8;            // rows per workgroup of the eval forward

struct ProbeWork {
  unsigned* ticket;  // [0] launch 1, [1] launch 2 (self-resetting)
  float* istd;       // [hp]
  float* xhat;       // [n][hp]  (a, then xhat)
  float* dhm;        // [n][hp]  masked dh
  float* part;       // [slabs][n*c] partial logits
  float* dl;         // [n*c] logits, then dlogits
};
__host__ __device__ inline size_t pb_r16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline int pb_slabs(int h) { return (h + PB_S - 1) / PB_S; }
__host__ __device__ inline size_t probe_work_bytes(int n, int h, int c) {
  const size_t hp = (size_t)pb_slabs(h) * PB_S;
  return 64 + pb_r16(hp * 4) + 2 * pb_r16((size_t)n * hp * 4) + pb_r16((size_t)pb_slabs(h) * n * c * 4) +
         pb_r16((size_t)n * c * 4);
}
__host__ __device__ inline ProbeWork probe_work(void* base, int n, int h, int c) {
  const size_t hp = (size_t)pb_slabs(h) * PB_S;
  char* p = (char*)base;
  ProbeWork w;
  w.ticket = (unsigned*)p;
  p += 64;
  w.istd = (float*)p;
  p += pb_r16(hp * 4);
  w.xhat = (float*)p;
  p += pb_r16((size_t)n * hp * 4);
  w.dhm = (float*)p;
  p += pb_r16((size_t)n * hp * 4);
  w.part = (float*)p;
  p += pb_r16((size_t)pb_slabs(h) * n * c * 4);
  w.dl = (float*)p;
  return w;
}

struct ProbeArgs {
  cv_probe P;
  const float* x; int ldx;
  const int64_t* label;
  int n;
  void* work;
  float* loss_out;
  cv_probe_grad G;
  // Adam (optional): flat arena
  float* params; const float* grads; float* m; float* v; long numel;
  const float* hyper; int64_t* step;
};

// last-arriving workgroup detection (the form of cv_mi.hip last_block): every thread drains its stores, thread 0
// releases at agent scope and takes a ticket; the last one acquires before the barrier that publishes the verdict
// and resets the ticket for the next call
__device__ __forceinline__ bool pb_last_block(unsigned* ticket, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = prev == gridDim.x - 1;
    *flag = last ? 1 : 0;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return *flag != 0;
}

// the BatchNorm output before the ReLU; the backward's mask is the sign of the same expression on the same bits
__device__ __forceinline__ float pb_pre(float gamma, float xhat, float beta) { return fmaf(gamma, xhat, beta); }

// rows [i0, i0 + PB_TR) of x into LDS with pitch dp (rows past n as zeros); rows of x may start at any 4-byte boundary
__device__ __forceinline__ void pb_stage_x(float* xs, const float* x, int ldx, int d, int dp, int i0, int n) {
  for (int idx = threadIdx.x; idx < PB_TR * d; idx += PB_NT) {
    const int r = idx / d, k = idx - r * d, i = i0 + r;
    xs[r * dp + k] = i < n ? x[(size_t)i * ldx + k] : 0.f;
  }
}

// ---------------------------------------------------------------- launch 1: forward of each slab, loss by the last
__global__ __launch_bounds__(PB_NT) void probe_fwd_kernel(const ProbeArgs A) {
  __shared__ float w1s[PB_S * PB_XP];
  __shared__ float xs[PB_TR * PB_XP];
  __shared__ float hs[PB_TR * PB_SP];
  __shared__ float w2s[PB_MAXC * PB_SP];
  __shared__ double red[2 * PB_NT];
  __shared__ double cmean[PB_S], cistd[PB_S];
  __shared__ float cb1[PB_S], cgam[PB_S], cbet[PB_S];
  __shared__ int flag;
  const cv_probe& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x, j0 = slab * PB_S;
  const int n = A.n, d = P.d, h = P.h, c = P.c, dp = d | 1;
  const int hp = gridDim.x * PB_S;
  const ProbeWork W = probe_work(A.work, n, h, c);

  for (int idx = t; idx < PB_S * d; idx += PB_NT) {
    const int j = idx / d, k = idx - j * d;
    w1s[j * dp + k] = j0 + j < h ? P.w1[(size_t)(j0 + j) * d + k] : 0.f;
  }
  for (int idx = t; idx < c * PB_S; idx += PB_NT) {
    const int k = idx / PB_S, j = idx % PB_S;
    w2s[k * PB_SP + j] = j0 + j < h ? P.w2[(size_t)k * h + j0 + j] : 0.f;
  }
  if (t < PB_S) {
    const bool ok = j0 + t < h;
    cb1[t] = ok ? P.b1[j0 + t] : 0.f;
    cgam[t] = ok ? P.gamma[j0 + t] : 0.f;
    cbet[t] = ok ? P.beta[j0 + t] : 0.f;
  }

  // pass 1: a = x W1^T + b1 for the slab (thread = 4 rows of a tile x 1 column), fp64 column sums
  const int col = t % PB_S, rl = t / PB_S;
  double s = 0.0, q = 0.0;
  for (int i0 = 0; i0 < n; i0 += PB_TR) {
    __syncthreads();
    pb_stage_x(xs, A.x, A.ldx, d, dp, i0, n);
    __syncthreads();
    float acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = cb1[col];
    for (int k = 0; k < d; ++k) {
      const float w = w1s[col * dp + k];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(xs[(rl + 16 * u) * dp + k], w, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + rl + 16 * u;
      if (i < n) {
        W.xhat[(size_t)i * hp + j0 + col] = acc[u];
        s += (double)acc[u];
        q += (double)acc[u] * (double)acc[u];
      }
    }
  }
  red[t] = s;
  red[PB_NT + t] = q;
  __syncthreads();
  if (t < PB_S) {
    double ss = 0.0, qq = 0.0;
    for (int r = 0; r < PB_NT / PB_S; ++r) {  // row lanes in order
      ss += red[r * PB_S + t];
      qq += red[PB_NT + r * PB_S + t];
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

  // pass 2: xhat, h = relu(gamma xhat + beta), the slab's partial logits (thread = 1 row x every 4th class)
  {
    const double mean = cmean[col], istd = cistd[col];
    const float gam = cgam[col], bet = cbet[col];
    for (int i0 = 0; i0 < n; i0 += PB_TR) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = rl + 16 * u, i = i0 + r;
        float hv = 0.f;
        if (i < n) {
          float* px = W.xhat + (size_t)i * hp + j0 + col;  // (this thread's own store of pass 1)
          const float xh = (float)(((double)*px - mean) * istd);
          *px = xh;
          hv = fmaxf(pb_pre(gam, xh, bet), 0.f);
        }
        hs[r * PB_SP + col] = hv;
      }
      __syncthreads();
      const int r = t >> 2, i = i0 + r;
      if (i < n) {
        float* dst = W.part + (size_t)slab * n * c + (size_t)i * c;
        for (int k = t & 3; k < c; k += 4) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < PB_S; ++j) acc = fmaf(hs[r * PB_SP + j], w2s[k * PB_SP + j], acc);
          dst[k] = acc;
        }
      }
      __syncthreads();
    }
  }

  if (!pb_last_block(W.ticket, &flag)) return;
  // the last arriver: logits = b2 + partials in slab order
  const int nslab = gridDim.x, nc = n * c;
  for (int e = t; e < nc; e += PB_NT) {
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
  for (int i = t; i < n; i += PB_NT) {
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
    for (int r = 0; r < PB_NT; ++r) tot += red[r];  // thread order
    A.loss_out[0] = (float)(tot / (double)n);
  }
  // db2[k] = sum_i dlogits[i][k]: 8 row classes per k, folded in order
  {
    const int k = t % PB_MAXC, pr = t / PB_MAXC;
    float acc = 0.f;
    if (k < c)
      for (int i = pr; i < n; i += PB_NT / PB_MAXC) acc += W.dl[(size_t)i * c + k];
    xs[pr * PB_MAXC + k] = acc;
    __syncthreads();
    if (t < c) {
      float g = 0.f;
      for (int r = 0; r < PB_NT / PB_MAXC; ++r) g += xs[r * PB_MAXC + t];
      A.G.b2[t] = g;
    }
  }
}

// ---------------------------------------------------------------- launch 2: backward of each slab, Adam
struct PbAdam {
  float step_size, bc2s, omb1, omb2, b2f, eps, wd;
};

// torch.optim.Adam (foreach) on arena word i with gradient g (the arithmetic of adam_kernel, cv_mi.hip)
__device__ __forceinline__ void pb_adam(const ProbeArgs& A, const PbAdam& K, long i, float g) {
  const float p = A.params[i];
  if (K.wd != 0.f) g = g + K.wd * p;
  float m = A.m[i];
  m = m + K.omb1 * (g - m);
  float v = A.v[i] * K.b2f;
  v = v + K.omb2 * g * g;
  A.m[i] = m;
  A.v[i] = v;
  const float den = sqrtf(v) / K.bc2s + K.eps;
  A.params[i] = p + K.step_size * (m / den);
}

__global__ __launch_bounds__(PB_NT) void probe_bwd_kernel(const ProbeArgs A) {
  __shared__ float xs[PB_TR * PB_XP];
  __shared__ float dls[PB_TR * PB_CP];
  __shared__ float hs[PB_TR * PB_SP];
  __shared__ float w2s[PB_MAXC * PB_SP];
  __shared__ double red[2 * PB_TR * PB_S];
  __shared__ double cdb[PB_S], cdg[PB_S];
  __shared__ float cgam[PB_S], cbet[PB_S], cistd[PB_S];
  __shared__ float cst[8];
  __shared__ long s_step;
  __shared__ int flag;
  const cv_probe& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x, j0 = slab * PB_S;
  const int n = A.n, d = P.d, h = P.h, c = P.c, dp = d | 1;
  const int hp = gridDim.x * PB_S;
  const ProbeWork W = probe_work(A.work, n, h, c);
  const bool adam = A.params != nullptr;
  if (adam && t == 0) {  // the bias corrections of this launch's own t (read on the device: replays advance)
    const long t_step = A.step[0] + 1;
    const double b1 = A.hyper[1], b2 = A.hyper[2];
    const double bc1 = 1.0 - pow(b1, (double)t_step);
    const double bc2 = 1.0 - pow(b2, (double)t_step);
    cst[0] = (float)(-(double)A.hyper[0] / bc1);
    cst[1] = (float)sqrt(bc2);
    cst[2] = (float)(1.0 - b1);
    cst[3] = (float)(1.0 - b2);
    cst[4] = A.hyper[2];
    cst[5] = A.hyper[3];
    cst[6] = A.hyper[4];
    s_step = t_step;
  }
  for (int idx = t; idx < c * PB_S; idx += PB_NT) {
    const int k = idx / PB_S, j = idx % PB_S;
    w2s[k * PB_SP + j] = j0 + j < h ? P.w2[(size_t)k * h + j0 + j] : 0.f;
  }
  if (t < PB_S) {
    const bool ok = j0 + t < h;
    cgam[t] = ok ? P.gamma[j0 + t] : 0.f;
    cbet[t] = ok ? P.beta[j0 + t] : 0.f;
    cistd[t] = W.istd[j0 + t];
  }
  __syncthreads();
  PbAdam K;
  K.step_size = cst[0]; K.bc2s = cst[1]; K.omb1 = cst[2]; K.omb2 = cst[3]; K.b2f = cst[4]; K.eps = cst[5];
  K.wd = cst[6];
  // arena word of element e of a gradient buffer (with Adam the buffers live in the grads arena)
  auto word = [&](const float* gbuf, long e) -> long { return (long)(gbuf - A.grads) + e; };

  // pass A: dh = dlogits W2[:,slab], the mask, dbeta / dgamma (fp64), dW2[:,slab]  (thread = 1 row x 4 columns)
  const int r = t >> 2, cq = (t & 3) * 4;
  double dbs[4] = {0.0, 0.0, 0.0, 0.0}, dgs[4] = {0.0, 0.0, 0.0, 0.0};
  float acc2[2] = {0.f, 0.f};
  for (int i0 = 0; i0 < n; i0 += PB_TR) {
    for (int idx = t; idx < PB_TR * c; idx += PB_NT) {
      const int rr = idx / c, k = idx - rr * c, i = i0 + rr;
      dls[rr * PB_CP + k] = i < n ? W.dl[(size_t)i * c + k] : 0.f;
    }
    __syncthreads();
    const int i = i0 + r;
    float4 hv4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
      const float4 xh4 = *reinterpret_cast<const float4*>(W.xhat + (size_t)i * hp + j0 + cq);
      const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w};
      float dh[4] = {0.f, 0.f, 0.f, 0.f}, hv[4];
      for (int k = 0; k < c; ++k) {
        const float g = dls[r * PB_CP + k];
#pragma unroll
        for (int u = 0; u < 4; ++u) dh[u] = fmaf(g, w2s[k * PB_SP + cq + u], dh[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float pre = pb_pre(cgam[cq + u], xh[u], cbet[cq + u]);
        hv[u] = fmaxf(pre, 0.f);
        dh[u] = pre > 0.f ? dh[u] : 0.f;
        dbs[u] += (double)dh[u];
        dgs[u] += (double)dh[u] * (double)xh[u];
      }
      *reinterpret_cast<float4*>(W.dhm + (size_t)i * hp + j0 + cq) = make_float4(dh[0], dh[1], dh[2], dh[3]);
      hv4 = make_float4(hv[0], hv[1], hv[2], hv[3]);
    }
    hs[r * PB_SP + cq + 0] = hv4.x;
    hs[r * PB_SP + cq + 1] = hv4.y;
    hs[r * PB_SP + cq + 2] = hv4.z;
    hs[r * PB_SP + cq + 3] = hv4.w;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = t + PB_NT * u;
      if (o < c * PB_S) {
        const int k = o / PB_S, j = o % PB_S;
        float a2 = acc2[u];
#pragma unroll 8  // (rows in order; unrolled whole, the kernel ran out of registers)
        for (int rr = 0; rr < PB_TR; ++rr) a2 = fmaf(dls[rr * PB_CP + k], hs[rr * PB_SP + j], a2);
        acc2[u] = a2;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    red[r * PB_S + cq + u] = dbs[u];
    red[PB_TR * PB_S + r * PB_S + cq + u] = dgs[u];
  }
  __syncthreads();
  if (t < PB_S) {
    double sb = 0.0, sg = 0.0;
    for (int rr = 0; rr < PB_TR; ++rr) {  // row lanes in order
      sb += red[rr * PB_S + t];
      sg += red[PB_TR * PB_S + rr * PB_S + t];
    }
    cdb[t] = sb / (double)n;
    cdg[t] = sg / (double)n;
    if (j0 + t < h) {
      A.G.beta[j0 + t] = (float)sb;
      A.G.gamma[j0 + t] = (float)sg;
      A.G.b1[j0 + t] = 0.f;  // the bias feeds a train-mode BatchNorm: its gradient is exactly zero
      if (adam) {
        pb_adam(A, K, word(A.G.beta, j0 + t), (float)sb);
        pb_adam(A, K, word(A.G.gamma, j0 + t), (float)sg);
        pb_adam(A, K, word(A.G.b1, j0 + t), 0.f);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int o = t + PB_NT * u;
    if (o < c * PB_S) {
      const int k = o / PB_S, j = o % PB_S;
      if (j0 + j < h) {
        const long e = (long)k * h + j0 + j;
        A.G.w2[e] = acc2[u];
        if (adam) pb_adam(A, K, word(A.G.w2, e), acc2[u]);
      }
    }
  }
  __syncthreads();

  // pass B: da = gamma istd (dh - mean(dh) - xhat mean(dh xhat)), dW1[slab,:] = da^T x
  float acc1[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < n; i0 += PB_TR) {
    pb_stage_x(xs, A.x, A.ldx, d, dp, i0, n);
    const int i = i0 + r;
    float da[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      const float4 xh4 = *reinterpret_cast<const float4*>(W.xhat + (size_t)i * hp + j0 + cq);
      const float4 dh4 = *reinterpret_cast<const float4*>(W.dhm + (size_t)i * hp + j0 + cq);
      const float xh[4] = {xh4.x, xh4.y, xh4.z, xh4.w}, dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        da[u] = (float)((double)(cgam[cq + u] * cistd[cq + u]) *
                        ((double)dh[u] - cdb[cq + u] - (double)xh[u] * cdg[cq + u]));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) hs[r * PB_SP + cq + u] = da[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = t + PB_NT * u;
      if (o < PB_S * d) {
        const int j = o / d, k = o - j * d;
        float a1 = acc1[u];
#pragma unroll 8  // (rows in order)
        for (int rr = 0; rr < PB_TR; ++rr) a1 = fmaf(hs[rr * PB_SP + j], xs[rr * dp + k], a1);
        acc1[u] = a1;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = t + PB_NT * u;
    if (o < PB_S * d) {
      const int j = o / d, k = o - j * d;
      if (j0 + j < h) {
        const long e = (long)(j0 + j) * d + k;
        A.G.w1[e] = acc1[u];
        if (adam) pb_adam(A, K, word(A.G.w1, e), acc1[u]);
      }
    }
  }
  if (!adam) return;
  // b2 (its gradient came from launch 1) belongs to slab 0
  if (slab == 0 && t < c) pb_adam(A, K, word(A.G.b2, t), A.G.b2[t]);
  // the arena words outside the six gradient buffers (padding), shared out by index, with the gradient found there
  {
    const float* seg[6] = {A.G.w1, A.G.b1, A.G.gamma, A.G.beta, A.G.w2, A.G.b2};
    const long len[6] = {(long)h * d, h, h, h, (long)c * h, c};
    for (long i = (long)slab * PB_NT + t; i < A.numel; i += (long)gridDim.x * PB_NT) {
      const float* p = A.grads + i;
      bool owned = false;
#pragma unroll
      for (int sgi = 0; sgi < 6; ++sgi) owned = owned || (p >= seg[sgi] && p < seg[sgi] + len[sgi]);
      if (!owned) pb_adam(A, K, i, A.grads[i]);
    }
  }
  // every workgroup read the step counter before taking its ticket: the last one advances it
  if (pb_last_block(W.ticket + 1, &flag) && t == 0) A.step[0] = s_step;
}

// ---------------------------------------------------------------- eval forward (running statistics), one launch
__global__ __launch_bounds__(PB_NT) void probe_eval_kernel(const cv_probe P, const float* x, int ldx, int n,
                                                           float* logits) {
  __shared__ float xs[PB_ER * PB_MAXD];
  __shared__ float hs[PB_ER * PB_MAXH];
  const int t = threadIdx.x, i0 = blockIdx.x * PB_ER;
  const int d = P.d, h = P.h, c = P.c;
  for (int idx = t; idx < PB_ER * d; idx += PB_NT) {
    const int r = idx / d, k = idx - r * d, i = i0 + r;
    xs[r * d + k] = i < n ? x[(size_t)i * ldx + k] : 0.f;
  }
  __syncthreads();
  for (int j = t; j < h; j += PB_NT) {
    const float mu = P.running_mean[j];
    const float istd = (float)(1.0 / sqrt((double)P.running_var[j] + (double)P.eps));
    const float sc = P.gamma[j] * istd, be = P.beta[j], b = P.b1[j];
    const float* wr = P.w1 + (size_t)j * d;
    float acc[PB_ER];
#pragma unroll
    for (int r = 0; r < PB_ER; ++r) acc[r] = b;
    for (int k = 0; k < d; ++k) {
      const float w = wr[k];
#pragma unroll
      for (int r = 0; r < PB_ER; ++r) acc[r] = fmaf(xs[r * d + k], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < PB_ER; ++r) hs[r * PB_MAXH + j] = fmaxf(fmaf(acc[r] - mu, sc, be), 0.f);
  }
  __syncthreads();
  const int r = t / PB_MAXC, k = t % PB_MAXC, i = i0 + r;
  if (k < c && i < n) {
    const float* wr = P.w2 + (size_t)k * h;
    float acc = P.b2[k];
    for (int j = 0; j < h; ++j) acc = fmaf(hs[r * PB_MAXH + j], wr[j], acc);
    logits[(size_t)i * c + k] = acc;
  }
}

}  // namespace cv

using namespace cv;

extern "C" int cv_probe_supported(int n, int d, int h, int c) {
  return n >= 2 && n <= PB_MAXN && d >= 1 && d <= PB_MAXD && h >= 1 && h <= PB_MAXH && c >= 2 && c <= PB_MAXC;
}

extern "C" size_t cv_probe_workspace_bytes(int n, int h, int c) {
  if (n < 1 || h < 1 || c < 1) return 0;
  return probe_work_bytes(n, h, c);
}

static int check_probe(const cv_probe* P, const char* who) {
  CV_REQUIRE(P && P->w1 && P->b1 && P->gamma && P->beta && P->w2 && P->b2 && P->running_mean && P->running_var,
             "%s: probe weights or running statistics missing", who);
  return 0;
}

extern "C" int cv_probe_step(const cv_probe* P, const float* x, int ldx, const int64_t* label, int n, void* work,
                             float* loss_out, const cv_probe_grad* g, float* params, const float* grads,
                             float* exp_avg, float* exp_avg_sq, int64_t numel, const float* hyper, int64_t* step,
                             cv_stream_t stream) {
  clear_error();
  if (check_probe(P, "probe_step")) return 1;
  CV_REQUIRE(cv_probe_supported(n, P->d, P->h, P->c),
             "probe_step: unsupported shape n=%d d=%d h=%d c=%d (2 <= n <= %d, d <= %d, h <= %d, 2 <= c <= %d)", n,
             P->d, P->h, P->c, PB_MAXN, PB_MAXD, PB_MAXH, PB_MAXC);
  CV_REQUIRE(x && label && work && loss_out, "probe_step: x, label, work or loss_out missing");
  CV_REQUIRE((uintptr_t)work % 16 == 0, "probe_step: work must be 16-byte aligned");
  CV_REQUIRE(g && g->w1 && g->b1 && g->gamma && g->beta && g->w2 && g->b2, "probe_step: gradient buffers missing");
  CV_REQUIRE(ldx >= P->d, "probe_step: ldx=%d < d=%d", ldx, P->d);
  const int d = P->d, h = P->h, c = P->c;
  if (params) {
    CV_REQUIRE(grads && exp_avg && exp_avg_sq && hyper && step && numel > 0, "probe_step: Adam arena incomplete");
    float* const gp[6] = {g->w1, g->b1, g->gamma, g->beta, g->w2, g->b2};
    const float* const pp[6] = {P->w1, P->b1, P->gamma, P->beta, P->w2, P->b2};
    const long ln[6] = {(long)h * d, h, h, h, (long)c * h, c};
    for (int s = 0; s < 6; ++s) {
      CV_REQUIRE(gp[s] >= grads && gp[s] + ln[s] <= grads + numel,
                 "probe_step: with Adam the gradients must live in the grads arena");
      CV_REQUIRE(pp[s] == params + (gp[s] - grads),
                 "probe_step: with Adam each parameter sits in params where its gradient sits in grads");
    }
  }
  ProbeArgs a;
  memset(&a, 0, sizeof(a));
  a.P = *P;
  a.x = x; a.ldx = ldx; a.label = label; a.n = n;
  a.work = work;
  a.loss_out = loss_out;
  a.G = *g;
  a.params = params; a.grads = grads; a.m = exp_avg; a.v = exp_avg_sq; a.numel = (long)numel;
  a.hyper = hyper; a.step = step;
  const int nslab = pb_slabs(h);
  hipLaunchKernelGGL(probe_fwd_kernel, dim3(nslab), dim3(PB_NT), 0, S(stream), a);
  CV_LAUNCH_CHECK("probe_step.forward");
  hipLaunchKernelGGL(probe_bwd_kernel, dim3(nslab), dim3(PB_NT), 0, S(stream), a);
  CV_LAUNCH_CHECK("probe_step.backward");
  return 0;
}

extern "C" int cv_probe_forward(const cv_probe* P, const float* x, int ldx, int n, float* logits,
                                cv_stream_t stream) {
  clear_error();
  if (check_probe(P, "probe_forward")) return 1;
  CV_REQUIRE(n >= 1 && cv_probe_supported(n < 2 ? 2 : n, P->d, P->h, P->c),
             "probe_forward: unsupported shape n=%d d=%d h=%d c=%d", n, P->d, P->h, P->c);
  CV_REQUIRE(x && logits, "probe_forward: x or logits missing");
  CV_REQUIRE(ldx >= P->d, "probe_forward: ldx=%d < d=%d", ldx, P->d);
  hipLaunchKernelGGL(probe_eval_kernel, dim3(cdiv(n, PB_ER)), dim3(PB_NT), 0, S(stream), *P, x, ldx, n, logits);
  CV_LAUNCH_CHECK("probe_forward");
  return 0;
}
