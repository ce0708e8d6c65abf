// LAM baseline tail (code/src/models/cnn.py:57-66: cls_head = Linear(2048, c) on the flattened trunk; code/src/
// trainer.py:249-257 ss_pairing, :259-288 the training step; code/src/losses.py:173-187 lam_loss).  The reference
// step runs the trunk three times (cnn(X), cnn.net(X), cnn.net(X_tilde)); X_tilde = X[pair] for a permutation `pair`
// and a conv + train-mode-BatchNorm trunk is permutation-equivariant, so with h = ReLU(BN(y_last)) the step is one
// trunk forward, this tail, and one trunk backward with the summed upstream gradient:
//   logits = h W^T + b, ce = mean cross-entropy, dlogits = (softmax - onehot) / n
//   lam    = (1/n) sum_i sum_f ((h[i,f] - h[p_i,f]) W[y_i,f])^2                         (loss = ce + lambda lam)
//   gb[k]  = sum_i dlogits[i,k]
//   gW[k,f] = sum_i dlogits[i,k] h[i,f] + lambda (2/n) W[k,f] sum_{i: y_i = k} (h[i,f] - h[p_i,f])^2
//   dh[i,f] = sum_k dlogits[i,k] W[k,f]
//             + lambda (2/n) (W[y_i,f]^2 (h[i,f] - h[p_i,f]) - W[y_q,f]^2 (h[q,f] - h[i,f])),  q = pair^-1(i)
//   gin = dh [BN(y_last) > 0], and that BatchNorm2d's backward sums (sum dz, sum dz xhat) per channel.
//
// The slab decomposition of cv_cnn.hip, over channels: a workgroup owns whole channels (LM_S columns at most) for all
// n rows, so the BatchNorm constants, gstat, gW[:,slab], dh[:,slab] and the slab's share of lam are slab-local; only
// the logits cross slabs:
//   launch 1 (lam_fwd_kernel)  per slab: h, the slab's partial logits and its fp64 share of lam; the last-arriving
//                              workgroup folds the partials in slab order and computes ce, dlogits, gb and lam
//   launch 2 (lam_bwd_kernel)  per slab: dh, the ReLU mask, gin, the fp64 channel sums, gW[:,slab]
// Partner rows h[p_i], h[q_i] are recomputed from y (L2-resident).  No workgroup waits for another; every sum has a
// fixed order (no floating-point atomics): the same state and batch give the same bits, eager or replayed.
#include "cv_common.hpp"

namespace cv {

constexpr int LM_S = 16;    // columns per workgroup at most (whole channels: max(1, 16 / pix) of them)
constexpr int LM_TR = 64;   // rows per tile
constexpr int LM_NT = 256;  // threads per workgroup
constexpr int LM_MAXC = 32, LM_MAXN = 1024, LM_MAXF = 2048, LM_MAXPIX = 16;
constexpr int LM_SP = LM_S + 1;     // pitch of a slab-wide LDS row
constexpr int LM_CP = LM_MAXC + 1;  // pitch of a staged dlogits row
constexpr int LM_ER = 4;            // rows per workgroup of the eval forward (one wave each)

struct LamWork {
  unsigned* ticket;  // [0] launch 1 (self-resetting); the first 64 bytes of the workspace
  double* lampart;   // [slabs] each slab's share of sum_i sum_f (...)^2
  float* part;       // [slabs][n*c] partial logits
  float* dl;         // [n*c] logits, then dlogits
};
__host__ __device__ inline size_t lm_r16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline int lm_cs(int pix) { return pix >= LM_S ? 1 : LM_S / pix; }  // channels per slab
__host__ __device__ inline int lm_slabs(int ch, int pix) { return (ch + lm_cs(pix) - 1) / lm_cs(pix); }
__host__ __device__ inline size_t lam_work_bytes(int n, int ch, int pix, int c) {
  const size_t ns = (size_t)lm_slabs(ch, pix);
  return 64 + lm_r16(ns * 8) + lm_r16(ns * n * c * 4) + lm_r16((size_t)n * c * 4);
}
__host__ __device__ inline LamWork lam_work(void* base, int n, int ch, int pix, int c) {
  const size_t ns = (size_t)lm_slabs(ch, pix);
  char* p = (char*)base;
  LamWork w;
  w.ticket = (unsigned*)p;
  p += 64;
  w.lampart = (double*)p;
  p += lm_r16(ns * 8);
  w.part = (float*)p;
  p += lm_r16(ns * n * c * 4);
  w.dl = (float*)p;
  return w;
}

struct LamArgs {
  cv_lam P;
  const float* y;
  cv_bn bn;
  const int64_t* label;
  const int64_t* pair;
  int n;
  void* work;
  float* loss_out;
  float* gin;
  double* gstat_out;
  cv_lam_grad G;
};

// last-arriving workgroup detection (cv_cnn.hip's cl_last_block): every thread drains and releases its own global
// stores at agent scope, thread 0 takes a ticket; the last workgroup acquires before it reads the others' partials
// and resets the ticket for the next call
__device__ __forceinline__ bool lm_last_block(unsigned* ticket, int* flag) {
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

// The slab of workgroup `slab`: channels [c0, c0 + nch), local column j = cl * pix + p <-> storage column
// p * C + c0 + cl of y / gin and PyTorch feature (c0 + cl) * pix + p = c0 * pix + j of W (contiguous).  Fills the
// storage columns, the BatchNorm constants (finalised by the layer's producer, or folded from the replicas, as
// cv_heads_backward) and W[:,slab]; pad columns (j >= ncols) read column 0 and carry W = 0.  Ends with a barrier.
__device__ __forceinline__ int lm_setup(const cv_lam& P, const cv_bn& bn, int slab, int* gcol, BnFwdC* kf, float* ws) {
  const int t = threadIdx.x, C = P.in_ch, pix = P.in_pix, F = C * pix, cs = lm_cs(pix);
  const int c0 = slab * cs, nch = min(cs, C - c0), ncols = nch * pix;
  if (t < LM_S) {
    const bool ok = t < ncols;
    const int cl = ok ? t / pix : 0, p = ok ? t - cl * pix : 0, cc = c0 + cl;
    gcol[t] = ok ? p * C + cc : 0;
    if (bn.train && bn.cfwd && bn.ticket && bn.ticket[0] != 0u)
      kf[t] = BnFwdC{bn.cfwd[cc], bn.cfwd[C + cc], bn.cfwd[2 * C + cc], bn.cfwd[3 * C + cc]};
    else
      kf[t] = bn_fwd_const(bn, cc);
  }
  for (int idx = t; idx < P.c * LM_S; idx += LM_NT) {
    const int k = idx / LM_S, j = idx % LM_S;
    ws[k * LM_SP + j] = j < ncols ? P.w[(size_t)k * F + (size_t)c0 * pix + j] : 0.f;
  }
  __syncthreads();
  return ncols;
}

// q = pair^-1 in LDS: -1 where no in-range pair entry points (pair is then no permutation)
__device__ __forceinline__ void lm_inverse(const int64_t* pair, int n, int* qs) {
  const int t = threadIdx.x;
  for (int i = t; i < n; i += LM_NT) qs[i] = -1;
  __syncthreads();
  for (int i = t; i < n; i += LM_NT) {
    const int64_t p = pair[i];
    if (p >= 0 && p < (int64_t)n) qs[(int)p] = i;
  }
  __syncthreads();
}

// ---------------------------------------------------------------- launch 1: forward of each slab, losses by the last
__global__ __launch_bounds__(LM_NT) void lam_fwd_kernel(const LamArgs A) {
  __shared__ float hs[LM_TR * LM_SP];
  __shared__ float ws[LM_MAXC * LM_SP];
  __shared__ double red[LM_NT];
  __shared__ int gcol[LM_S];
  __shared__ BnFwdC kf[LM_S];
  __shared__ float gbr[(LM_NT / LM_MAXC) * LM_MAXC];
  __shared__ int qs[LM_MAXN];
  __shared__ int flag;
  const cv_lam& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x;
  const int n = A.n, c = P.c, F = P.in_ch * P.in_pix;
  const LamWork W = lam_work(A.work, n, P.in_ch, P.in_pix, c);
  const int ncols = lm_setup(P, A.bn, slab, gcol, kf, ws);
  const float nanv = __builtin_nanf("");

  // thread = 1 row x 4 columns: h, the partner's h, the slab's share of lam (fp64); then 1 row x every 4th class of
  // the partial logits
  const int r = t >> 2, cq = (t & 3) * 4;
  double lsum = 0.0;
  for (int i0 = 0; i0 < n; i0 += LM_TR) {
    const int i = i0 + r;
    float hv[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      const int64_t pi = A.pair[i], li = A.label[i];
      const bool ok = pi >= 0 && pi < (int64_t)n && li >= 0 && li < (int64_t)c;
      const int ip = ok ? (int)pi : i, lab = ok ? (int)li : 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = cq + u;
        if (j < ncols) {
          const float h = bn_relu(A.y[(size_t)i * F + gcol[j]], kf[j]);
          const float hp = bn_relu(A.y[(size_t)ip * F + gcol[j]], kf[j]);
          const float d = (h - hp) * ws[lab * LM_SP + j];
          hv[u] = h;
          lsum += (double)d * (double)d;
        }
      }
      if (!ok) lsum = (double)nanv;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) hs[r * LM_SP + cq + u] = hv[u];
    __syncthreads();
    if (i < n) {
      float* dst = W.part + (size_t)slab * n * c + (size_t)i * c;
      for (int k = t & 3; k < c; k += 4) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < LM_S; ++j) acc = fmaf(hs[r * LM_SP + j], ws[k * LM_SP + j], acc);
        dst[k] = acc;
      }
    }
    __syncthreads();
  }
  red[t] = lsum;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int q = 0; q < LM_NT; ++q) tot += red[q];  // thread order
    W.lampart[slab] = tot;
  }

  if (!lm_last_block(W.ticket, &flag)) return;
  // the last arriver: logits = b + partials in slab order
  const int nslab = gridDim.x, nc = n * c;
  for (int e = t; e < nc; e += LM_NT) {
    float v = P.b[e % c];
    const float* pp = W.part + e;
#pragma unroll 8
    for (int sidx = 0; sidx < nslab; ++sidx) v += pp[(size_t)sidx * nc];
    W.dl[e] = v;
  }
  lm_inverse(A.pair, n, qs);  // (ends with a barrier)
  // ce and dlogits = (softmax - onehot) / n, one row per thread; a label outside [0, c), a pair entry outside [0, n)
  // or a pair that is no permutation indexes nothing and makes both losses (and the row's dlogits) NaN
  const float inv_n = 1.0f / (float)n;
  double csum = 0.0;
  for (int i = t; i < n; i += LM_NT) {
    float* row = W.dl + (size_t)i * c;
    const int64_t lab = A.label[i], pi = A.pair[i];
    const bool valid = lab >= 0 && lab < (int64_t)c && pi >= 0 && pi < (int64_t)n && qs[i] >= 0;
    float mx = row[0];
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, row[k]);
    float se = 0.f;
    for (int k = 0; k < c; ++k) se += expf(row[k] - mx);
    const float lse = mx + logf(se);
    csum += valid ? (double)(lse - row[(int)(valid ? lab : 0)]) : (double)nanv;
    for (int k = 0; k < c; ++k) {
      const float p = expf(row[k] - mx) / se;
      row[k] = valid ? (p - ((int64_t)k == lab ? 1.f : 0.f)) * inv_n : nanv;
    }
  }
  red[t] = csum;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0, lam = 0.0;
    for (int q = 0; q < LM_NT; ++q) tot += red[q];             // thread order
    for (int sidx = 0; sidx < nslab; ++sidx) lam += W.lampart[sidx];  // slab order
    A.loss_out[0] = (float)(tot / (double)n);
    A.loss_out[1] = tot != tot ? nanv : (float)(lam / (double)n);
  }
  // gb[k] = sum_i dlogits[i][k]: 8 row classes per k, folded in order
  {
    const int k = t % LM_MAXC, pr = t / LM_MAXC;
    float acc = 0.f;
    if (k < c)
      for (int i = pr; i < n; i += LM_NT / LM_MAXC) acc += W.dl[(size_t)i * c + k];
    gbr[pr * LM_MAXC + k] = acc;
    __syncthreads();
    if (t < c) {
      float g = 0.f;
      for (int q = 0; q < LM_NT / LM_MAXC; ++q) g += gbr[q * LM_MAXC + t];
      A.G.b[t] = g;
    }
  }
}

// ---------------------------------------------------------------- launch 2: backward of each slab
__global__ __launch_bounds__(LM_NT) void lam_bwd_kernel(const LamArgs A) {
  __shared__ float dls[LM_TR * LM_CP];
  __shared__ float hs[LM_TR * LM_SP];
  __shared__ float dq[LM_TR * LM_SP];  // (h - h[pair])^2
  __shared__ float ws[LM_MAXC * LM_SP];
  __shared__ double red[2 * LM_TR * LM_S];
  __shared__ double cdb[LM_S], cdg[LM_S];
  __shared__ int gcol[LM_S];
  __shared__ BnFwdC kf[LM_S];
  __shared__ int labs[LM_TR];
  __shared__ int qs[LM_MAXN];
  const cv_lam& P = A.P;
  const int t = threadIdx.x, slab = blockIdx.x;
  const int n = A.n, c = P.c, C = P.in_ch, pix = P.in_pix, F = C * pix;
  const LamWork W = lam_work(A.work, n, C, pix, c);
  const int ncols = lm_setup(P, A.bn, slab, gcol, kf, ws);
  lm_inverse(A.pair, n, qs);
  const float coef = P.lam[0] * (2.0f / (float)n);

  // thread = 1 row x 4 columns: dh, the mask, gin, the fp64 column sums; then gW[:,slab] (thread = up to 2 (k, j))
  const int r = t >> 2, cq = (t & 3) * 4;
  double dbs[4] = {0.0, 0.0, 0.0, 0.0}, dgs[4] = {0.0, 0.0, 0.0, 0.0};
  double acc2[2] = {0.0, 0.0}, accs[2] = {0.0, 0.0};
  for (int i0 = 0; i0 < n; i0 += LM_TR) {
    for (int idx = t; idx < LM_TR * c; idx += LM_NT) {
      const int rr = idx / c, k = idx - rr * c, i = i0 + rr;
      dls[rr * LM_CP + k] = i < n ? W.dl[(size_t)i * c + k] : 0.f;
    }
    if (t < LM_TR) {
      const int64_t li = i0 + t < n ? A.label[i0 + t] : -1;
      labs[t] = li >= 0 && li < (int64_t)c ? (int)li : -1;
    }
    __syncthreads();
    const int i = i0 + r;
    float hv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      const int64_t pi = A.pair[i];
      const int ip = pi >= 0 && pi < (int64_t)n ? (int)pi : i;
      const int iq = qs[i] >= 0 ? qs[i] : i;
      const int64_t lq64 = A.label[iq];
      const int li = labs[r], lq = lq64 >= 0 && lq64 < (int64_t)c ? (int)lq64 : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = cq + u;
        if (j < ncols) {
          const BnFwdC k = kf[j];
          const float yv = A.y[(size_t)i * F + gcol[j]];
          const float pre = bn_out(yv, k);
          const float h = fmaxf(pre, 0.f);
          const float hp = bn_relu(A.y[(size_t)ip * F + gcol[j]], k);
          const float hq = bn_relu(A.y[(size_t)iq * F + gcol[j]], k);
          const float d = h - hp, e = hq - h;
          float base = 0.f;
          for (int kk = 0; kk < c; ++kk) base = fmaf(dls[r * LM_CP + kk], ws[kk * LM_SP + j], base);
          const float wi = li >= 0 ? ws[li * LM_SP + j] : 0.f, wq = lq >= 0 ? ws[lq * LM_SP + j] : 0.f;
          const float dh = base + coef * (wi * wi * d - wq * wq * e);
          const float dz = pre > 0.f ? dh : 0.f;
          A.gin[(size_t)i * F + gcol[j]] = dz;
          dbs[u] += (double)dz;
          dgs[u] += (double)(dz * ((yv - k.mu) * k.istd));
          hv[u] = h;
          dv[u] = d * d;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      hs[r * LM_SP + cq + u] = hv[u];
      dq[r * LM_SP + cq + u] = dv[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = t + LM_NT * u;
      if (o < c * LM_S) {
        const int k = o / LM_S, j = o % LM_S;
        float a2 = 0.f, s2 = 0.f;
#pragma unroll 8  // (rows in order)
        for (int rr = 0; rr < LM_TR; ++rr) {
          a2 = fmaf(dls[rr * LM_CP + k], hs[rr * LM_SP + j], a2);
          s2 += labs[rr] == k ? dq[rr * LM_SP + j] : 0.f;
        }
        acc2[u] += (double)a2;  // (tiles in order)
        accs[u] += (double)s2;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    red[r * LM_S + cq + u] = dbs[u];
    red[LM_TR * LM_S + r * LM_S + cq + u] = dgs[u];
  }
  __syncthreads();
  if (t < LM_S) {
    double sb = 0.0, sg = 0.0;
    for (int rr = 0; rr < LM_TR; ++rr) {  // row lanes in order
      sb += red[rr * LM_S + t];
      sg += red[LM_TR * LM_S + rr * LM_S + t];
    }
    cdb[t] = sb;
    cdg[t] = sg;
  }
  __syncthreads();
  // the channel's sums over its pixels (in order) into replica 0 of [REPL][2][C]; the other replicas stay zero
  {
    const int cs = lm_cs(pix), c0 = slab * cs;
    if (t < cs && c0 + t < C) {
      double sb = 0.0, sg = 0.0;
      for (int p = 0; p < pix; ++p) {
        sb += cdb[t * pix + p];
        sg += cdg[t * pix + p];
      }
      A.gstat_out[c0 + t] = sb;
      A.gstat_out[C + c0 + t] = sg;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = t + LM_NT * u;
      if (o < c * LM_S) {
        const int k = o / LM_S, j = o % LM_S;
        if (j < ncols)
          A.G.w[(size_t)k * F + (size_t)c0 * pix + j] =
              fmaf(coef * ws[k * LM_SP + j], (float)accs[u], (float)acc2[u]);
      }
    }
  }
}

// ---------------------------------------------------------------- eval forward, one launch
// LM_ER rows per workgroup: h in PyTorch feature order in LDS, then one wave per row and a lane-strided dot per class
__global__ __launch_bounds__(LM_NT) void lam_eval_kernel(const cv_lam P, const float* y, const cv_bn bn, int n,
                                                         float* logits) {
  __shared__ float hs[LM_ER * LM_MAXF];
  const int t = threadIdx.x, i0 = blockIdx.x * LM_ER;
  const int C = P.in_ch, pix = P.in_pix, F = C * pix, c = P.c;
  for (int col = t; col < F; col += LM_NT) {
    const int p = col / C, cc = col - p * C;
    const BnFwdC k = bn_fwd_const(bn, cc);
#pragma unroll
    for (int r = 0; r < LM_ER; ++r) {
      const int i = i0 + r;
      hs[r * LM_MAXF + cc * pix + p] = i < n ? bn_relu(y[(size_t)i * F + col], k) : 0.f;
    }
  }
  __syncthreads();
  const int w = t >> 6, l = t & 63, i = i0 + w;
  for (int k = 0; k < c; ++k) {
    const float* wr = P.w + (size_t)k * F;
    float acc = 0.f;
    for (int f = l; f < F; f += 64) acc = fmaf(hs[w * LM_MAXF + f], wr[f], acc);
    acc = wave_sum(acc);
    if (l == 0 && i < n) logits[(size_t)i * c + k] = acc + P.b[k];
  }
}

// ---------------------------------------------------------------- stratified pairing, one workgroup
// pair = a uniformly random permutation inside each label stratum (trainer.py:249-257): every row draws a Philox
// key; with start_i = #{j: label_j < label_i}, ord_i = #{j < i: label_j = label_i} (the row's place in its stratum
// in index order) and rank_i = #{j: label_j = label_i, (key_j, j) < (key_i, i)} (its place in key order),
// slot[start_i + rank_i] = i lists each stratum in key order and pair[i] = slot[start_i + ord_i].
__global__ __launch_bounds__(LM_MAXN) void lam_pair_kernel(const int64_t* label, int n, uint64_t seed,
                                                           uint64_t* offset, int64_t* pair_out) {
  __shared__ int64_t labs[LM_MAXN];
  __shared__ unsigned keys[LM_MAXN];
  __shared__ unsigned short slot[LM_MAXN];
  const int t = threadIdx.x;
  const uint64_t off = offset ? offset[0] : 0;
  if (t < n) {
    labs[t] = label[t];
    keys[t] = philox(seed, off ^ 0x6c616d70616972ull, (uint64_t)t).x;
  }
  __syncthreads();
  int start = 0, ord = 0, rank = 0;
  if (t < n) {
    const int64_t lt = labs[t];
    const unsigned kt = keys[t];
    for (int j = 0; j < n; ++j) {
      const int64_t lj = labs[j];
      const unsigned kj = keys[j];
      start += lj < lt ? 1 : 0;
      if (lj == lt) {
        ord += j < t ? 1 : 0;
        rank += (kj < kt || (kj == kt && j < t)) ? 1 : 0;
      }
    }
    slot[start + rank] = (unsigned short)t;
  }
  __syncthreads();
  if (t < n) pair_out[t] = (int64_t)slot[start + ord];
  if (t == 0 && offset) offset[0] = off + 1;
}

}  // namespace cv

using namespace cv;

extern "C" int cv_lam_supported(int n, int in_ch, int in_pix, int c) {
  return n >= 2 && n <= LM_MAXN && in_ch >= 1 && in_pix >= 1 && in_pix <= LM_MAXPIX &&
         (long)in_ch * in_pix <= LM_MAXF && c >= 2 && c <= LM_MAXC;
}

extern "C" size_t cv_lam_workspace_bytes(int n, int in_ch, int in_pix, int c) {
  if (!cv_lam_supported(n, in_ch, in_pix, c)) return 0;
  return lam_work_bytes(n, in_ch, in_pix, c);
}

static int check_lam(const cv_lam* P, const cv_bn* bn, const char* who) {
  CV_REQUIRE(P && P->w && P->b, "%s: head weight or bias missing", who);
  CV_REQUIRE(bn && bn->C == P->in_ch, "%s: BatchNorm missing or its C != in_ch", who);
  CV_REQUIRE(bn->train ? bn->stat != nullptr : (bn->running_mean && bn->running_var),
             "%s: the BatchNorm lacks its forward sums (train) or running statistics (eval)", who);
  return 0;
}

extern "C" int cv_lam_pair(const int64_t* label, int n, uint64_t seed, uint64_t* offset, int64_t* pair_out,
                           cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(n >= 1 && n <= LM_MAXN, "lam_pair: unsupported n=%d (1 <= n <= %d)", n, LM_MAXN);
  CV_REQUIRE(label && pair_out, "lam_pair: label or pair_out missing");
  hipLaunchKernelGGL(lam_pair_kernel, dim3(1), dim3(LM_MAXN), 0, S(stream), label, n, seed, offset, pair_out);
  CV_LAUNCH_CHECK("lam_pair");
  return 0;
}

extern "C" int cv_lam_step(const cv_lam* P, const float* y, const cv_bn* bn, const int64_t* label, const int64_t* pair,
                           int n, void* work, float* loss_out, float* gin, double* gstat_out, const cv_lam_grad* g,
                           cv_stream_t stream) {
  clear_error();
  if (check_lam(P, bn, "lam_step")) return 1;
  CV_REQUIRE(cv_lam_supported(n, P->in_ch, P->in_pix, P->c),
             "lam_step: unsupported shape n=%d ch=%d pix=%d c=%d (2 <= n <= %d, 1 <= pix <= %d, ch pix <= %d, "
             "2 <= c <= %d)", n, P->in_ch, P->in_pix, P->c, LM_MAXN, LM_MAXPIX, LM_MAXF, LM_MAXC);
  CV_REQUIRE(P->lam, "lam_step: the device lam_coef is missing");
  CV_REQUIRE(bn->train && (long)bn->count == (long)n * P->in_pix,
             "lam_step: the BatchNorm must be in train mode with count = n pix");
  CV_REQUIRE(y && label && pair && work && loss_out && gin && gstat_out,
             "lam_step: y, label, pair, work, loss_out, gin or gstat_out missing");
  CV_REQUIRE((uintptr_t)work % 16 == 0, "lam_step: work must be 16-byte aligned");
  CV_REQUIRE(g && g->w && g->b, "lam_step: gradient buffers missing");
  LamArgs A;
  memset(&A, 0, sizeof(A));
  A.P = *P;
  A.y = y; A.bn = *bn; A.label = label; A.pair = pair; A.n = n;
  A.work = work;
  A.loss_out = loss_out;
  A.gin = gin;
  A.gstat_out = gstat_out;
  A.G = *g;
  const int nslab = lm_slabs(P->in_ch, P->in_pix);
  hipLaunchKernelGGL(lam_fwd_kernel, dim3(nslab), dim3(LM_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("lam_step.forward");
  hipLaunchKernelGGL(lam_bwd_kernel, dim3(nslab), dim3(LM_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("lam_step.backward");
  return 0;
}

extern "C" int cv_lam_forward(const cv_lam* P, const float* y, const cv_bn* bn, int n, float* logits,
                              cv_stream_t stream) {
  clear_error();
  if (check_lam(P, bn, "lam_forward")) return 1;
  CV_REQUIRE(n >= 1 && cv_lam_supported(2, P->in_ch, P->in_pix, P->c),
             "lam_forward: unsupported shape n=%d ch=%d pix=%d c=%d (n >= 1, 1 <= pix <= %d, ch pix <= %d, "
             "2 <= c <= %d)", n, P->in_ch, P->in_pix, P->c, LM_MAXPIX, LM_MAXF, LM_MAXC);
  CV_REQUIRE(y && logits, "lam_forward: y or logits missing");
  hipLaunchKernelGGL(lam_eval_kernel, dim3(cdiv(n, LM_ER)), dim3(LM_NT), 0, S(stream), *P, y, *bn, n, logits);
  CV_LAUNCH_CHECK("lam_forward");
  return 0;
}
