// SupCon contrastive losses (reference src/losses.py:140-170: supcon_in_loss, supcon_out_loss, composed by
// contrastive_loss :98-126) in O(n d) memory: the C-ABI cv_supcon (include/clearvae.h).  Beside cv_ntxent, not in
// it: the similarities, their row derivatives and the log-sum-exp merge are cv_ntxent.hpp's device functions, the
// kernels are this file's own.
//
// With S = pairwise_<sim>(mu, logvar), P_ij = [label_i == label_j] (ps: !=), s = S / tau:
//   in   n_k[i] = sum_j P_ij - 1 (ps: the diagonal of P is 0, so this is one less than the number of
//        different-label rows: the reference's off-by-one, kept), diagonal of S = -inf,
//        row_i = log n_k[i] - LSE_{P_ij, j != i} s_ij + LSE_{j != i} s_ij
//   out  diagonal of S = -999 (finite: exp(-999 / tau) is a term of the log-sum-exp, without gradient),
//        n_k[i] = off-diagonal positives, rows with n_k = 0 dropped,
//        row_i = -(sum_{j != i} P_ij S_ij) / n_k[i] + LSE_j s_ij        (first term NOT divided by tau)
//   loss = mean over the rows whose value is finite (none: NaN, zero gradients).
// Gradient, m kept rows, upstream g:  d theta_i = (g / m) sum_{j != i} (keep_i G_ij + keep_j G_ji) dS_ij/d theta_i,
//   in   G_ij = (softmax_all_ij - P_ij softmax_pos_ij) / tau
//   out  G_ij = softmax_all_ij / tau - P_ij / n_k[i]   (softmax over the LSE that includes the diagonal term).
//
// Phase 0: sc_rows (one wave per row) writes six floats per row into the stats workspace, then sc_loss (one
// workgroup, fixed order) folds the kept rows into loss_out and the kept-row count.  A dropped row is stored with
// its maxima = +inf and its 1 / n_k = 0, so that every weight it would contribute in phase 1 is exp(-inf) = 0 or 0:
// the gradient kernel needs no keep flag.  The log-sum-exps are kept as (max, log sum) pairs: with logits of 1e5
// (l2 at large |mu|) max + log(sum) rounds at 1e-2, (s - max) - log(sum) does not.
// Phase 1: sc_grad (one wave per row i) walks all j, S_ij once per pair, lane-private gradient registers, a wave
// reduction, lane k stores component k.  No atomics: two runs are bit-identical.
//
// Variants (template FULL): the mu / logvar rows of the columns are staged in LDS with the odd pitch d + 1 (lanes on
// consecutive rows hit distinct banks) — all n rows at once when sc_lds_bytes(n, ...) <= 144 KiB (FULL), else in
// tiles of SC_TJ rows that every workgroup walks through (the global-walk variant, any n up to NT_MAXBIG).
//
// The step form, cv_supcon_step (the fused CLEAR step's two contrastive terms, reference trainer.py:456-480: the
// content and the style branch of losses.py:98-126, 140-170 on the same labels): the same row / loss / gradient
// bodies (sc_rows_body, sc_loss_body, cv_supcon_grad.inc) over up to two branches in one launch each, the branch index
// as a grid dimension (sc_step_*_kernel), reading the [n][4d] heads in place through the row stride.  Its phase 1
// (ACC in cv_supcon_grad.inc) ADDS gmul * gscale[0] * dloss / d theta
// onto what dmu / dlogvar hold: lane k of row i's wave reads and writes element (i, k) of its branch, nobody else
// does, so the sum has one order and two runs give the same bits; for cosine / l2 the logvar columns are not touched.
#include "cv_ntxent.hpp"

namespace cv {

struct ScArgs {
  const float* mu;
  const float* lv;
  int ld;
  const int64_t* label;
  int n, d, sim, ps, kind;
  float tau;
  float* stats;  // [6][n] + 4: max_all, log sum_all, max_pos | 1/n_k, log sum_pos | 0, n_k, row value; [6n] = kept rows
  float* loss_out;
  float* dmu;
  float* dlv;
  int gld;
  const float* gscale;
};

struct ScStepArgs {  // cv_supcon_step: branch b is blockIdx.y
  ScArgs br[2];
  float gmul[2];
  int nbr;
};

constexpr int SC_ROWS = 4;    // rows (waves) per 256-thread workgroup
constexpr int SC_TJ = 256;    // columns per LDS tile of the global-walk variant
constexpr size_t SC_LDS_MAX = 144 * 1024;
constexpr float SC_OUT_DIAG = -999.f;

inline size_t sc_lds_bytes(int rows, int d, bool need_lv) {
  return (size_t)rows * ((size_t)d + 1) * 4 * (need_lv ? 2 : 1);
}

// rows [j0, j0 + tn) of mu (and logvar) into LDS, pitch d + 1; ends with a barrier
__device__ __forceinline__ void sc_stage(const ScArgs& A, int j0, int tn, bool need_lv, float* smu, float* slv) {
  const int d = A.d, pd = d + 1, total = tn * d;
  const FDiv fd = FDiv::make(d);
  constexpr int U = 4;
  for (int base = threadIdx.x; base < total; base += 256 * U) {
    float vm[U], vl[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int e = base + q * 256, ec = e < total ? e : 0;
      const int r = fd.div(ec), k = ec - r * d;
      vm[q] = A.mu[(size_t)(j0 + r) * A.ld + k];
      vl[q] = need_lv ? A.lv[(size_t)(j0 + r) * A.ld + k] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int e = base + q * 256;
      if (e < total) {
        const int r = fd.div(e), k = e - r * d;
        smu[r * pd + k] = vm[q];
        if (need_lv) slv[r * pd + k] = vl[q];
      }
    }
  }
  __syncthreads();
}

template <int DM>
__device__ __forceinline__ void sc_theta(const float* smu, const float* slv, int r, int d, float* m, float* l,
                                         bool need_lv) {
  const int pd = d + 1;
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    m[k] = (k < d) ? smu[r * pd + k] : 0.f;
    l[k] = (need_lv && k < d) ? slv[r * pd + k] : 0.f;
  }
}

template <int DM>
__device__ __forceinline__ void sc_row(const ScArgs& A, int r, float* m, float* l, bool need_lv) {
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    m[k] = (k < A.d) ? A.mu[(size_t)r * A.ld + k] : 0.f;
    l[k] = (need_lv && k < A.d) ? A.lv[(size_t)r * A.ld + k] : 0.f;
  }
}

// ---------------------------------------------------------------- phase 0: row statistics
template <int DM, bool FULL>
__device__ __forceinline__ void sc_rows_body(const ScArgs& A) {
  extern __shared__ __attribute__((aligned(16))) char sc_smem[];
  const int n = A.n, d = A.d;
  const bool cosine = A.sim == CV_SIM_COSINE;
  const bool need_lv = !(A.sim == CV_SIM_COSINE || A.sim == CV_SIM_L2);
  const bool out = A.kind == CV_SUPCON_OUT;
  const int T = FULL ? n : SC_TJ;
  float* smu = reinterpret_cast<float*>(sc_smem);
  float* slv = smu + (size_t)T * (d + 1);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * SC_ROWS + w;
  const bool valid = i < n;  // (a wave past the last row still stages and meets the barriers)
  const int ic = valid ? i : 0;
  float mi[DM], li[DM], mj[DM], lj[DM];
  sc_row<DM>(A, ic, mi, li, need_lv);
  const float ni = cosine ? fmaxf(reg_norm<DM>(mi, d), 1e-8f) : 1.f;
  const int64_t lab = A.label[ic];
  float ma = -INFINITY, sa = 0.f, mp = -INFINITY, sp = 0.f, psum = 0.f, cnt = 0.f;
  for (int j0 = 0; j0 < n; j0 += T) {
    const int tn = min(T, n - j0);
    if (j0) __syncthreads();  // every wave is done with the previous tile
    sc_stage(A, j0, tn, need_lv, smu, slv);
    if (!valid) continue;
    for (int jj = lane; jj < tn; jj += 64) {
      const int j = j0 + jj;
      if (j == i) {
        if (out) lse_merge(ma, sa, SC_OUT_DIAG / A.tau, 1.f);
        continue;
      }
      sc_theta<DM>(smu, slv, jj, d, mj, lj, need_lv);
      const float nj = cosine ? fmaxf(reg_norm<DM>(mj, d), 1e-8f) : 1.f;
      const float S = sim_ij<DM>(A.sim, mi, li, ni, mj, lj, nj, d);
      const float s = S / A.tau;
      lse_merge(ma, sa, s, 1.f);
      const int64_t lj_ = A.label[j];
      const bool pos = A.ps ? (lj_ != lab) : (lj_ == lab);
      if (pos) {
        cnt += 1.f;
        if (out) psum += S;
        else lse_merge(mp, sp, s, 1.f);
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(ma, o, 64), s2 = __shfl_xor(sa, o, 64);
    const float m3 = __shfl_xor(mp, o, 64), s3 = __shfl_xor(sp, o, 64);
    lse_merge(ma, sa, m2, s2);
    lse_merge(mp, sp, m3, s3);
  }
  psum = wave_sum(psum);
  cnt = wave_sum(cnt);
  if (lane != 0) return;
  // in: sum_j P_ij - 1 with the diagonal of P (1 when !ps, 0 when ps); out: the off-diagonal positives
  const float nk = out ? cnt : (A.ps ? cnt - 1.f : cnt);
  const float la = (sa > 0.f) ? logf(sa) : -INFINITY, lp = (sp > 0.f) ? logf(sp) : -INFINITY;
  float row = NAN;
  if (out) {
    if (nk > 0.f) row = -psum / nk + (ma + la);
  } else if (nk > 0.f) {
    row = logf(nk) + ((ma - mp) + (la - lp));
  }
  const bool keep = isfinite(row);
  float* st = A.stats;
  st[i] = keep ? ma : INFINITY;
  st[(size_t)n + i] = keep ? la : 0.f;
  st[2 * (size_t)n + i] = keep ? (out ? 1.f / nk : mp) : (out ? 0.f : INFINITY);
  st[3 * (size_t)n + i] = (keep && !out) ? lp : 0.f;
  st[4 * (size_t)n + i] = nk;
  st[5 * (size_t)n + i] = row;
}

template <int DM, bool FULL>
__global__ __launch_bounds__(256) void sc_rows_kernel(const ScArgs A) {
  sc_rows_body<DM, FULL>(A);
}

template <int DM, bool FULL>
__global__ __launch_bounds__(256) void sc_step_rows_kernel(const ScStepArgs P) {
  sc_rows_body<DM, FULL>(P.br[blockIdx.y]);
}

// the loss and the kept-row count: one workgroup, thread t folds rows t, t + 1024, ... in order, then a fixed tree
__device__ __forceinline__ void sc_loss_body(const ScArgs& A, double* ssum, float* scnt) {
  const int n = A.n;
  const float* row = A.stats + 5 * (size_t)n;
  double s = 0.0;
  float c = 0.f;
  for (int j = threadIdx.x; j < n; j += 1024) {
    const float r = row[j];
    if (isfinite(r)) {
      s += (double)r;
      c += 1.f;
    }
  }
  const double tot = block_sum<1024>(s, ssum);
  const float m = block_sum<1024>(c, scnt);
  if (threadIdx.x == 0) {
    A.loss_out[0] = (m > 0.f) ? (float)(tot / (double)m) : NAN;
    A.stats[6 * (size_t)n] = m;
  }
}

__global__ __launch_bounds__(1024) void sc_loss_kernel(const ScArgs A) {
  __shared__ double ssum[16];
  __shared__ float scnt[16];
  sc_loss_body(A, ssum, scnt);
}

__global__ __launch_bounds__(1024) void sc_step_loss_kernel(const ScStepArgs P) {  // one workgroup per branch
  __shared__ double ssum[16];
  __shared__ float scnt[16];
  sc_loss_body(P.br[blockIdx.x], ssum, scnt);
}

// ---------------------------------------------------------------- phase 1: gradients
template <int DM, bool FULL>
__global__ __launch_bounds__(256) void sc_grad_kernel(const ScArgs A) {
  constexpr bool ACC = false;
  const float gmul = 1.f;
#include "cv_supcon_grad.inc"
}

template <int DM, bool FULL>
__global__ __launch_bounds__(256) void sc_step_grad_kernel(const ScStepArgs P) {
  constexpr bool ACC = true;
  const ScArgs A = P.br[blockIdx.y];  // (a copy: through a reference the tiled DM = 32 kernel spills 12 bytes)
  const float gmul = P.gmul[blockIdx.y];
#include "cv_supcon_grad.inc"
}

static int sc_launch(const void* kern, void* arg, dim3 grid, int phase, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024 && hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("supcon: %zu bytes of LDS refused", lds);
    return 2;
  }
  void* params[] = {arg};
  note_launch(kern);
  if (hipLaunchKernel(kern, grid, dim3(256), params, lds, st) != hipSuccess) {
    set_error("supcon: launch failed (phase %d)", phase);
    return 2;
  }
  return 0;
}

template <int DM, bool FULL>
static int sc_launch_t(const ScArgs& a, int phase, size_t lds, hipStream_t st) {
  const void* kern = phase == 0 ? (const void*)sc_rows_kernel<DM, FULL> : (const void*)sc_grad_kernel<DM, FULL>;
  ScArgs arg = a;
  return sc_launch(kern, &arg, dim3(cdiv(a.n, SC_ROWS)), phase, lds, st);
}

template <int DM, bool FULL>
static int sc_launch_t(const ScStepArgs& a, int phase, size_t lds, hipStream_t st) {
  const void* kern =
      phase == 0 ? (const void*)sc_step_rows_kernel<DM, FULL> : (const void*)sc_step_grad_kernel<DM, FULL>;
  ScStepArgs arg = a;
  return sc_launch(kern, &arg, dim3(cdiv(a.br[0].n, SC_ROWS), a.nbr), phase, lds, st);
}

template <bool FULL, class Args>
static int sc_launch_dm(const Args& a, int d, int phase, size_t lds, hipStream_t st) {
  if (d <= 8) return sc_launch_t<8, FULL>(a, phase, lds, st);
  if (d <= 16) return sc_launch_t<16, FULL>(a, phase, lds, st);
  if (d <= 32) return sc_launch_t<32, FULL>(a, phase, lds, st);
  return sc_launch_t<64, FULL>(a, phase, lds, st);
}

static bool sc_supported(int n, int d, int sim) {
  return n >= 1 && n <= NT_MAXBIG && d >= 1 && d <= 64 && sim >= CV_SIM_COSINE && sim <= CV_SIM_MAHALANOBIS;
}

}  // namespace cv

using namespace cv;

extern "C" int cv_supcon_supported(int n, int d, int sim) { return sc_supported(n, d, sim) ? 1 : 0; }

extern "C" size_t cv_supcon_stats_floats(int n) { return n > 0 ? 6 * (size_t)n + 4 : 0; }

extern "C" int cv_supcon(const cv_supcon_args* p, int phase, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(p, "supcon: null args");
  CV_REQUIRE(phase == 0 || phase == 1, "supcon: phase must be 0 or 1 (phase=%d)", phase);
  CV_REQUIRE(p->n >= 1 && p->n <= NT_MAXBIG, "supcon: batch must be in 1..%d (n=%d)", NT_MAXBIG, p->n);
  CV_REQUIRE(p->d >= 1 && p->d <= 64, "supcon: width must be in 1..64 (d=%d)", p->d);
  CV_REQUIRE(p->sim >= CV_SIM_COSINE && p->sim <= CV_SIM_MAHALANOBIS, "supcon: unknown similarity %d", p->sim);
  CV_REQUIRE(p->kind == CV_SUPCON_IN || p->kind == CV_SUPCON_OUT, "supcon: unknown kind %d", p->kind);
  CV_REQUIRE(p->mu && p->label && p->stats, "supcon: mu, label and stats are required");
  const bool need_lv = !(p->sim == CV_SIM_COSINE || p->sim == CV_SIM_L2);
  CV_REQUIRE(!need_lv || p->logvar, "supcon: this similarity reads logvar");
  CV_REQUIRE(p->temperature > 0.f, "supcon: temperature must be positive");
  CV_REQUIRE(p->ld >= p->d, "supcon: row stride %d < d=%d", p->ld, p->d);
  if (phase == 0) CV_REQUIRE(p->loss_out, "supcon: phase 0 needs loss_out");
  if (phase == 1) {
    CV_REQUIRE(p->dmu && p->gscale, "supcon: phase 1 needs dmu and gscale");
    CV_REQUIRE(p->gld >= p->d, "supcon: gradient row stride %d < d=%d", p->gld, p->d);
  }
  ScArgs a;
  a.mu = p->mu;
  a.lv = need_lv ? p->logvar : nullptr;
  a.ld = p->ld;
  a.label = p->label;
  a.n = p->n;
  a.d = p->d;
  a.sim = p->sim;
  a.ps = p->ps ? 1 : 0;
  a.kind = p->kind;
  a.tau = p->temperature;
  a.stats = p->stats;
  a.loss_out = p->loss_out;
  a.dmu = p->dmu;
  a.dlv = p->dlogvar;
  a.gld = p->gld;
  a.gscale = p->gscale;
  const hipStream_t st = S(stream);
  const size_t full = sc_lds_bytes(a.n, a.d, need_lv);
  const int rc = full <= SC_LDS_MAX ? sc_launch_dm<true>(a, a.d, phase, full, st)
                                    : sc_launch_dm<false>(a, a.d, phase, sc_lds_bytes(SC_TJ, a.d, need_lv), st);
  if (rc) return rc;
  if (phase == 0) {
    note_launch((const void*)sc_loss_kernel);
    hipLaunchKernelGGL(sc_loss_kernel, dim3(1), dim3(1024), 0, st, a);
    CV_LAUNCH_CHECK("supcon_loss");
  }
  return 0;
}

extern "C" int cv_supcon_step(const cv_supcon_branch* br, int nbr, const int64_t* label, int n, int d, int sim, int kind,
                              float temperature, int phase, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(br, "supcon_step: null branches");
  CV_REQUIRE(nbr == 1 || nbr == 2, "supcon_step: 1 or 2 branches (nbr=%d)", nbr);
  CV_REQUIRE(phase == 0 || phase == 1, "supcon_step: phase must be 0 or 1 (phase=%d)", phase);
  CV_REQUIRE(n >= 1 && n <= NT_MAXBIG, "supcon_step: batch must be in 1..%d (n=%d)", NT_MAXBIG, n);
  CV_REQUIRE(d >= 1 && d <= 64, "supcon_step: width must be in 1..64 (d=%d)", d);
  CV_REQUIRE(sim >= CV_SIM_COSINE && sim <= CV_SIM_MAHALANOBIS, "supcon_step: unknown similarity %d", sim);
  CV_REQUIRE(kind == CV_SUPCON_IN || kind == CV_SUPCON_OUT, "supcon_step: unknown kind %d", kind);
  CV_REQUIRE(label, "supcon_step: label is required");
  CV_REQUIRE(temperature > 0.f, "supcon_step: temperature must be positive");
  const bool need_lv = !(sim == CV_SIM_COSINE || sim == CV_SIM_L2);
  ScStepArgs P;
  P.nbr = nbr;
  for (int b = 0; b < 2; ++b) {
    const cv_supcon_branch& q = br[b < nbr ? b : 0];  // (an unused slot repeats branch 0: never indexed)
    if (b < nbr) {
      CV_REQUIRE(q.mu && q.stats, "supcon_step: branch %d: mu and stats are required", b);
      CV_REQUIRE(!need_lv || q.logvar, "supcon_step: branch %d: this similarity reads logvar", b);
      CV_REQUIRE(q.ld >= d, "supcon_step: branch %d: row stride %d < d=%d", b, q.ld, d);
      if (phase == 0) CV_REQUIRE(q.loss_out, "supcon_step: branch %d: phase 0 needs loss_out", b);
      if (phase == 1) {
        CV_REQUIRE(q.dmu && q.gscale, "supcon_step: branch %d: phase 1 needs dmu and gscale", b);
        CV_REQUIRE(q.gld >= d, "supcon_step: branch %d: gradient row stride %d < d=%d", b, q.gld, d);
      }
    }
    ScArgs& a = P.br[b];
    a.mu = q.mu;
    a.lv = need_lv ? q.logvar : nullptr;
    a.ld = q.ld;
    a.label = label;
    a.n = n;
    a.d = d;
    a.sim = sim;
    a.ps = q.ps ? 1 : 0;
    a.kind = kind;
    a.tau = temperature;
    a.stats = q.stats;
    a.loss_out = q.loss_out;
    a.dmu = q.dmu;
    a.dlv = q.dlogvar;
    a.gld = q.gld;
    a.gscale = q.gscale;
    P.gmul[b] = q.gmul;
  }
  if (nbr == 2)
    CV_REQUIRE(br[0].stats != br[1].stats, "supcon_step: the branches need a stats workspace each");
  const hipStream_t st = S(stream);
  const size_t full = sc_lds_bytes(n, d, need_lv);
  const int rc = full <= SC_LDS_MAX ? sc_launch_dm<true>(P, d, phase, full, st)
                                    : sc_launch_dm<false>(P, d, phase, sc_lds_bytes(SC_TJ, d, need_lv), st);
  if (rc) return rc;
  if (phase == 0) {
    note_launch((const void*)sc_step_loss_kernel);
    hipLaunchKernelGGL(sc_step_loss_kernel, dim3(nbr), dim3(1024), 0, st, P);
    CV_LAUNCH_CHECK("supcon_step_loss");
  }
  return 0;
}
