// The body of sc_grad_kernel and sc_step_grad_kernel (cv_supcon.hip includes it once in each): one wave per row i walks
// all j.  The including kernel defines DM, FULL, ACC (the step form: the upstream factor is gmul * gscale[0] and the row
// is added onto dmu / dlogvar; else gscale[0] and overwritten), `A` (cv::ScArgs) and `gmul`.  Included text, not a
// device function the two kernels call: behind a function boundary, inlined or not, the register allocator spills 44 to
// 148 bytes per lane at DM = 32 (hipcc's resource remarks), the kernels with the body in place spill none up to DM = 32.
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
  const bool valid = i < n;
  const int ic = valid ? i : 0;
  const float* __restrict__ st = A.stats;
  const float m = st[6 * (size_t)n];
  const float up = ACC ? gmul * A.gscale[0] : A.gscale[0];
  const float c = (m > 0.f) ? up / m : 0.f;
  const float inv_tau = 1.f / A.tau;
  float mi[DM], li[DM], mj[DM], lj[DM], gm[DM], gl[DM];
  sc_row<DM>(A, ic, mi, li, need_lv);
#pragma unroll
  for (int k = 0; k < DM; ++k) { gm[k] = 0.f; gl[k] = 0.f; }
  const float rni = cosine ? reg_norm<DM>(mi, d) : 0.f;
  const float ni = cosine ? fmaxf(rni, 1e-8f) : 1.f;
  const bool clamped_i = cosine && !(rni > 1e-8f);
  const int64_t lab = A.label[ic];
  const float a0 = st[ic], a1 = st[(size_t)n + ic], a2 = st[2 * (size_t)n + ic], a3 = st[3 * (size_t)n + ic];
  for (int j0 = 0; j0 < n; j0 += T) {
    const int tn = min(T, n - j0);
    if (j0) __syncthreads();
    sc_stage(A, j0, tn, need_lv, smu, slv);
    if (!valid) continue;
    for (int jj = lane; jj < tn; jj += 64) {
      const int j = j0 + jj;
      if (j == i) continue;
      sc_theta<DM>(smu, slv, jj, d, mj, lj, need_lv);
      const float nj = cosine ? fmaxf(reg_norm<DM>(mj, d), 1e-8f) : 1.f;
      const float S = sim_ij<DM>(A.sim, mi, li, ni, mj, lj, nj, d);
      const float s = S / A.tau;
      const int64_t lj_ = A.label[j];
      const bool pos = A.ps ? (lj_ != lab) : (lj_ == lab);
      const float b0 = st[j], b1 = st[(size_t)n + j], b2 = st[2 * (size_t)n + j], b3 = st[3 * (size_t)n + j];
      // (a dropped row: max = +inf, 1 / n_k = 0, so each of its terms is exp(-inf) = 0 or 0)
      float H = (expf((s - a0) - a1) + expf((s - b0) - b1)) * inv_tau;
      if (pos) {
        if (out) H -= a2 + b2;
        else H -= (expf((s - a2) - a3) + expf((s - b2) - b3)) * inv_tau;
      }
      H *= c;
      if (H != 0.f) sim_grad_row<DM>(A.sim, mi, li, ni, clamped_i, mj, lj, nj, S, H, d, gm, gl);
    }
  }
  if (!valid) return;
#pragma unroll
  for (int k = 0; k < DM; ++k) {
    if (k < d) {
      gm[k] = wave_sum(gm[k]);
      if (need_lv) gl[k] = wave_sum(gl[k]);
    }
  }
  // lane k writes component k (one coalesced row store)
  float om = 0.f, ol = 0.f;
#pragma unroll
  for (int k = 0; k < DM; ++k)
    if (k == lane) { om = gm[k]; ol = need_lv ? gl[k] : 0.f; }
  if (lane < d) {
    if (ACC) {  // (this element of this branch belongs to this lane alone)
      float* pm = A.dmu + (size_t)i * A.gld + lane;
      *pm = *pm + om;
      if (need_lv && A.dlv) {
        float* pl = A.dlv + (size_t)i * A.gld + lane;
        *pl = *pl + ol;
      }
    } else {
      A.dmu[(size_t)i * A.gld + lane] = om;
      if (A.dlv) A.dlv[(size_t)i * A.gld + lane] = ol;
    }
  }
