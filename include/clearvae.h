/*
 * clearvae.h — C-ABI of libclearvae_hip.so, the MI355X (gfx950) hot path of CLEAR-VAE training.
 *
 * The reference (scotsun/clear-vae) is pure PyTorch eager and has no FFI; every entry point below
 * replaces a group of ATen calls made by the reference's Python code.  Each declaration cites the
 * reference lines (paths relative to the reference's repo root) whose arithmetic it implements.
 * The Python binding is clear-vae_amd/cvhip/_lib.py (ctypes); see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a device pointer owned by the caller (PyTorch's caching allocator); the library
 *     never allocates, frees or synchronises, so every call can be captured into a HIP graph;
 *   - activations are NHWC fp32 ("pixels x channels" row-major); weights keep PyTorch's layouts
 *     (Conv2d [Cout][Cin][kh][kw], ConvTranspose2d [Cin][Cout][kh][kw], Linear [out][in]);
 *   - BatchNorm batch statistics are accumulated in fp64 by the producing kernel's epilogue into
 *     CV_STAT_REPL(C) replicas of [2][C] doubles (sum, sum of squares / sum dz, sum dz*xhat); when the
 *     layer carries a ticket (cv_bn.ticket), the last workgroup of the producing launch folds them into
 *     per-channel constants (cv_bn.cfwd / cv_bn.cbwd) that consuming GEMMs load in their prologue,
 *     otherwise each consumer folds the replicas itself (the normalised activation is never written
 *     to HBM);
 *   - return value 0 = success; otherwise cv_last_error() describes the failure (host-side checks
 *     run before any launch, so a failing call enqueues nothing).
 */
#ifndef CLEARVAE_H
#define CLEARVAE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cv_stream_t; /* a hipStream_t (torch.cuda.current_stream().cuda_stream) */

/* Replicas of a C-feature statistics buffer: narrow layers get more replicas so that the fp64
 * atomics of thousands of producer workgroups do not serialise on a few addresses. */
#define CV_REC_REPL 32
#define CV_STAT_REPL(C) ((C) >= 256 ? 8 : (C) >= 64 ? 16 : 32)
#define CV_TICKET_WORDS 130

/* ---- BatchNorm as seen by a fused prologue/epilogue (nn.BatchNorm1d/2d, vae.py:17-44, 115-154) ---- */
typedef struct cv_bn {
  const float* gamma;        /* [C] PyTorch order                                              */
  const float* beta;         /* [C]                                                            */
  const double* stat;        /* [CV_STAT_REPL(C)][2][C] forward sums (sum x, sum x^2)         */
  const double* gstat;       /* [CV_STAT_REPL(C)][2][C] backward sums (sum dz, sum dz*xhat)   */
  const float* running_mean; /* [C]                                                            */
  const float* running_var;  /* [C]                                                            */
  int C;                     /* normalised features                                            */
  int count;                 /* elements per feature in the batch (N*H*W, or N for BN1d)       */
  int train;                 /* 1: batch statistics, 0: running statistics (eval mode)         */
  float eps;
  /* Finalised constants (train mode; optional).  A launch of the specialised GEMM core that produces
   * this layer's forward sums (CV_STAT_FWD epilogue with this layer as ebn) elects its last workgroup
   * with ticket[0] and writes cfwd = [sc][mu][beta][istd] (4*C floats, sc = gamma*istd); one that
   * produces the backward sums (CV_STAT_BWD epilogue) uses ticket[1] and writes
   * cbwd = [sc][c1][mu][istd][c2] (5*C floats, c1 = sum dz / n, c2 = sum dz*xhat / n).  A consuming
   * GEMM uses cfwd / cbwd only when the matching ticket is non-zero (its producer finalised) and
   * otherwise folds the replica sums itself; every other producer leaves the ticket at zero.  The
   * arrivals are counted in two levels (<= 64 groups of workgroups, CV_TICKET_WORDS words:
   * ticket[0..1] = groups done, then 64 group counters per direction) so thousands of workgroups do
   * not serialise on one address.  All words must be zero before the producing launch (they live in
   * the zeroed statistics arena). */
  float* cfwd;
  float* cbwd;
  unsigned int* ticket;      /* [CV_TICKET_WORDS] */
} cv_bn;

/* transform applied while an operand is staged into LDS */
enum { CV_XF_NONE = 0, CV_XF_BNRELU = 1, CV_XF_BNBWD = 2 };
/*   CV_XF_BNRELU : v = max(x*gamma*istd + (beta - mean*gamma*istd), 0)               (BN fwd + ReLU)
 *   CV_XF_BNBWD  : v = gamma*istd*(dz - sum(dz)/n - xhat*sum(dz*xhat)/n), xhat from y  (BN bwd)      */

typedef struct cv_operand {
  const float* x;  /* primary tensor: activation, or dz (masked upstream gradient) for BNBWD    */
  const float* y;  /* BNBWD only: the BN layer's input (pre-BN values), same layout as x        */
  int xf;          /* CV_XF_*                                                                  */
  int nchw;        /* 1: x is NCHW (network input, channels not a multiple of 4); else NHWC    */
  cv_bn bn;        /* constants source for the transform                                       */
} cv_operand;

/* epilogue statistics of the produced tensor */
enum { CV_STAT_NONE = 0, CV_STAT_FWD = 1, CV_STAT_BWD = 2 };
/*   CV_STAT_FWD: out is the input of a BN layer; accumulate (sum v, sum v^2) into stat_out.
 *   CV_STAT_BWD: out is d(post-ReLU activation) of BN layer `ebn` whose input is `ey`; the kernel
 *                stores dz = v * [relu active] and accumulates (sum dz, sum dz*xhat) into stat_out. */

typedef struct cv_epilogue {
  int stat_mode;      /* CV_STAT_*                                                  */
  double* stat_out;   /* [REPL][2][C]                                               */
  int stat_div;       /* feature index = column / stat_div (1 = per column)         */
  const float* ey;    /* STAT_BWD: pre-BN values at the output positions            */
  cv_bn ebn;          /* the BN layer fed by this output: STAT_BWD needs its batch statistics;
                         with ebn.ticket set (either mode) the producer finalises its constants */
  int erelu;          /* STAT_BWD: 1 if ReLU follows that BN                        */
} cv_epilogue;

/* Operand precision of a conv / linear contraction.  CV_MMA_BF16 (BASELINE configs[4], "bf16"): the
 * specialised MFMA core rounds both operands to bf16 as it stages them into LDS (after the fp32 BatchNorm
 * transform) and contracts on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; activations, BatchNorm
 * statistics and epilogues stay fp32.  Calls the core does not serve (image-facing edge layers) stay
 * fp32.  The reference is fp32 only (CV_MMA_FP32, the default). */
enum { CV_MMA_FP32 = 0, CV_MMA_BF16 = 1 };

/* ---- convolution geometry (nn.Conv2d / nn.ConvTranspose2d, vae.py:15-46, 113-156) ---- */
typedef struct cv_conv {
  int n;                          /* batch                                         */
  int c_in, h_in, w_in;           /* layer input  (NHWC)                           */
  int c_out, h_out, w_out;        /* layer output (NHWC)                           */
  int kh, kw, stride, pad;
  int transposed;                 /* 0 Conv2d, 1 ConvTranspose2d                   */
  int mma;                        /* CV_MMA_*: operand precision of the contraction */
} cv_conv;

/* GEMM-native copies of a conv / convT weight, refreshed once per optimizer step.  With
 * w(cs, cb, tap) = W[cs][cb][kh][kw] (PyTorch layout; cs = out channels for Conv2d, in channels for
 * ConvTranspose2d): gather = Wg[tap][cb][cs], scatter = Ws[tap][cs][cb].  Conv2d forward and
 * ConvTranspose2d backward-data read `gather`; Conv2d backward-data and ConvTranspose2d forward read
 * `scatter`.  Up to 16 weights per call (one launch). */
typedef struct cv_conv_pack {
  const float* src; float* gather; float* scatter;
  int cs, cb, kh, kw;
} cv_conv_pack;
int cv_pack_conv_weights(const cv_conv_pack* items, int n, cv_stream_t stream);
/* cv_pack_conv_weights plus, in the same launch, zeroing of up to 8 buffers (4-byte granular) that are not
 * touched by the packing: the first launch of a training step clears the step's accumulators with it. */
int cv_pack_conv_weights_zero(const cv_conv_pack* items, int n, void* const* zero_ptrs, const size_t* zero_bytes,
                              int zero_count, cv_stream_t stream);
/* (cv_pack_conv_weights_zero / _zero_copy accept n = 0 items when they have buffers to zero or copy) */
/* torch.optim.Adam over a flat parameter arena (cv_adam_step, trainer.py:483) with the weight packing of
 * cv_pack_conv_weights in the same launch: the packing workgroups update their tile's parameters and pack the new
 * values (the items' src must lie inside params[0, numel)), the rest of the arena is updated by the launch's other
 * workgroups; the last workgroup advances step[0] (and aux_counter).  The packed copies are then current for the
 * next step's forward without a packing launch. */
int cv_adam_pack_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel,
                      const float* hyper, int64_t* step, const float* grad_scale, int64_t* aux_counter,
                      const cv_conv_pack* items, int n, cv_stream_t stream);
/* cv_adam_pack_step over a part of the arena (params .. params + numel, the items inside it) that leaves the step
 * counters as they are when advance = 0: a split update whose parts run at different points of the step (the
 * decoder's parameters as soon as the step has read them, beside the encoder backward); the part with advance = 1
 * (issued after the others, same step) advances step[0] and aux_counter.  Every part computes the bias correction
 * from the same step[0]. */
int cv_adam_pack_step_part(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel,
                           const float* hyper, int64_t* step, const float* grad_scale, int64_t* aux_counter,
                           const cv_conv_pack* items, int n, int advance, cv_stream_t stream);
/* cv_pack_conv_weights_zero plus up to 4 device copies (16-byte aligned and sized) in the same launch: the fused
 * step's first launch of a replayed step also moves the batch (X, labels: trainer.py:447-450's `X.to(device)` of a
 * device-resident batch) into the step graph's static input buffers, so the copy is not a launch of its own. */
int cv_pack_conv_weights_zero_copy(const cv_conv_pack* items, int n, void* const* zero_ptrs, const size_t* zero_bytes,
                                   int zero_count, void* const* copy_dst, const void* const* copy_src,
                                   const size_t* copy_bytes, int copy_count, cv_stream_t stream);

/* y = conv(T(x)) + bias.  Replaces nn.Conv2d/ConvTranspose2d.forward (vae.py:15-46) with the
 * preceding BatchNorm2d+ReLU fused into the operand load and the following BatchNorm2d's batch
 * statistics fused into the epilogue.  wpacked: the `gather` (Conv2d) or `scatter`
 * (ConvTranspose2d) packing of cv_pack_conv_weights. */
int cv_conv_forward(const cv_conv* g, const cv_operand* in, const float* wpacked, const float* bias,
                    float* out, const cv_epilogue* ep, cv_stream_t stream);

/* dx = conv^T(T(dy)).  Replaces the grad_input half of aten::convolution_backward.
 * wpacked: `scatter` (Conv2d) or `gather` (ConvTranspose2d) packing. */
int cv_conv_backward_data(const cv_conv* g, const cv_operand* gout, const float* wpacked,
                          float* gin, const cv_epilogue* ep, cv_stream_t stream);

/* The same calls given also wkpack = the OTHER packing of the same weight (the one wpacked is not: for a
 * stride-2 SCATTER contraction — Conv2d backward-data, ConvTranspose2d forward — the `gather` packing
 * [tap][cb][cs]; for a GATHER — Conv2d forward, ConvTranspose2d backward-data — the `scatter` packing
 * [tap][cs][cb]; i.e. the contraction's B operand k-contiguous per output channel; NULL allowed).  Results are
 * those of the calls without it; with it the library may run the contraction as one direct launch that stages
 * the operand's band in LDS once per workgroup and walks all taps (and, for SCATTER, all four stride-parity
 * classes) from there (cv_direct.hip) instead of implicit GEMMs that re-load it per tap.  Replaces the same
 * ATen calls (vae.py:15-46, 113-156). */
int cv_conv_forward_kpack(const cv_conv* g, const cv_operand* in, const float* wpacked, const float* wkpack,
                          const float* bias, float* out, const cv_epilogue* ep, cv_stream_t stream);
int cv_conv_backward_data_kpack(const cv_conv* g, const cv_operand* gout, const float* wpacked,
                                const float* wkpack, float* gin, const cv_epilogue* ep, cv_stream_t stream);

/* dw += sum_pixels T(x) (x) T(dy).  Replaces the grad_weight half of aten::convolution_backward.
 * gbias (optional, Conv2d only) += sum_pixels T(dy).  The pixel sum is split over workgroups
 * (split_k <= 0: automatic); the partial tiles go to `work` (cv_conv_wgrad_workspace_bytes) and one
 * reduction launch adds them into gweight/gbias.  With work == NULL the partials are fp32 atomics
 * into gweight/gbias instead (correct, slower).  Either way the result is added to gweight/gbias. */
size_t cv_conv_wgrad_workspace_bytes(const cv_conv* g, int split_k);
int cv_conv_backward_weight(const cv_conv* g, const cv_operand* in, const cv_operand* gout,
                            float* gweight, float* gbias, int split_k, float* work, size_t work_bytes,
                            cv_stream_t stream);

/* Deferred weight gradients: the same contraction as cv_conv_backward_weight (split_k automatic, `work`
 * required) but the split-K partial tiles stay in `work` and their layout is written to *defer (host
 * struct, filled at enqueue time) instead of launching the reduction; cv_step_reduce sums them later,
 * together with every other deferred gradient of the step, in one launch.  defer->split == 0: the
 * launch wrote gweight / gbias directly (nothing to reduce).  `work` must stay untouched until then. */
typedef struct cv_wgrad_defer {
  const float* part;   /* [split][M][ntot] partial tiles                                   */
  int split, M, N, ntot, cb, kk;
  float* gweight;      /* += sum over splits, element (m, col = tap*cb + c) -> [m][c][tap]  */
  float* gbias;        /* column N (if ntot > N): += row sums                              */
} cv_wgrad_defer;
int cv_conv_backward_weight_deferred(const cv_conv* g, const cv_operand* in, const cv_operand* gout,
                                     float* gweight, float* gbias, float* work, size_t work_bytes,
                                     cv_wgrad_defer* defer, cv_stream_t stream);

/* Both halves of a conv / convT backward (aten::convolution_backward, trainer.py:482): dx as
 * cv_conv_backward_data and the deferred weight gradient as cv_conv_backward_weight_deferred, in one launch for
 * the image-side ConvTranspose2d (vae.py:43 / :153: the edge kernels' geometry, ep's BatchNorm = in's
 * transform), otherwise the two launches in that order. */
int cv_conv_backward_deferred(const cv_conv* g, const cv_operand* gout, const float* wpacked, float* gin,
                              const cv_epilogue* ep, const cv_operand* in, float* gweight, float* gbias, float* work,
                              size_t work_bytes, cv_wgrad_defer* defer, cv_stream_t stream);
/* cv_conv_backward_deferred with the other packing of the weight (see cv_conv_forward_kpack) */
int cv_conv_backward_deferred_kpack(const cv_conv* g, const cv_operand* gout, const float* wpacked,
                                    const float* wkpack, float* gin, const cv_epilogue* ep, const cv_operand* in,
                                    float* gweight, float* gbias, float* work, size_t work_bytes,
                                    cv_wgrad_defer* defer, cv_stream_t stream);
/* cv_conv_backward_deferred_kpack with the weight-gradient launch on `side` where the pair is not one dual grid:
 * `side` waits for the work issued on `stream` before the call (an event; in a capture the side stream joins the
 * graph there), then runs the weight gradient beside this and the next layers' backward-data launches.  The caller
 * joins `side` back into `stream` before the deferred partials are read (cv_step_reduce).  Dual grids, the
 * image-side ConvTranspose2d's fused launch and the self-reducing split (CV_WGRAD_SELF) stay on `stream`;
 * side = NULL or = stream: cv_conv_backward_deferred_kpack. */
int cv_conv_backward_deferred_kpack_side(const cv_conv* g, const cv_operand* gout, const float* wpacked,
                                         const float* wkpack, float* gin, const cv_epilogue* ep,
                                         const cv_operand* in, float* gweight, float* gbias, float* work,
                                         size_t work_bytes, cv_wgrad_defer* defer, cv_stream_t side,
                                         cv_stream_t stream);

/* ---- fully connected layers (nn.Linear heads vae.py:27-30; decoder Linear vae.py:33) ----
 * A linear layer whose input (or output) is the NCHW-flattened view of an NHWC activation with
 * `*_pix` pixels and `*_ch` channels (nn.Flatten vae.py:25 / nn.Unflatten vae.py:36).              */
typedef struct cv_linear {
  int n;               /* batch rows                         */
  int in_features, out_features;
  int in_pix, in_ch;   /* in_features = in_pix*in_ch, or in_pix = 1 for a plain row-major input   */
  int out_pix, out_ch; /* same for the output                                                      */
  int mma;             /* CV_MMA_*                                                                  */
} cv_linear;

int cv_linear_forward(const cv_linear* g, const cv_operand* in, const float* weight,
                      const float* bias, float* out, int accumulate, const cv_epilogue* ep,
                      cv_stream_t stream);
int cv_linear_backward_data(const cv_linear* g, const cv_operand* gout, const float* weight,
                            float* gin, int accumulate, const cv_epilogue* ep, cv_stream_t stream);
/* dW += sum_n gout[n] (x) T(in[n]) (+ gbias), same split/workspace contract as the conv version. */
size_t cv_linear_wgrad_workspace_bytes(const cv_linear* g, int split_k);
int cv_linear_backward_weight(const cv_linear* g, const cv_operand* gout, const cv_operand* in,
                              float* gweight, float* gbias, int split_k, float* work, size_t work_bytes,
                              cv_stream_t stream);

int cv_linear_backward_weight_deferred(const cv_linear* g, const cv_operand* gout, const cv_operand* in,
                                       float* gweight, float* gbias, float* work, size_t work_bytes,
                                       cv_wgrad_defer* defer, cv_stream_t stream);

/* Decoder Linear -> BatchNorm1d -> ReLU backward (vae.py:33-35).  da: gradient w.r.t. the ReLU
 * output in the Unflatten/NHWC order (g->out_pix, g->out_ch); h: the Linear output (BN1d input),
 * same order.  Two launches: (1) mask da in place (da <- dz) and accumulate the BN1d backward sums
 * into gstat_out (fp64, replicas; caller zeroes); (2) accumulate the Linear weight gradient
 * dW[f][k] += sum_n BNbwd(dz)[n][f] * zin[n][k] (caller zeroes).  gweight == NULL runs only (1);
 * gstat_out == NULL runs only (2) on an already masked da with bn->gstat holding the sums (so the
 * weight gradient can run off the critical path, on another stream, after (1)). */
int cv_declinear_backward_weight(const cv_linear* g, float* da, const float* h, const cv_bn* bn,
                                 double* gstat_out, const float* zin, float* gweight,
                                 cv_stream_t stream);

/* The decoder's input block in one launch each way (cv_declinear.hip): a workgroup owns 16 features of the
 * [n][out_features] activation for the whole batch, so the BatchNorm1d statistics are complete inside it.
 * Forward (VAE.sample vae.py:56-60, then decoder Linear -> BatchNorm1d -> ReLU vae.py:33-35): heads != NULL:
 * z = mu + eps*exp(lv/2) from heads [n][4d] exactly as cv_reparam_forward (eps injected, or Philox(seed,
 * offset[0]) with offset advanced once), written to z; heads == NULL: z [n][2d] is the input.  h = Linear(z)
 * (storage order out_pix/out_ch), ah = ReLU(BN1d(h)); train: the complete batch sums of h are written to
 * replica 0 of stat_out [REPL][2][F] (the other replicas must be zero).  Replaces cv_reparam_forward +
 * cv_linear_forward + cv_bn_apply.
 * Backward (trainer.py:482 through vae.py:33-35): ga [n][F] = d(ReLU output) is overwritten with d(h) (ReLU
 * mask, then the BN1d backward transform); gstat_out replica 0 receives the complete backward sums; gweight
 * [F][2d] += d(h)^T z; with dz != NULL also dz [n][2d] += d(h) W (weight = the Linear's [F][2d]; each workgroup
 * adds its 16 features' share with fp32 atomics, the caller zeroes dz), else dz is left to
 * cv_linear_backward_data on d(h).  Replaces the two launches of cv_declinear_backward_weight (and the dz GEMM).  Contract: cv_decoder_input_supported(n, d, F) (n*2d <= 16384,
  * 2d <= 128, F % 16 == 0, d even). */
int cv_decoder_input_supported(int n, int d, int features);
int cv_decoder_input_forward(const cv_linear* g, const float* heads, const float* eps, uint64_t seed,
                             uint64_t* offset, float* z, const float* weight, const float* bias, const cv_bn* bn,
                             double* stat_out, float* h, float* ah, cv_stream_t stream);
int cv_decoder_input_backward(const cv_linear* g, float* ga, const float* h, const cv_bn* bn, double* gstat_out,
                              const float* z, float* gweight, const float* weight, float* dz, cv_stream_t stream);

/* Encoder heads forward in one launch (the four nn.Linear heads vae.py:27-30 over the Flatten of the last conv
 * block vae.py:25, its BatchNorm2d + ReLU applied to y on load): heads [n][4d] = ReLU(BN(y)) W^T + bias with W
 * packed [in_features (storage order)][4d] (cv_conv_pack of the [4d][C][Hh][Wh] view, `gather` order), and, when
 * z != NULL, the reparameterisation of its rows exactly as cv_reparam_forward (vae.py:56-60).  Replaces
 * cv_linear_forward of the heads (+ cv_reparam_forward).  Contract: cv_heads_forward_supported(n,
 * in_features, in_ch, d) (d = 8 or a multiple of 16 up to 64, in_ch % 4 == 0, in_ch <= 512). */
int cv_heads_forward_supported(int n, int in_features, int in_ch, int d);
int cv_heads_forward(const cv_linear* g, const float* y, const cv_bn* bn, const float* wpacked, const float* bias,
                     float* heads, const float* eps, uint64_t seed, uint64_t* offset, float* z, cv_stream_t stream);

/* Encoder heads backward in one launch (the four nn.Linear heads vae.py:27-30 as one [4d][F] weight over the
 * Flatten of the last conv block, vae.py:25; trainer.py:482): gin [n][F] (storage order in_pix/in_ch) =
 * (dheads W) * [BN(y) > 0] with that BatchNorm2d's backward sums added to gstat_out (fp64 replicas; the layer's
 * cbwd constants are finalised by the last workgroup when bn carries a ticket), gweight [4d][F] +=
 * dheads^T ReLU(BN(y)), gbias [4d] += column sums of dheads.  Replaces cv_linear_backward_data with a
 * CV_STAT_BWD epilogue plus cv_linear_backward_weight(_deferred) of the heads.  Contract:
 * cv_heads_backward_supported(n, in_features, in_ch, out_features) (4d <= 128, dheads staged in LDS). */
int cv_heads_backward_supported(int n, int in_features, int in_ch, int out_features);
int cv_heads_backward(const cv_linear* g, const float* dheads, const float* weight, const float* y, const cv_bn* bn,
                      float* gin, double* gstat_out, float* gweight, float* gbias, cv_stream_t stream);
/* The decoder gradient chained through the reparameterisation z = mu + eps * exp(logvar / 2) (vae.py:56-60),
 * applied by cv_heads_backward_chain while it stages dheads: column block b of a row (mu_c, lv_c, mu_s, lv_s) gets
 * + dz[z index] (mu blocks) or + dz * (z - mu) / 2 (logvar blocks), z index = (b / 2) * d + k — the chain term of
 * cv_latent_combine, so that the KL part of the combine can run earlier in the step (cv_ntxent_aux_combine) and
 * the decoder's dz is consumed where dheads is.  dheads itself is not rewritten.  rec_in / losses (optional):
 * losses[0] = the sum of the CV_REC_REPL replicas of rec_in. */
typedef struct cv_latent_chain {
  const float* heads;  /* [n][4d] */
  const float* z;      /* [n][2d] */
  const float* dz;     /* [n][2d] */
  int d;
  const double* rec_in;
  float* losses;
} cv_latent_chain;
int cv_heads_backward_chain(const cv_linear* g, const float* dheads, const cv_latent_chain* chain, const float* weight,
                            const float* y, const cv_bn* bn, float* gin, double* gstat_out, float* gweight,
                            float* gbias, cv_stream_t stream);

/* out = max(BN(x), 0) elementwise for a BatchNorm1d over `features` PyTorch-order features whose
 * tensor is stored in the Unflatten/NHWC order (pix, ch) (vae.py:34-36); rows = batch. */
int cv_bn_apply(const cv_bn* bn, const float* x, float* out, int rows, int features, int pix, int ch,
                int relu, cv_stream_t stream);

/* ---- BatchNorm running statistics (nn.BatchNorm*, momentum 0.1, unbiased running var) ---- */
int cv_bn_update_running(const cv_bn* bn, int nlayers, float momentum,
                         int64_t* const* num_batches_tracked, cv_stream_t stream);
/* nsets forwards' momentum updates of the same nlayers BatchNorms in one launch, applied in set order: bn is
 * [nsets][nlayers] (set-major; layer i of every set names the same running buffers, count and C, with its own
 * batch sums in .stat); num_batches_tracked advances by nsets (CLEAR-MIM's five estimator forwards,
 * trainer.py:873-888). */
int cv_bn_update_running_sets(const cv_bn* bn, int nlayers, int nsets, float momentum, int64_t* const* nbt,
                              cv_stream_t stream);
/* copy batch stats into (mean, invstd) float arrays (for tests / PyTorch-visible save_mean) */
int cv_bn_batch_stats(const cv_bn* bn, float* mean, float* invstd, cv_stream_t stream);

/* ---- decoder output: BatchNorm2d(C) + Sigmoid (vae.py:44-45) ---- */
/* xhat = sigmoid(BN(y)), written NCHW [n][c][h][w]; y is NHWC [n][h][w][c]. */
int cv_output_forward(const cv_bn* bn, const float* y, int n, int c, int hw, float* xhat,
                      cv_stream_t stream);
/* fused output + reconstruction loss (losses.py:36-47): rec = mean_n sum_chw (xhat - x)^2,
 * accumulated into the CV_REC_REPL fp64 replicas rec_out[0..CV_REC_REPL) (caller zeroes; rec is
 * their sum), and when dv_out != NULL the gradient of
 * (rec_scale*rec) w.r.t. the BN output: dv = rec_scale*2(xhat-x)/n * xhat(1-xhat) (NHWC), plus the
 * BN backward sums into gstat_out.  rec_scale may be NULL (1.0). x is NCHW. */
int cv_output_loss(const cv_bn* bn, const float* y, const float* x, int n, int c, int hw,
                   float* xhat, double* rec_out, float* dv_out, double* gstat_out,
                   const float* rec_scale, cv_stream_t stream);
/* The last ConvTranspose2d (vae.py:43 / :153) and cv_output_loss in one call: y = convT(T(in)) + bias with its
 * output BatchNorm's sums (ep, CV_STAT_FWD into bn->stat), then the decoder output, the reconstruction term and
 * its backward seed exactly as cv_output_loss.  One launch when the edge kernel serves the layer and its whole
 * grid is resident at once (the workgroups meet at a bounded grid-wide wait for the BN sums); else the two
 * calls. */
int cv_convt_output_loss(const cv_conv* g, const cv_operand* in, const float* wpacked, const float* bias, float* y,
                         const cv_epilogue* ep, const cv_bn* bn, const float* x, float* xhat, double* rec_out,
                         float* dv_out, double* gstat_out, const float* rec_scale, cv_stream_t stream);
/* backward of xhat = sigmoid(BN(y)) given dxhat (NCHW): dv (NHWC) + BN backward sums. */
int cv_output_backward(const cv_bn* bn, const float* y, const float* xhat, const float* dxhat,
                       int n, int c, int hw, float* dv_out, double* gstat_out, cv_stream_t stream);

/* ---- reparameterisation (vae.py:56-79) ---- */
/* heads: [n][4d] = (mu_c | logvar_c | mu_s | logvar_s); z: [n][2d] = (z_c | z_s).
 * eps == NULL: eps ~ N(0,1) from a counter-based Philox4x32-10 stream keyed by (seed, offset[0]);
 * offset is a device uint64[2] (counter, zeroed arrival word) advanced by the kernel (graph-replay
 * safe).  eps != NULL: [n][2d]
 * injected noise (test hook).  eps_out (optional) receives the noise used. */
int cv_reparam_forward(const float* heads, int n, int d, const float* eps, uint64_t seed,
                       uint64_t* offset, float* z, float* eps_out, cv_stream_t stream);

/* VAE.sample for one factor (vae.py:56-60): z = mu + eps*exp(0.5*logvar), [n][d] contiguous;
 * eps injected or drawn from Philox(seed, offset[0]) (offset advanced).  Backward:
 * dmu = dz, dlogvar = dz*(z-mu)/2 (accumulated into dmu/dlogvar when accumulate != 0). */
int cv_sample_forward(const float* mu, const float* logvar, long numel, const float* eps,
                      uint64_t seed, uint64_t* offset, float* z, cv_stream_t stream);
int cv_sample_backward(const float* mu, const float* z, const float* dz, long numel, float* dmu,
                       float* dlogvar, int accumulate, cv_stream_t stream);

/* ---- latent-space losses (losses.py:41-137) ---- */
enum { CV_SIM_COSINE = 0, CV_SIM_L2 = 1, CV_SIM_MODIFIED_L2 = 2, CV_SIM_JEFFREY = 3,
       CV_SIM_MAHALANOBIS = 4 };

/* KL term of vae_loss (losses.py:48-49): kl = -0.5 * mean_n sum_d(1 + lv - mu^2 - exp(lv));
 * with dmu/dlogvar != NULL also writes (or accumulates) gscale[0] * d kl / d(mu, logvar). */
int cv_kl(const float* mu, const float* logvar, int ld, int n, int d, float* kl_out,
          const float* gscale, float* dmu, float* dlogvar, int gld, int accumulate,
          cv_stream_t stream);

/* Fused-step seed of d(heads): KL(c), KL(s) with the LogisticAnnealer weight
 * w = beta/(1+exp(-(t-loc)/scale)), t = anneal_step[0] (trainer.py:22-38, 474-477), plus the decoder
 * gradient dz chained through z = mu + eps*exp(lv/2).  losses[0] = sum of the CV_REC_REPL
 * replicas rec_in[] of cv_output_loss (if given),
 * losses[1], losses[2] = kl_c, kl_s; losses[7] = w.  dheads is overwritten. */
int cv_latent_combine(const float* heads, const float* z, const float* dz, int n, int d, float beta,
                      float loc, float scale, const int64_t* anneal_step, const double* rec_in,
                      float* dheads, float* losses, double* work, cv_stream_t stream);
/* cv_latent_combine with dheads += instead of overwritten: the fused step whose NT-Xent gradients were already
 * accumulated into a zeroed dheads — the default schedule (cvhip/engine.py LATENT_AUX: the NT-Xent phases ride in the
 * decoder's ConvTranspose2d forward grids and this call follows the decoder backward). */
int cv_latent_combine_acc(const float* heads, const float* z, const float* dz, int n, int d, float beta,
                          float loc, float scale, const int64_t* anneal_step, const double* rec_in,
                          float* dheads, float* losses, double* work, cv_stream_t stream);
/* work (or NULL): a caller-owned device workspace of cv_latent_combine_workspace_bytes(), zeroed once before its
 * first use (it is left zeroed after every call).  With it, batches of n x 2d >= 4096 elements run over several
 * workgroups whose KL partials are summed in workgroup order by the last to arrive (bit-reproducible, independent of
 * arrival order); NULL runs the one-workgroup kernel.  Two launches that may overlap in time (two streams) need two
 * workspaces. */
size_t cv_latent_combine_workspace_bytes(void);
/* cv_latent_combine(_acc) (accumulate 0 / 1) with the decoder-input gradient computed here: dz = d(h) W, d(h) the
 * decoder Linear's output gradient [n][F] in storage order (cv_decoder_input_backward's `ga` after the call, with
 * dz = NULL there), W the Linear weight [F][2d] (lin: the decoder Linear's geometry, out_pix / out_ch its Unflatten;
 * F % 64 == 0).  Deterministic: every dz element is one fixed-order sum (the atomics of the decoder-input backward's
 * dz partials were the fused step's only order-dependent sum).  dz_out (or NULL) receives dz.  work (required): a
 * caller-owned device workspace of cv_latent_combine_dz_workspace_bytes(n, d), zeroed once before its first use. */
size_t cv_latent_combine_dz_workspace_bytes(int n, int d);
int cv_latent_combine_dz(const float* heads, const float* z, const float* dh, const float* weight, const cv_linear* lin,
                         float beta, float loc, float scale, const int64_t* anneal_step, const double* rec_in,
                         float* dheads, float* losses, float* dz_out, int accumulate, double* work, cv_stream_t stream);

/* reconstruction term (losses.py:45-47) for the autograd path: rec = mean_n sum (xhat - x)^2;
 * work: one zeroed fp64 word.  dxhat != NULL: dxhat = gscale[0] * 2 (xhat - x) / n. */
int cv_mse_sum(const float* xhat, const float* x, int n, int per_sample, float* rec_out,
               const float* gscale, float* dxhat, double* work, cv_stream_t stream);

/* SNN / NT-Xent contrastive loss (losses.py:98-137) for up to 2 branches sharing labels
 * (content: pairs with equal labels; style with ps=1: pairs with different labels,
 * trainer.py:456-472).  phase 0: row log-sum-exps into lse; phase 1: loss (mean over finite rows,
 * losses.py:125-126) and, when dmu != NULL, the gradient gmul*gscale[0]*dloss/d(mu, logvar);
 * phase 2: both. */
typedef struct cv_ntxent_branch {
  const float* mu; const float* logvar; int ld;   /* [n] rows of stride ld               */
  int ps;
  float* dmu; float* dlogvar; int gld;            /* gradient outputs (may be NULL)       */
  const float* gscale; float gmul;                /* upstream gradient                    */
  float* loss_out;                                /* [1]                                  */
  float* lse;                                     /* workspace [2n]                       */
} cv_ntxent_branch;
int cv_ntxent(const cv_ntxent_branch* br, int nbr, const int64_t* label, int n, int d, int sim,
              float temperature, int phase, int accumulate, cv_stream_t stream);
/* An NT-Xent phase of cv_ntxent (phase 0: the row log-sum-exps; 1: the losses and gradients, accumulated into the
 * branches' d(mu) / d(logvar) when accumulate) queued to run as extra workgroups of this thread's next direct-kernel
 * conv launch on the SAME `stream` (cv_aux.hip: MNIST's decoder ConvTranspose2d forwards serve it; a launch on another
 * stream leaves it queued); the call after that conv must be cv_ntxent_aux_flush, which launches the phase on its own,
 * on the stream it was queued for, if no launch took it.  One phase at a time (a phase still queued when the next is
 * queued is launched first, on its own stream); the phases read only the heads and labels (trainer.py:474-479,
 * losses.py:98-137), so the fused step queues them into its decoder forward.  The branch gradients must not be read
 * before the flush.  cv_ntxent_aux_discard drops a queued phase without launching it (returns 1 if one was queued):
 * the engine calls it when a program raises between the queue and its flush.  cv_ntxent_aux_pending: 0, or 1 + the
 * queued phase (test hook). */
int cv_ntxent_aux(const cv_ntxent_branch* br, int nbr, const int64_t* label, int n, int d, int sim, float temperature,
                  int phase, int accumulate, cv_stream_t stream);
int cv_ntxent_aux_flush(cv_stream_t stream);
int cv_ntxent_aux_discard(void);
int cv_ntxent_aux_pending(void);
/* Attach the KL part of the latent combine (cv_latent_combine with dz = NULL and rec_in = NULL: losses[1], [2], [7]
 * and dheads = the KL gradient, overwritten — dheads must not hold anything yet) to the queued phase-0 request, as
 * one more workgroup of the same grid (or of the flush launch).  The decoder chain term follows in
 * cv_heads_backward_chain.  Requires a queued phase 0 (else an error). */
int cv_ntxent_aux_combine(const float* heads, const float* z, int n, int d, float beta, float loc, float scale,
                          const int64_t* anneal_step, float* dheads, float* losses, cv_stream_t stream);

/* The fused step's latent terms in two launches (trainer.py:452-480): cv_latent_combine (KL with the
 * annealer weight, the decoder gradient chained through z) and cv_ntxent phase 2 with accumulate = 1
 * on the same dheads.  The combine runs as an extra workgroup of the row-log-sum-exp launch (it does
 * not depend on it); every branch's dmu / dlogvar must point into dheads. */
int cv_latent_step(const float* heads, const float* z, const float* dz, int n, int d, float beta,
                   float loc, float scale, const int64_t* anneal_step, const double* rec_in,
                   float* dheads, float* losses, const cv_ntxent_branch* br, int nbr,
                   const int64_t* label, int sim, float temperature, cv_stream_t stream);

/* ---- SupCon contrastive losses (losses.py:140-170, composed by contrastive_loss :98-126) ----
 * S = pairwise_<sim>(mu, logvar), P_ij = [label_i == label_j] (ps: [label_i != label_j]), tau = temperature; cosine
 * clamps each norm at 1e-8 as cv_ntxent does.  The reference's quirks are kept:
 *   CV_SUPCON_IN  (losses.py:140-153): n_k[i] = sum_j P_ij - 1 — with ps the diagonal of P is 0, so that is one LESS
 *     than the number of different-label rows; diagonal of S = -inf;
 *     row_i = log n_k[i] - LSE_{j: P_ij, j != i}(S_ij / tau) + LSE_{j != i}(S_ij / tau).
 *   CV_SUPCON_OUT (losses.py:156-170): diagonal of S = -999, a finite value that takes part in the log-sum-exp as
 *     exp(-999 / tau) and carries no gradient; n_k[i] = the off-diagonal positives; rows with n_k = 0 are dropped;
 *     row_i = -(sum_{j != i} P_ij S_ij) / n_k[i] + LSE_j(S_ij / tau): the first term is NOT divided by tau.
 *   loss = the mean over the rows whose value is finite (losses.py:125-126); with no such row the loss is NaN and
 *     every gradient element is exactly 0.
 * Memory is O(n d): phase 0 writes per-row statistics into `stats` and the loss into loss_out; phase 1 reads them and
 * writes gscale[0] * dloss / d(mu, logvar) (overwritten, never accumulated; dlogvar = 0 for cosine / l2).  No atomics:
 * two runs give the same bits.  1 <= n <= 131072, 1 <= d <= 64, every CV_SIM_*, temperature > 0. */
enum { CV_SUPCON_IN = 0, CV_SUPCON_OUT = 1 };
typedef struct cv_supcon_args {
  const float* mu; const float* logvar; int ld;   /* rows of stride ld; logvar NULL allowed for cosine / l2 */
  const int64_t* label;
  int n, d, sim, ps, kind;
  float temperature;
  float* stats;                                   /* [cv_supcon_stats_floats(n)]: phase 0 writes, phase 1 reads */
  float* loss_out;                                /* [1], phase 0 */
  float* dmu; float* dlogvar; int gld;            /* phase 1 outputs (dlogvar NULL allowed for cosine / l2) */
  const float* gscale;                            /* [1] upstream gradient, device memory */
} cv_supcon_args;
/* 1 when the kernels serve the shape: the envelope above */
int    cv_supcon_supported(int n, int d, int sim);
/* floats of the stats workspace for batch n (linear in n) */
size_t cv_supcon_stats_floats(int n);
int    cv_supcon(const cv_supcon_args* a, int phase, cv_stream_t stream);   /* 0: rows + loss, 1: gradients */
/* The step form (the fused CLEAR step's contrastive terms, trainer.py:456-480 with losses.py:98-126, 140-170): up to
 * two branches on the same labels, n, d, sim, kind and temperature, both in the same launches (the branch is a grid
 * dimension): phase 0 is two launches (row statistics, loss fold), phase 1 one.  Per branch the semantics are
 * cv_supcon's, quirks included, but phase 1 ADDS gmul * gscale[0] * dloss / d(mu, logvar) onto what dmu / dlogvar hold
 * (the [n][4d] d(heads) of the step, read and written in place through ld / gld): every element is read and written
 * by one lane, no atomics, so two runs give the same bits; for cosine / l2 the logvar columns are not touched; with no
 * kept row the loss is NaN and exactly 0 is added. The branches' stats workspaces and gradient elements
 * must not overlap.  Same envelope as cv_supcon; no allocation, no synchronisation, capturable. */
typedef struct cv_supcon_branch {
  const float* mu; const float* logvar; int ld;   /* rows of stride ld (logvar NULL allowed for cosine / l2) */
  int ps;
  float* dmu; float* dlogvar; int gld;            /* phase 1: accumulated into, never overwritten */
  const float* gscale; float gmul;                /* upstream: gmul * gscale[0] (gscale: [1], device memory) */
  float* loss_out;                                /* [1], phase 0 */
  float* stats;                                   /* [cv_supcon_stats_floats(n)] per branch */
} cv_supcon_branch;
int    cv_supcon_step(const cv_supcon_branch* br, int nbr, const int64_t* label, int n, int d, int sim, int kind,
                      float temperature, int phase, cv_stream_t stream);   /* nbr 1 or 2; phase 0 | 1 */

/* ---- MI upper bounds (mi_estimator.py:108-198; CLUB: mi_estimator.py:43-55, VarUB: mi_estimator.py:222-224) ---- */
enum { CV_MI_NONE = 0, CV_MI_CLUBSAMPLE = 1, CV_MI_L1OUT = 2, CV_MI_CLUB = 3, CV_MI_VARUB = 4,
       /* CLUBMean (mi_estimator.py:65-105): CLUB with logvar == 0 and no p_logvar network; served by the cv_mi_*
        * entry points with a cv_mlp whose w3, b3, w4, b4 are NULL (and h = hidden_size, not hidden_size // 2) */
       CV_MI_CLUBMEAN = 5,
       /* InfoNCE (mi_estimator.py:245-273): a tag for callers that switch on the estimator; the cv_mi_* entry
        * points reject it, its kernels are the cv_infonce_* entry points below */
       CV_MI_INFONCE = 6 };

/* q(y|x) MLPs (mi_estimator.py:111-122): p_mu = L(dx,h)-ReLU-L(h,dy);
 * p_logvar = L(dx,h)-ReLU-L(h,dy)-Tanh; Linear weights [out][in]; h = hidden_size // 2.
 * CV_MI_CLUBMEAN only: w3 = b3 = w4 = b4 = NULL (logvar == 0), in cv_mlp_grad as well. */
typedef struct cv_mlp {
  const float *w1, *b1, *w2, *b2;   /* p_mu     */
  const float *w3, *b3, *w4, *b4;   /* p_logvar */
  int dx, h, dy;
} cv_mlp;
typedef struct cv_mlp_grad {
  float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
} cv_mlp_grad;

size_t cv_mi_workspace_bytes(int n);
/* CLUBSample.forward (mi_estimator.py:133-143; perm injected, or generated on device from
 * (seed, offset)) and L1OutUB.forward (mi_estimator.py:170-191, with the reference's [N,N,N]
 * broadcasting reduced to its O(N d) closed form).  CV_MI_CLUB (mi_estimator.py:43-55): the [N,N,d] negative
 * term through the fp64 column moments of y, O(N d); CV_MI_VARUB (mi_estimator.py:222-224): the mean over the N*dy
 * elements, independent of y.  Neither of the two needs perm or offset (an offset given advances as for L1OutUB).
 * Writes mi_out[0]; leaves perm / column sums in `work` for cv_mi_backward. */
int cv_mi_forward(int kind, const cv_mlp* mlp, const float* x, int ldx, const float* y, int ldy,
                  int n, const int64_t* perm, uint64_t seed, uint64_t* offset, void* work,
                  float* mi_out, cv_stream_t stream);
/* gradient of gmul*gscale[0]*mi w.r.t. x and y (written or accumulated) and, when g != NULL, the MLP
 * parameters (accumulated).  Chain mode (dheads != NULL): x = z_c, y = z_s are the two halves of z
 * and the gradient is accumulated into d(heads) through z = mu + eps*exp(lv/2). */
int cv_mi_backward(int kind, const cv_mlp* mlp, const float* x, int ldx, const float* y, int ldy,
                   int n, void* work, const float* gscale, float gmul, float* dx, float* dy,
                   int gld, int accumulate, const cv_mlp_grad* g, const float* heads,
                   const float* z, float* dheads, int d, cv_stream_t stream);
/* learning_loss = -loglikeli (mi_estimator.py:129-131, 193-198): loss and MLP gradients
 * (overwritten); with params != NULL also the Adam update of the estimator arena
 * (trainer.py:885-887), whose grads arena must then hold g's buffers.  `work`: a
 * cv_mi_workspace_bytes(n) buffer, zeroed once at allocation (its arrival counters reset
 * themselves). */
int cv_mi_learning_step(const cv_mlp* mlp, const float* x, int ldx, const float* y, int ldy, int n,
                        void* work, float* loss_out, const cv_mlp_grad* g, float* params,
                        const float* grads,
                        float* exp_avg, float* exp_avg_sq, int64_t numel, const float* hyper,
                        int64_t* step, cv_stream_t stream);

/* ---- InfoNCE lower bound (mi_estimator.py:245-273) ----
 * critic F = Linear(dx+dy, h) -> ReLU -> Linear(h, 1) -> Softplus (mi_estimator.py:250-253), Linear weights
 * [out][in]: w1 [h][dx+dy], b1 [h], w2 [h], b2 [1].  The [N, N, dx+dy] tiling of mi_estimator.py:262-266 factors
 * through the first Linear (a_j = W1[:, :dx] x_j, c_i = W1[:, dx:] y_i + b1), so the kernels keep O(N h) memory. */
typedef struct cv_critic {
  const float *w1, *b1, *w2, *b2;
  int dx, dy, h;
} cv_critic;
typedef struct cv_critic_grad {
  float *w1, *b1, *w2, *b2;
} cv_critic_grad;
/* 1 when the kernels serve the geometry: 2 <= n <= 16384, 1 <= dx, dy, h <= 64 */
int cv_infonce_supported(int n, int dx, int dy, int h);
/* workspace of one estimator for batch n (zeroed once at allocation); linear in n */
size_t cv_infonce_workspace_bytes(int n, int h);
/* InfoNCE.forward (mi_estimator.py:259-270): out[0] = mean_i F(x_i, y_i) - (mean_i logsumexp_j F(x_j, y_i) - log n).
 * Leaves the first-layer products and the row log-sum-exps in `work` for cv_infonce_backward. */
int cv_infonce_forward(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy, int n,
                       void* work, float* out, cv_stream_t stream);
/* gradient of gmul*gscale[0]*value (mi_estimator.py:259-270) w.r.t. x and y (written or accumulated) and, when
 * g != NULL, the critic parameters (written, folded in fixed order).  Chain mode as cv_mi_backward.  Needs the
 * `work` a cv_infonce_forward of the same inputs left. */
int cv_infonce_backward(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy, int n,
                        void* work, const float* gscale, float gmul, float* dx, float* dy, int gld,
                        int accumulate, const cv_critic_grad* g, const float* heads, const float* z,
                        float* dheads, int d, cv_stream_t stream);
/* learning_loss = -forward (mi_estimator.py:272-273): loss and critic gradients (overwritten); with
 * params != NULL also the Adam update of the estimator arena (trainer.py:885-887), as cv_mi_learning_step. */
int cv_infonce_learning_step(const cv_critic* critic, const float* x, int ldx, const float* y, int ldy, int n,
                             void* work, float* loss_out, const cv_critic_grad* g, float* params,
                             const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel,
                             const float* hyper, int64_t* step, cv_stream_t stream);

/* ---- CLEAR-TC factor discriminator (trainer.py:573-699, trainer_utils.py:133-138) ----
 * factor_cls = Linear(z, z) -> ReLU -> Linear(z, 1) -> Sigmoid, Linear weights [out][in]; z <= 64, even. */
typedef struct cv_tc_disc {
  const float *w1, *b1, *w2, *b2;
  int zdim;
} cv_tc_disc;
typedef struct cv_tc_grad {
  float *w1, *b1, *w2, *b2;
} cv_tc_grad;
size_t cv_tc_workspace_bytes(int zdim);
/* mi_out[0] = relu(log(d / (1 - d))).mean(), d = factor_cls(z) (trainer.py:664-665), z [n][zdim].  With
 * dheads != NULL also accumulates the gradient of lam * mi_loss into d(heads) through
 * z = mu + eps*exp(logvar/2) (heads / dheads [n][4d] = mu_c | lv_c | mu_s | lv_s, d = zdim/2). */
int cv_tc_forward(const cv_tc_disc* D, const float* z, int n, float lam, const float* heads, float* dheads, int d,
                  void* work, float* mi_out, cv_stream_t stream);
/* The discriminator's step loss (trainer.py:683-694): BCE of factor_cls on z (target 1) and on
 * factor_shuffling(z) "permute_1" (target 0); loss_out[0] and the parameter gradients (overwritten).
 * The optimizer update is cv_adam_step on the discriminator's arena. */
int cv_tc_learning_step(const cv_tc_disc* D, const float* z, int n, void* work, float* loss_out,
                        const cv_tc_grad* g, cv_stream_t stream);

/* ---- GVAE / ML-VAE group evidence (vae.py:159-223; HierarchicalVAETrainer, trainer.py:291-353) ----
 * Segmented by label on the device (n <= 4096, d <= 64): groups in sorted-label order, members in
 * ascending index (the reference's order).  `work`: cv_group_workspace_bytes(n, d) bytes holding
 * int32 m at byte 0, then int32 gid[n], pos[n], order[n], start[n+1] at byte 64 onwards and the group rows
 * mu_g | lv_g [n][2d] fp32 (first m valid) at the next 16-byte boundary. */
enum { CV_GROUP_MLVAE = 0, CV_GROUP_GVAE = 1 };
size_t cv_group_workspace_bytes(int n, int d);
/* accumulate_group_evidence (vae.py:159-190) into `work`; scale_out (or NULL) = n/m, the
 * _group_adjust factor B/m (trainer.py:322-324).  With z != NULL also groupwise_reparam_each + sample
 * (vae.py:193-223, 56-60): z [n][2d] = mu_g[gid] + eps_c * exp(lv_g/2) | mu_s + eps_s * exp(lv_s/2), where
 * row r of the c-noise belongs to the sample at group-order position r (the reference's per-group
 * torch.randn order).  eps [n][ld_eps] injected (c columns [0,d) in group order, s columns [d,2d) per
 * sample) or NULL: Philox from (seed, offset[0]), offset[0] += 1. */
int cv_group_forward(int mode, const float* mu_c, const float* lv_c, int ld, const int64_t* label, int n, int d,
                     void* work, float* scale_out, const float* mu_s, const float* lv_s, int lds,
                     const float* eps, int ld_eps, uint64_t seed, uint64_t* offset, float* z, cv_stream_t stream);
/* The fused step's latent terms (trainer.py:342-349): kl_c over the m group rows, rec and kl_s times
 * B/m, the annealer weight beta/(1+exp(-(t-loc)/scale)) at t = anneal_step[0], and d(heads) [n][4d]
 * (written) from dz [n][2d] through the reparameterisation and the evidence.  losses[0..2] = rec
 * (sum of the CV_REC_REPL rec_in replicas, times B/m), kl_c, kl_s (times B/m); losses[7] = weight. */
int cv_group_backward(int mode, const float* heads, const float* z, const float* dz, const void* work, int n,
                      int d, float beta, float loc, float scale, const int64_t* anneal_step,
                      const double* rec_in, float* dheads, float* losses, cv_stream_t stream);
/* accumulate_group_evidence backward (module path): d(mu_c), d(lv_c) [n][ldo] (written) from d(mu_g),
 * d(lv_g) [m][d] (either may be NULL = zero) and the `work` of the matching cv_group_forward. */
int cv_group_evidence_backward(int mode, const float* mu_c, const float* lv_c, int ld, const void* work, int n,
                               int d, const float* dmu_g, const float* dlv_g, float* dmu_c, float* dlv_c, int ldo,
                               cv_stream_t stream);

/* ---- input pipeline (run_pacs_downstream_expr.py:88-98, run_camelyon17_downstream_expr.ipynb cell 6,
 * data_utils.py:55-73): transforms.Resize((h, w)) + ToTensor() of uint8 images, on the device ----
 * Resize of a PIL image is Image.resize(size, BILINEAR): Pillow's separable antialiased triangle filter
 * with 22-bit fixed-point coefficients and an 8-bit intermediate (src/libImaging/Resample.c).  The plan
 * (int32 words: header, then per output column / row the (first source index, taps) bounds and the
 * fixed-point coefficients) is built on the host with Pillow's double-precision recipe; copy it to the
 * device once. */
size_t cv_resize_plan_words(int in_h, int in_w, int out_h, int out_w);
int cv_resize_plan(int in_h, int in_w, int out_h, int out_w, int32_t* plan, size_t words);
/* source rows of the horizontal pass that a tile of `ty` output rows needs (host plan) */
int cv_resize_tile_rows(const int32_t* plan, int ty);
/* One batch: out [n][c][out_h][out_w] fp32 = Resize + ToTensor of images[index[i]] (uint8 [count][in_h][in_w][c],
 * HWC; index NULL = images 0..n-1), identical to Pillow + torchvision bit for bit; labels_out[i] =
 * labels[index[i]] and styles_out likewise when given.  ty output rows per workgroup, tile_rows =
 * cv_resize_tile_rows(plan, ty); stage = 1 copies each tile's source rows into LDS first (coalesced).
 * LDS per workgroup: the plan body + tile_rows * (out_w + stage * in_w) * c bytes, at most 64 KiB. */
int cv_load_batch_u8(const uint8_t* images, int in_h, int in_w, int c, const int64_t* index, int n,
                     const int32_t* plan, int out_h, int out_w, int ty, int tile_rows, int stage, float* out,
                     const int64_t* labels, int64_t* labels_out, const int64_t* styles, int64_t* styles_out,
                     cv_stream_t stream);

/* ---- evaluation metric: kNN mutual information, the estimator behind gMIG (losses.py:10-16, where
 * mutual_info_gap calls sklearn's mutual_info_classif twice: Ross 2014, continuous feature against a discrete
 * label, one KD-tree per latent dimension on the host) ----
 * x: [n][d] fp32 with row stride ldx >= d; cls: the compact class id of each point, or -1 for a point that takes
 * part in nothing (its label occurs once).  Per feature f and kept point i, with D_ij = |(double)x_jf - (double)x_if|
 * and neighbours ordered by the key (D_ij, j): j* = the min(k, cnt_i - 1)-th smallest key among kept j != i of i's
 * class, m_i = 1 + #{kept j != i : (D_ij, j) < (D_ij*, j*)} (sklearn's radius count, ties broken by index where
 * sklearn adds noise).  m_out [d][n] (or NULL) receives m_i (0 where not kept), psi_sum_out [d] = sum over kept i
 * of psi[m_i] with psi a device table psi[1..n] (n + 1 entries; entry 0 unused), added in a fixed order: the result
 * is bit-reproducible.  1 <= k <= 8, n >= 2; work: cv_knn_mi_workspace_bytes(n, d) bytes, need not be zeroed. */
size_t cv_knn_mi_workspace_bytes(int n, int d);
int cv_knn_mi(const float* x, int ldx, int n, int d, const int32_t* cls, int k, const double* psi, int32_t* m_out,
              double* psi_sum_out, void* work, cv_stream_t stream);

/* ---- evaluation metric: the rank counts behind average precision and AUROC (losses.py:24-33, where auc calls
 * sklearn's average_precision_score and roc_auc_score once per class on host copies of the softmax) ----
 * score: [n][c] fp32 with row stride lds >= c; label: [n] with values in [0, c); order: [n] sample indices sorted by
 * label (stable); start: [c + 1], class k owns order[start[k] .. start[k+1]).  For class k, with s_j = score[j][k],
 * P positives (label == k) and N = n - P negatives, every positive i gets ge_pos_i = #{j positive : s_j >= s_i}
 * (itself included), ge_neg_i = #{j negative : s_j >= s_i} and gt_neg_i = #{j negative : s_j > s_i}; 0.0 and -0.0
 * are equal.  counts_out [n][3] (or NULL) receives (ge_pos, ge_neg, gt_neg) of every sample for its own class,
 * ap_sum_out [c] = sum_i ge_pos_i / (ge_pos_i + ge_neg_i) in fp64 (AP_k = ap_sum / P), added in a fixed order: the
 * result is bit-reproducible; u2_out [c] = sum_i [2 (N - ge_neg_i) + (ge_neg_i - gt_neg_i)], an exact integer
 * (AUROC_k = u2 / (2 P N): Mann-Whitney with ties counted one half).  A class without positives gets 0 in both.
 * The scores must be finite and the labels in range: the caller checks that, the kernel does not.  The grid is
 * sized from n and c alone (no host read of the class sizes).  1 <= n <= 2^22, 1 <= c <= 2^22;
 * work: cv_rank_auc_workspace_bytes(n, c) bytes (0 for sizes outside those limits), need not be zeroed. */
size_t cv_rank_auc_workspace_bytes(int n, int c);
int cv_rank_auc(const float* score, int lds, int n, int c, const int32_t* label, const int32_t* order,
                const int32_t* start, uint32_t* counts_out, double* ap_sum_out, unsigned long long* u2_out, void* work,
                cv_stream_t stream);

/* ---- the tail of one evaluate() batch (trainer.py:495-570 for the CLEAR trainers, :366-412 for the GVAE / ML-VAE
 * one; the terms are vae_loss's, losses.py:41-50) ----
 * The accumulators of one evaluation epoch, all in device memory: the batches' latents and labels in call order
 * (what trainer.py:531-541 / :390-396 collect in Python lists and torch.cat) and the running sums of the printed
 * values (trainer.py:524-530, 548-560). */
typedef struct cv_eval_sink {
  float* lat_c; float* lat_s;   /* [cap][d] each                                                   */
  int64_t* label;               /* [cap]                                                           */
  int64_t cap;                  /* rows of the three buffers                                       */
  int64_t* cursor;              /* [2]: rows appended so far, sticky overflow flag                 */
  double* totals;               /* [8]: rec, kl_c, kl_s, term 0, term 1, (5, 6 unused), batches    */
} cv_eval_sink;
/* bytes of cv_eval_batch's `work` for a batch of n images of c channels and hw pixels (three fp64 partials per
 * workgroup of the element pass; need not be zeroed); 0 for a shape cv_eval_batch refuses */
size_t cv_eval_workspace_bytes(int n, int c, int hw);
/* One batch (trainer.py:517-541, losses.py:41-50), from what the eval-mode forward left on the device:
 *   rec  = mean_n sum_chw (sigmoid(BN(y)) - x)^2 with y the last ConvTranspose2d's pre-BN output, NHWC [n][hw][c] (the
 *          layout cv_output_forward takes), bn its BatchNorm (eval mode: the running statistics) and x the NCHW
 *          input; every element's value is cv_output_forward's, xhat itself is not written.  1 <= c <= 4.
 *   kl_c, kl_s = -0.5 mean_n sum_d (1 + lv - mu^2 - exp(lv)) over the heads [n][4d] = mu_c | lv_c | mu_s | lv_s.
 *   append: z[:, :d] -> lat_c, z[:, d:] -> lat_s, label -> label, at rows cursor[0] .. cursor[0] + n.
 *   totals[0..2] += rec, kl_c, kl_s; totals[3 + k] += term_scale[k] * terms[k][0] for k < nterm <= 2 (terms: a host
 *          array of device scalars written earlier on the stream, e.g. the contrastive and MI losses; term_scale: a
 *          host array read at the call); totals[7] += 1; cursor[0] += n.
 * The cursor lives on the device and the kernels advance it, so one captured graph serves every batch of its size.
 * A batch whose rows do not all fit under cap (or any batch once the flag is set) appends nothing, leaves totals and
 * cursor[0] as they are and sets cursor[1] = 1; nothing is written at or beyond row cap.
 * Two launches on the stream (the element pass writes fp64 partials into indexed slots of `work`, the finish pass adds
 * them in a fixed order): no atomics and no grid-wide wait; two runs from equal state give equal bits. */
int cv_eval_batch(const cv_bn* bn, const float* y, const float* x, int n, int c, int hw, const float* heads,
                  const float* z, int d, const int64_t* label, const float* const* terms, const float* term_scale,
                  int nterm, const cv_eval_sink* sink, double* work, cv_stream_t stream);

/* ---- exact t-SNE for the latent plots (the demo notebooks and expr/visual_utils.py:144-183 call sklearn's
 * TSNE(n_components=2, perplexity=30, learning_rate=200, init='pca').fit_transform on host copies of mu_c and mu_s);
 * sklearn's method="exact" (manifold/_t_sne.py, _utils.pyx), matrix-free: O(n d) memory, no n x n array ----
 * x: [n][d] fp32 with row stride ldx >= d, 1 <= d <= 64, 2 <= n <= 65536; d_ij = the squared Euclidean distance;
 * the embedding y is [n][2] fp32.  Every sum is added in a fixed order and nothing uses atomics: all results are
 * bit-reproducible.  work: cv_tsne_workspace_bytes(n) bytes (0 for n outside the limits), need not be zeroed;
 * cv_tsne_pair fills it and cv_tsne_update reads it.
 *
 * cv_tsne_affinity (_utils.pyx _binary_search_perplexity, as _joint_probabilities calls it): per row i the precision
 * beta_i of the conditional Gaussian with entropy H_i = ln(perplexity), 0 < perplexity < n, by sklearn's search
 * (beta = 1; double / halve while the bracket is open, else the midpoint; at most 100 evaluations; stop at
 * |H_i - ln perplexity| <= 1e-5), with H_i = ln S_i + beta_i sum_{j!=i} d_ij exp(-beta_i d_ij) / S_i and
 * S_i = sum_{j!=i} exp(-beta_i d_ij), evaluated with every exponent shifted by the row's smallest distance.
 * beta_out [n] = beta_i rounded to fp32, logz_out [n] = ln S_i at that rounded value.
 *
 * cv_tsne_pair (_t_sne.py _joint_probabilities:60-66 and _kl_divergence:130-178): with
 * p_ij = max((exp(-beta_i d_ij - logz_i) + exp(-beta_j d_ij - logz_j)) / 2n, 2.220446e-16) and
 * q_ij = 1 / (1 + |y_i - y_j|^2), the per-row sums over j != i of  e p q (y_i - y_j),  q^2 (y_i - y_j),  q  and,
 * when with_kl,  e p (ln(e p) - ln q)  and  e p  (e = exaggeration > 0), one fp64 partial per slab of j, into work.
 *
 * cv_tsne_update (_t_sne.py _kl_divergence:170-178 and _gradient_descent:390-404): Z = sum_ij q_ij,
 * grad_i = 4 (A_i - R_i / Z) -> grad_out [n][2] (or NULL), KL = sum e p ln(e p Z / q) -> kl_out (or NULL; only
 * after a cv_tsne_pair with with_kl), and, when y is given, one descent step on y, update and gains ([n][2] each):
 * gains += 0.2 where update * grad < 0, gains *= 0.8 elsewhere, gains >= 0.01,
 * update = momentum * update - learning_rate * gains * grad, y += update.  reset != 0: update and gains are taken
 * as 0 and 1 instead of being read.
 *
 * cv_tsne_run (_t_sne.py _tsne:1080-1130): n_iter rounds of pair + update on `stream`: exaggeration
 * early_exaggeration and momentum 0.5 for the first exploration_iter rounds, then 1 and 0.8, with update and gains
 * reset at round 0 and at the switch (sklearn starts a second _gradient_descent there); no early stopping.  With
 * kl_out, one more pair pass stores the KL divergence of the final y (exaggeration 1). */
size_t cv_tsne_workspace_bytes(int n);
int cv_tsne_affinity(const float* x, int ldx, int n, int d, double perplexity, float* beta_out, float* logz_out,
                     cv_stream_t stream);
int cv_tsne_pair(const float* x, int ldx, int n, int d, const float* beta, const float* logz, const float* y,
                 float exaggeration, int with_kl, void* work, cv_stream_t stream);
int cv_tsne_update(int n, void* work, float* y, float* update, float* gains, float momentum, float learning_rate,
                   int reset, float* grad_out, double* kl_out, cv_stream_t stream);
int cv_tsne_run(const float* x, int ldx, int n, int d, const float* beta, const float* logz, float* y, float* update,
                float* gains, int n_iter, int exploration_iter, float early_exaggeration, float learning_rate,
                void* work, double* kl_out, cv_stream_t stream);

/* ---- downstream probe(run_styledmnist_downstream_expr.py:110-117, trainer.py:125-131): the reference's `mlp` =
 * Linear(d,h) -> BatchNorm1d(h) -> ReLU -> Linear(h,c) on mu_c of the frozen VAE, nn.CrossEntropyLoss() defaults ----
 * Linear weights [out][in]; running statistics are the module's own buffers (updated in place by a training step:
 * momentum, unbiased running_var; nbt += 1 when given). */
typedef struct cv_probe {
  const float *w1, *b1, *gamma, *beta, *w2, *b2;   /* [h][d], [h], [h], [h], [c][h], [c] */
  float *running_mean, *running_var;               /* [h] */
  int64_t* nbt;                                    /* or NULL */
  int d, h, c;
  float eps, momentum;
} cv_probe;
typedef struct cv_probe_grad { float *w1, *b1, *gamma, *beta, *w2, *b2; } cv_probe_grad;

/* 1 when cv_probe_step serves the shape: 2 <= n <= 1024, 1 <= d <= 64, 1 <= h <= 512, 2 <= c <= 32 */
int cv_probe_supported(int n, int d, int h, int c);
/* bytes of `work`: 16-byte aligned, zeroed once at allocation (its arrival counters reset themselves) */
size_t cv_probe_workspace_bytes(int n, int h, int c);
/* One training step of the probe in train mode (trainer.py:125-131): x [n][d] fp32 with row stride ldx >= d (mu_c:
 * columns 0..d of the heads, ldx = 4d; rows may start at any 4-byte boundary), label [n] in [0, c) (a label outside
 * makes the loss and its dlogits row NaN and indexes nothing).  Writes loss_out[0] = the mean cross-entropy, the
 * gradients of W2, b2, gamma, beta, W1 (overwritten; BatchNorm column sums in fp64) and d(b1) = exact zeros (the bias
 * feeds a train-mode BatchNorm), and updates the running statistics.  With params != NULL the same call applies
 * torch.optim.Adam (foreach) to the whole arena (hyper / step as for cv_adam_step; the bias corrections are read on
 * the device, step[0] += 1, step[1] stays 0): g's buffers must lie in `grads`, and each parameter of P in `params`
 * at its gradient's offset.  params == NULL: loss + gradients only.  Two launches, no floating-point atomics: the
 * same state and batch give the same bits.  Host validation failures return non-zero before any launch. */
int cv_probe_step(const cv_probe* P, const float* x, int ldx, const int64_t* label, int n, void* work,
                  float* loss_out, const cv_probe_grad* g,
                  float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t numel,
                  const float* hyper, int64_t* step, cv_stream_t stream);
/* The probe in eval mode (trainer.py:146-165): logits [n][c] from the running statistics; writes nothing else.
 * One launch; n >= 1. */
int cv_probe_forward(const cv_probe* P, const float* x, int ldx, int n, float* logits, cv_stream_t stream);

/* ---- CNN baseline, the classifier tail (code/src/models/cnn.py:22-27: cls_head[1:] = BatchNorm1d(h) -> ReLU ->
 * Linear(h,c); code/src/trainer.py:196-199 the training step's loss and backward, :228 the eval forward) ----
 * `a` [n][h] row-major is the output of cls_head[0] = Linear(2048, h), bias included.  Linear weight [c][h]; the
 * running statistics are the module's own buffers. */
typedef struct cv_cls {
  const float *gamma, *beta, *w2, *b2;      /* [h], [h], [c][h], [c] */
  float *running_mean, *running_var;        /* [h] */
  int64_t* nbt;                             /* or NULL */
  int h, c; float eps, momentum;
} cv_cls;
typedef struct cv_cls_grad { float *gamma, *beta, *w2, *b2; } cv_cls_grad;

/* 1 when cv_cls_step serves the shape: 2 <= n <= 1024, 1 <= h <= 512, 2 <= c <= 32 */
int cv_cls_supported(int n, int h, int c);
/* bytes of `work` (a positive multiple of 16): 16-byte aligned, zeroed once at allocation; its arrival counters (the
 * first 64 bytes) reset themselves, so they read zero again after every call */
size_t cv_cls_workspace_bytes(int n, int h, int c);
/* One training step of the tail in train mode (cnn.py:22-27 under trainer.py:196-199): BatchNorm1d with batch mean
 * and biased variance (fp64 column sums), running_mean/var <- (1-m) old + m (mean, unbiased variance), nbt += 1 when
 * given; y = ReLU(gamma xhat + beta), logits = y W2^T + b2; loss_out[0] = the mean cross-entropy (stable
 * log-softmax); label [n] in [0, c) (a label outside makes the loss and its dlogits row NaN and indexes nothing).
 * Writes (overwritten, not accumulated) g->w2 = dlogits^T y, g->b2, g->gamma, g->beta (fp64 column sums) and
 * da [n][h] = gamma istd (dy_m - dbeta/n - xhat dgamma/n), the gradient handed back to cls_head[0].  No optimizer
 * inside.  Two launches, no floating-point atomics, no workgroup waits for another: the same state and batch give
 * the same bits.  Host validation failures return non-zero before any launch. */
int cv_cls_step(const cv_cls* P, const float* a, const int64_t* label, int n, void* work, float* loss_out,
                float* da, const cv_cls_grad* g, cv_stream_t stream);
/* The tail in eval mode (trainer.py:228 under model.eval()): logits [n][c] from the running statistics; writes
 * nothing else.  One launch; any n >= 1 (rows are independent: the batch limit of cv_cls_step does not apply), h and c
 * as for cv_cls_supported. */
int cv_cls_forward(const cv_cls* P, const float* a, int n, float* logits, cv_stream_t stream);

/* ---- LAM baseline, the tail (code/src/models/cnn.py:57-66: cls_head = Linear(2048, c) on the flattened trunk;
 * code/src/trainer.py:259-288 the training step, :249-257 ss_pairing; code/src/losses.py:173-187 lam_loss) ----
 * The reference's three train-mode trunk forwards per step (cnn(X), cnn.net(X), cnn.net(X[pair])) are one: batch
 * statistics do not see row order, so net(X[pair]) = net(X)[pair].  With h = ReLU(BN(y)) [n][F] the flattened trunk
 * output, p = pair, q = pair^-1 and lambda = *lam:
 *   logits = h W^T + b;  ce = mean cross-entropy;  dlogits = (softmax - onehot) / n
 *   lam = (1/n) sum_i sum_f ((h[i,f] - h[p_i,f]) W[y_i,f])^2                 (the trainer's loss is ce + lambda lam)
 *   gb[k] = sum_i dlogits[i,k]
 *   gW[k,f] = sum_i dlogits[i,k] h[i,f] + lambda (2/n) W[k,f] sum_{i: y_i = k} (h[i,f] - h[p_i,f])^2
 *   dh[i,f] = sum_k dlogits[i,k] W[k,f]
 *             + lambda (2/n) (W[y_i,f]^2 (h[i,f] - h[p_i,f]) - W[y_q,f]^2 (h[q,f] - h[i,f])),  q = q_i
 * (right for any permutation, label-preserving or not).  w [c][F] is in PyTorch feature order f = ch * in_pix + p;
 * y and gin are in storage order [n][in_pix][in_ch].  lam is a DEVICE float the caller rewrites when the
 * hyperparameter changes (a replayed graph sees the change). */
typedef struct cv_lam {
  const float *w, *b;   /* [c][in_ch * in_pix], [c] */
  const float* lam;     /* device float: lam_coef */
  int c, in_ch, in_pix;
} cv_lam;
typedef struct cv_lam_grad { float *w, *b; } cv_lam_grad;

/* 1 when cv_lam_step serves the shape: 2 <= n <= 1024, in_ch >= 1, 1 <= in_pix <= 16, in_ch * in_pix <= 2048,
 * 2 <= c <= 32 (both reference trunks: 128 channels x 16 pixels and 512 x 4) */
int cv_lam_supported(int n, int in_ch, int in_pix, int c);
/* bytes of `work` (a positive multiple of 16; 0 for an unsupported shape): 16-byte aligned, zeroed once at
 * allocation; its arrival counter (the first 64 bytes) resets itself, so it reads zero again after every call */
size_t cv_lam_workspace_bytes(int n, int in_ch, int in_pix, int c);
/* The device ss_pairing (trainer.py:249-257): pair_out [n] = a uniformly random permutation inside each label
 * stratum (label[pair[i]] == label[i]; any int64 labels, they only compare), 1 <= n <= 1024, one workgroup.  The
 * Philox keys come from (seed, *offset); *offset (device, or NULL = 0) is advanced by one afterwards, so a replayed
 * graph draws a fresh pairing each time and the same (seed, offset, label) gives the same pair. */
int cv_lam_pair(const int64_t* label, int n, uint64_t seed, uint64_t* offset, int64_t* pair_out, cv_stream_t stream);
/* One training step of the tail.  y: the last conv block's pre-BN output; bn: that block's BatchNorm2d in train mode
 * with its forward sums (count = n * in_pix; finalised cfwd constants are used when bn->ticket[0] says so, else the
 * replicas are folded, as cv_heads_backward).  label [n] in [0, c); pair [n] a permutation of [0, n) (the kernel
 * builds its inverse).  Writes loss_out[0] = ce, loss_out[1] = lam (unscaled), g->w, g->b (overwritten),
 * gin [n][F] = dh [BN(y) > 0] and the complete backward sums (sum dz, sum dz xhat; fp64) into replica 0 of
 * gstat_out [CV_STAT_REPL(C)][2][C] (the other replicas are left as they are: zeroed by the step).  bn->ticket is
 * left untouched (zero), so consumers fold the sums themselves.  A label outside [0, c), a pair entry outside
 * [0, n) or a pair that is no permutation makes both losses NaN and indexes nothing.  Two launches, no
 * floating-point atomics, no workgroup waits for another: the same state and batch give the same bits.  Host
 * validation failures return non-zero before any launch. */
int cv_lam_step(const cv_lam* P, const float* y, const cv_bn* bn, const int64_t* label, const int64_t* pair, int n,
                void* work, float* loss_out, float* gin, double* gstat_out, const cv_lam_grad* g, cv_stream_t stream);
/* The tail in eval mode (trainer.py:215-233 under model.eval()): logits [n][c] with bn as given (train = 0: running
 * statistics); writes nothing else.  One launch; any n >= 1; the other limits as for cv_lam_supported. */
int cv_lam_forward(const cv_lam* P, const float* y, const cv_bn* bn, int n, float* logits, cv_stream_t stream);

/* ---- Styled-MNIST generation (corruption_utils/corruptions.py:230 identity, :712-716 stripe, :665-704 zigzag with
 * :202-221 line_from_points, :719-722 canny_edges, :602-622 scale, :455-466 brightness; the per-image style draw of
 * data_utils.py:29-52 StyledMNISTGenerator and expr_utils.py:18-32 KStyledMNISTGenerator) ----
 * One launch, one workgroup per image: images uint8 [n][28][28] (4-byte aligned) -> out fp32 [n][28][28] in [0, 255],
 * the corruption functions' return values.  label: [n] int64 in [0, n_class) (the caller checks that; the kernel
 * clamps); table: device fp32 [n_class][n_style], each row a probability vector; kind / severity: host arrays
 * [n_style], kind one of CV_STYLE_*, severity in 1..5 for scale and brightness (ignored for the others).
 * For image i, u = philox(seed, *offset ^ tag, i): the style is the first index whose cumulative probability in row
 * label[i] exceeds u.x 2^-32 (the last style with non-zero probability catches rounding), the zigzag start row is
 * r0 = floor(u.y 2^-32 27) and its slope index dr = floor(u.z 2^-32 10) - 5 (np.random.randint(0, 27) and
 * randint(-5, 5)).  style_in int32 [n] / zz_in int32 [n][2] (or NULL) give the style / (r0, dr) instead (test hooks;
 * clamped to their ranges); cand_in uint8 [n][28][28] (or NULL; test hook) gives canny images their candidate map
 * (0 none, 1 weak, 2 strong) in place of the front end.  offset: device uint64[2] = (counter, arrival count = 0) or
 * NULL = counter 0; the counter is advanced by one unless both style_in and zz_in are given.
 * zz_pts: device fp64 [10][8][2], the (column, row) endpoints of the zigzag polyline for dr = -5..4 with r0 = 0;
 * zz_cols: device int32 [10][7][2], every segment's (floor(c0), ceil(c1)) column range.
 * style_out int64 [n]; zz_out int32 [n][2] = the (r0, dr) of every image (used by its zigzag, if that is its style).
 * The canny and warp semantics are those DESIGN 4g writes out.  Every loop is bounded at compile time (the canny
 * hysteresis: at most 784 sweeps).  Returns non-zero before any launch for a geometry other than 28x28, n_style
 * outside 1..16, n <= 0, an unknown kind, a severity outside 1..5 or a missing pointer. */
enum { CV_STYLE_IDENTITY = 0, CV_STYLE_STRIPE = 1, CV_STYLE_ZIGZAG = 2, CV_STYLE_CANNY = 3, CV_STYLE_SCALE = 4,
       CV_STYLE_BRIGHTNESS = 5 };
int cv_style_mnist(const uint8_t* images, int n, int h, int w, const int64_t* label, const float* table, int n_class,
                   int n_style, const int* kind, const int* severity, const double* zz_pts, const int32_t* zz_cols,
                   uint64_t seed, uint64_t* offset, const int32_t* style_in, const int32_t* zz_in,
                   const uint8_t* cand_in, float* out, int64_t* style_out, int32_t* zz_out, cv_stream_t stream);

/* ---- The swap and interpolation figures (expr/visual_utils.py:13-128; torchvision.utils.make_grid) ----
 * Three data-movement kernels, one launch per call, no atomics (the same inputs give the same bits).  Every
 * host-side check fails with a non-zero return before anything is launched.
 *
 * cv_latent_pairs (visual_utils.py:34-36, the repeat / repeat / cat of feature_swapping_plot): z_c [n][dc] with row
 * stride ldc, z_s [n][ds] with row stride lds (elements; column slices of one [n][dc + ds] array pass as they are)
 * -> out, contiguous [n * n][dc + ds]: row i * n + j = (z_c[i], z_s[j]), copied bit for bit.  n * n * (dc + ds) must
 * be below 2^31. */
int cv_latent_pairs(const float* z_c, int ldc, const float* z_s, int lds, int n, int dc, int ds, float* out,
                    cv_stream_t stream);
/* cv_latent_interp (visual_utils.py:86-105 with display_utils.py:11-21 interpolate_latent): z [n][d] with row stride
 * ldz; content = columns [0, z_dim), style = [z_dim, d); src_ids / tgt_ids: device int64 [s]; out, contiguous
 * [2][s][steps][d].  With z1 = z[src_ids[i]], z2 = z[tgt_ids[i]] and p = torch.linspace(1, 0, steps) formed in fp32
 * as torch forms it (step = -1 / (steps - 1); p_k = 1 + step k in the first half, 0 - step (steps - 1 - k) in the
 * second; steps = 1: p = [1]):
 *   out[0][i][k] = (z1.content, p_k z1.style + (1 - p_k) z2.style)       the style interpolation
 *   out[1][i][k] = (p_k z1.content + (1 - p_k) z2.content, z1.style)     the content interpolation
 * The copied halves are bit-exact; for steps >= 2 the rows k = 0 and k = steps - 1 of the interpolated half are z1 and
 * z2 bit for bit (finite inputs).  The caller checks the ids; a pair with an id outside [0, n) reads nothing and gets
 * NaN rows.  2 * s * steps * d must be below 2^31. */
int cv_latent_interp(const float* z, int ldz, int n, int d, int z_dim, const int64_t* src_ids, const int64_t* tgt_ids,
                     int s, int steps, float* out, cv_stream_t stream);
/* cv_make_grid (torchvision.utils.make_grid(images, nrow, padding, pad_value=...) without normalize / scale_each,
 * with visual_utils.py:13-26 make_colored_grid folded in), written into a sub-rectangle of a canvas (the torch.cat
 * of visual_utils.py:44-52 and :80-118): images fp32 [m][c][h][w], contiguous, c = 1 (written to all three channels)
 * or 3.  xmaps = min(nrow, m), ymaps = ceil(m / xmaps); the grid is ymaps (h + padding) + padding high and
 * xmaps (w + padding) + padding wide; image k = y xmaps + x starts at (y (h + padding) + padding,
 * x (w + padding) + padding); everything else, the cells past m in a ragged last row included, is pad_value.
 * m = 1 gives the image alone, without padding, as torchvision does.
 * mode = CV_GRID_FILL (m = 0; images, c, nrow and padding are not looked at): an h x w rectangle of pad_value.
 * frame, applied to the value about to be written, pad or pixel alike (NaN never matches):
 *   CV_FRAME_RED   where channel 0 is 0.25, channel 0 becomes 1; channels 1 and 2 stay (the reference's second and
 *                  third masked assignments test channel 0 after the first has changed it: the frame is
 *                  (1, 0.25, 0.25))
 *   CV_FRAME_BLUE  where channel 2 is 0.25, the pixel becomes (0, 0, 1)
 * Destination: element (ch, y, x) of a [3][dst_h][dst_w] canvas lies at dst[ch chan_pitch + y row_pitch + x]; the
 * grid's top left corner goes to (y0, x0); nothing outside the grid's rectangle is written.
 * Rejected: a null pointer, c not 1 or 3, padding < 0, nrow < 1, m outside 1..65536 (0 for CV_GRID_FILL), h or w
 * outside 1..4096 (CV_GRID_FILL: below 1), row_pitch < dst_w, chan_pitch < dst_h row_pitch, a rectangle that does not
 * fit the destination, a destination that spans 2^31 elements or more. */
enum { CV_GRID_IMAGES = 0, CV_GRID_FILL = 1 };
enum { CV_FRAME_NONE = 0, CV_FRAME_RED = 1, CV_FRAME_BLUE = 2 };
int cv_make_grid(const float* images, int m, int c, int h, int w, int nrow, int padding, float pad_value, int frame,
                 int mode, float* dst, int dst_h, int dst_w, long long chan_pitch, long long row_pitch, int y0, int x0,
                 cv_stream_t stream);

/* ---- Adam (torch.optim.Adam foreach semantics) over a flat fp32 arena ----
 * hyper: device float[8] = lr, beta1, beta2, eps, weight_decay; step: device int64[2] =
 * (steps taken, arrival counter = 0).  grad_scale (device float or NULL) multiplies the gradient
 * first (data-parallel averaging); aux_counter (or NULL) is incremented once per call
 * (LogisticAnnealer.step, trainer.py:484). */
int cv_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                 int64_t numel, const float* hyper, int64_t* step, const float* grad_scale,
                 int64_t* aux_counter, cv_stream_t stream);

/* End-of-backward reduction in ONE launch (the step before the optimizer, trainer.py:482-483):
 * the partial tiles of up to 24 deferred weight gradients (fixed split order: deterministic), the
 * BatchNorm affine gradients dgamma = sum dz*xhat, dbeta = sum dz of up to 16 layers (when dgamma or
 * dbeta is given; written, not accumulated) and, with running = 1, their running statistics
 * (nn.BatchNorm*, momentum, unbiased running var; num_batches_tracked += 1 when nbt is given). */
int cv_step_reduce(const cv_wgrad_defer* defers, int ndefer, const cv_bn* bn, int nbn, float* const* dgamma,
                   float* const* dbeta, int running, float momentum, int64_t* const* nbt, cv_stream_t stream);

/* BatchNorm affine gradients from the backward sums: dgamma = sum dz*xhat, dbeta = sum dz
 * (nn.BatchNorm weight/bias grads); written (not accumulated) for up to 16 layers. */
int cv_bn_param_grads(const cv_bn* bn, int nlayers, float* const* dgamma, float* const* dbeta,
                      cv_stream_t stream);

/* ---- misc ---- */
/* hipMemsetAsync(ptr, 0, bytes, stream) (graph-capturable) */
int cv_zero(void* ptr, size_t bytes, cv_stream_t stream);
/* zero up to 8 buffers (4-byte granular: sizes multiples of 4, 4-byte aligned) in one launch */
int cv_zero_many(void* const* ptrs, const size_t* bytes, int count, cv_stream_t stream);
/* device-to-device copy of up to 8 buffers (4-byte granular) in one launch (the step's input batch) */
int cv_copy_many(void* const* dst, const void* const* src, const size_t* bytes, int count, cv_stream_t stream);
/* Step graphs: capture the calls enqueued on `stream` between cv_graph_begin and cv_graph_end (thread-local
 * capture mode; the stream must not be the legacy default stream) into an executable graph, replay it with
 * cv_graph_launch on any stream, free it with cv_graph_destroy. */
int cv_graph_begin(cv_stream_t stream);
int cv_graph_end(cv_stream_t stream, void** exec_out);
int cv_graph_launch(void* exec, cv_stream_t stream);
int cv_graph_destroy(void* exec);
const char* cv_last_error(void);
int cv_version(void);
/* test hook: 1 routes every conv/linear GEMM to the generic implicit-GEMM kernel instead of the
 * specialised core (both compute the same contraction); returns the previous setting */
int cv_debug_force_generic_gemm(int on);
/* test hook: launches of the direct conv kernel (cv_conv_*_kpack) since the last reset */
int cv_debug_direct_count(int reset);
/* test hook: the fewest workgroups for which a stride-2 conv takes the direct kernel (default 256; smaller
 * grids run the GEMM core); returns the previous setting (-1: not yet initialised) */
int cv_debug_direct_minwg(int minwg);
/* test hook: 1 (default) serves a stride-2 GATHER by the direct kernel only where it measured faster than the GEMM
 * core (one resident round of workgroups, >= 32 output pixels per tile); 0 serves every geometry it can plan
 * (kernel tests); returns the previous setting */
int cv_debug_direct_gather_rule(int on);
/* test hook: 1 (default) issues a served backward-data + weight-gradient pair as one dual grid (cv_dual.hip), 0 runs
 * the two launches back to back (the arithmetic of each role is the same); a negative value only queries; returns
 * the previous setting */
int cv_debug_dual(int on);
/* test hook: 1 (default) lets the GEMM core take pixel-major tiles where they skip >= 10 % padding work
 * (cv_gemm_tile.inc), 0 never; a negative value only queries; returns the previous setting (-1: not yet read
 * from CV_PM) */
int cv_debug_pm(int on);
/* test hook: conv contractions planned with pixel-major tiles since the last reset */
int cv_debug_pm_count(int reset);
/* test hook: 1 (default) lets a queued NT-Xent phase ride in a served direct launch (cv_ntxent_aux), 0 launches it
 * on its own at the flush; a negative value only queries; returns the previous setting */
/* test hook: 1 (CV_WGRAD_SELF=1; measured slower, off by default) lets a deferred split-K weight gradient reduce its
 * own slices (the split's last slice adds the tile into gweight; the defer record says split 0), 0 (default) leaves
 * the partials for cv_step_reduce;
 * -1 queries; returns the previous setting (-1: not yet read from the environment) */
int cv_debug_wgrad_self(int on);
int cv_debug_aux(int on);
/* test hook: direct + NT-Xent grids issued since the last reset */
int cv_debug_aux_count(int reset);
/* Test hook: the register-resident NT-Xent variants (cosine, n <= 512, d <= 8; cv_ntxent.hpp) on (1) / off (0:
 * the LDS-staged kernels), -1 queries; returns the previous setting.  Diagnostics only. */
int cv_debug_nt_reg(int on);
/* test hook: dual grids issued since the last reset */
int cv_debug_dual_count(int reset);
/* measurement hook: 1 starts recording (on this thread) the kernels the conv / linear calls launch, clearing the
 * record; 0 stops; returns the previous setting.  cv_debug_kernel_names writes the recorded kernels' demangled
 * names, one per line, into buf (truncated to cap - 1 bytes, NUL-terminated) and returns how many were recorded
 * (bench.py: the PMC passes a roofline quotes must have been taken on the kernels the priced call issues). */
int cv_debug_kernel_log(int on);
int cv_debug_kernel_names(char* buf, size_t cap);

/* ---- GEMM workspace (in-launch split-K of under-filled long-K conv forward / ConvT backward-data
 * launches, e.g. VAE64's conv5 at 32-256 images per GPU): a caller-owned device buffer of at least
 * cv_gemm_workspace_bytes(), ZEROED before registration, for the current device (NULL: unregister).
 * Calls on one stream share it; without one the launches run unsplit.  CONTRACT: the split launches of a
 * device must be serialised — one stream at a time (the fused step engine issues them all on its step
 * stream; the autograd path on torch's current stream).  Two split launches in flight on different streams
 * would race on its fragment slabs and leave its self-resetting per-tile tickets non-zero, corrupting every
 * later split launch; a caller that runs conv layers on several streams concurrently registers NULL (no
 * split) or serialises them with events.  No reference counterpart
 * (the reference's convolutions are ATen's, code/src/models/vae.py:15-46 / :113-156). */
size_t cv_gemm_workspace_bytes(void);
int cv_set_gemm_workspace(void* work, size_t bytes);

/* ---- the MI-bound study (code/mi_experiment.ipynb) ----
 * cv_blobs replaces the notebook's code cell 3 (generate_gaussian_blobs) for B trials at once:
 *   x[b*ld_trial + i*ld_row + k] = centers[i / (n / n_blobs)] + stds[b] * eps,   b < B, i < n, k < d
 * with eps standard normal from the library's Philox4x32-10 + Box-Muller.  The strides select [B][n][d] storage
 * (ld_row >= d, ld_trial >= n*ld_row) or [n][B][d] storage (ld_trial >= d, ld_row >= B*ld_trial); the element at
 * position q of the storage order (padding not counted) takes normal (q & 1) of philox(seed, *offset ^ tag, q / 2),
 * so both normals of a draw are used and the writes are contiguous in memory.  centers: host [n_blobs]; stds: device
 * [B]; offset: device uint64[2] = (counter, arrival count = 0) or NULL = counter 0; the counter is advanced by one on
 * the device (a captured graph draws fresh blobs at every replay).  Returns non-zero before any launch unless
 * B >= 1, d >= 1, 1 <= n_blobs <= 16, n a positive multiple of n_blobs and the strides are one of the two forms. */
int cv_blobs(float* x, long long ld_trial, long long ld_row, int B, int n, int d, const float* centers, int n_blobs,
             const float* stds, uint64_t seed, uint64_t* offset, cv_stream_t stream);
/* cv_snn_bounds replaces the notebook's code cells 1-2 (logsumexp, PSSNN, SNN; losses.py:98-137 with the cosine
 * similarity) for B trials and T temperatures in one pass.  For trial b, row i, temperature tau, with
 * u_j = x_j / max(|x_j|, 1e-8) and s_ij = u_i . u_j:
 *   lse_all = log sum_{j != i} exp(s_ij / tau),  lse_pos over j != i with label_j == label_i,  lse_neg over
 *   label_j != label_i (an empty set: -inf);  SNN row term = lse_all - lse_pos, PS-SNN row term = lse_all - lse_neg;
 *   bound[b][t][0 SNN, 1 PS-SNN] = the mean of the finite row terms, count[b][t][.] = how many there are
 *   (none: bound NaN, count 0, the mean of an empty tensor).
 * A NaN or infinity in a trial makes that trial's bounds NaN with count 0 and touches no other trial.
 * x: fp32, element (b, i, k) at x[b*ld_trial + i*ld_row + k]; label: int64 (compared as int64), label of (b, i) at
 * label[b*ld_label + i] (ld_label = 0: one [n] vector for every trial); taus: host [T]; rows: NULL or fp32
 * [B][T][3][n] = lse_all, lse_pos, lse_neg; work: cv_snn_bounds_workspace_bytes(B, n, T) bytes (0 outside the
 * envelope), need not be zeroed.  Each pair is evaluated once for all temperatures; the sets keep running maxima
 * of the similarity, so nothing underflows at small tau; no atomics, fixed summation orders: the same inputs give
 * the same bits, and trial b of a batch has the bits of a B = 1 call on it.  Two launches.  Returns non-zero before
 * any launch unless 2 <= n <= 65536, 1 <= d <= 64, 1 <= T <= 8, every tau finite and > 0, B >= 1, B*n < 2^31. */
size_t cv_snn_bounds_workspace_bytes(int B, int n, int T);
int cv_snn_bounds(const float* x, long long ld_trial, long long ld_row, int B, int n, int d, const int64_t* label,
                  long long ld_label, const float* taus, int T, double* bound, int32_t* count, float* rows,
                  void* work, cv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CLEARVAE_H */
