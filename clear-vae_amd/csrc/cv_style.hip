// Styled-MNIST generation on the device: the six style corruptions the reference's Styled-MNIST scripts use
// (code/corruption_utils/corruptions.py:230 identity, :712-722 stripe / canny_edges, :665-704 zigzag with :202-221
// line_from_points, :602-622 scale, :455-466 brightness), the per-image style draw of StyledMNISTGenerator
// (code/src/utils/data_utils.py:29-52) and KStyledMNISTGenerator (code/expr/expr_utils.py:18-32), as one launch over
// the whole dataset.  The semantics of the skimage parts (warp order 1 / mode constant, feature.canny with its
// defaults) are those written out in DESIGN §4g; they have not been compared with a skimage install.
//
// One image per workgroup of 256 threads (4 waves) at a time.  The canny front end keeps two fp64 28x28 planes, the
// fp32 image and an int state plane in LDS (18.8 KiB: 8 workgroups per CU), which one image per wave would quadruple
// past the 32 KiB budget; a workgroup per image also makes the style branch uniform for the whole workgroup and lets
// every stage run over the 784 pixels with all four waves.  The style and the zigzag (r0, dr) are drawn by thread 0
// from one Philox call per image; the counter is advanced by the last workgroup to finish (reparam_kernel's pattern).
// A large launch gives every workgroup ipw <= SY_MAXIPW consecutive images to work through one after the other
// (about SY_GRID workgroups in all); DESIGN 4g has the measurement behind that.
//
// Numerics: identity / stripe are exact; brightness, scale, the zigzag line distance and the canny front end
// (Gaussian, bleed-over normalisation, Sobel, magnitude, non-maximum suppression) are evaluated in fp64, the zigzag
// decay uses logf.  The hysteresis is a flood over the int state plane from the strong candidates, repeated until a
// sweep changes nothing and at most SY_SWEEPS = 784 times: every sweep but the last promotes at least one of at most
// 784 pixels, so the bound is never what ends it, and no data can make the kernel spin.
#include <math.h>

#include "cv_common.hpp"

namespace cv {

constexpr int SY_W = 28, SY_PIX = SY_W * SY_W, SY_NT = 256;
constexpr int SY_PP = (SY_PIX + SY_NT - 1) / SY_NT;  // pixels per thread
constexpr int SY_MAXS = 16;                          // styles at most
constexpr int SY_SEG = 7;                            // segments of every zigzag polyline
constexpr int SY_SWEEPS = SY_PIX;                    // hysteresis sweeps at most
constexpr int SY_MAXIPW = 32;                        // consecutive images a workgroup works through at most
constexpr int SY_GRID = 16384;                      // workgroups a large launch aims for (64 per CU)
constexpr uint64_t SY_TAG = 0x7374796c65ull;

struct StyleArgs {
  const uint8_t* images;
  const int64_t* label;
  const float* table;
  const double* zz_pts;     // [10][8][2] (col, row) with r0 = 0
  const int32_t* zz_cols;   // [10][7][2] (floor(c0), ceil(c1))
  const int32_t* style_in;
  const int32_t* zz_in;
  const uint8_t* cand_in;
  uint64_t* offset;
  float* out;
  int64_t* style_out;
  int32_t* zz_out;
  uint64_t seed;
  int n, n_class, n_style;
  int ipw;  // images per workgroup, 1..SY_MAXIPW
  uint64_t kinds, sevs;  // 4 bits per style: CV_STYLE_*, the severity
};

// the sigma = 1, truncate = 4 Gaussian taps exp(-k^2 / 2) / sum for |k| = 0..4, as scipy.ndimage rounds them
__device__ __forceinline__ double sy_tap(int k) {
  const int a = k < 4 ? 4 - k : k - 4;
  return a == 0 ? 0.39894346935609776 : a == 1 ? 0.24197144565660073 : a == 2 ? 0.05399112742070441
       : a == 3 ? 0.0044318616200312655 : 0.00013383062461474175;
}

__device__ __forceinline__ int sy_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum of the Gaussian taps that fall inside the image at index i (the filter applied to an all-ones line)
__device__ __forceinline__ double sy_ones(int i) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int j = i + k - 4;
    s += (j >= 0 && j < SY_W) ? sy_tap(k) : 0.0;
  }
  return s;
}

__global__ __launch_bounds__(SY_NT, 5) void style_mnist_kernel(const StyleArgs A) {
  __shared__ float xs[SY_PIX];      // the digit, 0..255
  __shared__ double pa[SY_PIX];     // canny: blur along axis 0, later the gradient magnitude
  __shared__ double pb[SY_PIX];     // canny: the normalised smoothed image
  __shared__ int st[SY_PIX];        // canny: 0 no candidate, 1 weak candidate, 2 kept
  __shared__ double sgd[SY_SEG][3];  // zigzag segment: c0, r0, slope
  __shared__ int sgc[SY_SEG][2];     // zigzag segment: first column, one past the last
  __shared__ int hd[8];              // style, kind, severity, r0, dr, -, the two sweep flags
  const uint64_t off = A.offset ? A.offset[0] : 0;

#pragma unroll 1
  for (int it = 0; it < SY_MAXIPW; ++it) {  // this workgroup's images, one after the other
    const size_t img = (size_t)blockIdx.x * A.ipw + it;
    if (it >= A.ipw || img >= (size_t)A.n) break;  // (uniform)
    // the thread index, opaque per image: otherwise every per-pixel constant of every style (rows, columns, border
    // predicates, sample coordinates, tap sums) is hoisted out of this loop and kept live: 237 VGPRs and two waves
    // per SIMD, against 96 and five
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    if (t < SY_PIX / 4) {  // (the host checked that images is 4-byte aligned; 784 = 4 * 196)
      const uint32_t v = reinterpret_cast<const uint32_t*>(A.images + img * SY_PIX)[t];
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[4 * t + k] = (float)((v >> (8 * k)) & 255u);
    }
    if (t == 0) {
      const u32x4 u = philox(A.seed, off ^ SY_TAG, (uint64_t)img);
      int style;
      if (A.style_in) {
        style = sy_clamp(A.style_in[img], 0, A.n_style - 1);
      } else {
        const int64_t lab = A.label[img];
        const int row = lab < 0 ? 0 : (lab >= (int64_t)A.n_class ? A.n_class - 1 : (int)lab);
        const float* pr = A.table + (size_t)row * A.n_style;
        const double ux = (double)u.x * (1.0 / 4294967296.0);
        double cum = 0.0;
        int lastnz = 0;
        style = -1;
        for (int s = 0; s < SY_MAXS; ++s) {
          if (s < A.n_style) {
            const float p = pr[s];
            if (p > 0.f) lastnz = s;
            cum += (double)p;
            if (style < 0 && cum > ux) style = s;
          }
        }
        if (style < 0) style = lastnz;  // (rounding: the row summed to a little under u)
      }
      int r0, dr;
      if (A.zz_in) {
        r0 = sy_clamp(A.zz_in[2 * img], 0, 26);
        dr = sy_clamp(A.zz_in[2 * img + 1], -5, 4);
      } else {
        r0 = (int)floor((double)u.y * (1.0 / 4294967296.0) * 27.0);
        dr = (int)floor((double)u.z * (1.0 / 4294967296.0) * 10.0) - 5;
      }
      const int kind = (int)((A.kinds >> (4 * style)) & 15u), sev = (int)((A.sevs >> (4 * style)) & 15u);
      hd[0] = style; hd[1] = kind; hd[2] = sev; hd[3] = r0; hd[4] = dr;
      A.style_out[img] = (int64_t)style;
      A.zz_out[2 * img] = r0;
      A.zz_out[2 * img + 1] = dr;
    }
    __syncthreads();
    const int kind = hd[1], sev = hd[2];
    float* dst = A.out + img * SY_PIX;

    if (kind == CV_STYLE_IDENTITY || kind == CV_STYLE_STRIPE) {
#pragma unroll
      for (int k = 0; k < SY_PP; ++k) {
        const int p = t + k * SY_NT;
        if (p < SY_PIX) {
          const int c = p % SY_W;
          const float x = xs[p];
          dst[p] = (kind == CV_STYLE_STRIPE && (c < 7 || c >= 21)) ? 255.f - x : x;
        }
      }
    } else if (kind == CV_STYLE_BRIGHTNESS) {
      const double add = 0.1 * (double)sev;
#pragma unroll
      for (int k = 0; k < SY_PP; ++k) {
        const int p = t + k * SY_NT;
        if (p < SY_PIX) dst[p] = (float)(fmin((double)xs[p] / 255.0 + add, 1.0) * 255.0);
      }
    } else if (kind == CV_STYLE_SCALE) {
      // s = 1 / (1 - 0.1 sev) as the reference's literals
      const double s = sev == 1 ? 1.0 / 0.9 : sev == 2 ? 1.0 / 0.8 : sev == 3 ? 1.0 / 0.7 : sev == 4 ? 1.0 / 0.6 : 2.0;
      const double tr = 13.5 * (1.0 - s);
#pragma unroll
      for (int k = 0; k < SY_PP; ++k) {
        const int p = t + k * SY_NT;
        if (p < SY_PIX) {
          const int r = p / SY_W, c = p - r * SY_W;
          const double yr = s * (double)r + tr, xc = s * (double)c + tr;
          const double fr = floor(yr), fc = floor(xc);
          const int r0 = (int)fr, c0 = (int)fc;
          const double ty = yr - fr, tx = xc - fc;
          double v[2][2];
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const int rr = r0 + a, cc = c0 + b;
              const bool in = rr >= 0 && rr < SY_W && cc >= 0 && cc < SY_W;
              v[a][b] = in ? (double)xs[in ? rr * SY_W + cc : 0] / 255.0 : 0.0;
            }
          const double top = (1.0 - tx) * v[0][0] + tx * v[0][1];
          const double bot = (1.0 - tx) * v[1][0] + tx * v[1][1];
          const double val = (1.0 - ty) * top + ty * bot;
          dst[p] = (float)(fmin(fmax(val, 0.0), 1.0) * 255.0);
        }
      }
    } else if (kind == CV_STYLE_ZIGZAG) {
      const int r0 = hd[3], di = hd[4] + 5;
      if (t < SY_SEG) {
        const double* q = A.zz_pts + ((size_t)di * 8 + t) * 2;
        const double c0 = q[0], ra = q[1] + (double)r0, c1 = q[2], rb = q[3] + (double)r0;
        sgd[t][0] = c0;
        sgd[t][1] = ra;
        sgd[t][2] = (rb - ra) / (c1 - c0);
        sgc[t][0] = sy_clamp(A.zz_cols[((size_t)di * SY_SEG + t) * 2], 0, SY_W);
        sgc[t][1] = sy_clamp(A.zz_cols[((size_t)di * SY_SEG + t) * 2 + 1], 0, SY_W);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < SY_PP; ++k) {
        const int p = t + k * SY_NT;
        if (p < SY_PIX) {
          const int r = p / SY_W, c = p - r * SY_W;
          double x = (double)xs[p] / 255.0;
#pragma unroll
          for (int g = 0; g < SY_SEG; ++g) {
            if (c >= sgc[g][0] && c < sgc[g][1]) {
              const double f = sgd[g][2] * ((double)c - sgd[g][0]) + sgd[g][1];
              const double dist = fmin(fabs((double)r - f), 2.3 - 1e-10);
              const float seg = fminf(fmaxf(logf((float)(1.0 - dist / 2.3)) + 1.f, 0.f), 1.f);
              x = fmin(fmax(x + (double)seg, 0.0), 1.0);
            }
          }
          dst[p] = (float)(x * 255.0);
        }
      }
    } else {  // CV_STYLE_CANNY
      if (A.cand_in) {
        // test hook: the candidate classes are given, the front end is skipped
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          if (p < SY_PIX) st[p] = min((int)A.cand_in[img * SY_PIX + p], 2);
        }
      } else {
        // 1. Gaussian along axis 0 (zero outside the image)
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          if (p < SY_PIX) {
            const int r = p / SY_W, c = p - r * SY_W;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
              const int rr = r + j - 4;
              const bool in = rr >= 0 && rr < SY_W;
              acc += in ? sy_tap(j) * ((double)xs[in ? rr * SY_W + c : 0] / 255.0) : 0.0;
            }
            pa[p] = acc;
          }
        }
        __syncthreads();
        // 2. along axis 1, divided by the same filter over an all-ones image + eps
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          if (p < SY_PIX) {
            const int r = p / SY_W, c = p - r * SY_W;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
              const int cc = c + j - 4;
              const bool in = cc >= 0 && cc < SY_W;
              acc += in ? sy_tap(j) * pa[in ? r * SY_W + cc : 0] : 0.0;
            }
            pb[p] = acc / (sy_ones(r) * sy_ones(c) + 2.220446049250313e-16);
          }
        }
        __syncthreads();
        // 3./4. Sobel (reflect = clamped indices) and the magnitude; gi, gj stay in registers for step 5
        double gi[SY_PP], gj[SY_PP];
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          gi[k] = gj[k] = 0.0;
          if (p < SY_PIX) {
            const int r = p / SY_W, c = p - r * SY_W;
            const int ru = max(r - 1, 0), rd = min(r + 1, SY_W - 1), cl = max(c - 1, 0), cr = min(c + 1, SY_W - 1);
            const double a00 = pb[ru * SY_W + cl], a01 = pb[ru * SY_W + c], a02 = pb[ru * SY_W + cr];
            const double a10 = pb[r * SY_W + cl], a12 = pb[r * SY_W + cr];
            const double a20 = pb[rd * SY_W + cl], a21 = pb[rd * SY_W + c], a22 = pb[rd * SY_W + cr];
            gi[k] = (a20 - a00) + 2.0 * (a21 - a01) + (a22 - a02);
            gj[k] = (a02 - a00) + 2.0 * (a12 - a10) + (a22 - a20);
            pa[p] = sqrt(gi[k] * gi[k] + gj[k] * gj[k]);
          }
        }
        __syncthreads();
        // 5. non-maximum suppression with the linearly interpolated neighbours along +- the gradient
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          if (p < SY_PIX) {
            const int r = p / SY_W, c = p - r * SY_W;
            const double m = pa[p];
            int state = 0;
            if (r >= 1 && r < SY_W - 1 && c >= 1 && c < SY_W - 1 && m >= 0.1) {
              const double i_ = gi[k], j_ = gj[k], ai = fabs(i_), aj = fabs(j_);
              const bool same = (i_ >= 0.0 && j_ >= 0.0) || (i_ <= 0.0 && j_ <= 0.0);  // the diagonal is (+1, +1)
              const int dd = same ? 1 : -1;  // column step of the diagonal that goes with a row step of +1
              double w, ax1, ax2, dg1, dg2;
              if (ai > aj) {  // nearer the row axis
                w = aj / ai;
                const int s = same ? 1 : -1;  // (cond2 takes the row step -1 first; the pair is symmetric)
                ax1 = pa[(r + s) * SY_W + c];
                dg1 = pa[(r + s) * SY_W + c + s * dd];
                ax2 = pa[(r - s) * SY_W + c];
                dg2 = pa[(r - s) * SY_W + c - s * dd];
              } else {  // nearer the column axis
                w = ai / aj;
                ax1 = pa[r * SY_W + c + 1];
                dg1 = pa[(r + dd) * SY_W + c + 1];
                ax2 = pa[r * SY_W + c - 1];
                dg2 = pa[(r - dd) * SY_W + c - 1];
              }
              const bool keep = (dg1 * w + ax1 * (1.0 - w) <= m) && (dg2 * w + ax2 * (1.0 - w) <= m);
              state = keep ? (m >= 0.2 ? 2 : 1) : 0;
            }
            st[p] = state;
          }
        }
      }
      // 6. hysteresis: flood the kept state from the strong candidates through 8-connected weak ones
      volatile int* sv = st;
      for (int sweep = 0; sweep < SY_SWEEPS; ++sweep) {
        volatile int* flag = hd + 6 + (sweep & 1);
        if (t == 0) *flag = 0;
        __syncthreads();
        bool changed = false;
#pragma unroll
        for (int k = 0; k < SY_PP; ++k) {
          const int p = t + k * SY_NT;
          if (p < SY_PIX && sv[p] == 1) {
            const int r = p / SY_W, c = p - r * SY_W;
            bool hit = false;
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
              for (int dc = -1; dc <= 1; ++dc) {
                const int rr = r + dr, cc = c + dc;
                const bool in = rr >= 0 && rr < SY_W && cc >= 0 && cc < SY_W;
                hit = hit || (in && sv[in ? rr * SY_W + cc : p] == 2);
              }
            if (hit) {
              sv[p] = 2;
              changed = true;
            }
          }
        }
        if (changed) *flag = 1;
        __syncthreads();
        if (*flag == 0) break;  // (uniform: every thread reads the same flag after the barrier)
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < SY_PP; ++k) {
        const int p = t + k * SY_NT;
        if (p < SY_PIX) dst[p] = st[p] == 2 ? 255.f : 0.f;
      }
    }
    __syncthreads();  // (the next image overwrites xs and hd)
  }

  if (A.offset && !(A.style_in && A.zz_in)) {  // the last workgroup to finish advances the counter
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

}  // namespace cv

using namespace cv;

extern "C" int cv_style_mnist(const uint8_t* images, int n, int h, int w, const int64_t* label, const float* table,
                              int n_class, int n_style, const int* kind, const int* severity, const double* zz_pts,
                              const int32_t* zz_cols, uint64_t seed, uint64_t* offset, const int32_t* style_in,
                              const int32_t* zz_in, const uint8_t* cand_in, float* out, int64_t* style_out,
                              int32_t* zz_out, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(h == SY_W && w == SY_W, "style_mnist: only 28x28 images are supported (got %dx%d)", h, w);
  CV_REQUIRE(n_style >= 1 && n_style <= SY_MAXS, "style_mnist: n_style=%d outside 1..%d", n_style, SY_MAXS);
  CV_REQUIRE(n > 0, "style_mnist: n=%d must be positive", n);
  CV_REQUIRE(n_class >= 1, "style_mnist: n_class=%d must be positive", n_class);
  CV_REQUIRE(images && label && table && kind && severity && zz_pts && zz_cols && out && style_out && zz_out,
             "style_mnist: images, label, table, kind, severity, the zigzag table or an output is missing");
  CV_REQUIRE((uintptr_t)images % 4 == 0, "style_mnist: images must be 4-byte aligned");
  StyleArgs A;
  memset(&A, 0, sizeof(A));
  for (int s = 0; s < n_style; ++s) {
    CV_REQUIRE(kind[s] >= CV_STYLE_IDENTITY && kind[s] <= CV_STYLE_BRIGHTNESS, "style_mnist: kind[%d]=%d unknown", s,
               kind[s]);
    const bool graded = kind[s] == CV_STYLE_SCALE || kind[s] == CV_STYLE_BRIGHTNESS;
    CV_REQUIRE(!graded || (severity[s] >= 1 && severity[s] <= 5), "style_mnist: severity[%d]=%d outside 1..5", s,
               severity[s]);
    A.kinds |= (uint64_t)kind[s] << (4 * s);
    A.sevs |= (uint64_t)(graded ? severity[s] : 1) << (4 * s);
  }
  A.images = images; A.label = label; A.table = table; A.zz_pts = zz_pts; A.zz_cols = zz_cols;
  A.style_in = style_in; A.zz_in = zz_in; A.cand_in = cand_in; A.offset = offset;
  A.out = out; A.style_out = style_out; A.zz_out = zz_out;
  A.seed = seed; A.n = n; A.n_class = n_class; A.n_style = n_style;
  A.ipw = cdiv(n, SY_GRID) > SY_MAXIPW ? SY_MAXIPW : cdiv(n, SY_GRID);
  hipLaunchKernelGGL(style_mnist_kernel, dim3(cdiv(n, A.ipw)), dim3(SY_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("style_mnist");
  return 0;
}
