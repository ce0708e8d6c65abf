// The feature-swapping grid and the style / content interpolation strips of expr/visual_utils.py on the device:
// the n x n swap latents (:34-36), every latent of interpolation_plot's loop (:86-105, with
// src/utils/display_utils.py:11-21 interpolate_latent) and torchvision.utils.make_grid with make_colored_grid's
// recolouring (:13-26) folded in, written straight into a sub-rectangle of the figure's canvas (:44-52, :80-118).
//
// All three kernels are pure data movement: one thread per output element (cv_make_grid: per output pixel, which
// is three elements, because the frame rule couples the channels), consecutive threads on consecutive addresses of
// the output's fastest axis, no LDS, no atomics (two runs give the same bits), every loop-free.  The branches are
// taken per element where the geometry decides them (a pad column next to an image column), uniformly for a wave
// where it allows: a wave of grid_kernel is 64 consecutive pixels of ONE output row, so everything that depends on
// the row alone (pad row or image row, the row of cells, the row inside the image) is wave-uniform.  The sizes the
// figures have (a few hundred KiB) are bounded by launch latency, not by bandwidth, which is why the
// loads and stores are plain 4-byte ones: 256 B per wave and instruction, fully coalesced.
#include "cv_common.hpp"

namespace cv {

constexpr int FG_NT = 256;            // latent kernels: threads per workgroup
constexpr int FG_BX = 64, FG_BY = 4;  // grid_kernel: one wave per output row, four rows per workgroup
constexpr int FG_MAXM = 65536, FG_MAXHW = 4096;

// row i * n + j of out = (z_c[i], z_s[j])
__global__ __launch_bounds__(FG_NT) void latent_pairs_kernel(const float* __restrict__ zc, int ldc,
                                                             const float* __restrict__ zs, int lds, int n, int dc,
                                                             int ds, FDiv fd, FDiv fn, int total,
                                                             float* __restrict__ out) {
  const int idx = blockIdx.x * FG_NT + threadIdx.x;
  if (idx >= total) return;
  const int row = fd.div(idx), col = idx - row * (dc + ds);
  const int i = fn.div(row), j = row - i * n;
  out[idx] = col < dc ? zc[(size_t)i * ldc + col] : zs[(size_t)j * lds + (col - dc)];
}

struct InterpArgs {
  const float* z;
  const int64_t* src;
  const int64_t* tgt;
  float* out;
  FDiv fd, ft;
  int ldz, n, d, z_dim, s, t, total;  // total = 2 * s * t * d
};

// out[0][i][k] = (z1.content, p_k z1.style + (1 - p_k) z2.style), out[1][i][k] = (p_k z1.content + (1 - p_k)
// z2.content, z1.style); p = torch.linspace(1, 0, t) in fp32
__global__ __launch_bounds__(FG_NT) void latent_interp_kernel(const InterpArgs A) {
  const int idx = blockIdx.x * FG_NT + threadIdx.x;
  if (idx >= A.total) return;
  const int row = A.fd.div(idx), col = idx - row * A.d;  // row = (which * s + i) * t + k
  const int pair = A.ft.div(row), k = row - pair * A.t;
  const int which = pair >= A.s ? 1 : 0, i = pair - which * A.s;
  const int64_t a_id = A.src[i], b_id = A.tgt[i];
  // the wrapper checked the ids; a row that is not there is never read
  if (a_id < 0 || a_id >= (int64_t)A.n || b_id < 0 || b_id >= (int64_t)A.n) {
    A.out[idx] = __builtin_nanf("");
    return;
  }
  const float a = A.z[(size_t)a_id * A.ldz + col];
  const bool content = col < A.z_dim;
  if (content != (which == 1)) {  // the copied half: z1, bit for bit
    A.out[idx] = a;
    return;
  }
  const float b = A.z[(size_t)b_id * A.ldz + col];
  float p = 1.f;
  if (A.t > 1) {
    const float step = (0.f - 1.f) / (float)(A.t - 1);
    p = k < A.t / 2 ? 1.f + step * (float)k : 0.f - step * (float)(A.t - 1 - k);
  }
  A.out[idx] = p * a + (1.f - p) * b;
}

struct GridArgs {
  const float* img;  // [m][c][h][w] (null when m = 0)
  float* dst;        // the canvas: element (ch, y, x) at dst[ch * cpitch + y * rpitch + x]
  FDiv fy, fx;       // division by h + pad, w + pad
  FDiv ftx;          // division by the number of workgroups along x
  int m, c, h, w, xmaps, pad, gh, gw;  // gh x gw: the rectangle written
  int cpitch, rpitch, y0, x0, frame;
  float pad_value;
};

__global__ __launch_bounds__(FG_BX* FG_BY) void grid_kernel(const GridArgs A) {
  // (the workgroups are numbered along one axis: a tall grid has more rows of them than gridDim.y allows)
  const int by = A.ftx.div((int)blockIdx.x), bx = (int)blockIdx.x - by * (int)A.ftx.d;
  const int gx = bx * FG_BX + threadIdx.x, gy = by * FG_BY + threadIdx.y;
  if (gx >= A.gw || gy >= A.gh) return;
  float v0 = A.pad_value, v1 = A.pad_value, v2 = A.pad_value;
  if (A.m > 0) {
    // cell (cy, cx) covers rows cy (h + pad) + pad .. + h - 1; the last `pad` rows and columns belong to no cell
    const int cy = A.fy.div(gy), ry = gy - cy * (A.h + A.pad) - A.pad;
    const int cx = A.fx.div(gx), rx = gx - cx * (A.w + A.pad) - A.pad;
    const int k = cy * A.xmaps + cx;
    if (ry >= 0 && rx >= 0 && cx < A.xmaps && k < A.m) {  // (k < m: cy is inside too, and the ragged row ends)
      const float* p = A.img + ((size_t)k * A.c * A.h + ry) * A.w + rx;
      v0 = p[0];
      if (A.c == 3) {
        v1 = p[(size_t)A.h * A.w];
        v2 = p[(size_t)2 * A.h * A.w];
      } else {
        v1 = v2 = v0;
      }
    }
  }
  // make_colored_grid, by value (NaN == 0.25 is false)
  if (A.frame == CV_FRAME_RED) {
    if (v0 == 0.25f) v0 = 1.f;  // the reference's second and third assignments see the mask already cleared
  } else if (A.frame == CV_FRAME_BLUE) {
    if (v2 == 0.25f) {
      v0 = 0.f;
      v1 = 0.f;
      v2 = 1.f;
    }
  }
  float* q = A.dst + (size_t)(A.y0 + gy) * A.rpitch + (A.x0 + gx);
  q[0] = v0;
  q[(size_t)A.cpitch] = v1;
  q[(size_t)2 * A.cpitch] = v2;
}

}  // namespace cv

using namespace cv;

extern "C" int cv_latent_pairs(const float* z_c, int ldc, const float* z_s, int lds, int n, int dc, int ds,
                               float* out, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(z_c && z_s && out, "latent_pairs: z_c, z_s and out must be given");
  CV_REQUIRE(n >= 1 && dc >= 1 && ds >= 1, "latent_pairs: n, dc and ds must be positive (n=%d, dc=%d, ds=%d)", n, dc,
             ds);
  CV_REQUIRE(ldc >= dc && lds >= ds,
             "latent_pairs: a row stride is smaller than its row (ldc=%d, dc=%d, lds=%d, ds=%d)", ldc, dc, lds, ds);
  const long long total = (long long)n * n * ((long long)dc + ds);
  CV_REQUIRE(total < (1ll << 31), "latent_pairs: n * n * (dc + ds) = %lld must be below 2^31", total);
  note_launch((const void*)latent_pairs_kernel);
  hipLaunchKernelGGL(latent_pairs_kernel, dim3(cdiv(total, FG_NT)), dim3(FG_NT), 0, S(stream), z_c, ldc, z_s, lds, n,
                     dc, ds, FDiv::make((uint32_t)(dc + ds)), FDiv::make((uint32_t)n), (int)total, out);
  CV_LAUNCH_CHECK("latent_pairs");
  return 0;
}

extern "C" int cv_latent_interp(const float* z, int ldz, int n, int d, int z_dim, const int64_t* src_ids,
                                const int64_t* tgt_ids, int s, int steps, float* out, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(z && src_ids && tgt_ids && out, "latent_interp: z, src_ids, tgt_ids and out must be given");
  CV_REQUIRE(n >= 1 && d >= 2 && ldz >= d, "latent_interp: needs n >= 1, d >= 2 and a row stride >= d (n=%d, d=%d, "
             "ldz=%d)", n, d, ldz);
  CV_REQUIRE(z_dim >= 1 && z_dim < d, "latent_interp: z_dim=%d must be in 1..%d", z_dim, d - 1);
  CV_REQUIRE(s >= 1 && steps >= 1, "latent_interp: the number of pairs and of steps must be positive (s=%d, steps=%d)",
             s, steps);
  const long long total = 2ll * s * steps * d;
  CV_REQUIRE(total < (1ll << 31), "latent_interp: 2 * s * steps * d = %lld must be below 2^31", total);
  InterpArgs A;
  A.z = z; A.src = src_ids; A.tgt = tgt_ids; A.out = out;
  A.fd = FDiv::make((uint32_t)d); A.ft = FDiv::make((uint32_t)steps);
  A.ldz = ldz; A.n = n; A.d = d; A.z_dim = z_dim; A.s = s; A.t = steps; A.total = (int)total;
  note_launch((const void*)latent_interp_kernel);
  hipLaunchKernelGGL(latent_interp_kernel, dim3(cdiv(total, FG_NT)), dim3(FG_NT), 0, S(stream), A);
  CV_LAUNCH_CHECK("latent_interp");
  return 0;
}

extern "C" int cv_make_grid(const float* images, int m, int c, int h, int w, int nrow, int padding, float pad_value,
                            int frame, int mode, float* dst, int dst_h, int dst_w, long long chan_pitch,
                            long long row_pitch, int y0, int x0, cv_stream_t stream) {
  clear_error();
  CV_REQUIRE(mode == CV_GRID_IMAGES || mode == CV_GRID_FILL, "make_grid: unknown mode %d", mode);
  CV_REQUIRE(frame == CV_FRAME_NONE || frame == CV_FRAME_RED || frame == CV_FRAME_BLUE, "make_grid: unknown frame %d",
             frame);
  CV_REQUIRE(dst, "make_grid: the destination must be given");
  CV_REQUIRE(h >= 1 && w >= 1, "make_grid: h and w must be positive (h=%d, w=%d)", h, w);
  long long gh, gw;
  int xmaps = 1;
  if (mode == CV_GRID_FILL) {
    CV_REQUIRE(m == 0, "make_grid: CV_GRID_FILL takes no images (m=%d)", m);
    gh = h;
    gw = w;
    padding = 0;
  } else {
    CV_REQUIRE(images, "make_grid: images must be given");
    CV_REQUIRE(c == 1 || c == 3, "make_grid: images must have 1 or 3 channels (c=%d)", c);
    CV_REQUIRE(padding >= 0, "make_grid: padding=%d must not be negative", padding);
    CV_REQUIRE(nrow >= 1, "make_grid: nrow=%d must be at least 1", nrow);
    CV_REQUIRE(m >= 1 && m <= FG_MAXM, "make_grid: the number of images must be in 1..%d (m=%d)", FG_MAXM, m);
    CV_REQUIRE(h <= FG_MAXHW && w <= FG_MAXHW, "make_grid: h and w must be at most %d (h=%d, w=%d)", FG_MAXHW, h, w);
    if (m == 1) padding = 0;  // torchvision returns a single image as it is, without a border
    xmaps = nrow < m ? nrow : m;
    const int ymaps = (m + xmaps - 1) / xmaps;
    gh = (long long)ymaps * ((long long)h + padding) + padding;
    gw = (long long)xmaps * ((long long)w + padding) + padding;
  }
  CV_REQUIRE(dst_h >= 1 && dst_w >= 1 && row_pitch >= dst_w && chan_pitch >= (long long)dst_h * row_pitch,
             "make_grid: the destination [3][%d][%d] does not fit its pitches (channel %lld, row %lld)", dst_h, dst_w,
             chan_pitch, row_pitch);
  CV_REQUIRE(2 * chan_pitch + (long long)dst_h * row_pitch < (1ll << 31),
             "make_grid: the destination must span fewer than 2^31 elements");
  CV_REQUIRE(y0 >= 0 && x0 >= 0 && y0 + gh <= dst_h && x0 + gw <= dst_w,
             "make_grid: the %lld x %lld grid at (%d, %d) does not fit the %d x %d destination", gh, gw, y0, x0, dst_h,
             dst_w);
  GridArgs A;
  A.img = mode == CV_GRID_FILL ? nullptr : images;
  A.dst = dst;
  A.fy = FDiv::make((uint32_t)(h + padding));
  A.fx = FDiv::make((uint32_t)(w + padding));
  A.m = m; A.c = c; A.h = h; A.w = w; A.xmaps = xmaps; A.pad = padding; A.gh = (int)gh; A.gw = (int)gw;
  A.cpitch = (int)chan_pitch; A.rpitch = (int)row_pitch; A.y0 = y0; A.x0 = x0; A.frame = frame;
  A.pad_value = pad_value;
  const int tx = cdiv(gw, FG_BX), ty = cdiv(gh, FG_BY);  // (tx * ty < 2^31: gh * gw is below 2^31 / 3)
  A.ftx = FDiv::make((uint32_t)tx);
  note_launch((const void*)grid_kernel);
  hipLaunchKernelGGL(grid_kernel, dim3((unsigned)tx * (unsigned)ty), dim3(FG_BX, FG_BY), 0, S(stream), A);
  CV_LAUNCH_CHECK("make_grid");
  return 0;
}
