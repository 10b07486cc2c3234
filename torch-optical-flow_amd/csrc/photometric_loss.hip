// photometric_loss (gfx950): the SSIM and Charbonnier photometric terms of the unsupervised flow methods (UnFlow, UFlow,
// ARFlow: census, SSIM and robust L1 are the three they ablate between), forward and backward. include/oflow.h states
// the two contracts and the closed-form gradients.
//
// SSIM forward: one tiled launch. A workgroup of 256 threads owns a kTileW x kTileH = 64 x 8 tile of output pixels of
// one image, two pixels per thread (rows ly and ly + 4, so a wave reads 64 consecutive values of an LDS row: no bank
// conflict). It loops over the channels and stages x, y and e = x - y (formed in fp64, which is exact for fp32 frames,
// and rounded once) with a halo of r = window / 2 in LDS, so each frame is read once plus the halo. A thread evaluates
// a pixel in two passes over the window, rows weighted after the columns, on the values less the centre pixel's: the
// means mu_x, mu_y and dm = sum w e, then the centred sums v_x, v_y and v_d = sum w (e - dm)^2. 1 - SSIM is formed
// without the textbook quotient's cancellation: (A1 v_d + dm^2 B2) / ((A1 + dm^2) B2), every term non-negative on
// non-negative frames. The workgroup
// reduces (sum M d, sum M) in fp64 -- per thread, __shfl_xor within the wave, LDS across the waves -- and writes one
// partial row into the caller's workspace; a one-workgroup finalize kernel adds the rows in index order. No atomics,
// no last-arriver, the grid depends on the shapes only: bit-identical from run to run.
//
// SSIM backward: a pure gather over the same tiles. d(1 - SSIM(p)) / dx(q) = w(q - p) (Px(p) + al(p) (x(q) - x(p)) +
// be(p) (y(q) - y(p)) + ga(p) (e(q) - e(p))), and for y the same with x and y swapped, Py and -ga (coefficients()
// below), so a tile needs the five coefficient planes (three per gradient and side of the contrast term's switch),
// scaled by the pixel's share of the loss, with a halo of r, and the staged planes with a halo of 2r to recompute the
// statistics under them. Every element of a requested gradient is written; nothing is accumulated in memory. LDS at
// window 11: 3 x 28 x 84 + 5 x 18 x 74 floats = 53.6 KiB, two workgroups per CU.
//
// Charbonnier: a streaming forward (four consecutive pixels per thread, 16-byte loads where the plane size and the
// pointers allow them, the same reduction tail) and an elementwise backward.
#include "oflow_internal.h"

#include <climits>
#include <cmath>

namespace oflow {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 8;  // output pixels of a workgroup: rows ly and ly + kTileH / 2 of each thread
constexpr int kMaxWindow = 11;

struct SsimArgs {
  const float* frame[2];
  const void* mask;
  int mask_kind;
  int B, C, H, W;
  int tiles_x, tiles_y;
  float w[kMaxWindow];  // the 1-D weights, window of them
  float c1, c2;
  float k;  // 1 - (sum w)^2: the fp32 weights do not add up to exactly 1
};

__device__ __forceinline__ float mask_at(const void* m, int kind, long long i) {
  if (kind == OFLOW_VALID_F32) return static_cast<const float*>(m)[i];
  if (kind == OFLOW_VALID_U8) return static_cast<const unsigned char*>(m)[i] ? 1.f : 0.f;
  return 1.f;
}

// Channel c of tile (b, y0, x0) with a halo of HALO into s[3][LH * LW]: x, y and e = x - y, the difference formed in
// fp64 and rounded once (it would otherwise be lost between two similar frames); 0 outside the image.
template <int HALO>
__device__ __forceinline__ void stage_channel(const SsimArgs& a, int b, int c, int y0, int x0, float* s) {
  constexpr int LH = kTileH + 2 * HALO, LW = kTileW + 2 * HALO;
  const long long plane = static_cast<long long>(a.H) * a.W;
  const long long base = (static_cast<long long>(b) * a.C + c) * plane;
  for (int i = threadIdx.x; i < LH * LW; i += kThreads) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gy = y0 - HALO + ly, gx = x0 - HALO + lx;
    float x = 0.f, y = 0.f, e = 0.f;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const long long o = base + static_cast<long long>(gy) * a.W + gx;
      x = a.frame[0][o];
      y = a.frame[1][o];
      e = static_cast<float>(static_cast<double>(x) - static_cast<double>(y));
    }
    s[i] = x;
    s[LH * LW + i] = y;
    s[2 * LH * LW + i] = e;
  }
}

struct Stats {
  float mx, my, dm, vx, vy, vd;
  float ox, oy, oe;  // the means' offsets from the centre values: mu_x - x(p), mu_y - y(p), dm - e(p)
  float cxy;         // (CROSS only)
};

// The window statistics of the pixel at (cy, cx) of the staged planes (row stride LW, plane stride PS); the whole window
// is inside the planes. wy: the weights in LDS (the rows are rolled, so their index is dynamic); the columns' come
// from the kernel arguments with static indices. Two passes, both on the values less the centre pixel's (x(p), y(p),
// e(p)), so that a flat neighbourhood keeps its small deviations instead of losing them under the mean's rounding:
// the offsets o = sum w (t(p + d) - t(p)) - k t(p) of the means (mu = t(p) + o; k = 1 - (sum w)^2), then the sums of
// ((t(p + d) - t(p)) - o)^2 -- and, for the backward (CROSS), the cross sum c_xy of x and y.
template <int WIN, bool CROSS>
__device__ __forceinline__ Stats window_stats(const SsimArgs& a, const float* s, int PS, int LW, int cy, int cx,
                                              const float* wy) {
  constexpr int R = WIN / 2;
  const float* sx = s + (cy - R) * LW + cx - R;
  const float xp = sx[R * LW + R], yp = sx[PS + R * LW + R], ep = sx[2 * PS + R * LW + R];
  Stats t = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int dy = 0; dy < WIN; ++dy) {
    float rx = 0.f, ry = 0.f, re = 0.f;
#pragma unroll
    for (int dx = 0; dx < WIN; ++dx) {
      const int o = dy * LW + dx;
      rx = fmaf(a.w[dx], sx[o] - xp, rx);
      ry = fmaf(a.w[dx], sx[PS + o] - yp, ry);
      re = fmaf(a.w[dx], sx[2 * PS + o] - ep, re);
    }
    const float w = wy[dy];
    t.ox = fmaf(w, rx, t.ox);
    t.oy = fmaf(w, ry, t.oy);
    t.oe = fmaf(w, re, t.oe);
  }
  t.ox = fmaf(-a.k, xp, t.ox);
  t.oy = fmaf(-a.k, yp, t.oy);
  t.oe = fmaf(-a.k, ep, t.oe);
  t.mx = xp + t.ox;
  t.my = yp + t.oy;
  t.dm = ep + t.oe;
#pragma unroll 1
  for (int dy = 0; dy < WIN; ++dy) {
    float rx = 0.f, ry = 0.f, re = 0.f, rc = 0.f;
#pragma unroll
    for (int dx = 0; dx < WIN; ++dx) {
      const int o = dy * LW + dx;
      const float ax = (sx[o] - xp) - t.ox, ay = (sx[PS + o] - yp) - t.oy, ae = (sx[2 * PS + o] - ep) - t.oe;
      rx = fmaf(a.w[dx], ax * ax, rx);
      ry = fmaf(a.w[dx], ay * ay, ry);
      re = fmaf(a.w[dx], ae * ae, re);
      if (CROSS) rc = fmaf(a.w[dx], ax * ay, rc);
    }
    const float w = wy[dy];
    t.vx = fmaf(w, rx, t.vx);
    t.vy = fmaf(w, ry, t.vy);
    t.vd = fmaf(w, re, t.vd);
    if (CROSS) t.cxy = fmaf(w, rc, t.cxy);
  }
  return t;
}

// 1 - SSIM in the cancellation-free form
__device__ __forceinline__ float one_minus_ssim(const Stats& t, float c1, float c2) {
  const float a1 = 2.f * t.mx * t.my + c1, b2 = t.vx + t.vy + c2, dm2 = t.dm * t.dm;
  return (a1 * t.vd + dm2 * b2) / ((a1 + dm2) * b2);
}

__device__ __forceinline__ void tile_of(const SsimArgs& a, int& b, int& y0, int& x0) {
  const int t = blockIdx.x;
  const int per_image = a.tiles_x * a.tiles_y;
  b = t / per_image;
  const int r = t - b * per_image;
  const int ty = r / a.tiles_x;
  y0 = ty * kTileH;
  x0 = (r - ty * a.tiles_x) * kTileW;
}

// the weights into LDS, with static indices into the kernel arguments
template <int WIN>
__device__ __forceinline__ void stage_weights(const SsimArgs& a, float* wy) {
#pragma unroll
  for (int i = 0; i < WIN; ++i)
    if (threadIdx.x == i) wy[i] = a.w[i];
}

template <int WIN>
__global__ __launch_bounds__(kThreads) void ssim_forward_kernel(SsimArgs a, float* __restrict__ ssim_map,
                                                                double* __restrict__ partials) {
  constexpr int R = WIN / 2, LH = kTileH + 2 * R, LW = kTileW + 2 * R;
  __shared__ float s[3 * LH * LW];
  __shared__ float wy[kMaxWindow];
  int b, y0, x0;
  tile_of(a, b, y0, x0);
  stage_weights<WIN>(a, wy);
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int px = x0 + lx;
  bool interior[2];
  float f[2] = {0.f, 0.f};  // sum over the channels of 1 - SSIM_c
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int py = y0 + ly + k * (kTileH / 2);
    interior[k] = py >= R && py < a.H - R && px >= R && px < a.W - R;
  }
  for (int c = 0; c < a.C; ++c) {
    if (c) __syncthreads();  // the previous channel's planes have been read
    stage_channel<R>(a, b, c, y0, x0, s);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!interior[k]) continue;
      const Stats t = window_stats<WIN, false>(a, s, LH * LW, LW, ly + k * (kTileH / 2) + R, lx + R, wy);
      f[k] += one_minus_ssim(t, a.c1, a.c2);
    }
  }
  double sum_d = 0.0, sum_m = 0.0;
  const float inv_c = 1.f / static_cast<float>(a.C);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int py = y0 + ly + k * (kTileH / 2);
    if (py < a.H && px < a.W) {
      const long long o = (static_cast<long long>(b) * a.H + py) * a.W + px;
      if (interior[k]) {
        const float m = mask_at(a.mask, a.mask_kind, o);
        sum_d += static_cast<double>(m * (f[k] * (0.5f * inv_c)));
        sum_m += static_cast<double>(m);
      }
      if (ssim_map) ssim_map[o] = interior[k] ? 1.f - f[k] * inv_c : 0.f;
    }
  }
  block_sum2_f64(sum_d, sum_m);
  if (threadIdx.x == 0) {
    partials[2LL * blockIdx.x] = sum_d;
    partials[2LL * blockIdx.x + 1] = sum_m;
  }
}

// one workgroup: thread t adds the rows t, t + 256, ... in index order, then block_sum2_f64's fixed order
__global__ __launch_bounds__(kThreads) void photometric_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                        float* __restrict__ loss,
                                                                        double* __restrict__ sum_m_out) {
  double sr = 0.0, sm = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) {
    sr += partials[2LL * i];
    sm += partials[2LL * i + 1];
  }
  block_sum2_f64(sr, sm);
  if (threadIdx.x == 0) {
    loss[0] = static_cast<float>(sr / (sm + 1e-6));
    sum_m_out[0] = sm;
  }
}

// The coefficients of one pixel and channel (include/oflow.h has the derivation): with l = A1 / T, T = A1 + dm^2,
// G = 2 l / B2 and cs = (2 c_xy + C2) / B2 = 1 - csl, csl = v_d / B2 -- cs taken from whichever side is not a difference
// of near-equal numbers (v_d <= B2 / 2: the frames are similar, 1 - csl; else from c_xy) --
//   Fx = 2 cs dm (mu_y (mu_x + mu_y) + C1) / T^2,  Fy = -2 cs dm (mu_x (mu_x + mu_y) + C1) / T^2,
//   dF(p)/dx(q) = w(q - p) (Fx' + al (x(q) - mu_x) + be (y(q) - mu_y) + ga (e(q) - dm)),  Fx' = Fx - k G (dm - csl mu_x),
//   dF(p)/dy(q) = w(q - p) (Fy' + al (y(q) - mu_y) + be (x(q) - mu_x) - ga (e(q) - dm)),  Fy' = Fy + k G (dm + csl mu_y),
// with (al, be, ga) = (-G csl, 0, G) for similar frames, G ((e - dm) - csl (x - mu_x)), and (G cs, -G, 0) otherwise,
// G (cs (x - mu_x) - (y - mu_y)): the same number, each where it does not cancel. The gather takes its differences from
// the centre pixel's values, t(q) - mu = (t(q) - t(p)) - o, so the planes are Px = Fx' - (al ox + be oy + ga oe),
// Py = Fy' - (al oy + be ox - ga oe), al, be and ga.
__device__ __forceinline__ void coefficients(const Stats& t, float c1, float c2, float k, float& px, float& py, float& al,
                                             float& be, float& ga) {
  const float a1 = 2.f * t.mx * t.my + c1, b2 = t.vx + t.vy + c2, dm2 = t.dm * t.dm;
  const float tt = a1 + dm2;
  const bool far = t.vd > 0.5f * b2;
  const float cs = far ? (2.f * t.cxy + c2) / b2 : 1.f - t.vd / b2;
  const float csl = far ? 1.f - cs : t.vd / b2;
  const float g = 2.f * (a1 / tt) / b2;
  const float sum_mu = t.mx + t.my;
  const float lum = (2.f * cs * t.dm) / (tt * tt);
  const float fx = lum * (t.my * sum_mu + c1), fy = -lum * (t.mx * sum_mu + c1);
  al = far ? g * cs : -(g * csl);
  be = far ? -g : 0.f;
  ga = far ? 0.f : g;
  px = (fx - k * g * (t.dm - csl * t.mx)) - (al * t.ox + be * t.oy + ga * t.oe);
  py = (fy + k * g * (t.dm + csl * t.my)) - (al * t.oy + be * t.ox - ga * t.oe);
}

template <int WIN>
__global__ __launch_bounds__(kThreads) void ssim_backward_kernel(SsimArgs a, const float* __restrict__ grad_loss,
                                                                 const double* __restrict__ sum_m,
                                                                 float* __restrict__ grad0, float* __restrict__ grad1) {
  constexpr int R = WIN / 2, GH = 2 * R;  // the staged planes' halo
  constexpr int LH = kTileH + 2 * GH, LW = kTileW + 2 * GH;
  constexpr int CH = kTileH + 2 * R, CW = kTileW + 2 * R;
  __shared__ float s[3 * LH * LW];
  __shared__ float cf[5 * CH * CW];
  __shared__ float wy[kMaxWindow];
  int b, y0, x0;
  tile_of(a, b, y0, x0);
  stage_weights<WIN>(a, wy);
  // a pixel's share of the loss: grad_loss * M / (sum M + 1e-6) / (2 C)
  const float scale = static_cast<float>(static_cast<double>(grad_loss[0]) / (sum_m[0] + 1e-6) * (0.5 / a.C));
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const long long plane = static_cast<long long>(a.H) * a.W;
  for (int c = 0; c < a.C; ++c) {
    if (c) __syncthreads();  // the previous channel's planes have been read
    stage_channel<GH>(a, b, c, y0, x0, s);
    __syncthreads();
    for (int i = threadIdx.x; i < CH * CW; i += kThreads) {
      const int cy = i / CW, cx = i - cy * CW;
      const int gy = y0 - R + cy, gx = x0 - R + cx;
      float px = 0.f, py = 0.f, al = 0.f, be = 0.f, ga = 0.f;
      if (gy >= R && gy < a.H - R && gx >= R && gx < a.W - R) {  // interior (so inside the image)
        const float gm = scale * mask_at(a.mask, a.mask_kind, (static_cast<long long>(b) * a.H + gy) * a.W + gx);
        if (gm != 0.f) {
          const Stats t = window_stats<WIN, true>(a, s, LH * LW, LW, cy + R, cx + R, wy);
          coefficients(t, a.c1, a.c2, a.k, px, py, al, be, ga);
          px *= gm, py *= gm, al *= gm, be *= gm, ga *= gm;
        }
      }
      cf[i] = px;
      cf[CH * CW + i] = py;
      cf[2 * CH * CW + i] = al;
      cf[3 * CH * CW + i] = be;
      cf[4 * CH * CW + i] = ga;
    }
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
      const int ty = ly + k * (kTileH / 2);
      const int qy = y0 + ty, qx = x0 + lx;
      if (qy >= a.H || qx >= a.W) continue;
      // the pixels p = q - d whose windows hold q: the coefficient planes' rows ty .. ty + 2r, weight w(d) = w(q - p);
      // p's own values are the staged planes' at the same place (their halo is r wider)
      const float* cq = cf + ty * CW + lx;
      const float* sq = s + (ty + R) * LW + lx + R;
      const int q = R * LW + R;
      const float xq = sq[q], yq = sq[LH * LW + q], eq = sq[2 * LH * LW + q];
      float gx = 0.f, gy = 0.f;
#pragma unroll 1
      for (int dy = 0; dy < WIN; ++dy) {
        float rx = 0.f, ry = 0.f;
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) {
          const int oc = dy * CW + dx, os = dy * LW + dx;
          const float al = cq[2 * CH * CW + oc], be = cq[3 * CH * CW + oc];
          const float ge = cq[4 * CH * CW + oc] * (eq - sq[2 * LH * LW + os]);
          const float tx = xq - sq[os], ty_ = yq - sq[LH * LW + os];
          const float w = a.w[WIN - 1 - dx];
          rx = fmaf(w, (cq[oc] + ge) + (al * tx + be * ty_), rx);
          ry = fmaf(w, (cq[CH * CW + oc] - ge) + (al * ty_ + be * tx), ry);
        }
        const float w = wy[WIN - 1 - dy];
        gx = fmaf(w, rx, gx);
        gy = fmaf(w, ry, gy);
      }
      const long long o = (static_cast<long long>(b) * a.C + c) * plane + static_cast<long long>(qy) * a.W + qx;
      if (grad0) grad0[o] = gx;
      if (grad1) grad1[o] = gy;
    }
  }
}

// tiles of one launch, 0 when the shape is outside the kernels' range
long long ssim_tiles(int B, int H, int W, int& tiles_x, int& tiles_y) {
  if (B < 1 || H < 1 || W < 1 || B > 65535 || static_cast<long long>(H) * W > (1LL << 28)) return 0;
  tiles_x = (W + kTileW - 1) / kTileW;
  tiles_y = (H + kTileH - 1) / kTileH;
  const long long n = static_cast<long long>(B) * tiles_x * tiles_y;
  return n <= INT_MAX ? n : 0;
}

int frame_args(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind) {
  if (!d_frame0 || !d_frame1) return OFLOW_E_NULL;
  if (mask_kind < OFLOW_VALID_NONE || mask_kind > OFLOW_VALID_U8) return OFLOW_E_MODE;
  if (mask_kind != OFLOW_VALID_NONE && !d_mask) return OFLOW_E_NULL;
  return OFLOW_OK;
}

bool frames_aligned(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind) {
  return aligned_to(d_frame0, 4) && aligned_to(d_frame1, 4) && (mask_kind != OFLOW_VALID_F32 || aligned_to(d_mask, 4));
}

int ssim_args(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B, int C, int H, int W,
              int window, const float* weights, float c1, float c2, SsimArgs& a, long long& tiles) {
  const int st0 = frame_args(d_frame0, d_frame1, d_mask, mask_kind);
  if (st0 != OFLOW_OK) return st0;
  if (!weights) return OFLOW_E_NULL;
  if (window < 3 || window > kMaxWindow || window % 2 == 0) return OFLOW_E_MODE;
  tiles = ssim_tiles(B, H, W, a.tiles_x, a.tiles_y);
  if (tiles == 0 || C < 1 || !(c1 > 0.f) || !(c2 > 0.f) || !std::isfinite(c1) || !std::isfinite(c2)) return OFLOW_E_SHAPE;
  double sum = 0.0;
  for (int i = 0; i < kMaxWindow; ++i) {
    a.w[i] = i < window ? weights[i] : 0.f;
    if (!std::isfinite(a.w[i])) return OFLOW_E_SHAPE;
    sum += static_cast<double>(a.w[i]);
  }
  if (!frames_aligned(d_frame0, d_frame1, d_mask, mask_kind)) return OFLOW_E_ALIGN;
  a.frame[0] = d_frame0, a.frame[1] = d_frame1;
  a.mask = mask_kind != OFLOW_VALID_NONE ? d_mask : nullptr;
  a.mask_kind = mask_kind;
  a.B = B, a.C = C, a.H = H, a.W = W;
  a.c1 = c1, a.c2 = c2;
  a.k = static_cast<float>(1.0 - sum * sum);
  return OFLOW_OK;
}

// ---------------------------------------------------------------------------------------------------- Charbonnier
constexpr int kPixelsPerThread = 4;

struct CharbArgs {
  const float* frame[2];
  const void* mask;
  int mask_kind;
  int C;
  long long plane, total;  // H * W and B * H * W
  float range, eps2, alpha;
  int root;  // alpha == 0.5: sqrtf instead of powf
};

// q = ((x - y) / image_range)^2 + eps^2 with the difference formed in fp64 and rounded once; z = (x - y) / image_range
__device__ __forceinline__ float charb_q(const CharbArgs& a, float x, float y, float& z) {
  z = static_cast<float>(static_cast<double>(x) - static_cast<double>(y)) / a.range;
  return fmaf(z, z, a.eps2);
}

// The four consecutive pixels i0 .. i0 + 3 of a thread (indices into (B, H, W)): their offsets into a (B, C, H, W) frame
// at channel 0, and whether they exist. VEC: plane is a multiple of 4, so the four share an image and are contiguous.
template <bool VEC>
__device__ __forceinline__ void pixel_offsets(const CharbArgs& a, long long i0, long long off[4], bool ok[4]) {
#pragma unroll
  for (int j = 0; j < kPixelsPerThread; ++j) {
    const long long i = VEC ? i0 : i0 + j;
    ok[j] = i < a.total;
    const long long b = ok[j] ? i / a.plane : 0;
    off[j] = ok[j] ? b * a.C * a.plane + (i - b * a.plane) + (VEC ? j : 0) : 0;
  }
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* f, const long long off[4], const bool ok[4], long long co, float v[4]) {
  if (VEC) {
    const float4 t = ok[0] ? *reinterpret_cast<const float4*>(f + off[0] + co) : make_float4(0.f, 0.f, 0.f, 0.f);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < kPixelsPerThread; ++j) v[j] = ok[j] ? f[off[j] + co] : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void charbonnier_forward_kernel(CharbArgs a, double* __restrict__ partials) {
  const long long i0 = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * kPixelsPerThread;
  long long off[4];
  bool ok[4];
  pixel_offsets<VEC>(a, i0, off, ok);
  float rho[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < a.C; ++c) {
    float x[4], y[4];
    load4<VEC>(a.frame[0], off, ok, c * a.plane, x);
    load4<VEC>(a.frame[1], off, ok, c * a.plane, y);
#pragma unroll
    for (int j = 0; j < kPixelsPerThread; ++j) {
      float z;
      const float q = charb_q(a, x[j], y[j], z);
      rho[j] += a.root ? sqrtf(q) : powf(q, a.alpha);
    }
  }
  double sum_rho = 0.0, sum_m = 0.0;
  const float inv_c = 1.f / static_cast<float>(a.C);
#pragma unroll
  for (int j = 0; j < kPixelsPerThread; ++j) {
    if (!ok[j]) continue;
    const float m = mask_at(a.mask, a.mask_kind, i0 + j);
    sum_rho += static_cast<double>(m * (rho[j] * inv_c));
    sum_m += static_cast<double>(m);
  }
  block_sum2_f64(sum_rho, sum_m);
  if (threadIdx.x == 0) {
    partials[2LL * blockIdx.x] = sum_rho;
    partials[2LL * blockIdx.x + 1] = sum_m;
  }
}

// d loss / d x = grad_loss * M / (sum M + 1e-6) * (2 alpha / (C image_range)) * z * q^(alpha - 1), and the negative for y
template <bool VEC>
__global__ __launch_bounds__(kThreads) void charbonnier_backward_kernel(CharbArgs a, const float* __restrict__ grad_loss,
                                                                        const double* __restrict__ sum_m,
                                                                        float* __restrict__ grad0,
                                                                        float* __restrict__ grad1) {
  const long long i0 = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * kPixelsPerThread;
  long long off[4];
  bool ok[4];
  pixel_offsets<VEC>(a, i0, off, ok);
  if (!ok[0]) return;
  const float scale = static_cast<float>(static_cast<double>(grad_loss[0]) / (sum_m[0] + 1e-6));
  const float cfac = static_cast<float>(2.0 * a.alpha / (static_cast<double>(a.C) * a.range));
  float gm[4];
#pragma unroll
  for (int j = 0; j < kPixelsPerThread; ++j) gm[j] = ok[j] ? scale * mask_at(a.mask, a.mask_kind, i0 + j) : 0.f;
  for (int c = 0; c < a.C; ++c) {
    const long long co = c * a.plane;
    float x[4], y[4], g[4];
    load4<VEC>(a.frame[0], off, ok, co, x);
    load4<VEC>(a.frame[1], off, ok, co, y);
#pragma unroll
    for (int j = 0; j < kPixelsPerThread; ++j) {
      float z;
      const float q = charb_q(a, x[j], y[j], z);
      g[j] = gm[j] * (cfac * (z * (a.root ? 1.f / sqrtf(q) : powf(q, a.alpha - 1.f))));
    }
    if (VEC) {
      if (grad0) *reinterpret_cast<float4*>(grad0 + off[0] + co) = make_float4(g[0], g[1], g[2], g[3]);
      if (grad1) *reinterpret_cast<float4*>(grad1 + off[0] + co) = make_float4(-g[0], -g[1], -g[2], -g[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPixelsPerThread; ++j) {
        if (!ok[j]) continue;
        if (grad0) grad0[off[j] + co] = g[j];
        if (grad1) grad1[off[j] + co] = -g[j];
      }
    }
  }
}

// workgroups of one launch, 0 when the shape is outside the kernels' range; never more than ssim_tiles (a tile holds at
// most 512 pixels, a workgroup here takes 1024), so one workspace query serves both losses
long long charb_blocks(int B, int H, int W) {
  int tx, ty;
  if (ssim_tiles(B, H, W, tx, ty) == 0) return 0;
  const long long per = static_cast<long long>(kThreads) * kPixelsPerThread;
  return (static_cast<long long>(B) * H * W + per - 1) / per;
}

int charb_args(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B, int C, int H, int W,
               float eps, float alpha, float image_range, CharbArgs& a, long long& blocks) {
  const int st0 = frame_args(d_frame0, d_frame1, d_mask, mask_kind);
  if (st0 != OFLOW_OK) return st0;
  blocks = charb_blocks(B, H, W);
  if (blocks == 0 || C < 1 || !(image_range > 0.f) || !std::isfinite(image_range) || !(eps > 0.f) || !std::isfinite(eps) ||
      !(alpha > 0.f) || !(alpha <= 1.f))
    return OFLOW_E_SHAPE;
  if (!frames_aligned(d_frame0, d_frame1, d_mask, mask_kind)) return OFLOW_E_ALIGN;
  a.frame[0] = d_frame0, a.frame[1] = d_frame1;
  a.mask = mask_kind != OFLOW_VALID_NONE ? d_mask : nullptr;
  a.mask_kind = mask_kind;
  a.C = C;
  a.plane = static_cast<long long>(H) * W;
  a.total = a.plane * B;
  a.range = image_range;
  a.eps2 = static_cast<float>(static_cast<double>(eps) * eps);
  a.alpha = alpha;
  a.root = alpha == 0.5f;
  return OFLOW_OK;
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" long long oflow_ssim_loss_workspace_bytes(int B, int H, int W) {
  int tx, ty;
  return 16 * ssim_tiles(B, H, W, tx, ty);
}

extern "C" int oflow_ssim_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B,
                                   int C, int H, int W, int window, const float* weights, float c1, float c2,
                                   float* d_ssim_map, double* d_workspace, float* d_loss, double* d_sum_m, void* stream) {
  if (!d_workspace || !d_loss || !d_sum_m) return OFLOW_E_NULL;
  SsimArgs a;
  long long tiles;
  const int st0 = ssim_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, window, weights, c1, c2, a, tiles);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_ssim_map, 4) || !aligned_to(d_workspace, 8) || !aligned_to(d_loss, 4) || !aligned_to(d_sum_m, 8))
    return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto kernel = window == 11  ? ssim_forward_kernel<11>
                : window == 9 ? ssim_forward_kernel<9>
                : window == 7 ? ssim_forward_kernel<7>
                : window == 5 ? ssim_forward_kernel<5>
                              : ssim_forward_kernel<3>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, st, a, d_ssim_map, d_workspace);
  const int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(photometric_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, static_cast<int>(tiles),
                     d_loss, d_sum_m);
  return launch_status();
}

extern "C" int oflow_ssim_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                            const void* d_mask, int mask_kind, const double* d_sum_m, int B, int C, int H,
                                            int W, int window, const float* weights, float c1, float c2,
                                            float* d_grad_frame0, float* d_grad_frame1, void* stream) {
  if (!d_grad_loss || !d_sum_m || (!d_grad_frame0 && !d_grad_frame1)) return OFLOW_E_NULL;
  SsimArgs a;
  long long tiles;
  const int st0 = ssim_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, window, weights, c1, c2, a, tiles);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_grad_loss, 4) || !aligned_to(d_sum_m, 8) || !aligned_to(d_grad_frame0, 4) ||
      !aligned_to(d_grad_frame1, 4))
    return OFLOW_E_ALIGN;
  auto kernel = window == 11  ? ssim_backward_kernel<11>
                : window == 9 ? ssim_backward_kernel<9>
                : window == 7 ? ssim_backward_kernel<7>
                : window == 5 ? ssim_backward_kernel<5>
                              : ssim_backward_kernel<3>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a,
                     d_grad_loss, d_sum_m, d_grad_frame0, d_grad_frame1);
  return launch_status();
}

extern "C" int oflow_charbonnier_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind,
                                          int B, int C, int H, int W, float eps, float alpha, float image_range,
                                          double* d_workspace, float* d_loss, double* d_sum_m, void* stream) {
  if (!d_workspace || !d_loss || !d_sum_m) return OFLOW_E_NULL;
  CharbArgs a;
  long long blocks;
  const int st0 = charb_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, eps, alpha, image_range, a, blocks);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_workspace, 8) || !aligned_to(d_loss, 4) || !aligned_to(d_sum_m, 8)) return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = a.plane % 4 == 0 && aligned_to(d_frame0, 16) && aligned_to(d_frame1, 16);
  hipLaunchKernelGGL(vec ? charbonnier_forward_kernel<true> : charbonnier_forward_kernel<false>,
                     dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, a, d_workspace);
  const int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(photometric_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, static_cast<int>(blocks),
                     d_loss, d_sum_m);
  return launch_status();
}

extern "C" int oflow_charbonnier_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                                   const void* d_mask, int mask_kind, const double* d_sum_m, int B, int C,
                                                   int H, int W, float eps, float alpha, float image_range,
                                                   float* d_grad_frame0, float* d_grad_frame1, void* stream) {
  if (!d_grad_loss || !d_sum_m || (!d_grad_frame0 && !d_grad_frame1)) return OFLOW_E_NULL;
  CharbArgs a;
  long long blocks;
  const int st0 = charb_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, eps, alpha, image_range, a, blocks);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_grad_loss, 4) || !aligned_to(d_sum_m, 8) || !aligned_to(d_grad_frame0, 4) ||
      !aligned_to(d_grad_frame1, 4))
    return OFLOW_E_ALIGN;
  const bool vec = a.plane % 4 == 0 && aligned_to(d_frame0, 16) && aligned_to(d_frame1, 16) &&
                   aligned_to(d_grad_frame0, 16) && aligned_to(d_grad_frame1, 16);
  hipLaunchKernelGGL(vec ? charbonnier_backward_kernel<true> : charbonnier_backward_kernel<false>,
                     dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a,
                     d_grad_loss, d_sum_m, d_grad_frame0, d_grad_frame1);
  return launch_status();
}
