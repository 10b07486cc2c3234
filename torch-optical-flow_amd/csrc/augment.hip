// Training-batch augmentation on the device (gfx950): the reference's FlowAugmentor / SparseFlowAugmentor
// (methods/raft/data/augmentor.py) for a whole batch, without writing a jittered or resized intermediate.
// include/oflow.h states the arithmetic; everything is integer or once-rounded IEEE arithmetic in a fixed order
// (contraction off, explicit _rn intrinsics), so the outputs are the same bits on every run and equal a NumPy
// restatement exactly (tests/augment_cases.py).
//
// Three kernels, all driven by one packed (B, OFLOW_AUG_PARAM_DOUBLES) float64 parameter array:
//   * stats: per-channel integer sums over source pixels -- stage 0 the grey sum of each frame as it stands when
//     contrast's turn comes (the ops drawn before contrast applied on the fly), stage 1 the RGB sums of the fully
//     jittered frame 2 (the eraser's fill colour; needs stage 0's result, hence a second launch of the same kernel;
//     samples without a rectangle leave at once). Per-thread uint32 partials, wave shuffles, one 64-bit integer
//     atomic per block and channel: integer sums do not depend on the order, so they are exact and bit-stable.
//   * dense: one thread per output crop pixel. crop -> flip -> resized -> source coordinates; the 2 x 2 source taps
//     of each frame are jittered (and erased) in registers, blended horizontally then vertically, rounded half-even
//     and written CHW fp32; the same thread blends, scales and sign-flips the flow and writes valid. A tap whose
//     weight is zero is not read (S0 * 1 + S1 * 0 == S0 exactly), so a sample without resize costs one tap.
//   * sparse flow: a gather. An output pixel (xx, yy) of the resized map scans the sources whose coordinate can
//     round to it, last row / last column first, and keeps the first valid hit: NumPy's last-write-wins of
//     resize_sparse_flow_map in row-major source order, with no atomics and no scatter.
// Source indices are clamped into the frame in every kernel, so a malformed parameter row (the Python layer rejects
// those before any launch) can give wrong values but never an out-of-bounds access.
//
// The per-pixel cost is the jitter (the hue round trip runs in fp64, as Pillow's C does), up to 8 taps per output
// pixel; the HWC uint8 taps of neighbouring lanes lie in the same or adjacent 64-B lines and the whole batch of
// sources is L2-resident, so the 3-byte stride is not staged through LDS (DESIGN.md §4 "Augmentation").
#include "oflow_internal.h"

// No FMA contraction anywhere in this file: every product and sum below is rounded on its own, as the specification
// (and Pillow's / NumPy's host arithmetic) rounds it. hipcc's default fuses a * b + c across statements and through
// the __fmul_rn / __fadd_rn wrappers -- seen as saturation results one level off where f * (x - d) lies just under an
// integer. The Makefile passes -ffp-contract=off for this file as well.
#pragma clang fp contract(off)

namespace oflow {
namespace {

constexpr int kP = OFLOW_AUG_PARAM_DOUBLES;
constexpr int kStatsThreads = 256;
constexpr int kThreads = 256;

// parameter row (float64): see include/oflow.h
constexpr int P_ASYM = 0, P_FRAME = 1 /* + 8 * frame: order[4], brightness, contrast, saturation, hue */,
              P_NRECT = 17, P_RECT = 18, P_RESIZE = 26, P_SX = 27, P_SY = 28, P_HFLIP = 29, P_VFLIP = 30, P_Y0 = 31,
              P_X0 = 32;

struct Jitter {
  int order[4];
  float fb, fc, fs;
  int hshift;
  int dcontrast;  // the contrast op's grey level (set from the stats)
};

__device__ __forceinline__ Jitter load_jitter(const double* __restrict__ p, int frame) {
  Jitter j;
  const double* q = p + P_FRAME + 8 * frame;
#pragma unroll
  for (int k = 0; k < 4; ++k) j.order[k] = (int)q[k];
  j.fb = (float)q[4];
  j.fc = (float)q[5];
  j.fs = (float)q[6];
  j.hshift = ((int)(q[7] * 255.0)) & 255;  // trunc toward zero, then mod 256
  j.dcontrast = 0;
  return j;
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow's ImagingBlend of a degenerate level d and the pixel x: d + f * (x - d) in fp32, one product and one sum
__device__ __forceinline__ int blend8(int d, int x, float f) {
  const float fd = (float)d;
  const float v = __fadd_rn(fd, __fmul_rn(f, __fsub_rn((float)x, fd)));
  if (f >= 0.0f && f <= 1.0f) return (int)v;
  return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int rnd8(double v) { return clip8((int)round(v)); }  // half away from zero, as C's round

__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = __fdiv_rn(cr, (float)mx);
    const float rc = __fdiv_rn((float)(mx - r), cr);
    const float gc = __fdiv_rn((float)(mx - g), cr);
    const float bc = __fdiv_rn((float)(mx - b), cr);
    float h;
    if (r == mx) h = __fsub_rn(bc, gc);
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double hf = (double)H * 6.0 / 255.0;
  const double fi = floor(hf);
  const int i = (int)fi % 6;
  const double f = (double)(float)(hf - fi);
  const double fs = (double)(float)((double)S / 255.0);
  const double dv = (double)V;
  const int p = rnd8(dv * (1.0 - fs));
  const int q = rnd8(dv * (1.0 - fs * f));
  const int t = rnd8(dv * (1.0 - fs * (1.0 - f)));
  switch (i) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// ops order[0..n) of the draw; stop_at_contrast: stop in front of the contrast op (the grey sum's state)
__device__ __forceinline__ void jitter_pixel(const Jitter& j, bool stop_at_contrast, int& r, int& g, int& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = j.order[k];
    if (op == 0) {
      r = blend8(0, r, j.fb), g = blend8(0, g, j.fb), b = blend8(0, b, j.fb);
    } else if (op == 1) {
      if (stop_at_contrast) return;
      const int d = j.dcontrast;
      r = blend8(d, r, j.fc), g = blend8(d, g, j.fc), b = blend8(d, b, j.fc);
    } else if (op == 2) {
      const int d = luma(r, g, b);
      r = blend8(d, r, j.fs), g = blend8(d, g, j.fs), b = blend8(d, b, j.fs);
    } else if (op == 3) {
      hue_shift(r, g, b, j.hshift);
    }
  }
}

// int(mean + 0.5) of the grey sums: over both frames for a symmetric draw, over the frame's own for an asymmetric one
__device__ __forceinline__ int contrast_level(const unsigned long long* __restrict__ st, bool asym, int frame,
                                              long long hw) {
  const double m = asym ? (double)st[frame] / (double)hw : (double)(st[0] + st[1]) / (double)(2 * hw);
  return (int)(m + 0.5);
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid (blocks per image, frames, B). stage 0: stats[b][frame] += grey sum in front of contrast (frames 0, 1);
// stage 1 (grid.y == 1): stats[b][2 + c] += channel c of jittered frame 2, only where the sample erases.
// A block handles at most 2^16 pixels (the host sizes the grid), so uint32 partials cannot overflow.
__global__ __launch_bounds__(kStatsThreads) void augment_stats_kernel(const uint8_t* __restrict__ img1,
                                                                      const uint8_t* __restrict__ img2,
                                                                      const double* __restrict__ params, int HW,
                                                                      int per_block, int stage,
                                                                      unsigned long long* __restrict__ stats) {
  __shared__ unsigned sm[3][kStatsThreads / 64];
  const int b = blockIdx.z;
  const double* p = params + (long long)b * kP;
  unsigned long long* st = stats + (long long)b * OFLOW_AUG_STATS_WORDS;
  const int frame = stage == 0 ? (int)blockIdx.y : 1;
  if (stage == 1 && (int)p[P_NRECT] <= 0) return;
  Jitter j = load_jitter(p, frame);
  if (stage == 1) j.dcontrast = contrast_level(st, p[P_ASYM] != 0.0, 1, HW);
  const uint8_t* src = (frame == 0 ? img1 : img2) + (long long)b * HW * 3;
  const int s0 = blockIdx.x * per_block, s1 = min(s0 + per_block, HW);
  unsigned a0 = 0, a1 = 0, a2 = 0;
  for (int s = s0 + threadIdx.x; s < s1; s += kStatsThreads) {
    int r = src[3 * (long long)s], g = src[3 * (long long)s + 1], bl = src[3 * (long long)s + 2];
    jitter_pixel(j, stage == 0, r, g, bl);
    if (stage == 0) {
      a0 += luma(r, g, bl);
    } else {
      a0 += r, a1 += g, a2 += bl;
    }
  }
  a0 = wave_sum(a0), a1 = wave_sum(a1), a2 = wave_sum(a2);
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) sm[0][wave] = a0, sm[1][wave] = a1, sm[2][wave] = a2;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t0 = 0, t1 = 0, t2 = 0;
    for (int w = 0; w < kStatsThreads / 64; ++w) t0 += sm[0][w], t1 += sm[1][w], t2 += sm[2][w];
    if (stage == 0) {
      atomicAdd(&st[frame], t0);
    } else {
      atomicAdd(&st[2], t0), atomicAdd(&st[3], t1), atomicAdd(&st[4], t2);
    }
  }
}

// OpenCV's INTER_LINEAR source coordinate of output index d on an axis of n source pixels, inv = 1 / scale (fp64)
__device__ __forceinline__ void linear_coord(int d, double inv, int n, int& i, float& a) {
  const float f = (float)(((double)d + 0.5) * inv - 0.5);
  const float fl = floorf(f);
  i = (int)fl;
  a = __fsub_rn(f, fl);
  if (i < 0) i = 0, a = 0.0f;
  if (i >= n - 1) i = n - 1, a = 0.0f;
}

__device__ __forceinline__ float lerp_rn(float s0, float s1, float a) {
  return __fadd_rn(__fmul_rn(s0, __fsub_rn(1.0f, a)), __fmul_rn(s1, a));
}

struct Rects {
  int n, x0[2], y0[2], x1[2], y1[2];
};

__device__ __forceinline__ bool erased(const Rects& rc, int x, int y) {
  bool e = false;
#pragma unroll
  for (int k = 0; k < 2; ++k) e = e || (k < rc.n && x >= rc.x0[k] && x < rc.x1[k] && y >= rc.y0[k] && y < rc.y1[k]);
  return e;
}

// where the output pixel (oy, ox) of sample b reads: the resized-frame position (before the flips are undone: what
// the sparse pass needs), the source taps and their weights
struct Geo {
  int rx, ry, ix, iy, ix1, iy1;
  float ax, ay;
  bool resize, hflip, vflip;
  double sx, sy;
};

__device__ __forceinline__ Geo geometry(const double* __restrict__ p, int H, int W, int oy, int ox) {
  Geo g;
  g.resize = p[P_RESIZE] != 0.0;
  g.hflip = p[P_HFLIP] != 0.0;
  g.vflip = p[P_VFLIP] != 0.0;
  g.sx = p[P_SX];
  g.sy = p[P_SY];
  const int ht1 = g.resize ? (int)rint((double)H * g.sy) : H;
  const int wd1 = g.resize ? (int)rint((double)W * g.sx) : W;
  const int cy = oy + (int)p[P_Y0], cx = ox + (int)p[P_X0];
  g.ry = g.vflip ? ht1 - 1 - cy : cy;
  g.rx = g.hflip ? wd1 - 1 - cx : cx;
  if (g.resize) {
    linear_coord(g.rx, 1.0 / g.sx, W, g.ix, g.ax);
    linear_coord(g.ry, 1.0 / g.sy, H, g.iy, g.ay);
  } else {
    g.ix = g.rx, g.iy = g.ry, g.ax = 0.0f, g.ay = 0.0f;
  }
  g.ix = min(max(g.ix, 0), W - 1);
  g.iy = min(max(g.iy, 0), H - 1);
  g.ix1 = min(g.ix + 1, W - 1);
  g.iy1 = min(g.iy + 1, H - 1);
  return g;
}

__device__ __forceinline__ void tap(const uint8_t* __restrict__ src, int W, int x, int y, const Jitter& j,
                                    const Rects& rc, bool erase, const int* fill, float* out) {
  if (erase && erased(rc, x, y)) {
    out[0] = (float)fill[0], out[1] = (float)fill[1], out[2] = (float)fill[2];
    return;
  }
  const uint8_t* q = src + ((long long)y * W + x) * 3;
  int r = q[0], g = q[1], b = q[2];
  jitter_pixel(j, false, r, g, b);
  out[0] = (float)r, out[1] = (float)g, out[2] = (float)b;
}

// one frame's output pixel: taps -> horizontal blend -> vertical blend -> round half-even, clamp
__device__ __forceinline__ void frame_pixel(const uint8_t* __restrict__ src, int W, const Geo& g, const Jitter& j,
                                            const Rects& rc, bool erase, const int* fill,
                                            float* __restrict__ out, long long plane, long long o) {
  float t00[3], t01[3], t10[3], t11[3];
  tap(src, W, g.ix, g.iy, j, rc, erase, fill, t00);
  const bool nx = g.ax != 0.0f, ny = g.ay != 0.0f;
  if (nx) tap(src, W, g.ix1, g.iy, j, rc, erase, fill, t01);
  if (ny) {
    tap(src, W, g.ix, g.iy1, j, rc, erase, fill, t10);
    if (nx) tap(src, W, g.ix1, g.iy1, j, rc, erase, fill, t11);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = t00[c];
    if (g.resize) {
      // (a zero weight's tap is not read: S0 * (1 - 0) + S1 * 0 == S0 for any finite S1)
      const float top = nx ? lerp_rn(t00[c], t01[c], g.ax) : t00[c];
      const float bot = ny ? (nx ? lerp_rn(t10[c], t11[c], g.ax) : t10[c]) : top;
      v = ny ? lerp_rn(top, bot, g.ay) : top;
      v = fminf(fmaxf(rintf(v), 0.0f), 255.0f);
    }
    out[c * plane + o] = v;
  }
}

__device__ __forceinline__ float flow_tap(const float* __restrict__ f, int W, const Geo& g) {
  const float v00 = f[(long long)g.iy * W + g.ix];
  if (!g.resize) return v00;
  const float top = lerp_rn(v00, f[(long long)g.iy * W + g.ix1], g.ax);
  const float bot = lerp_rn(f[(long long)g.iy1 * W + g.ix], f[(long long)g.iy1 * W + g.ix1], g.ax);
  return lerp_rn(top, bot, g.ay);
}

// grid (ceil(ch * cw / kThreads), B). flow == nullptr: images only (the sparse class)
__global__ __launch_bounds__(kThreads) void augment_dense_kernel(
    const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, const float* __restrict__ flow,
    const double* __restrict__ params, const unsigned long long* __restrict__ stats, int H, int W, int ch, int cw,
    float* __restrict__ out1, float* __restrict__ out2, float* __restrict__ oflow, float* __restrict__ ovalid) {
  const int b = blockIdx.y;
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= ch * cw) return;
  const long long HW = (long long)H * W, plane = (long long)ch * cw;
  const double* p = params + (long long)b * kP;
  const unsigned long long* st = stats + (long long)b * OFLOW_AUG_STATS_WORDS;
  const Geo g = geometry(p, H, W, o / cw, o % cw);
  const bool asym = p[P_ASYM] != 0.0;

  Jitter j1 = load_jitter(p, 0), j2 = load_jitter(p, 1);
  j1.dcontrast = contrast_level(st, asym, 0, HW);
  j2.dcontrast = contrast_level(st, asym, 1, HW);
  Rects rc;
  rc.n = min(max((int)p[P_NRECT], 0), 2);
  int fill[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // clipped at the frame edge, as a NumPy slice is
    const int x0 = (int)p[P_RECT + 4 * k], y0 = (int)p[P_RECT + 4 * k + 1];
    rc.x0[k] = x0, rc.y0[k] = y0;
    rc.x1[k] = x0 + (int)p[P_RECT + 4 * k + 2], rc.y1[k] = y0 + (int)p[P_RECT + 4 * k + 3];
  }
  if (rc.n > 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) fill[c] = (int)((double)st[2 + c] / (double)HW);
  }
  frame_pixel(img1 + (long long)b * HW * 3, W, g, j1, rc, false, fill, out1 + (long long)b * 3 * plane, plane, o);
  frame_pixel(img2 + (long long)b * HW * 3, W, g, j2, rc, rc.n > 0, fill, out2 + (long long)b * 3 * plane, plane, o);
  if (flow != nullptr) {
    const float* fl = flow + (long long)b * 2 * HW;
    float u = flow_tap(fl, W, g), v = flow_tap(fl + HW, W, g);
    // the reference's flow * [sx, sy] (and the flips' * [-1, 1]) promote to float64; one rounding back to fp32
    if (g.resize) u = (float)((double)u * g.sx), v = (float)((double)v * g.sy);
    if (g.hflip) u = -u;
    if (g.vflip) v = -v;
    oflow[(long long)b * 2 * plane + o] = u;
    oflow[(long long)b * 2 * plane + plane + o] = v;
    ovalid[(long long)b * plane + o] = (fabsf(u) < 1000.0f && fabsf(v) < 1000.0f) ? 1.0f : 0.0f;
  }
}

// sources x in [lo, hi] are the only ones whose (double)x * f can round (half-even) to t
__device__ __forceinline__ void source_window(int t, double f, int n, int& lo, int& hi) {
  lo = max((int)floor(((double)t - 0.5) / f) - 1, 0);
  hi = min((int)ceil(((double)t + 0.5) / f) + 1, n - 1);
}

// grid (ceil(ch * cw / kThreads), B): flow and valid of the sparse class
__global__ __launch_bounds__(kThreads) void augment_sparse_flow_kernel(const float* __restrict__ flow,
                                                                       const float* __restrict__ valid,
                                                                       const double* __restrict__ params, int H,
                                                                       int W, int ch, int cw,
                                                                       float* __restrict__ oflow,
                                                                       float* __restrict__ ovalid) {
  const int b = blockIdx.y;
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= ch * cw) return;
  const long long HW = (long long)H * W, plane = (long long)ch * cw;
  const double* p = params + (long long)b * kP;
  const Geo g = geometry(p, H, W, o / cw, o % cw);
  const float* fl = flow + (long long)b * 2 * HW;
  const float* va = valid + (long long)b * HW;
  float u = 0.0f, v = 0.0f, ok = 0.0f;
  if (!g.resize) {
    const long long s = (long long)g.iy * W + g.ix;
    u = fl[s], v = fl[HW + s], ok = va[s];
  } else {
    const int ht1 = (int)rint((double)H * g.sy), wd1 = (int)rint((double)W * g.sx);
    const int xx = g.rx, yy = g.ry;
    if (xx > 0 && xx < wd1 && yy > 0 && yy < ht1 && g.sx > 0.0 && g.sy > 0.0) {
      int xlo, xhi, ylo, yhi;
      source_window(xx, g.sx, W, xlo, xhi);
      source_window(yy, g.sy, H, ylo, yhi);
      bool found = false;
      for (int y = yhi; y >= ylo && !found; --y) {  // the last source in row-major order wins
        if ((int)rint((double)(float)y * g.sy) != yy) continue;
        for (int x = xhi; x >= xlo; --x) {
          if ((int)rint((double)(float)x * g.sx) != xx) continue;
          const long long s = (long long)y * W + x;
          if (va[s] >= 1.0f) {
            u = (float)((double)fl[s] * g.sx);
            v = (float)((double)fl[HW + s] * g.sy);
            ok = 1.0f;
            found = true;
            break;
          }
        }
      }
    }
  }
  if (g.hflip) u = -u;
  oflow[(long long)b * 2 * plane + o] = u;
  oflow[(long long)b * 2 * plane + plane + o] = v;
  ovalid[(long long)b * plane + o] = ok;
}

bool bad_shape(int B, int H, int W, int ch, int cw) {
  return B <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0 || B > 65535 || (long long)H * W > (1LL << 28) ||
         (long long)ch * cw > (1LL << 28);
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_augment_stats_u8(const unsigned char* d_img1, const unsigned char* d_img2, const double* d_params,
                                      int B, int H, int W, int stage, long long* d_stats, void* stream) {
  if (!d_img1 || !d_img2 || !d_params || !d_stats) return OFLOW_E_NULL;
  if (bad_shape(B, H, W, 1, 1) || (stage != 0 && stage != 1)) return OFLOW_E_SHAPE;
  const int HW = H * W;
  const int per_block = 8192;  // <= 2^16: 255 * 32 pixels per thread stays far inside uint32
  hipLaunchKernelGGL(augment_stats_kernel, dim3((HW + per_block - 1) / per_block, stage == 0 ? 2 : 1, B),
                     dim3(kStatsThreads), 0, static_cast<hipStream_t>(stream), d_img1, d_img2, d_params, HW, per_block,
                     stage, reinterpret_cast<unsigned long long*>(d_stats));
  return launch_status();
}

extern "C" int oflow_augment_dense_f32(const unsigned char* d_img1, const unsigned char* d_img2, const float* d_flow,
                                       const double* d_params, const long long* d_stats, int B, int H, int W,
                                       int crop_h, int crop_w, float* d_out1, float* d_out2, float* d_out_flow,
                                       float* d_out_valid, void* stream) {
  if (!d_img1 || !d_img2 || !d_params || !d_stats || !d_out1 || !d_out2) return OFLOW_E_NULL;
  if (d_flow && (!d_out_flow || !d_out_valid)) return OFLOW_E_NULL;
  if (bad_shape(B, H, W, crop_h, crop_w)) return OFLOW_E_SHAPE;
  hipLaunchKernelGGL(augment_dense_kernel, dim3((crop_h * crop_w + kThreads - 1) / kThreads, B), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), d_img1, d_img2, d_flow, d_params,
                     reinterpret_cast<const unsigned long long*>(d_stats), H, W, crop_h, crop_w, d_out1, d_out2,
                     d_out_flow, d_out_valid);
  return launch_status();
}

extern "C" int oflow_augment_sparse_flow_f32(const float* d_flow, const float* d_valid, const double* d_params, int B,
                                             int H, int W, int crop_h, int crop_w, float* d_out_flow,
                                             float* d_out_valid, void* stream) {
  if (!d_flow || !d_valid || !d_params || !d_out_flow || !d_out_valid) return OFLOW_E_NULL;
  if (bad_shape(B, H, W, crop_h, crop_w)) return OFLOW_E_SHAPE;
  hipLaunchKernelGGL(augment_sparse_flow_kernel, dim3((crop_h * crop_w + kThreads - 1) / kThreads, B), dim3(kThreads),
                     0, static_cast<hipStream_t>(stream), d_flow, d_valid, d_params, H, W, crop_h, crop_w, d_out_flow,
                     d_out_valid);
  return launch_status();
}
