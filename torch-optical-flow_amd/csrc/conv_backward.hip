// Backward of the model's convolutions (gfx950): what a training step (raft.py:149-175) differentiates through the
// nn.Conv2d layers of update.py:31-161 (stride 1) and of the encoders (extractor.py, stride 1 and 2). Stride 1 first: dilation 1, groups 1, odd kh, kw <= 7 with zero padding (kh/2, kw/2)
// ("same"), fp32 NCHW. With oy = ky - kh/2, ox = kx - kw/2 and out-of-image terms zero:
//   dx[b, c, y, x]   = sum_{ky, kx, n} gy[b, n, y - oy, x - ox] * w[n, c, ky, kx]       (input gradient, gather form)
//   dw[n, c, ky, kx] = sum_{b, y, x}   gy[b, n, y, x] * x[b, c, y + oy, x + ox]         (weight gradient)
//   db[n]            = sum_{b, y, x}   gy[b, n, y, x]                                    (bias gradient)
// All products run on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chains in a fixed k order), not on
// the forward's split-fp16 scheme: gradients of a mean-reduced loss sit below fp16's normal range.
//
// dgrad is a GEMM D[c][p] = sum_k Wt[c][k] G[k][p] over the flattened pixels p of the whole batch (a tile may span two
// images), k = (tap, n) with taps outermost. Workgroup tile 64 c x 64 p, 4 waves as 2 x 2 of 32 x 32; K in chunks of
// 16 output channels of one tap through LDS as [k][c] / [k][p]; the shifted gy rows load coalesced straight from NCHW
// (lanes along pixels), the weights with stride kh*kw (they are small and stay in cache). Pixels are the accumulator's
// lane dimension, so the stores are coalesced rows of dx. Every output element is owned by one accumulator: no atomics.
//
// wgrad is, per tap, a GEMM D[n][c] = sum_p G[n][p] X_tap[c][p] whose K (the pixel count) is huge and whose M x N is
// small: K is split into fixed slabs of kSlab flattened pixels; workgroup (n tile, c tile) x tap x slab runs a 64 x 64
// tile over its slab in chunks of 32 pixels (both operands have pixels along K: loaded with lanes along pixels,
// transposed through LDS) and writes its partial to workspace[slab][n][c][tap]; conv_slab_reduce_kernel sums the slabs
// in ascending order. The bias gradient takes the same route (a fixed-order block sum per (n, slab)). No atomics: the
// result is bit-reproducible for a given shape. Ragged channel / pixel edges stage zeros.
//
// Stride s = 2 (output H' = (H + 1) / 2, W' = (W + 1) / 2; py = kh / 2, px = kw / 2):
//   dx[b, c, y, x]   = sum gy[b, n, Y, X] * w[n, c, ky, kx] over (ky, kx, n) with 2Y = y + py - ky, 2X = x + px - kx
//   dw[n, c, ky, kx] = sum_{b, Y, X} gy[b, n, Y, X] * x[b, c, 2Y + ky - py, 2X + kx - px]
// dgrad: an input pixel only meets the taps with ky = (y + py) mod 2, kx = (x + px) mod 2. blockIdx.z is that parity
// class; a workgroup's 64 pixels are flattened over the class's pixels (y = y0 + 2i, x = x0 + 2j) and its K loop runs
// over the class's taps only (ascending ky, kx), so no K step is spent on an absent tap. A class without taps (three of
// the four under a 1x1 kernel) stores zeros. With s = 1 there is one class holding every pixel and every tap: the
// stride-1 kernel, the same bits. wgrad: the slabs are 2048 flattened OUTPUT pixels and x is read at stride s.
// wgrad with Cin <= 4 (the 3 -> 64 7x7 stem): the tile's column dimension is (c, tap) folded, Cin * kh * kw columns in
// tiles of 64 (147 = 3 tiles for the stem) instead of one launch slice per tap with Cin of 64 columns filled.
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kCT = 64;        // tile edge (channels; dgrad: pixels too)
constexpr int kCThreads = 256;
constexpr int kDK = 16;        // dgrad: output channels per K chunk
constexpr int kWK = 32;        // wgrad: pixels per K chunk
constexpr int kSlab = 2048;    // wgrad: flattened (output) pixels per K slab
constexpr int kMaxPixels = 65535 * kSlab;  // grid.z of the wgrad launch: one slab each
constexpr int kFoldMaxCin = 4;  // strided entry points: wgrad folds (c, tap) into the columns up to this Cin
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvGeom {
  int B, Cout, Cin, H, W, kh, kw;
  int s, Ho, Wo;  // stride and output size (s = 1: Ho = H, Wo = W)
};

__global__ __launch_bounds__(kCThreads) void conv_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ wt,
                                                               float* __restrict__ dx, ConvGeom g) {
  __shared__ float sA[2][kDK][kCT + 4];  // weights [k][c]
  __shared__ float sB[2][kDK][kCT + 4];  // shifted gy [k][p]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int py = g.kh / 2, px = g.kw / 2;
  // parity class (s = 2): qy = (y + py) & 1 picks the taps ky = qy, qy + 2, ...; its pixels are y = y0 + 2i
  const int qy = g.s == 2 ? (int)(blockIdx.z >> 1) : 0, qx = g.s == 2 ? (int)(blockIdx.z & 1) : 0;
  const int y0 = (qy + py) & (g.s - 1), x0 = (qx + px) & (g.s - 1);
  const int Hc = (g.H - y0 + g.s - 1) / g.s, Wc = (g.W - x0 + g.s - 1) / g.s;  // the class's pixel grid
  const int nty = g.s == 2 ? (g.kh - qy + 1) / 2 : g.kh, ntx = g.s == 2 ? (g.kw - qx + 1) / 2 : g.kw;
  const int HWc = Hc * Wc, P = g.B * HWc, T = g.kh * g.kw;
  const int HWo = g.Ho * g.Wo;
  const int p0 = blockIdx.x * kCT, c0 = blockIdx.y * kCT;
  if (p0 >= P) return;  // (the grid is sized for the largest class)
  // staging: element (tid & 63) of rows k = 4 * wave + e: one coalesced row of 64 pixels per wave and k
  const int sp = p0 + lane, sc = c0 + lane;
  const bool p_ok = sp < P, c_ok = sc < g.Cin;
  int sb = 0, sy = 0, sx = 0;
  if (p_ok) {
    sb = sp / HWc;
    const int rem = sp - sb * HWc;
    const int i = rem / Wc;
    sy = y0 + g.s * i;
    sx = x0 + g.s * (rem - i * Wc);
  }
  const int nch = (g.Cout + kDK - 1) / kDK;  // chunks per tap
  const int nk = nty * ntx * nch;
  float ra[4], rb[4];
  auto load = [&](int kc) {
    const int tc = kc / nch, n0 = (kc - tc * nch) * kDK + 4 * wave;
    const int ta = tc / ntx;
    const int ky = qy + g.s * ta, kx = qx + g.s * (tc - ta * ntx);
    const int tap = ky * g.kw + kx;
    const int yy = sy - (ky - py), xx = sx - (kx - px);  // s * Y, s * X (even for s = 2 by the class's choice of taps)
    const int Y = yy / g.s, X = xx / g.s;
    const bool in = p_ok && yy >= 0 && Y < g.Ho && xx >= 0 && X < g.Wo;
    const size_t gbase = ((size_t)sb * g.Cout * g.Ho + Y) * g.Wo + X;  // (used only when in)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + e;
      const bool n_ok = n < g.Cout;
      ra[e] = (n_ok && c_ok) ? wt[((size_t)n * g.Cin + sc) * T + tap] : 0.f;
      rb[e] = (n_ok && in) ? gy[gbase + (size_t)n * HWo] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sA[buf][4 * wave + e][lane] = ra[e];
      sB[buf][4 * wave + e][lane] = rb[e];
    }
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  if (nk > 0) {  // (a class without taps keeps its zeros)
    load(0);
    store(0);
  }
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) load(kc + 1);
#pragma unroll
    for (int kk = 0; kk < kDK; kk += 2) {
      const float av = sA[buf][kk + (lane >> 5)][wm * 32 + (lane & 31)];
      const float bv = sB[buf][kk + (lane >> 5)][wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (kc + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  // C/D map: acc[e] <-> row c = 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2), column p = lane & 31
  const int p = p0 + wn * 32 + (lane & 31);
  if (p >= P) return;
  const int b = p / HWc, rem = p - b * HWc;
  const int i = rem / Wc;
  const int HW = g.H * g.W;
  float* out = dx + (size_t)b * g.Cin * HW + (size_t)(y0 + g.s * i) * g.W + (x0 + g.s * (rem - i * Wc));
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = c0 + wm * 32 + 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2);
    if (c < g.Cin) out[(size_t)c * HW] = acc[e];
  }
}

// FOLD: the columns are (c, tap) pairs, column j = c * T + tap (the weight's own layout), blockIdx.y is 0
template <bool FOLD>
__global__ __launch_bounds__(kCThreads) void conv_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ xin,
                                                               float* __restrict__ ws, ConvGeom g, int tiles_c) {
  __shared__ float sA[2][kWK][kCT + 1];  // gy [p][n]
  __shared__ float sB[2][kWK][kCT + 1];  // shifted x [p][c]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int HWo = g.Ho * g.Wo, P = g.B * HWo, T = g.kh * g.kw;
  const int n0 = (blockIdx.x / tiles_c) * kCT, c0 = (blockIdx.x % tiles_c) * kCT;
  const int tap = FOLD ? 0 : blockIdx.y, slab = blockIdx.z;
  const int ncols = FOLD ? g.Cin * T : g.Cin;
  const int s0 = slab * kSlab, s1 = min(s0 + kSlab, P);
  // staging: pixel (tid & 31) of the chunk, rows (tid >> 5) + 8 i: two coalesced 32-pixel rows per wave and i
  const int pl = tid & 31, r0 = tid >> 5;
  int rc[8], roy[8], rox[8];  // per staged column: input channel and tap offset (FOLD: its own; else the block's)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = c0 + r0 + 8 * i;
    const int c = FOLD ? col / T : col, t = FOLD ? col - c * T : tap;
    rc[i] = col < ncols ? c : -1;
    roy[i] = t / g.kw - g.kh / 2;
    rox[i] = t % g.kw - g.kw / 2;
  }
  float ra[8], rb[8];
  auto load = [&](int pc) {
    const int p = pc + pl;
    const bool p_ok = p < s1;
    int b = 0, y = 0, x = 0;
    if (p_ok) {
      b = p / HWo;
      const int rem = p - b * HWo;
      y = rem / g.Wo;
      x = rem - y * g.Wo;
    }
    const size_t abase = (size_t)b * g.Cout * HWo + (size_t)y * g.Wo + x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 8 * i;
      const int yy = g.s * y + roy[i], xx = g.s * x + rox[i];
      const bool in = p_ok && rc[i] >= 0 && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
      ra[i] = (p_ok && n0 + r < g.Cout) ? gy[abase + (size_t)(n0 + r) * HWo] : 0.f;
      rb[i] = in ? xin[(((size_t)b * g.Cin + rc[i]) * g.H + yy) * g.W + xx] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sA[buf][pl][r0 + 8 * i] = ra[i];
      sB[buf][pl][r0 + 8 * i] = rb[i];
    }
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int nk = (s1 - s0 + kWK - 1) / kWK;
  load(s0);
  store(0);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) load(s0 + (kc + 1) * kWK);
#pragma unroll
    for (int kk = 0; kk < kWK; kk += 2) {
      const float av = sA[buf][kk + (lane >> 5)][wm * 32 + (lane & 31)];
      const float bv = sB[buf][kk + (lane >> 5)][wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (kc + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  // acc[e] <-> row n = 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2), column c = lane & 31
  float* out = ws + (size_t)slab * g.Cout * g.Cin * T;
  const int c = c0 + wn * 32 + (lane & 31);
  if (c >= ncols) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int n = n0 + wm * 32 + 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2);
    if (n < g.Cout) out[FOLD ? (size_t)n * ncols + c : ((size_t)n * g.Cin + c) * T + tap] = acc[e];
  }
}

// ws[slab][n] = sum of gy[b, n, pixel] over the slab's pixels: each thread adds its pixels in ascending order, then a
// fixed LDS tree folds the 256 partial sums
__global__ __launch_bounds__(kCThreads) void conv_bias_slab_kernel(const float* __restrict__ gy, float* __restrict__ ws,
                                                                   int Cout, int HW, int P) {
  __shared__ float sS[kCThreads];
  const int n = blockIdx.x, slab = blockIdx.y, tid = threadIdx.x;
  const int s0 = slab * kSlab, s1 = min(s0 + kSlab, P);
  float s = 0.f;
  for (int p = s0 + tid; p < s1; p += kCThreads) {
    const int b = p / HW, rem = p - b * HW;
    s += gy[((size_t)b * Cout + n) * HW + rem];
  }
  sS[tid] = s;
  __syncthreads();
  for (int w = kCThreads / 2; w > 0; w >>= 1) {
    if (tid < w) sS[tid] += sS[tid + w];
    __syncthreads();
  }
  if (tid == 0) ws[(size_t)slab * Cout + n] = sS[0];
}

// out[i] = ws[0][i] + ws[1][i] + ... in ascending slab order
__global__ __launch_bounds__(kCThreads) void conv_slab_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                     int count, int slabs) {
  const int i = blockIdx.x * kCThreads + threadIdx.x;
  if (i >= count) return;
  float s = ws[i];
  for (int k = 1; k < slabs; ++k) s += ws[(size_t)k * count + i];
  out[i] = s;
}

// sizes inside the kernels' index range: int pixel and weight indices, grid dimensions (the pixel limit is on the
// output pixels, which the wgrad slabs run over; the input pixels, at most four times as many, stay below 2^31)
bool geom_ok(int B, int Cout, int Cin, int H, int W, int kh, int kw, int s) {
  if (B <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0) return false;
  if (kh < 1 || kw < 1 || kh > 7 || kw > 7 || !(kh & 1) || !(kw & 1)) return false;
  if (s != 1 && s != 2) return false;
  if (Cout > 65535 || Cin > 65535) return false;
  if ((long long)B * ((H + s - 1) / s) * ((W + s - 1) / s) > kMaxPixels) return false;
  if ((long long)B * H * W >= (1ll << 31)) return false;
  if ((long long)Cout * Cin * kh * kw >= (1ll << 31)) return false;
  return true;
}

ConvGeom geom(int B, int Cout, int Cin, int H, int W, int kh, int kw, int s) {
  return ConvGeom{B, Cout, Cin, H, W, kh, kw, s, (H + s - 1) / s, (W + s - 1) / s};
}

int dgrad(const float* gy, const float* wt, const ConvGeom& g, float* dx, void* stream) {
  const int Pc = g.B * g.Ho * g.Wo;  // the largest parity class (y0 = x0 = 0) has the output's pixel count
  const dim3 grid((Pc + kCT - 1) / kCT, (g.Cin + kCT - 1) / kCT, g.s * g.s);
  hipLaunchKernelGGL(conv_dgrad_kernel, grid, dim3(kCThreads), 0, static_cast<hipStream_t>(stream), gy, wt, dx, g);
  return launch_status();
}

int wgrad(const float* gy, const float* x, const ConvGeom& g, bool fold, float* dw, float* db, float* ws, void* stream) {
  const int HWo = g.Ho * g.Wo, P = g.B * HWo, T = g.kh * g.kw;
  const int slabs = (P + kSlab - 1) / kSlab;  // <= 65535 (geom_ok)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int wcount = g.Cout * g.Cin * T;
  if (dw) {
    const int tiles_n = (g.Cout + kCT - 1) / kCT;
    if (fold) {
      const int tiles_c = (g.Cin * T + kCT - 1) / kCT;
      hipLaunchKernelGGL(conv_wgrad_kernel<true>, dim3(tiles_n * tiles_c, 1, slabs), dim3(kCThreads), 0, st, gy, x, ws, g,
                         tiles_c);
    } else {
      const int tiles_c = (g.Cin + kCT - 1) / kCT;
      hipLaunchKernelGGL(conv_wgrad_kernel<false>, dim3(tiles_n * tiles_c, T, slabs), dim3(kCThreads), 0, st, gy, x, ws, g,
                         tiles_c);
    }
    hipLaunchKernelGGL(conv_slab_reduce_kernel, dim3((wcount + kCThreads - 1) / kCThreads), dim3(kCThreads), 0, st, ws, dw,
                       wcount, slabs);
  }
  if (db) {
    float* wb = ws + (size_t)slabs * wcount;
    hipLaunchKernelGGL(conv_bias_slab_kernel, dim3(g.Cout, slabs), dim3(kCThreads), 0, st, gy, wb, g.Cout, HWo, P);
    hipLaunchKernelGGL(conv_slab_reduce_kernel, dim3((g.Cout + kCThreads - 1) / kCThreads), dim3(kCThreads), 0, st, wb, db,
                       g.Cout, slabs);
  }
  return launch_status();
}

long long workspace_floats(int B, int Cout, int Cin, int H, int W, int kh, int kw, int s) {
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, s)) return 0;
  const long long slabs = ((long long)B * ((H + s - 1) / s) * ((W + s - 1) / s) + kSlab - 1) / kSlab;
  return slabs * ((long long)Cout * Cin * kh * kw + Cout);
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_conv2d_backward_input_f32(const float* d_grad_out, const float* d_weight, int B, int Cout, int Cin,
                                               int H, int W, int kh, int kw, float* d_grad_input, void* stream) {
  if (!d_grad_out || !d_weight || !d_grad_input) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, 1)) return OFLOW_E_SHAPE;
  return dgrad(d_grad_out, d_weight, geom(B, Cout, Cin, H, W, kh, kw, 1), d_grad_input, stream);
}

extern "C" long long oflow_conv2d_backward_weight_workspace_floats(int B, int Cout, int Cin, int H, int W, int kh, int kw) {
  return workspace_floats(B, Cout, Cin, H, W, kh, kw, 1);
}

extern "C" int oflow_conv2d_backward_weight_slab_pixels(void) { return kSlab; }

extern "C" int oflow_conv2d_backward_weight_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin, int H,
                                                int W, int kh, int kw, float* d_grad_weight, float* d_grad_bias,
                                                float* d_workspace, void* stream) {
  if (!d_grad_out || !d_workspace || (!d_grad_weight && !d_grad_bias) || (d_grad_weight && !d_x)) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, 1)) return OFLOW_E_SHAPE;
  return wgrad(d_grad_out, d_x, geom(B, Cout, Cin, H, W, kh, kw, 1), false, d_grad_weight, d_grad_bias, d_workspace, stream);
}

// ---- stride 1 or 2 (the encoders' convolutions); H, W are the input's, grad_out is (B, Cout, (H+s-1)/s, (W+s-1)/s)
extern "C" int oflow_conv2d_strided_backward_input_f32(const float* d_grad_out, const float* d_weight, int B, int Cout,
                                                       int Cin, int H, int W, int kh, int kw, int stride,
                                                       float* d_grad_input, void* stream) {
  if (!d_grad_out || !d_weight || !d_grad_input) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, stride)) return OFLOW_E_SHAPE;
  return dgrad(d_grad_out, d_weight, geom(B, Cout, Cin, H, W, kh, kw, stride), d_grad_input, stream);
}

extern "C" long long oflow_conv2d_strided_backward_weight_workspace_floats(int B, int Cout, int Cin, int H, int W, int kh,
                                                                           int kw, int stride) {
  return workspace_floats(B, Cout, Cin, H, W, kh, kw, stride);
}

extern "C" int oflow_conv2d_strided_backward_weight_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin,
                                                        int H, int W, int kh, int kw, int stride, float* d_grad_weight,
                                                        float* d_grad_bias, float* d_workspace, void* stream) {
  if (!d_grad_out || !d_workspace || (!d_grad_weight && !d_grad_bias) || (d_grad_weight && !d_x)) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, stride)) return OFLOW_E_SHAPE;
  return wgrad(d_grad_out, d_x, geom(B, Cout, Cin, H, W, kh, kw, stride), Cin <= kFoldMaxCin, d_grad_weight, d_grad_bias,
               d_workspace, stream);
}

// test / benchmark hook: the strided weight gradient on the generic per-tap path whatever Cin is (what the folded
// Cin <= 4 path is compared with); otherwise oflow_conv2d_strided_backward_weight_f32
extern "C" int oflow_conv2d_strided_backward_weight_generic_f32(const float* d_grad_out, const float* d_x, int B, int Cout,
                                                                int Cin, int H, int W, int kh, int kw, int stride,
                                                                float* d_grad_weight, float* d_grad_bias,
                                                                float* d_workspace, void* stream) {
  if (!d_grad_out || !d_workspace || (!d_grad_weight && !d_grad_bias) || (d_grad_weight && !d_x)) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw, stride)) return OFLOW_E_SHAPE;
  return wgrad(d_grad_out, d_x, geom(B, Cout, Cin, H, W, kh, kw, stride), false, d_grad_weight, d_grad_bias, d_workspace,
               stream);
}
