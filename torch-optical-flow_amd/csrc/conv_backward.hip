// Backward of the update block's convolutions (gfx950): what a training step (raft.py:149-175) differentiates through
// update.py:31-161's nn.Conv2d layers. Stride 1, dilation 1, groups 1, odd kh, kw <= 7 with zero padding (kh/2, kw/2)
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
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kCT = 64;        // tile edge (channels; dgrad: pixels too)
constexpr int kCThreads = 256;
constexpr int kDK = 16;        // dgrad: output channels per K chunk
constexpr int kWK = 32;        // wgrad: pixels per K chunk
constexpr int kSlab = 2048;    // wgrad: flattened pixels per K slab
constexpr int kMaxPixels = 65535 * kSlab;  // grid.z of the wgrad launch: one slab each
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvGeom {
  int B, Cout, Cin, H, W, kh, kw;
};

__global__ __launch_bounds__(kCThreads) void conv_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ wt,
                                                               float* __restrict__ dx, ConvGeom g) {
  __shared__ float sA[2][kDK][kCT + 4];  // weights [k][c]
  __shared__ float sB[2][kDK][kCT + 4];  // shifted gy [k][p]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int HW = g.H * g.W, P = g.B * HW, T = g.kh * g.kw;
  const int p0 = blockIdx.x * kCT, c0 = blockIdx.y * kCT;
  // staging: element (tid & 63) of rows k = 4 * wave + e: one coalesced row of 64 pixels per wave and k
  const int sp = p0 + lane, sc = c0 + lane;
  const bool p_ok = sp < P, c_ok = sc < g.Cin;
  int sb = 0, sy = 0, sx = 0;
  if (p_ok) {
    sb = sp / HW;
    const int rem = sp - sb * HW;
    sy = rem / g.W;
    sx = rem - sy * g.W;
  }
  const int nch = (g.Cout + kDK - 1) / kDK;  // chunks per tap
  const int nk = T * nch;
  float ra[4], rb[4];
  auto load = [&](int kc) {
    const int tap = kc / nch, n0 = (kc - tap * nch) * kDK + 4 * wave;
    const int ky = tap / g.kw, kx = tap - ky * g.kw;
    const int yy = sy - (ky - g.kh / 2), xx = sx - (kx - g.kw / 2);
    const bool in = p_ok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
    const size_t gbase = ((size_t)sb * g.Cout * g.H + yy) * g.W + xx;  // (used only when in)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + e;
      const bool n_ok = n < g.Cout;
      ra[e] = (n_ok && c_ok) ? wt[((size_t)n * g.Cin + sc) * T + tap] : 0.f;
      rb[e] = (n_ok && in) ? gy[gbase + (size_t)n * HW] : 0.f;
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
  load(0);
  store(0);
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
  const int b = p / HW, rem = p - b * HW;
  float* out = dx + (size_t)b * g.Cin * HW + rem;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = c0 + wm * 32 + 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2);
    if (c < g.Cin) out[(size_t)c * HW] = acc[e];
  }
}

__global__ __launch_bounds__(kCThreads) void conv_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ xin,
                                                               float* __restrict__ ws, ConvGeom g, int tiles_c) {
  __shared__ float sA[2][kWK][kCT + 1];  // gy [p][n]
  __shared__ float sB[2][kWK][kCT + 1];  // shifted x [p][c]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int HW = g.H * g.W, P = g.B * HW, T = g.kh * g.kw;
  const int n0 = (blockIdx.x / tiles_c) * kCT, c0 = (blockIdx.x % tiles_c) * kCT;
  const int tap = blockIdx.y, slab = blockIdx.z;
  const int oy = tap / g.kw - g.kh / 2, ox = tap % g.kw - g.kw / 2;
  const int s0 = slab * kSlab, s1 = min(s0 + kSlab, P);
  // staging: pixel (tid & 31) of the chunk, rows (tid >> 5) + 8 i: two coalesced 32-pixel rows per wave and i
  const int pl = tid & 31, r0 = tid >> 5;
  float ra[8], rb[8];
  auto load = [&](int pc) {
    const int p = pc + pl;
    const bool p_ok = p < s1;
    int b = 0, y = 0, x = 0;
    if (p_ok) {
      b = p / HW;
      const int rem = p - b * HW;
      y = rem / g.W;
      x = rem - y * g.W;
    }
    const int yy = y + oy, xx = x + ox;
    const bool in = p_ok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
    const size_t abase = (size_t)b * g.Cout * HW + (size_t)y * g.W + x;
    const size_t bbase = ((size_t)b * g.Cin * g.H + yy) * g.W + xx;  // (used only when in)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 8 * i;
      ra[i] = (p_ok && n0 + r < g.Cout) ? gy[abase + (size_t)(n0 + r) * HW] : 0.f;
      rb[i] = (in && c0 + r < g.Cin) ? xin[bbase + (size_t)(c0 + r) * HW] : 0.f;
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
  if (c >= g.Cin) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int n = n0 + wm * 32 + 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2);
    if (n < g.Cout) out[((size_t)n * g.Cin + c) * T + tap] = acc[e];
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

// sizes inside the kernels' index range: int pixel and weight indices, grid dimensions
bool geom_ok(int B, int Cout, int Cin, int H, int W, int kh, int kw) {
  if (B <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0) return false;
  if (kh < 1 || kw < 1 || kh > 7 || kw > 7 || !(kh & 1) || !(kw & 1)) return false;
  if (Cout > 65535 || Cin > 65535) return false;
  if ((long long)B * H * W > kMaxPixels) return false;
  if ((long long)Cout * Cin * kh * kw >= (1ll << 31)) return false;
  return true;
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_conv2d_backward_input_f32(const float* d_grad_out, const float* d_weight, int B, int Cout, int Cin,
                                               int H, int W, int kh, int kw, float* d_grad_input, void* stream) {
  if (!d_grad_out || !d_weight || !d_grad_input) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw)) return OFLOW_E_SHAPE;
  const ConvGeom g{B, Cout, Cin, H, W, kh, kw};
  const int P = B * H * W;
  const dim3 grid((P + kCT - 1) / kCT, (Cin + kCT - 1) / kCT);
  hipLaunchKernelGGL(conv_dgrad_kernel, grid, dim3(kCThreads), 0, static_cast<hipStream_t>(stream), d_grad_out, d_weight,
                     d_grad_input, g);
  return launch_status();
}

extern "C" long long oflow_conv2d_backward_weight_workspace_floats(int B, int Cout, int Cin, int H, int W, int kh, int kw) {
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw)) return 0;
  const long long slabs = ((long long)B * H * W + kSlab - 1) / kSlab;
  return slabs * ((long long)Cout * Cin * kh * kw + Cout);
}

extern "C" int oflow_conv2d_backward_weight_slab_pixels(void) { return kSlab; }

extern "C" int oflow_conv2d_backward_weight_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin, int H,
                                                int W, int kh, int kw, float* d_grad_weight, float* d_grad_bias,
                                                float* d_workspace, void* stream) {
  if (!d_grad_out || !d_workspace || (!d_grad_weight && !d_grad_bias) || (d_grad_weight && !d_x)) return OFLOW_E_NULL;
  if (!geom_ok(B, Cout, Cin, H, W, kh, kw)) return OFLOW_E_SHAPE;
  const ConvGeom g{B, Cout, Cin, H, W, kh, kw};
  const int HW = H * W, P = B * HW, T = kh * kw;
  const int slabs = (P + kSlab - 1) / kSlab;  // <= 65535 (geom_ok)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int wcount = Cout * Cin * T;
  if (d_grad_weight) {
    const int tiles_n = (Cout + kCT - 1) / kCT, tiles_c = (Cin + kCT - 1) / kCT;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3(tiles_n * tiles_c, T, slabs), dim3(kCThreads), 0, st, d_grad_out, d_x,
                       d_workspace, g, tiles_c);
    hipLaunchKernelGGL(conv_slab_reduce_kernel, dim3((wcount + kCThreads - 1) / kCThreads), dim3(kCThreads), 0, st,
                       d_workspace, d_grad_weight, wcount, slabs);
  }
  if (d_grad_bias) {
    float* wb = d_workspace + (size_t)slabs * wcount;
    hipLaunchKernelGGL(conv_bias_slab_kernel, dim3(Cout, slabs), dim3(kCThreads), 0, st, d_grad_out, wb, Cout, HW, P);
    hipLaunchKernelGGL(conv_slab_reduce_kernel, dim3((Cout + kCThreads - 1) / kCThreads), dim3(kCThreads), 0, st, wb,
                       d_grad_bias, Cout, slabs);
  }
  return launch_status();
}
