// splat (gfx950): forward warping of a frame along a flow in pixel units -- summation, average, linear and softmax
// splatting (Niklaus and Liu, CVPR 2020) -- with sums that do not depend on arrival order. include/oflow.h states the
// contract; csrc/splat_backward.hip is the gradient.
//
// A scatter with float atomics gives last bits that change from run to run (csrc/warp_backward.hip's frame gradient is
// that scatter). Here every contribution is turned into a 64-bit fixed-point integer and added with an integer atomic:
// integer addition is associative, so the sum is the same whatever order the adds arrive in. atomicAdd(unsigned long
// long*) with the result unused compiles to one no-return global_atomic_add_x2 (no compare-and-swap loop).
//
// Four steps on the stream, nothing returns to the host:
//   0. hipMemsetAsync zeroes the workspace (accumulators and the per-image words).
//   1. splat_range_kernel: per image, max |frame| and the metric's maximum (SOFT) or max |metric| (LINEAR), block
//      reductions finished with integer atomicMax on the value's bit pattern (order-independent as well);
//      splat_exponent_kernel then writes the image's two binary exponents eN, eD. Per-image scales are what make an
//      image's bits independent of the rest of its batch.
//   2. splat_scatter_kernel: one thread per source pixel. It forms the landing position, the four fp64 tap weights and
//      m once, adds the four D contributions, then loops over the channels.
//   3. splat_finish_kernel: a streaming pass, int64 -> fp64 value, normalise, write out and D in fp32.
//
// Overflow: a target receives at most 4 * H * W contributions (in fact at most one tap of every source), each at most
// 2^K in magnitude after scaling (|w m f| <= 2^eN by the choice of eN), and K = 62 - ceil(log2(4 * H * W))
// (oflow_splat_frac_bits: 38 at the largest frame, H * W = 2^22), so |sum| <= 4 * H * W * 2^K <= 2^62 < 2^63.
//
// Accumulator layout: planar, (B, C + 1, H, W) int64 with the D plane last. Under a smooth flow the 64 lanes of a wave
// are 64 neighbouring sources of a row and land on 64 neighbouring targets, so each atomic wave-instruction of a tap
// covers one contiguous 512-byte run of a plane (two where the run crosses a row end): the contiguous shape the float
// atomics want. Interleaving the channels per pixel would put the lanes (C + 1) * 8 bytes apart. Only the planar layout
// was built and timed (DESIGN.md §4 "splat").
#include "splat_common.h"

namespace oflow {
namespace {

constexpr int kThreads = kSplatThreads;

// a scaled contribution as an integer; anything that is not a finite number below 2^62 (a non-finite frame or metric
// value: unspecified output) adds nothing, so no conversion is ever out of range
__device__ __forceinline__ long long quantise(double v) {
  return fabs(v) < 4611686018427387904.0 ? __double2ll_rn(v) : 0LL;
}

__device__ __forceinline__ void add_fixed(long long* p, long long q) {
  if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(q));
}

struct ScatterArgs {
  const float* frame;
  const float* flow;
  const float* metric;
  long long* acc;       // (B, C + 1, HW)
  const unsigned* hdr;  // (B, kHdrWords)
  int C, H, W, mode, frac;
};

__global__ __launch_bounds__(kThreads) void splat_scatter_kernel(ScatterArgs a) {
  const int H = a.H, W = a.W, C = a.C;
  const int HW = H * W;
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= HW) return;
  const int b = blockIdx.y;
  const int i = s / W, j = s - i * W;
  const float* fl = a.flow + 2LL * b * HW;
  const float px = static_cast<float>(j) + fl[s], py = static_cast<float>(i) + fl[HW + s];
  // before any float-to-int conversion; false for NaN
  if (!(px > -1.f && px < static_cast<float>(W) && py > -1.f && py < static_cast<float>(H))) return;
  const float x0f = floorf(px), y0f = floorf(py);
  // in fp64, where the difference is exact (in fp32 it is not for -1 < px < 0)
  const double fx = static_cast<double>(px) - static_cast<double>(x0f), fy = static_cast<double>(py) - static_cast<double>(y0f);
  const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);  // in [-1, W - 1], [-1, H - 1]

  const unsigned* h = a.hdr + b * kHdrWords;
  float m = 1.f;
  if (a.mode == OFLOW_SPLAT_LINEAR) m = a.metric[static_cast<long long>(b) * HW + s];
  if (a.mode == OFLOW_SPLAT_SOFT) m = expf(a.metric[static_cast<long long>(b) * HW + s] - __uint_as_float(h[1]));
  const double scale_n = ldexp(1.0, a.frac - static_cast<int>(h[2]));
  const double scale_d = ldexp(1.0, a.frac - static_cast<int>(h[3]));

  const double ax[2] = {1.0 - fx, fx};
  const double ay[2] = {1.0 - fy, fy};
  double wm[4];  // w * m per tap
  int at[4];     // target index, -1 = dropped
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + (t & 1), y = y0 + (t >> 1);
    at[t] = (x >= 0 && x < W && y >= 0 && y < H) ? y * W + x : -1;
    wm[t] = (ax[t & 1] * ay[t >> 1]) * static_cast<double>(m);
  }
  long long* plane = a.acc + (static_cast<long long>(b) * (C + 1) + C) * HW;  // D
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (at[t] >= 0) add_fixed(plane + at[t], quantise(wm[t] * scale_d));
  const float* fr = a.frame + static_cast<long long>(b) * C * HW + s;
  plane = a.acc + static_cast<long long>(b) * (C + 1) * HW;
  for (int c = 0; c < C; ++c, fr += HW, plane += HW) {
    const double f = static_cast<double>(*fr);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (at[t] >= 0) add_fixed(plane + at[t], quantise((wm[t] * f) * scale_n));
  }
}

struct FinishArgs {
  const long long* acc;
  const unsigned* hdr;
  float* out;
  float* weight;
  int C, HW, mode, frac;
};

__global__ __launch_bounds__(kThreads) void splat_finish_kernel(FinishArgs a) {
  const int HW = a.HW, C = a.C;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= HW) return;
  const int b = blockIdx.y;
  const unsigned* h = a.hdr + b * kHdrWords;
  const double quantum_n = ldexp(1.0, static_cast<int>(h[2]) - a.frac);
  const double quantum_d = ldexp(1.0, static_cast<int>(h[3]) - a.frac);
  const long long* acc = a.acc + static_cast<long long>(b) * (C + 1) * HW + t;
  const double d = static_cast<double>(acc[static_cast<long long>(C) * HW]) * quantum_d;
  a.weight[static_cast<long long>(b) * HW + t] = static_cast<float>(d);
  const double den = d + OFLOW_SPLAT_EPS;
  float* out = a.out + static_cast<long long>(b) * C * HW + t;
  for (int c = 0; c < C; ++c, acc += HW, out += HW) {
    const double n = static_cast<double>(*acc) * quantum_n;
    *out = static_cast<float>(a.mode == OFLOW_SPLAT_SUM ? n : n / den);
  }
}

}  // namespace

// the argument checks the forward and the backward share; OFLOW_OK or the first error
int splat_check_shape(int B, int C, int H, int W, int mode) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || B > 65535 || static_cast<long long>(H) * W > OFLOW_SPLAT_MAX_PIXELS)
    return OFLOW_E_SHAPE;
  if (mode < OFLOW_SPLAT_SUM || mode > OFLOW_SPLAT_SOFT) return OFLOW_E_MODE;
  return OFLOW_OK;
}

}  // namespace oflow

using namespace oflow;

extern "C" int oflow_splat_frac_bits(int H, int W) {
  if (H < 1 || W < 1 || static_cast<long long>(H) * W > OFLOW_SPLAT_MAX_PIXELS) return 0;
  int bits = 0;  // ceil(log2(4 * H * W))
  while ((1LL << bits) < 4LL * H * W) ++bits;
  return 62 - bits;
}

extern "C" long long oflow_splat_workspace_bytes(int B, int C, int H, int W) {
  if (splat_check_shape(B, C, H, W, OFLOW_SPLAT_SUM) != OFLOW_OK) return 0;
  return splat_acc_bytes(B, C, H, W) + 4LL * kHdrWords * B;
}

extern "C" int oflow_splat_f32(const float* d_frame, const float* d_flow, const float* d_metric, int B, int C, int H,
                               int W, int mode, float* d_out, float* d_weight, void* d_workspace, void* stream) {
  if (!d_frame || !d_flow || !d_out || !d_weight || !d_workspace) return OFLOW_E_NULL;
  const int st = splat_check_shape(B, C, H, W, mode);
  if (st != OFLOW_OK) return st;
  const bool metric_mode = mode == OFLOW_SPLAT_LINEAR || mode == OFLOW_SPLAT_SOFT;
  if (metric_mode && !d_metric) return OFLOW_E_NULL;
  if (!metric_mode && d_metric) return OFLOW_E_MODE;
  if ((reinterpret_cast<uintptr_t>(d_frame) | reinterpret_cast<uintptr_t>(d_flow) | reinterpret_cast<uintptr_t>(d_metric) |
       reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_weight)) & 3)
    return OFLOW_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(d_workspace) & 7) return OFLOW_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int HW = H * W;
  long long* acc = static_cast<long long*>(d_workspace);
  unsigned* hdr = reinterpret_cast<unsigned*>(static_cast<char*>(d_workspace) + splat_acc_bytes(B, C, H, W));
  const hipError_t e = hipMemsetAsync(d_workspace, 0, static_cast<size_t>(oflow_splat_workspace_bytes(B, C, H, W)), s);
  if (e != hipSuccess) return static_cast<int>(e);

  splat_launch_range(d_frame, d_metric, B, static_cast<long long>(C) * HW, HW, mode, hdr, s);

  const unsigned blocks = static_cast<unsigned>((HW + kThreads - 1) / kThreads);
  ScatterArgs sa;
  sa.frame = d_frame, sa.flow = d_flow, sa.metric = d_metric, sa.acc = acc, sa.hdr = hdr;
  sa.C = C, sa.H = H, sa.W = W, sa.mode = mode, sa.frac = oflow_splat_frac_bits(H, W);
  hipLaunchKernelGGL(splat_scatter_kernel, dim3(blocks, B), dim3(kThreads), 0, s, sa);
  FinishArgs fa;
  fa.acc = acc, fa.hdr = hdr, fa.out = d_out, fa.weight = d_weight;
  fa.C = C, fa.HW = HW, fa.mode = mode, fa.frac = sa.frac;
  hipLaunchKernelGGL(splat_finish_kernel, dim3(blocks, B), dim3(kThreads), 0, s, fa);
  return launch_status();
}
