// Backward of the encoders' norm layers (gfx950), each with the ReLU the block applies directly after it folded in
// (extractor.py: relu(norm(conv(x)))). fp32 NCHW, one workgroup per plane (b, c) of HW elements; at the training shape
// that is 2 * B * 64 planes of 45 k elements at half resolution, more planes than CUs.
//
// Per plane: mu, r = 1 / sqrt(var_biased + eps), xh = (x - mu) * r, g = gy * [y > 0] with the ReLU (y the layer's
// output before it), g = gy without.
//   instance norm, no affine (fnet):  dx = r * (g - mean(g) - xh * mean(g * xh))
//     Only x is kept from the forward: mu, r and the ReLU mask (xh > 0) are recomputed here. The statistics are
//     shifted sums in fp64 (d = x - x[0]: sum d, sum d^2), so a plane with |mu| >> sigma keeps its variance (a naive
//     fp32 E[x^2] - E[x]^2 gives 0.01074 for a true 0.00998 at mean 100, sigma 0.1) and a constant plane has var = 0
//     exactly. Three sweeps: statistics, the two means (they need the mask, hence mu), apply; the second and third find
//     the plane in L2.
//   frozen batch norm (cnet with running statistics): y = (x - rm) * gamma / sqrt(rv + eps) + beta
//     dx = g * gamma / sqrt(rv + eps), dgamma = sum g * (x - rm) / sqrt(rv + eps), dbeta = sum g over (B, H, W).
//     One sweep writes dx and the plane's two partial sums to workspace[2][B][C]; a second kernel adds the B partials
//     of a channel in ascending order.
// Sums: each thread adds its elements in ascending order in fp64, a fixed LDS tree folds the 256 partials. No atomics,
// nothing for the caller to zero: the result is bit-reproducible for a given shape and alignment. Rows that are
// 16-byte aligned move as float4 (a plane's unaligned head and tail, at most 3 elements each, as scalars); with a
// base pointer that is not 16-byte aligned everything moves as scalars.
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kNThreads = 256;

// the sum of a and of b over the workgroup, returned to every thread (fixed tree)
__device__ inline void block_sum2(double& a, double& b, double (*sS)[kNThreads]) {
  const int tid = threadIdx.x;
  __syncthreads();  // (the previous use of sS is over)
  sS[0][tid] = a;
  sS[1][tid] = b;
  __syncthreads();
  for (int w = kNThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      sS[0][tid] += sS[0][tid + w];
      sS[1][tid] += sS[1][tid + w];
    }
    __syncthreads();
  }
  a = sS[0][0];
  b = sS[1][0];
}

// f(gy[i], x[i]) -> dx[i] for the plane's elements i in [0, n): scalar head up to the first 16-byte boundary, float4
// body, scalar tail. GY / ST: whether gy is read / dx is stored.
template <bool GY, bool ST, typename F>
__device__ inline void sweep(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ dx, size_t base,
                             int n, bool vec, F f) {
  const int tid = threadIdx.x;
  const int head = vec ? min(n, (int)((4 - (base & 3)) & 3)) : n;
  const int nv = (n - head) / 4;
  const float* px = x + base;
  const float* pg = GY ? gy + base : nullptr;
  float* pd = ST ? dx + base : nullptr;
  for (int i = tid; i < head; i += kNThreads) {
    const float d = f(GY ? pg[i] : 0.f, px[i]);
    if (ST) pd[i] = d;
  }
  for (int v = tid; v < nv; v += kNThreads) {
    const int i = head + 4 * v;
    const float4 xv = *reinterpret_cast<const float4*>(px + i);
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (GY) gv = *reinterpret_cast<const float4*>(pg + i);
    float4 dv;
    dv.x = f(gv.x, xv.x);
    dv.y = f(gv.y, xv.y);
    dv.z = f(gv.z, xv.z);
    dv.w = f(gv.w, xv.w);
    if (ST) *reinterpret_cast<float4*>(pd + i) = dv;
  }
  for (int i = head + 4 * nv + tid; i < n; i += kNThreads) {
    const float d = f(GY ? pg[i] : 0.f, px[i]);
    if (ST) pd[i] = d;
  }
}

__global__ __launch_bounds__(kNThreads) void instance_norm_backward_kernel(const float* __restrict__ gy,
                                                                           const float* __restrict__ x,
                                                                           float* __restrict__ dx, int HW, double eps,
                                                                           int relu, int vec) {
  __shared__ double sS[2][kNThreads];
  const size_t base = (size_t)blockIdx.x * HW;
  const double shift = x[base];
  double a = 0.0, b = 0.0;
  sweep<false, false>(gy, x, dx, base, HW, vec, [&](float, float xv) {
    const double d = (double)xv - shift;
    a += d;
    b += d * d;
    return 0.f;
  });
  block_sum2(a, b, sS);
  const double md = a / HW, mu = shift + md;
  const double var = fmax(b / HW - md * md, 0.0);
  const double r = 1.0 / sqrt(var + eps);
  const float rf = (float)r;
  a = 0.0, b = 0.0;
  sweep<true, false>(gy, x, dx, base, HW, vec, [&](float gv, float xv) {
    const double dc = (double)xv - mu;
    const float xh = (float)(dc * r);
    const float g = (relu && !(dc > 0.0)) ? 0.f : gv;
    a += g;
    b += (double)g * xh;
    return 0.f;
  });
  block_sum2(a, b, sS);
  const float mg = (float)(a / HW), mgx = (float)(b / HW);
  sweep<true, true>(gy, x, dx, base, HW, vec, [&](float gv, float xv) {
    const double dc = (double)xv - mu;
    const float xh = (float)(dc * r);
    const float g = (relu && !(dc > 0.0)) ? 0.f : gv;
    return rf * (g - mg - xh * mgx);
  });
}

// ws[0][b][c] = sum g * (x - rm) * rstd, ws[1][b][c] = sum g over the plane (when ws is given); dx when given
__global__ __launch_bounds__(kNThreads) void frozen_bn_backward_kernel(
    const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ weight,
    const float* __restrict__ bias, const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ dx,
    float* __restrict__ ws, int C, int HW, int planes, double eps, int relu, int vec) {
  __shared__ double sS[2][kNThreads];
  const int plane = blockIdx.x, c = plane % C;
  const size_t base = (size_t)plane * HW;
  const double rm = rmean[c], rstd = 1.0 / sqrt((double)rvar[c] + eps);
  const double alpha = (double)weight[c] * rstd, beta = bias[c];
  const float af = (float)alpha;
  double a = 0.0, b = 0.0;
  auto body = [&](float gv, float xv) {
    const double dc = (double)xv - rm;
    const float g = (relu && !(dc * alpha + beta > 0.0)) ? 0.f : gv;
    a += (double)g * (float)(dc * rstd);
    b += g;
    return g * af;
  };
  if (dx)
    sweep<true, true>(gy, x, dx, base, HW, vec, body);
  else
    sweep<true, false>(gy, x, dx, base, HW, vec, body);
  if (!ws) return;  // (uniform)
  block_sum2(a, b, sS);
  if (threadIdx.x == 0) {
    ws[plane] = (float)a;
    ws[planes + plane] = (float)b;
  }
}

// dweight[c] = ws[0][0][c] + ws[0][1][c] + ..., dbias[c] likewise from ws[1]: ascending b
__global__ __launch_bounds__(kNThreads) void frozen_bn_combine_kernel(const float* __restrict__ ws, float* __restrict__ dweight,
                                                                      float* __restrict__ dbias, int B, int C) {
  const int c = blockIdx.x * kNThreads + threadIdx.x;
  if (c >= C) return;
  const size_t planes = (size_t)B * C;
  float sw = ws[c], sb = ws[planes + c];
  for (int b = 1; b < B; ++b) {
    sw += ws[(size_t)b * C + c];
    sb += ws[planes + (size_t)b * C + c];
  }
  if (dweight) dweight[c] = sw;
  if (dbias) dbias[c] = sb;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// planes is the grid's x dimension; HW an int element count per plane
bool norm_geom_ok(long long planes, int HW) { return planes >= 1 && planes <= 2147483647ll && HW >= 1; }

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_instance_norm_backward_f32(const float* d_grad_out, const float* d_x, int planes, int HW, double eps,
                                                int relu, float* d_grad_input, void* stream) {
  if (!d_grad_out || !d_x || !d_grad_input) return OFLOW_E_NULL;
  if (!norm_geom_ok(planes, HW) || !(eps >= 0.0)) return OFLOW_E_SHAPE;
  const int vec = aligned16(d_grad_out) && aligned16(d_x) && aligned16(d_grad_input);
  hipLaunchKernelGGL(instance_norm_backward_kernel, dim3(planes), dim3(kNThreads), 0, static_cast<hipStream_t>(stream),
                     d_grad_out, d_x, d_grad_input, HW, eps, relu != 0, vec);
  return launch_status();
}

extern "C" long long oflow_frozen_batch_norm_backward_workspace_floats(int B, int C, int HW) {
  if (B < 1 || C < 1 || !norm_geom_ok((long long)B * C, HW)) return 0;
  return 2ll * B * C;
}

extern "C" int oflow_frozen_batch_norm_backward_f32(const float* d_grad_out, const float* d_x, const float* d_weight,
                                                    const float* d_bias, const float* d_running_mean,
                                                    const float* d_running_var, int B, int C, int HW, double eps, int relu,
                                                    float* d_grad_input, float* d_grad_weight, float* d_grad_bias,
                                                    float* d_workspace, void* stream) {
  const bool params = d_grad_weight || d_grad_bias;
  if (!d_grad_out || !d_x || !d_weight || !d_bias || !d_running_mean || !d_running_var) return OFLOW_E_NULL;
  if ((!d_grad_input && !params) || (params && !d_workspace)) return OFLOW_E_NULL;
  if (B < 1 || C < 1 || !norm_geom_ok((long long)B * C, HW) || !(eps >= 0.0)) return OFLOW_E_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int vec = aligned16(d_grad_out) && aligned16(d_x) && (!d_grad_input || aligned16(d_grad_input));
  hipLaunchKernelGGL(frozen_bn_backward_kernel, dim3(B * C), dim3(kNThreads), 0, st, d_grad_out, d_x, d_weight, d_bias,
                     d_running_mean, d_running_var, d_grad_input, params ? d_workspace : nullptr, C, HW, B * C, eps,
                     relu != 0, vec);
  if (params)
    hipLaunchKernelGGL(frozen_bn_combine_kernel, dim3((C + kNThreads - 1) / kNThreads), dim3(kNThreads), 0, st, d_workspace,
                       d_grad_weight, d_grad_bias, B, C);
  return launch_status();
}
