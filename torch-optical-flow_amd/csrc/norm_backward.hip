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
#include "norm_sweep.h"  // kNThreads, block_sum2, sweep, aligned16 (shared with batch_norm.hip)

namespace oflow {
namespace {

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
