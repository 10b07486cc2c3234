// smoothness_loss (gfx950): the edge-aware first- or second-order smoothness term that accompanies the census loss in
// the unsupervised flow methods (UFlow, Jonschkowski et al., ECCV 2020; their published constants), forward and
// backward, each as one streaming launch. include/oflow.h states the contract.
//
// One thread per pixel. The forward forms the pixel's x and y differences of both flow channels, weights them by the
// image edge term and reduces (sum x, sum y) in fp64 as flow_metrics.hip does -- per thread, __shfl_xor within the
// wave, LDS across the waves, one partial row per workgroup in the caller's workspace -- and a one-workgroup finalize
// kernel adds the rows in index order and forms (Lx + Ly) / 2. The backward is a gather: a flow pixel takes part in
// order + 1 differences per direction and adds their derivatives in a fixed order. No atomics, the grid depends on the
// shapes only: both directions are bit-identical from run to run. The neighbours come from L1 / L2; HBM sees every
// input once (8 + 4 C bytes per pixel).
#include "oflow_internal.h"

#include <climits>
#include <cmath>

namespace oflow {
namespace {

constexpr int kThreads = 256;

struct SmoothArgs {
  const float* flow;   // (B, 2, H, W)
  const float* image;  // (B, C, H, W)
  int B, C, H, W, order;
  float k;  // edge_weight / image_range
  long long pixels;  // B * H * W
};

// The difference that starts at plane offset p (of image b) and runs along stride st: its edge weight
// w = exp(-k mean_c |I_c(p + order st) - I_c(p)|) and the two flow channels' differences.
__device__ __forceinline__ void difference(const SmoothArgs& a, long long b, long long p, long long st, float& w,
                                           float& d0, float& d1) {
  const long long plane = static_cast<long long>(a.H) * a.W;
  const float* im = a.image + b * a.C * plane + p;
  float sum = 0.f;
  for (int c = 0; c < a.C; ++c) sum += fabsf(im[c * plane + a.order * st] - im[c * plane]);
  w = expf(-a.k * (sum / static_cast<float>(a.C)));
  const float* f0 = a.flow + b * 2 * plane + p;
  const float* f1 = f0 + plane;
  // the flow differences in fp64 (exact for fp32 flows), rounded once: near 0 the derivative of sqrt(d^2 + 0.001^2)
  // changes by 1 over a span of 0.001, so fp32 rounding inside the stencil would show in the gradient
  const double m = a.order == 1 ? 0.0 : 1.0;  // order 2: f(+2) - 2 f(+1) + f(0) = (f(+2) - f(+1)) - (f(+1) - f(0))
  const long long hi = a.order * st, lo = (a.order - 1) * st;
  d0 = static_cast<float>((static_cast<double>(f0[hi]) - f0[lo]) - m * (static_cast<double>(f0[lo]) - f0[0]));
  d1 = static_cast<float>((static_cast<double>(f1[hi]) - f1[lo]) - m * (static_cast<double>(f1[lo]) - f1[0]));
}

__device__ __forceinline__ float charbonnier(float d) { return sqrtf(d * d + 1e-6f); }  // 0.001^2

__global__ __launch_bounds__(kThreads) void smoothness_forward_kernel(SmoothArgs a, double* __restrict__ partials) {
  const long long n = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  double sx = 0.0, sy = 0.0;
  if (n < a.pixels) {
    const long long plane = static_cast<long long>(a.H) * a.W;
    const long long b = n / plane, p = n - b * plane;
    const int y = static_cast<int>(p / a.W), x = static_cast<int>(p - static_cast<long long>(y) * a.W);
    float w, d0, d1;
    if (x + a.order < a.W) {
      difference(a, b, p, 1, w, d0, d1);
      sx = static_cast<double>(w * charbonnier(d0)) + static_cast<double>(w * charbonnier(d1));
    }
    if (y + a.order < a.H) {
      difference(a, b, p, a.W, w, d0, d1);
      sy = static_cast<double>(w * charbonnier(d0)) + static_cast<double>(w * charbonnier(d1));
    }
  }
  block_sum2_f64(sx, sy);
  if (threadIdx.x == 0) {
    partials[2LL * blockIdx.x] = sx;
    partials[2LL * blockIdx.x + 1] = sy;
  }
}

// elements of a direction's mean: B * 2 * H * (W - order) for x, 0 when the domain is empty
inline double domain(int B, int along, int across, int order) {
  return along > order ? 2.0 * B * static_cast<double>(across) * (along - order) : 0.0;
}

__global__ __launch_bounds__(kThreads) void smoothness_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                       double nx, double ny, float* __restrict__ loss) {
  double sx = 0.0, sy = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) {
    sx += partials[2LL * i];
    sy += partials[2LL * i + 1];
  }
  block_sum2_f64(sx, sy);
  if (threadIdx.x == 0) loss[0] = static_cast<float>(0.5 * ((nx > 0.0 ? sx / nx : 0.0) + (ny > 0.0 ? sy / ny : 0.0)));
}

// The derivative of one direction's sum with respect to the flow at position i of a line of length len (plane offset
// p, stride st): the differences that start at i - j, j = 0..order, where they exist, with the stencil's coefficient
// of their element j ((-1, 1) or (1, -2, 1)), in the order j = 0, 1, 2.
__device__ __forceinline__ void gather(const SmoothArgs& a, long long b, long long p, long long st, int i, int len,
                                       float& g0, float& g1) {
  g0 = g1 = 0.f;
  for (int j = 0; j <= a.order; ++j) {
    const int s = i - j;
    if (s < 0 || s + a.order >= len) continue;
    float w, d0, d1;
    difference(a, b, p - j * st, st, w, d0, d1);
    const float coef = a.order == 1 ? (j == 0 ? -1.f : 1.f) : (j == 1 ? -2.f : 1.f);
    g0 += coef * (w * (d0 / charbonnier(d0)));
    g1 += coef * (w * (d1 / charbonnier(d1)));
  }
}

__global__ __launch_bounds__(kThreads) void smoothness_backward_kernel(SmoothArgs a, const float* __restrict__ grad_loss,
                                                                       float inv_nx, float inv_ny,
                                                                       float* __restrict__ grad_flow) {
  const long long n = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (n >= a.pixels) return;
  const long long plane = static_cast<long long>(a.H) * a.W;
  const long long b = n / plane, p = n - b * plane;
  const int y = static_cast<int>(p / a.W), x = static_cast<int>(p - static_cast<long long>(y) * a.W);
  const float go = 0.5f * grad_loss[0];
  float x0, x1, y0, y1;
  gather(a, b, p, 1, x, a.W, x0, x1);
  gather(a, b, p, a.W, y, a.H, y0, y1);
  float* out = grad_flow + b * 2 * plane + p;
  out[0] = go * (inv_nx * x0 + inv_ny * y0);
  out[plane] = go * (inv_nx * x1 + inv_ny * y1);
}

// workgroups of one launch, 0 when the shape is outside the kernels' range
long long smooth_blocks(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || B > 65535 || static_cast<long long>(H) * W > (1LL << 28)) return 0;
  const long long n = (static_cast<long long>(B) * H * W + kThreads - 1) / kThreads;
  return n <= INT_MAX ? n : 0;
}

int smooth_args(const float* d_flow, const float* d_image, int B, int C, int H, int W, int order, float edge_weight,
                float image_range, SmoothArgs& a, long long& blocks) {
  if (!d_flow || !d_image) return OFLOW_E_NULL;
  if (order != 1 && order != 2) return OFLOW_E_MODE;
  blocks = smooth_blocks(B, H, W);
  if (blocks == 0 || C < 1 || !(image_range > 0.f) || !std::isfinite(image_range) || !std::isfinite(edge_weight))
    return OFLOW_E_SHAPE;
  if (!aligned_to(d_flow, 4) || !aligned_to(d_image, 4)) return OFLOW_E_ALIGN;
  a.flow = d_flow, a.image = d_image;
  a.B = B, a.C = C, a.H = H, a.W = W, a.order = order;
  a.k = edge_weight / image_range;
  a.pixels = static_cast<long long>(B) * H * W;
  return OFLOW_OK;
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" long long oflow_smoothness_loss_workspace_bytes(int B, int H, int W) { return 16 * smooth_blocks(B, H, W); }

extern "C" int oflow_smoothness_loss_f32(const float* d_flow, const float* d_image, int B, int C, int H, int W,
                                         int order, float edge_weight, float image_range, double* d_workspace,
                                         float* d_loss, void* stream) {
  if (!d_workspace || !d_loss) return OFLOW_E_NULL;
  SmoothArgs a;
  long long blocks;
  const int st0 = smooth_args(d_flow, d_image, B, C, H, W, order, edge_weight, image_range, a, blocks);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_workspace, 8) || !aligned_to(d_loss, 4)) return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(smoothness_forward_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, a, d_workspace);
  const int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(smoothness_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, static_cast<int>(blocks),
                     domain(B, W, H, order), domain(B, H, W, order), d_loss);
  return launch_status();
}

extern "C" int oflow_smoothness_loss_backward_f32(const float* d_grad_loss, const float* d_flow, const float* d_image,
                                                  int B, int C, int H, int W, int order, float edge_weight,
                                                  float image_range, float* d_grad_flow, void* stream) {
  if (!d_grad_loss || !d_grad_flow) return OFLOW_E_NULL;
  SmoothArgs a;
  long long blocks;
  const int st0 = smooth_args(d_flow, d_image, B, C, H, W, order, edge_weight, image_range, a, blocks);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_grad_loss, 4) || !aligned_to(d_grad_flow, 4)) return OFLOW_E_ALIGN;
  const double nx = domain(B, W, H, order), ny = domain(B, H, W, order);
  hipLaunchKernelGGL(smoothness_backward_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a, d_grad_loss, nx > 0.0 ? static_cast<float>(1.0 / nx) : 0.f,
                     ny > 0.0 ? static_cast<float>(1.0 / ny) : 0.f, d_grad_flow);
  return launch_status();
}
