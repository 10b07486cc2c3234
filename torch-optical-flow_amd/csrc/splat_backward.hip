// splat backward (gfx950): the gradients of oflow_splat_f32 with respect to the frame, the flow and the metric, as a
// pure gather: no float atomics, every output element written exactly once, the same bits on every run and whichever
// outputs are asked for. include/oflow.h states the formulas.
//
//   0. SOFT only: the image maxima of the metric, by the forward's range kernel (integer atomicMax on order keys: the
//      same value whatever the order), into the per-image words at the end of the workspace.
//   1. splat_prep_kernel (normalised modes only), one thread per target pixel: r = 1 / (D + EPS) and
//      gd = -r * sum_c g_c * out_c, the gradient that reaches D. These two planes are the only temporaries (g * r is
//      never materialised: the gather multiplies by r at the tap).
//   2. splat_gather_kernel, one thread per source pixel: the forward's landing position, taps and m once, then a loop
//      over the channels that reads g_c at the four taps. Neighbouring sources read neighbouring targets under a smooth
//      flow, so the tap reads are contiguous per wave like the forward's adds.
// fp32 arithmetic throughout (the tolerance of tests/splat_cases.py is calibrated on an fp32 composition).
#include "splat_common.h"

namespace oflow {
namespace {

constexpr int kThreads = kSplatThreads;
constexpr float kEps = static_cast<float>(OFLOW_SPLAT_EPS);

// grid (blocks, B): r and gd of every target pixel
__global__ __launch_bounds__(kThreads) void splat_prep_kernel(const float* __restrict__ gout,
                                                              const float* __restrict__ out,
                                                              const float* __restrict__ weight, int C, int HW,
                                                              float* __restrict__ r_plane, float* __restrict__ gd_plane) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= HW) return;
  const int b = blockIdx.y;
  const long long p = static_cast<long long>(b) * HW + t;
  const float r = 1.0f / (weight[p] + kEps);
  const float* g = gout + static_cast<long long>(b) * C * HW + t;
  const float* o = out + static_cast<long long>(b) * C * HW + t;
  float acc = 0.f;
  for (int c = 0; c < C; ++c, g += HW, o += HW) acc = fmaf(*g, *o, acc);
  r_plane[p] = r;
  gd_plane[p] = -r * acc;
}

struct GatherArgs {
  const float* gout;
  const float* frame;
  const float* flow;
  const float* metric;
  const float* r_plane;   // NULL for SUM
  const float* gd_plane;  // NULL for SUM
  const unsigned* hdr;    // per-image words (SOFT: word 1 = the metric's maximum), else NULL
  float* g_frame;         // each may be NULL
  float* g_flow;
  float* g_metric;
  int C, H, W, mode;
};

__global__ __launch_bounds__(kThreads) void splat_gather_kernel(GatherArgs a) {
  const int H = a.H, W = a.W, C = a.C;
  const int HW = H * W;
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= HW) return;
  const int b = blockIdx.y;
  const int i = s / W, j = s - i * W;
  const long long img = static_cast<long long>(b) * HW;
  const float* fl = a.flow + 2 * img;
  const float px = static_cast<float>(j) + fl[s], py = static_cast<float>(i) + fl[HW + s];
  float* gf = a.g_frame ? a.g_frame + img * C + s : nullptr;
  if (!(px > -1.f && px < static_cast<float>(W) && py > -1.f && py < static_cast<float>(H))) {  // skipped: zeros
    if (gf)
      for (int c = 0; c < C; ++c) gf[static_cast<long long>(c) * HW] = 0.f;
    if (a.g_flow) a.g_flow[2 * img + s] = 0.f, a.g_flow[2 * img + HW + s] = 0.f;
    if (a.g_metric) a.g_metric[img + s] = 0.f;
    return;
  }
  const float x0f = floorf(px), y0f = floorf(py);
  const float fx = px - x0f, fy = py - y0f;
  const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
  float m = 1.f;
  if (a.mode == OFLOW_SPLAT_LINEAR) m = a.metric[img + s];
  if (a.mode == OFLOW_SPLAT_SOFT) m = expf(a.metric[img + s] - __uint_as_float(a.hdr[b * kHdrWords + 1]));

  const float ax[2] = {1.f - fx, fx}, ay[2] = {1.f - fy, fy};
  float w[4], r[4], q[4];  // q_t starts as gd_t and gathers sum_c frame_c r_t g_c(t)
  int at[4];
  bool in[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + (t & 1), y = y0 + (t >> 1);
    in[t] = x >= 0 && x < W && y >= 0 && y < H;
    at[t] = in[t] ? y * W + x : 0;  // a dropped tap is never read
    w[t] = in[t] ? ax[t & 1] * ay[t >> 1] : 0.f;
    r[t] = (in[t] && a.r_plane) ? a.r_plane[img + at[t]] : 1.f;
    q[t] = (in[t] && a.gd_plane) ? a.gd_plane[img + at[t]] : 0.f;
  }
  float gm = fmaf(w[3], q[3], fmaf(w[2], q[2], fmaf(w[1], q[1], w[0] * q[0])));  // GD
  const float* g = a.gout + img * C;
  const float* fr = a.frame + img * C + s;
  for (int c = 0; c < C; ++c, g += HW, fr += HW) {
    const float f = *fr;
    float G = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float rg = in[t] ? r[t] * g[at[t]] : 0.f;
      G = fmaf(w[t], rg, G);
      q[t] = fmaf(f, rg, q[t]);
    }
    if (gf) gf[static_cast<long long>(c) * HW] = m * G;
    gm = fmaf(f, G, gm);
  }
  if (a.g_metric) a.g_metric[img + s] = a.mode == OFLOW_SPLAT_SOFT ? m * gm : gm;
  if (a.g_flow) {
    // dw_t/dpx = -ay[dy] (dx = 0), +ay[dy] (dx = 1); dw_t/dpy = -ax[dx] (dy = 0), +ax[dx] (dy = 1); dropped: q = 0
    const float dx = ay[0] * (q[1] - q[0]) + ay[1] * (q[3] - q[2]);
    const float dy = ax[0] * (q[2] - q[0]) + ax[1] * (q[3] - q[1]);
    a.g_flow[2 * img + s] = m * dx;
    a.g_flow[2 * img + HW + s] = m * dy;
  }
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_splat_backward_f32(const float* d_grad_out, const float* d_frame, const float* d_flow,
                                        const float* d_metric, const float* d_out, const float* d_weight, int B, int C,
                                        int H, int W, int mode, float* d_grad_frame, float* d_grad_flow,
                                        float* d_grad_metric, void* d_workspace, void* stream) {
  if (!d_grad_out || !d_frame || !d_flow) return OFLOW_E_NULL;
  if (!d_grad_frame && !d_grad_flow && !d_grad_metric) return OFLOW_E_NULL;
  const int st = splat_check_shape(B, C, H, W, mode);
  if (st != OFLOW_OK) return st;
  const bool metric_mode = mode == OFLOW_SPLAT_LINEAR || mode == OFLOW_SPLAT_SOFT;
  if (metric_mode && !d_metric) return OFLOW_E_NULL;
  if (!metric_mode && (d_metric || d_grad_metric)) return OFLOW_E_MODE;
  const bool norm = mode != OFLOW_SPLAT_SUM;
  if (norm && (!d_out || !d_weight || !d_workspace)) return OFLOW_E_NULL;
  if ((reinterpret_cast<uintptr_t>(d_grad_out) | reinterpret_cast<uintptr_t>(d_frame) | reinterpret_cast<uintptr_t>(d_flow) |
       reinterpret_cast<uintptr_t>(d_metric) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_weight) |
       reinterpret_cast<uintptr_t>(d_grad_frame) | reinterpret_cast<uintptr_t>(d_grad_flow) |
       reinterpret_cast<uintptr_t>(d_grad_metric)) & 3)
    return OFLOW_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(d_workspace) & 7) return OFLOW_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int HW = H * W;
  const unsigned blocks = static_cast<unsigned>((HW + kThreads - 1) / kThreads);
  GatherArgs ga;
  ga.gout = d_grad_out, ga.frame = d_frame, ga.flow = d_flow, ga.metric = d_metric;
  ga.r_plane = nullptr, ga.gd_plane = nullptr, ga.hdr = nullptr;
  ga.g_frame = d_grad_frame, ga.g_flow = d_grad_flow, ga.g_metric = d_grad_metric;
  ga.C = C, ga.H = H, ga.W = W, ga.mode = mode;
  if (norm) {
    // the workspace's first 8 * B * HW bytes: the r and gd planes; its last 4 * kHdrWords * B bytes: the per-image words
    float* r_plane = static_cast<float*>(d_workspace);
    float* gd_plane = r_plane + static_cast<long long>(B) * HW;
    hipLaunchKernelGGL(splat_prep_kernel, dim3(blocks, B), dim3(kThreads), 0, s, d_grad_out, d_out, d_weight, C, HW,
                       r_plane, gd_plane);
    ga.r_plane = r_plane, ga.gd_plane = gd_plane;
    if (mode == OFLOW_SPLAT_SOFT) {
      unsigned* hdr = reinterpret_cast<unsigned*>(static_cast<char*>(d_workspace) + splat_acc_bytes(B, C, H, W));
      const hipError_t e = hipMemsetAsync(hdr, 0, sizeof(unsigned) * kHdrWords * B, s);
      if (e != hipSuccess) return static_cast<int>(e);
      splat_launch_range(nullptr, d_metric, B, 0, HW, mode, hdr, s);
      ga.hdr = hdr;
    }
  }
  hipLaunchKernelGGL(splat_gather_kernel, dim3(blocks, B), dim3(kThreads), 0, s, ga);
  return launch_status();
}
