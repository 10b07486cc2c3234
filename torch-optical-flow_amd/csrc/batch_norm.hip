// Batch norm on batch statistics (gfx950), forward and backward, each with the ReLU the block applies directly after it
// folded in (extractor.py: relu(norm(conv(x))) with cnet's BatchNorm2d in train mode: the Chairs stage). fp32 NCHW,
// n = B * HW elements per channel.
//   forward:   mean[c], var[c] (biased) over (B, H, W); r = 1 / sqrt(var + eps); y = (x - mean) * r * gamma + beta [ReLU]
//   backward:  g = gy * [y > 0] with the ReLU, g = gy without; xh = (x - mean) * r
//              dbeta = sum g, dgamma = sum g * xh, dx = gamma * r * (g - dbeta / n - xh * dgamma / n)
//
// Work split. A channel's statistics reduce across its B planes, and a channel holds only B planes of work (64 to 128
// channels at the training shapes against 256 CUs), so a workgroup per channel would leave most of the chip idle and a
// workgroup per plane (norm_backward.hip) cannot finish a channel sum. Work is cut by plane and by chunks of kChunk
// elements of a plane, one workgroup per (plane, chunk), and the channel sums go through fp64 partials in the workspace:
//   forward:  stats sweep -> finalize (mean, var) -> apply sweep;  backward:  sums sweep -> combine -> apply sweep.
// kChunk is a compile-time constant, so the grid and every summation order depend on the shape only. The finalize /
// combine launch is one thread per channel, a serial fp64 loop over the channel's B * chunks partials (48 at most at
// the training shapes) in ceil(C / 256) workgroups: it moves a few KiB and costs its launch latency only. It cannot be
// folded into the last-arriving workgroup of the sweep without an atomic counter, which this file does without.
//   kChunk = 8192 elements (32 KiB of x): at cnet's training shapes 8 x 64 x 184 x 248, 8 x 96 x 92 x 124 and
//   8 x 128 x 46 x 62 that is 6, 2 and 1 chunks per plane = 3072, 1536 and 1024 workgroups. A CU holds at most 8
//   workgroups of 256 threads (32 waves per CU; 4 KiB of LDS and few registers do not bind), so 2048 are resident at a
//   time: the two larger layers fill the chip, the smallest (23 MB, inside the Infinity Cache) cannot be cut finer than
//   its planes without chunks of under 3 k elements. Each thread then moves 8 float4 per operand per sweep, enough
//   independent loads to cover the HBM latency without unrolling by hand, and the workgroup's fixed cost (two 8-step
//   LDS trees of fp64 pairs) is spread over 32 KiB per operand. A smaller chunk doubles the partials and the trees for
//   no more parallelism than the chip can hold; a larger one leaves the 96-channel layer under one wave of workgroups.
//   256 threads: the block size of norm_backward.hip, whose sweep and tree this file shares (norm_sweep.h). These
//   choices are reasoned, not tuned: tools/batch_norm_bench.py reports what they achieve.
//
// Statistics are shifted sums in fp64, d = x - x[0, c, 0, 0] (sum d, sum d^2): one shift per channel, so the partials of
// different planes add directly, a channel with |mean| >> sigma keeps its variance and a constant channel has var = 0
// exactly (instance_norm_backward_kernel's scheme, for the reason its header gives). The backward does not recompute
// them: it takes mean and var (fp32, C each) as the forward returned them and forms r from them exactly as the forward's
// apply sweep did. The ReLU mask is recomputed from x by bn_pre(), the function the forward's apply sweep stores y from,
// so both decide y > 0 identically.
//
// Workspace (doubles): partials[c][b][chunk][2] (a channel's partials contiguous, in the order they are added), then
// totals[c][2]: the channel sums (forward: sum d, sum d^2; backward: sum g, sum g * xh). Every call writes all of it.
// Sums: each thread adds its elements in ascending order in fp64, a fixed LDS tree folds the 256 partials, one thread
// per channel adds the channel's partials in ascending (b, chunk) order. No atomics, nothing for the caller to zero:
// the result is bit-reproducible for a given shape and alignment. Rows that are 16-byte aligned move as float4 (a
// chunk's unaligned head and tail, at most 3 elements each, as scalars); with a base pointer that is not 16-byte aligned
// everything moves as scalars.
#include "norm_sweep.h"

namespace oflow {
namespace {

constexpr int kChunk = 8192;

__host__ __device__ inline int chunks_of(int HW) { return (HW + kChunk - 1) / kChunk; }

// the layer's output before the ReLU, as the fp32 value the forward stores (alpha = gamma * r)
__device__ __forceinline__ float bn_pre(float xv, double mean, double alpha, double beta) {
  return (float)(((double)xv - mean) * alpha + beta);
}

struct Geom {
  int C, HW, nch;
};

// the (plane, chunk) of this workgroup: element range [base, base + n) and the partial's slot
__device__ __forceinline__ void locate(const Geom& gm, int B, int& c, size_t& base, int& n, size_t& slot) {
  const int plane = blockIdx.x / gm.nch, chunk = blockIdx.x - plane * gm.nch;
  const int b = plane / gm.C;
  c = plane - b * gm.C;
  base = (size_t)plane * gm.HW + (size_t)chunk * kChunk;
  n = min(kChunk, gm.HW - chunk * kChunk);
  slot = (((size_t)c * B + b) * gm.nch + chunk) * 2;
}

// part[c][b][chunk] = (sum d, sum d^2) over the chunk, d = x - x[0, c, 0, 0]
__global__ __launch_bounds__(kNThreads) void bn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int B,
                                                             Geom gm, int vec) {
  __shared__ double sS[2][kNThreads];
  int c, n;
  size_t base, slot;
  locate(gm, B, c, base, n, slot);
  const double shift = x[(size_t)c * gm.HW];
  double a = 0.0, b = 0.0;
  sweep<false, false>(nullptr, x, nullptr, base, n, vec, [&](float, float xv) {
    const double d = (double)xv - shift;
    a += d;
    b += d * d;
    return 0.f;
  });
  block_sum2(a, b, sS);
  if (threadIdx.x == 0) {
    part[slot] = a;
    part[slot + 1] = b;
  }
}

// the channel's partials added in ascending (b, chunk) order -> totals; STATS: mean and var from them
// (x given), else dgamma and dbeta (each when given)
template <bool STATS>
__global__ __launch_bounds__(kNThreads) void bn_combine_kernel(const double* __restrict__ part, double* __restrict__ totals,
                                                               const float* __restrict__ x, float* __restrict__ out0,
                                                               float* __restrict__ out1, int B, Geom gm) {
  const int c = blockIdx.x * kNThreads + threadIdx.x;
  if (c >= gm.C) return;
  const size_t per = (size_t)B * gm.nch;
  const double* p = part + (size_t)c * per * 2;
  double a = p[0], b = p[1];
  for (size_t i = 1; i < per; ++i) {
    a += p[2 * i];
    b += p[2 * i + 1];
  }
  totals[2 * c] = a;
  totals[2 * c + 1] = b;
  if (STATS) {
    const double n = (double)B * gm.HW, md = a / n;
    out0[c] = (float)((double)x[(size_t)c * gm.HW] + md);
    out1[c] = (float)fmax(b / n - md * md, 0.0);
  } else {
    if (out0) out0[c] = (float)b;  // dgamma = sum g * xh
    if (out1) out1[c] = (float)a;  // dbeta = sum g
  }
}

__global__ __launch_bounds__(kNThreads) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                             const float* __restrict__ bias, const float* __restrict__ mean,
                                                             const float* __restrict__ var, float* __restrict__ y, int B,
                                                             Geom gm, double eps, int relu, int vec) {
  int c, n;
  size_t base, slot;
  locate(gm, B, c, base, n, slot);
  const double mu = mean[c], r = 1.0 / sqrt((double)var[c] + eps);
  const double alpha = (double)weight[c] * r, beta = bias[c];
  sweep<false, true>(nullptr, x, y, base, n, vec, [&](float, float xv) {
    const float pre = bn_pre(xv, mu, alpha, beta);
    return relu ? fmaxf(pre, 0.f) : pre;
  });
}

// part[c][b][chunk] = (sum g, sum g * xh) over the chunk
__global__ __launch_bounds__(kNThreads) void bn_backward_sums_kernel(
    const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ bias,
    const float* __restrict__ mean, const float* __restrict__ var, double* __restrict__ part, int B, Geom gm, double eps,
    int relu, int vec) {
  __shared__ double sS[2][kNThreads];
  int c, n;
  size_t base, slot;
  locate(gm, B, c, base, n, slot);
  const double mu = mean[c], r = 1.0 / sqrt((double)var[c] + eps);
  const double alpha = (double)weight[c] * r, beta = bias[c];
  double a = 0.0, b = 0.0;
  sweep<true, false>(gy, x, nullptr, base, n, vec, [&](float gv, float xv) {
    const float xh = (float)(((double)xv - mu) * r);
    const float g = (relu && !(bn_pre(xv, mu, alpha, beta) > 0.f)) ? 0.f : gv;
    a += g;
    b += (double)g * xh;
    return 0.f;
  });
  block_sum2(a, b, sS);
  if (threadIdx.x == 0) {
    part[slot] = a;
    part[slot + 1] = b;
  }
}

// dx = gamma * r * (g - sum g / n - xh * sum(g * xh) / n), the two channel sums from totals
__global__ __launch_bounds__(kNThreads) void bn_backward_apply_kernel(
    const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ bias,
    const float* __restrict__ mean, const float* __restrict__ var, const double* __restrict__ totals, float* __restrict__ dx,
    int B, Geom gm, double eps, int relu, int vec) {
  int c, n;
  size_t base, slot;
  locate(gm, B, c, base, n, slot);
  const double mu = mean[c], r = 1.0 / sqrt((double)var[c] + eps);
  const double alpha = (double)weight[c] * r, beta = bias[c];
  const double cnt = (double)B * gm.HW;
  const float af = (float)alpha, mg = (float)(totals[2 * c] / cnt), mgx = (float)(totals[2 * c + 1] / cnt);
  sweep<true, true>(gy, x, dx, base, n, vec, [&](float gv, float xv) {
    const float xh = (float)(((double)xv - mu) * r);
    const float g = (relu && !(bn_pre(xv, mu, alpha, beta) > 0.f)) ? 0.f : gv;
    return af * (g - mg - xh * mgx);
  });
}

// B * C * chunks workgroups on the grid's x dimension; HW an int element count per plane
bool bn_geom_ok(int B, int C, int HW) {
  return B >= 1 && C >= 1 && HW >= 1 && (long long)B * C * chunks_of(HW) <= 2147483647ll;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_batch_norm_chunk_elements(void) { return kChunk; }

extern "C" long long oflow_batch_norm_workspace_floats(int B, int C, int HW) {
  if (!bn_geom_ok(B, C, HW)) return 0;
  return 4ll * B * C * chunks_of(HW) + 4ll * C;  // (2 doubles per (plane, chunk) + 2 per channel) * 2 floats
}

extern "C" int oflow_batch_norm_forward_f32(const float* d_x, const float* d_weight, const float* d_bias, int B, int C,
                                            int HW, double eps, int relu, float* d_y, float* d_mean, float* d_var,
                                            float* d_workspace, void* stream) {
  if (!d_x || !d_mean || !d_var || !d_workspace || (d_y && (!d_weight || !d_bias))) return OFLOW_E_NULL;
  if (!bn_geom_ok(B, C, HW) || !(eps >= 0.0)) return OFLOW_E_SHAPE;
  if (!aligned8(d_workspace)) return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Geom gm{C, HW, chunks_of(HW)};
  const int grid = B * C * gm.nch;
  double* part = reinterpret_cast<double*>(d_workspace);
  double* totals = part + 2ll * grid;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(grid), dim3(kNThreads), 0, st, d_x, part, B, gm, (int)aligned16(d_x));
  hipLaunchKernelGGL(bn_combine_kernel<true>, dim3((C + kNThreads - 1) / kNThreads), dim3(kNThreads), 0, st, part, totals, d_x,
                     d_mean, d_var, B, gm);
  if (d_y)
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid), dim3(kNThreads), 0, st, d_x, d_weight, d_bias, d_mean, d_var, d_y, B, gm,
                       eps, relu != 0, (int)(aligned16(d_x) && aligned16(d_y)));
  return launch_status();
}

extern "C" int oflow_batch_norm_backward_f32(const float* d_grad_out, const float* d_x, const float* d_weight,
                                             const float* d_bias, const float* d_mean, const float* d_var, int B, int C, int HW,
                                             double eps, int relu, float* d_grad_input, float* d_grad_weight,
                                             float* d_grad_bias, float* d_workspace, void* stream) {
  if (!d_grad_out || !d_x || !d_weight || !d_bias || !d_mean || !d_var) return OFLOW_E_NULL;
  if ((!d_grad_input && !d_grad_weight && !d_grad_bias) || !d_workspace) return OFLOW_E_NULL;
  if (!bn_geom_ok(B, C, HW) || !(eps >= 0.0)) return OFLOW_E_SHAPE;
  if (!aligned8(d_workspace)) return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Geom gm{C, HW, chunks_of(HW)};
  const int grid = B * C * gm.nch;
  double* part = reinterpret_cast<double*>(d_workspace);
  double* totals = part + 2ll * grid;
  // (the sums' order inside a thread follows the alignment of what the sums sweep reads, not d_grad_input's: the
  // parameter gradients and the sums under dx are the same bits whichever outputs are asked for)
  const int vec_in = aligned16(d_grad_out) && aligned16(d_x), vec = vec_in && d_grad_input && aligned16(d_grad_input);
  hipLaunchKernelGGL(bn_backward_sums_kernel, dim3(grid), dim3(kNThreads), 0, st, d_grad_out, d_x, d_weight, d_bias, d_mean,
                     d_var, part, B, gm, eps, relu != 0, vec_in);
  hipLaunchKernelGGL(bn_combine_kernel<false>, dim3((C + kNThreads - 1) / kNThreads), dim3(kNThreads), 0, st, part, totals,
                     nullptr, d_grad_weight, d_grad_bias, B, gm);
  if (d_grad_input)
    hipLaunchKernelGGL(bn_backward_apply_kernel, dim3(grid), dim3(kNThreads), 0, st, d_grad_out, d_x, d_weight, d_bias, d_mean,
                       d_var, totals, d_grad_input, B, gm, eps, relu != 0, vec);
  return launch_status();
}
