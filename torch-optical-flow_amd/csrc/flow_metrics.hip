// Evaluation and training reductions (gfx950): the flow error statistics behind optical_flow.metrics and the
// forward / backward of RAFT's sequence loss, each as one streaming pass that reads every input byte once.
//
// flow_error_stats replaces AverageEndPointError.update / OutlierRatio.update / end_point_error
// (optical_flow/metrics/epe.py:24-65, optical_flow/metrics/f1.py:34-55): there ~10 ATen passes over full-resolution
// tensors plus a boolean index (`epe[valid]`: a device-to-host synchronisation per batch); here one partial kernel and
// a one-workgroup finalize kernel that ADDS into the metric's device accumulator -- no host synchronisation.
// sequence_loss replaces methods/raft/model/raft.py:239-258 (about four passes over each of the 12 predictions and
// three .item() calls) by one pass over all predictions, and its autograd by one pass that writes every gradient.
//
// Reductions: per thread in pixel order (fp64 sum, integer counts), within a wave by __shfl_xor, across the waves
// through LDS, one partial row per workgroup in a caller-owned workspace (at most OFLOW_FLOW_METRICS_PARTIALS rows),
// then the finalize kernel in a fixed order. No float atomics and no cross-workgroup last-arriver (the per-XCD L2s are
// not coherent): the grid depends on the shapes only, so results are bit-reproducible from run to run.
//
// Arithmetic per pixel is the reference's op for op in fp32 (each ATen op is its own kernel there, nothing is fused:
// contraction is off below; sqrt and division are the correctly rounded ones), so thresholds decide as they do there.
// All kernels are HBM-bound: 20 B per pixel (stats, fp32 valid), 8 N + 8 + 4 B per pixel (loss forward, N predictions).
#include "oflow_internal.h"

#include <cmath>

#pragma clang fp contract(off)

namespace oflow {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4 * kThreads;  // pixels of one work unit: a (row, chunk) pair, 4 pixels per thread
constexpr int kSlots = 8;             // doubles per partial row / accumulator (include/oflow.h)
constexpr int kBackwardGrid = 2048;

struct FlowView {  // (B, 2, H, W) fp32, W stride 1; strides in elements
  const float* p;
  long long sb, sc, sh;
};
struct ValidView {  // (B, H, W), W stride 1; kind OFLOW_VALID_*
  const void* p;
  long long sb, sh;
};
struct PredArgs {  // sequence loss: the predictions, by value in the kernel arguments
  const float* p[OFLOW_MAX_PREDS];
  float* g[OFLOW_MAX_PREDS];  // backward: gradient destinations (nullptr: not wanted)
  float w[OFLOW_MAX_PREDS];
};

template <int VK>
__device__ __forceinline__ float valid_at(const void* v, long long i) {
  if (VK == OFLOW_VALID_F32) return static_cast<const float*>(v)[i];
  if (VK == OFLOW_VALID_U8) return static_cast<const unsigned char*>(v)[i] ? 1.f : 0.f;
  return 1.f;
}
// 4 consecutive values (i % 4 == 0 and the base suitably aligned: checked by the host)
template <int VK>
__device__ __forceinline__ void valid_at4(const void* v, long long i, float* out) {
  if (VK == OFLOW_VALID_F32) {
    const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(v) + i);
    out[0] = f.x, out[1] = f.y, out[2] = f.z, out[3] = f.w;
  } else if (VK == OFLOW_VALID_U8) {
    const unsigned u = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(v) + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = ((u >> (8 * k)) & 0xffu) ? 1.f : 0.f;
  } else {
    out[0] = out[1] = out[2] = out[3] = 1.f;
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// Sum of v[k] over the workgroup, k < NV: thread t < kSlots returns slot t's total (0 for t >= NV), others 0.
// Fixed order: xor butterfly inside each wave, then the waves in index order.
template <int NV>
__device__ __forceinline__ double block_sum(const double* v) {
  __shared__ double s[kThreads / 64][kSlots];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double t = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) s[wave][k] = t;
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < NV)
    for (int w = 0; w < kThreads / 64; ++w) t += s[w][threadIdx.x];
  return t;
}

// ------------------------------------------------------------------------------------------------ flow error stats
struct ErrAcc {
  double sum = 0.0;
  unsigned n = 0, nout = 0, c1 = 0, c3 = 0, c5 = 0;
};

// epe.py:62 (norm of the residual), f1.py:38-42 (target norm, the two strict thresholds, a true division), the
// `valid >= 0.5` selection of both updates and sequence_loss's `mag < max_flow` (raft.py:244)
__device__ __forceinline__ float err_pixel(ErrAcc& a, float p0, float p1, float t0, float t1, float v, float abs_t,
                                           float rel_t, float max_flow, int use_max) {
  const float dx = p0 - t0, dy = p1 - t1;
  const float epe = sqrtf(dx * dx + dy * dy);
  const float mag = sqrtf(t0 * t0 + t1 * t1);
  const bool keep = (v >= 0.5f) && (!use_max || mag < max_flow);
  if (keep) {
    a.sum += static_cast<double>(epe);
    a.n += 1u;
    a.nout += ((epe > abs_t) && (epe / mag > rel_t)) ? 1u : 0u;
    a.c1 += epe < 1.f ? 1u : 0u;
    a.c3 += epe < 3.f ? 1u : 0u;
    a.c5 += epe < 5.f ? 1u : 0u;
  }
  return epe;
}

// grid: min(units, OFLOW_FLOW_METRICS_PARTIALS) workgroups striding over the units = rows x chunks of kChunk pixels.
// VEC: 16-B loads (every row base 16-B aligned: host-checked), else coalesced dword loads.
template <int VK, bool VEC>
__global__ __launch_bounds__(kThreads) void flow_error_partial_kernel(FlowView pr, FlowView tg, ValidView va, long long H,
                                                                      long long W, long long chunks, long long units,
                                                                      float abs_t, float rel_t, float max_flow, int use_max,
                                                                      float* __restrict__ epe_map, int map_vec,
                                                                      double* __restrict__ partials) {
  ErrAcc a;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long row = u / chunks, x0 = (u - row * chunks) * kChunk;
    const long long b = row / H, y = row - b * H;
    const float* p0 = pr.p + b * pr.sb + y * pr.sh;
    const float* p1 = p0 + pr.sc;
    const float* t0 = tg.p + b * tg.sb + y * tg.sh;
    const float* t1 = t0 + tg.sc;
    const long long vo = b * va.sb + y * va.sh;
    float* m = epe_map ? epe_map + row * W : nullptr;
    if (VEC) {
      const long long x = x0 + 4 * threadIdx.x;
      if (x + 4 <= W) {
        const float4 a0 = *reinterpret_cast<const float4*>(p0 + x), a1 = *reinterpret_cast<const float4*>(p1 + x);
        const float4 b0 = *reinterpret_cast<const float4*>(t0 + x), b1 = *reinterpret_cast<const float4*>(t1 + x);
        float v[4], e[4];
        valid_at4<VK>(va.p, vo + x, v);
        e[0] = err_pixel(a, a0.x, a1.x, b0.x, b1.x, v[0], abs_t, rel_t, max_flow, use_max);
        e[1] = err_pixel(a, a0.y, a1.y, b0.y, b1.y, v[1], abs_t, rel_t, max_flow, use_max);
        e[2] = err_pixel(a, a0.z, a1.z, b0.z, b1.z, v[2], abs_t, rel_t, max_flow, use_max);
        e[3] = err_pixel(a, a0.w, a1.w, b0.w, b1.w, v[3], abs_t, rel_t, max_flow, use_max);
        if (m) {
          if (map_vec) {
            *reinterpret_cast<float4*>(m + x) = make_float4(e[0], e[1], e[2], e[3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[x + k] = e[k];
          }
        }
      } else {
        for (long long xx = x; xx < W; ++xx) {  // the row's last, partial group
          const float e = err_pixel(a, p0[xx], p1[xx], t0[xx], t1[xx], valid_at<VK>(va.p, vo + xx), abs_t, rel_t,
                                    max_flow, use_max);
          if (m) m[xx] = e;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long xx = x0 + threadIdx.x + k * kThreads;
        if (xx < W) {
          const float e = err_pixel(a, p0[xx], p1[xx], t0[xx], t1[xx], valid_at<VK>(va.p, vo + xx), abs_t, rel_t,
                                    max_flow, use_max);
          if (m) m[xx] = e;
        }
      }
    }
  }
  const double v[6] = {a.sum,
                       static_cast<double>(a.n),
                       static_cast<double>(a.nout),
                       static_cast<double>(a.c1),
                       static_cast<double>(a.c3),
                       static_cast<double>(a.c5)};
  const double t = block_sum<6>(v);
  if (threadIdx.x < kSlots) partials[static_cast<long long>(blockIdx.x) * kSlots + threadIdx.x] = t;
}

// one workgroup: thread t sums the partial rows t, t + 256, ... in index order, then block_sum's fixed order
__device__ __forceinline__ double sum_partials(const double* __restrict__ partials, int nparts) {
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += partials[static_cast<long long>(i) * kSlots + k];
  }
  return block_sum<6>(v);
}

__global__ __launch_bounds__(kThreads) void flow_error_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                       double* __restrict__ accum) {
  const double t = sum_partials(partials, nparts);
  if (threadIdx.x < 6) accum[threadIdx.x] += t;
}

// ------------------------------------------------------------------------------------------------ sequence loss
struct LossAcc {
  double loss = 0.0, sum_epe = 0.0;
  unsigned n = 0, c1 = 0, c3 = 0, c5 = 0;
};

// raft.py:243-244: the mask as 0 / 1 (it multiplies the loss terms: `valid[:, None] * i_loss`)
__device__ __forceinline__ float loss_mask(float t0, float t1, float v, float max_flow) {
  const float mag = sqrtf(t0 * t0 + t1 * t1);
  return ((v >= 0.5f) && (mag < max_flow)) ? 1.f : 0.f;
}

// raft.py:246-252 for one pixel of prediction i: w_i * mask * (|dx| + |dy|) into the fp64 sum, and for the last
// prediction the end-point error's counts over the masked pixels
__device__ __forceinline__ void loss_pixel(LossAcc& a, float p0, float p1, float t0, float t1, float m, float w,
                                           bool last) {
  const float dx = p0 - t0, dy = p1 - t1;
  const double l = static_cast<double>(m * fabsf(dx)) + static_cast<double>(m * fabsf(dy));
  a.loss += static_cast<double>(w) * l;
  if (last && m != 0.f) {
    const float epe = sqrtf(dx * dx + dy * dy);
    a.sum_epe += static_cast<double>(epe);
    a.n += 1u;
    a.c1 += epe < 1.f ? 1u : 0u;
    a.c3 += epe < 3.f ? 1u : 0u;
    a.c5 += epe < 5.f ? 1u : 0u;
  }
}

// contiguous (B, 2, HW) tensors; units = B x chunks of kChunk pixels
template <int VK, bool VEC>
__global__ __launch_bounds__(kThreads) void sequence_loss_partial_kernel(PredArgs pa, int n, const float* __restrict__ gt,
                                                                         const void* __restrict__ valid, long long HW,
                                                                         long long chunks, long long units, float max_flow,
                                                                         double* __restrict__ partials) {
  LossAcc a;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long b = u / chunks, x0 = (u - b * chunks) * kChunk;
    const long long base = b * 2 * HW, vbase = b * HW;
    const long long x = x0 + 4 * threadIdx.x;
    if (VEC && x + 4 <= HW) {
      const float4 g0 = *reinterpret_cast<const float4*>(gt + base + x);
      const float4 g1 = *reinterpret_cast<const float4*>(gt + base + HW + x);
      float v[4];
      valid_at4<VK>(valid, vbase + x, v);
      const float m0 = loss_mask(g0.x, g1.x, v[0], max_flow), m1 = loss_mask(g0.y, g1.y, v[1], max_flow);
      const float m2 = loss_mask(g0.z, g1.z, v[2], max_flow), m3 = loss_mask(g0.w, g1.w, v[3], max_flow);
#pragma unroll 4
      for (int i = 0; i < n; ++i) {
        const float4 q0 = *reinterpret_cast<const float4*>(pa.p[i] + base + x);
        const float4 q1 = *reinterpret_cast<const float4*>(pa.p[i] + base + HW + x);
        const float w = pa.w[i];
        const bool last = i == n - 1;
        loss_pixel(a, q0.x, q1.x, g0.x, g1.x, m0, w, last);
        loss_pixel(a, q0.y, q1.y, g0.y, g1.y, m1, w, last);
        loss_pixel(a, q0.z, q1.z, g0.z, g1.z, m2, w, last);
        loss_pixel(a, q0.w, q1.w, g0.w, g1.w, m3, w, last);
      }
    } else if (!VEC) {  // (VEC needs HW % 4 == 0: a group is whole or outside)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long xx = x0 + threadIdx.x + k * kThreads;
        if (xx < HW) {
          const float t0 = gt[base + xx], t1 = gt[base + HW + xx];
          const float m = loss_mask(t0, t1, valid_at<VK>(valid, vbase + xx), max_flow);
          for (int i = 0; i < n; ++i)
            loss_pixel(a, pa.p[i][base + xx], pa.p[i][base + HW + xx], t0, t1, m, pa.w[i], i == n - 1);
        }
      }
    }
  }
  const double v[6] = {a.loss,
                       static_cast<double>(a.n),
                       static_cast<double>(a.c1),
                       static_cast<double>(a.c3),
                       static_cast<double>(a.c5),
                       a.sum_epe};
  const double t = block_sum<6>(v);
  if (threadIdx.x < kSlots) partials[static_cast<long long>(blockIdx.x) * kSlots + threadIdx.x] = t;
}

// loss = sum / (2 B H W) (the mean of raft.py:249 over (B, 2, H, W), weights already inside the sum) as fp32;
// stats = {n_valid, n(epe<1), n(epe<3), n(epe<5), sum epe, the fp64 loss sum, 0, 0}
__global__ __launch_bounds__(kThreads) void sequence_loss_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                          double elements, float* __restrict__ loss,
                                                                          double* __restrict__ stats) {
  __shared__ double tot[kSlots];
  const double t = sum_partials(partials, nparts);
  if (threadIdx.x < kSlots) tot[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = static_cast<float>(tot[0] / elements);
    stats[0] = tot[1];
    stats[1] = tot[2];
    stats[2] = tot[3];
    stats[3] = tot[4];
    stats[4] = tot[5];
    stats[5] = tot[0];
    stats[6] = 0.0;
    stats[7] = 0.0;
  }
}

// autograd of raft.py:246-249 for one element: c = (gout * w_i) / (2BHW) (the mean's backward after the weight's),
// times the 0 / 1 mask (the product's), times sgn(d) with sgn(0) = sgn(NaN) = 0 (ATen's abs backward)
__device__ __forceinline__ float loss_grad(float c, float m, float p, float t) {
  const float d = p - t;
  const float s = static_cast<float>(d > 0.f) - static_cast<float>(d < 0.f);
  return (c * m) * s;
}

template <int VK, bool VEC>
__global__ __launch_bounds__(kThreads) void sequence_loss_backward_kernel(PredArgs pa, int n, const float* __restrict__ gt,
                                                                          const void* __restrict__ valid,
                                                                          const float* __restrict__ gout, long long HW,
                                                                          long long chunks, long long units, float max_flow,
                                                                          float elements) {
  const float go = gout[0];
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long b = u / chunks, x0 = (u - b * chunks) * kChunk;
    const long long base = b * 2 * HW, vbase = b * HW;
    if (VEC) {
      const long long x = x0 + 4 * threadIdx.x;
      if (x + 4 > HW) continue;  // VEC needs HW % 4 == 0: a group is whole or outside
      const float4 g0 = *reinterpret_cast<const float4*>(gt + base + x);
      const float4 g1 = *reinterpret_cast<const float4*>(gt + base + HW + x);
      float v[4];
      valid_at4<VK>(valid, vbase + x, v);
      const float m0 = loss_mask(g0.x, g1.x, v[0], max_flow), m1 = loss_mask(g0.y, g1.y, v[1], max_flow);
      const float m2 = loss_mask(g0.z, g1.z, v[2], max_flow), m3 = loss_mask(g0.w, g1.w, v[3], max_flow);
      for (int i = 0; i < n; ++i) {
        float* g = pa.g[i];
        if (!g) continue;
        const float c = (go * pa.w[i]) / elements;
        const float4 q0 = *reinterpret_cast<const float4*>(pa.p[i] + base + x);
        const float4 q1 = *reinterpret_cast<const float4*>(pa.p[i] + base + HW + x);
        *reinterpret_cast<float4*>(g + base + x) =
            make_float4(loss_grad(c, m0, q0.x, g0.x), loss_grad(c, m1, q0.y, g0.y), loss_grad(c, m2, q0.z, g0.z),
                        loss_grad(c, m3, q0.w, g0.w));
        *reinterpret_cast<float4*>(g + base + HW + x) =
            make_float4(loss_grad(c, m0, q1.x, g1.x), loss_grad(c, m1, q1.y, g1.y), loss_grad(c, m2, q1.z, g1.z),
                        loss_grad(c, m3, q1.w, g1.w));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long xx = x0 + threadIdx.x + k * kThreads;
        if (xx >= HW) continue;
        const float t0 = gt[base + xx], t1 = gt[base + HW + xx];
        const float m = loss_mask(t0, t1, valid_at<VK>(valid, vbase + xx), max_flow);
        for (int i = 0; i < n; ++i) {
          float* g = pa.g[i];
          if (!g) continue;
          const float c = (go * pa.w[i]) / elements;
          g[base + xx] = loss_grad(c, m, pa.p[i][base + xx], t0);
          g[base + HW + xx] = loss_grad(c, m, pa.p[i][base + HW + xx], t1);
        }
      }
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
inline bool mult4(long long v) { return v % 4 == 0; }

// kernel instance by (valid kind, vector path)
#define OFLOW_BY_VALID_KIND(KERNEL, kind, vec)                                             \
  ((kind) == OFLOW_VALID_F32 ? ((vec) ? KERNEL<OFLOW_VALID_F32, true> : KERNEL<OFLOW_VALID_F32, false>) \
   : (kind) == OFLOW_VALID_U8 ? ((vec) ? KERNEL<OFLOW_VALID_U8, true> : KERNEL<OFLOW_VALID_U8, false>) \
                              : ((vec) ? KERNEL<OFLOW_VALID_NONE, true> : KERNEL<OFLOW_VALID_NONE, false>))

// the sequence loss's shared argument checks; fills the launch geometry
int loss_args(int n_preds, const float* const* d_preds, const float* d_weights_host, const float* d_gt,
              const void* d_valid, int valid_kind, int B, int H, int W, PredArgs& pa, bool& vec, long long& HW,
              long long& chunks, long long& units) {
  if (!d_preds || !d_weights_host || !d_gt || !d_valid) return OFLOW_E_NULL;
  if (n_preds < 1 || n_preds > OFLOW_MAX_PREDS || B <= 0 || H <= 0 || W <= 0) return OFLOW_E_SHAPE;
  if (valid_kind != OFLOW_VALID_F32 && valid_kind != OFLOW_VALID_U8) return OFLOW_E_MODE;
  HW = static_cast<long long>(H) * W;
  vec = mult4(HW) && aligned(d_gt, 16) && aligned(d_valid, valid_kind == OFLOW_VALID_F32 ? 16 : 4);
  if (!aligned(d_gt, 4) || (valid_kind == OFLOW_VALID_F32 && !aligned(d_valid, 4))) return OFLOW_E_ALIGN;
  for (int i = 0; i < OFLOW_MAX_PREDS; ++i) {
    pa.p[i] = nullptr;
    pa.g[i] = nullptr;
    pa.w[i] = 0.f;
  }
  for (int i = 0; i < n_preds; ++i) {
    if (!d_preds[i]) return OFLOW_E_NULL;
    if (!aligned(d_preds[i], 4)) return OFLOW_E_ALIGN;
    vec = vec && aligned(d_preds[i], 16);
    pa.p[i] = d_preds[i];
    pa.w[i] = d_weights_host[i];
  }
  chunks = (HW + kChunk - 1) / kChunk;
  units = chunks * B;
  return OFLOW_OK;
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_flow_error_stats_f32(const float* d_pred, long long pred_sb, long long pred_sc, long long pred_sh,
                                          const float* d_target, long long target_sb, long long target_sc,
                                          long long target_sh, const void* d_valid, int valid_kind, long long valid_sb,
                                          long long valid_sh, int B, int H, int W, float abs_threshold,
                                          float rel_threshold, float max_flow, float* d_epe_map, double* d_workspace,
                                          double* d_accum, void* stream) {
  if (!d_pred || !d_target || !d_workspace || !d_accum) return OFLOW_E_NULL;
  if (valid_kind < OFLOW_VALID_NONE || valid_kind > OFLOW_VALID_U8) return OFLOW_E_MODE;
  if (valid_kind != OFLOW_VALID_NONE && !d_valid) return OFLOW_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0) return OFLOW_E_SHAPE;
  if (pred_sb < 0 || pred_sc < 0 || pred_sh < 0 || target_sb < 0 || target_sc < 0 || target_sh < 0 || valid_sb < 0 ||
      valid_sh < 0)
    return OFLOW_E_SHAPE;
  if (!aligned(d_pred, 4) || !aligned(d_target, 4) || !aligned(d_epe_map, 4) || !aligned(d_workspace, 8) ||
      !aligned(d_accum, 8) || (valid_kind == OFLOW_VALID_F32 && !aligned(d_valid, 4)))
    return OFLOW_E_ALIGN;
  FlowView pr{d_pred, B > 1 ? pred_sb : 0, pred_sc, H > 1 ? pred_sh : 0};
  FlowView tg{d_target, B > 1 ? target_sb : 0, target_sc, H > 1 ? target_sh : 0};
  ValidView va{valid_kind != OFLOW_VALID_NONE ? d_valid : nullptr, B > 1 ? valid_sb : 0, H > 1 ? valid_sh : 0};
  long long rows_h = H, width = W;
  // rows that follow each other without a gap in every tensor are one long row (contiguous inputs: H * W pixels)
  if (H > 1 && pr.sh == W && tg.sh == W && (valid_kind == OFLOW_VALID_NONE || va.sh == W)) {
    rows_h = 1;
    width = static_cast<long long>(H) * W;
    pr.sh = tg.sh = va.sh = 0;
  }
  const bool vec = aligned(pr.p, 16) && mult4(pr.sb) && mult4(pr.sc) && mult4(pr.sh) && aligned(tg.p, 16) &&
                   mult4(tg.sb) && mult4(tg.sc) && mult4(tg.sh) &&
                   (valid_kind == OFLOW_VALID_NONE ||
                    (aligned(va.p, valid_kind == OFLOW_VALID_F32 ? 16 : 4) && mult4(va.sb) && mult4(va.sh)));
  const int map_vec = d_epe_map && mult4(width) && aligned(d_epe_map, 16);
  const int use_max = max_flow > 0.f && std::isfinite(max_flow);
  const long long chunks = (width + kChunk - 1) / kChunk;
  const long long units = chunks * rows_h * B;
  const int grid = static_cast<int>(units < OFLOW_FLOW_METRICS_PARTIALS ? units : OFLOW_FLOW_METRICS_PARTIALS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto partial = OFLOW_BY_VALID_KIND(flow_error_partial_kernel, valid_kind, vec);
  hipLaunchKernelGGL(partial, dim3(grid), dim3(kThreads), 0, st, pr, tg, va, rows_h, width, chunks, units, abs_threshold, rel_threshold, max_flow, use_max,
                     d_epe_map, map_vec, d_workspace);
  int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(flow_error_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, grid, d_accum);
  return launch_status();
}

extern "C" int oflow_sequence_loss_f32(const float* const* d_preds, int n_preds, const float* weights,
                                       const float* d_flow_gt, const void* d_valid, int valid_kind, int B, int H, int W,
                                       float max_flow, double* d_workspace, float* d_loss, double* d_stats,
                                       void* stream) {
  if (!d_workspace || !d_loss || !d_stats) return OFLOW_E_NULL;
  PredArgs pa;
  bool vec;
  long long HW, chunks, units;
  const int st0 = loss_args(n_preds, d_preds, weights, d_flow_gt, d_valid, valid_kind, B, H, W, pa, vec, HW, chunks, units);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned(d_workspace, 8) || !aligned(d_stats, 8) || !aligned(d_loss, 4)) return OFLOW_E_ALIGN;
  const int grid = static_cast<int>(units < OFLOW_FLOW_METRICS_PARTIALS ? units : OFLOW_FLOW_METRICS_PARTIALS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto partial = OFLOW_BY_VALID_KIND(sequence_loss_partial_kernel, valid_kind, vec);
  hipLaunchKernelGGL(partial, dim3(grid), dim3(kThreads), 0, st, pa, n_preds, d_flow_gt, d_valid, HW, chunks, units, max_flow, d_workspace);
  int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(sequence_loss_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, grid,
                     2.0 * static_cast<double>(B) * static_cast<double>(HW), d_loss, d_stats);
  return launch_status();
}

extern "C" int oflow_sequence_loss_backward_f32(const float* d_grad_out, const float* const* d_preds,
                                                float* const* d_grads, int n_preds, const float* weights,
                                                const float* d_flow_gt, const void* d_valid, int valid_kind, int B,
                                                int H, int W, float max_flow, void* stream) {
  if (!d_grad_out || !d_grads) return OFLOW_E_NULL;
  PredArgs pa;
  bool vec;
  long long HW, chunks, units;
  const int st0 = loss_args(n_preds, d_preds, weights, d_flow_gt, d_valid, valid_kind, B, H, W, pa, vec, HW, chunks, units);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned(d_grad_out, 4)) return OFLOW_E_ALIGN;
  bool any = false;
  for (int i = 0; i < n_preds; ++i) {
    if (!aligned(d_grads[i], 4)) return OFLOW_E_ALIGN;
    vec = vec && aligned(d_grads[i], 16);
    pa.g[i] = d_grads[i];
    any = any || d_grads[i];
  }
  if (!any) return OFLOW_OK;
  const int grid = static_cast<int>(units < kBackwardGrid ? units : kBackwardGrid);
  const float elements = static_cast<float>(2.0 * static_cast<double>(B) * static_cast<double>(HW));
  auto backward = OFLOW_BY_VALID_KIND(sequence_loss_backward_kernel, valid_kind, vec);
  hipLaunchKernelGGL(backward, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), pa, n_preds, d_flow_gt, d_valid, d_grad_out, HW, chunks, units,
                     max_flow, elements);
  return launch_status();
}
