// census_loss (gfx950): the ternary census loss of the unsupervised flow methods (UnFlow, Meister et al., AAAI 2018;
// UFlow, Jonschkowski et al., ECCV 2020; their published constants) over a patch x patch neighbourhood, forward and
// backward, each as one tiled launch. include/oflow.h states the contract.
//
// Forward: a workgroup of 256 threads owns a kTileW x kTileH = 64 x 8 tile of output pixels of one image, two pixels
// per thread (rows ly and ly + 4, so a wave reads 64 consecutive values of an LDS row: no bank conflict). It stages
// the two frames' channel sums (fp64, see stage_grey) with a halo of r = patch / 2 in LDS, adding the channels while
// staging, so the C-channel frames are read once (plus the halo: (8 + 2r)(64 + 2r) / 512 = 1.9 x at patch 7). LDS:
// 2 x 14 x 70 doubles = 15.3 KiB at patch 7, so LDS never limits occupancy (160 KiB per CU). Each thread evaluates
// its patch^2 - 1 pairs from LDS: the three grey differences of a pair in fp64, rounded once, then fp32 with
// IEEE sqrt and division (the torch composition's arithmetic, ternary_difference below included), the
// workgroup reduces (sum M rho, sum M) in fp64 -- per thread, __shfl_xor within the wave, LDS across the waves -- and
// writes one partial row into the caller's workspace; a one-workgroup finalize kernel adds the rows in index order.
// No atomics, no last-arriver, the grid depends on the shapes only: bit-identical from run to run.
//
// Backward: a pure gather over the same tiles. The gradient of g_k(q) is -sum_d A_k(q, d) + sum_d A_k(q - d, d), so a
// tile needs c(p) = grad * M / (sum M + 1e-6) * 0.4 (s + 0.01)^-0.6 with a halo of r and the grey planes with a halo of
// r around that. s comes from the forward's map (d_s_map) -- then the grey halo is r -- or is recomputed from a grey
// halo of 2r when d_s_map is NULL; the operator saves the map (DESIGN.md section 4 "losses" has the measurement).
// Every element of a requested gradient is written; nothing is accumulated in memory.
#include "oflow_internal.h"

#include <climits>
#include <cmath>

namespace oflow {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 8;  // output pixels of a workgroup: rows ly and ly + kTileH / 2 of each thread

struct CensusArgs {
  const float* frame[2];
  const void* mask;
  int B, C, H, W;
  int tiles_x, tiles_y;
  double grey_scale;  // 255 / (image_range * C)
};

template <int MK>
__device__ __forceinline__ float mask_at(const void* m, long long i) {
  if (MK == OFLOW_VALID_F32) return static_cast<const float*>(m)[i];
  if (MK == OFLOW_VALID_U8) return static_cast<const unsigned char*>(m)[i] ? 1.f : 0.f;
  return 1.f;
}

// The channel sums of tile (b, y0, x0) with a halo of HALO into g[2][LH * LW], in fp64 (exact for fp32 frames); 0 outside
// the image. The grey scale 255 / (image_range * C) is applied to the differences of these sums, which are formed in
// fp64 and rounded once: delta_0, delta_1 and delta_0 - delta_1, which would otherwise cancel between two similar frames.
template <int HALO>
__device__ __forceinline__ void stage_grey(const CensusArgs& a, int b, int y0, int x0, double* g) {
  constexpr int LH = kTileH + 2 * HALO, LW = kTileW + 2 * HALO;
  const long long plane = static_cast<long long>(a.H) * a.W;
  for (int i = threadIdx.x; i < LH * LW; i += kThreads) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gy = y0 - HALO + ly, gx = x0 - HALO + lx;
    double v0 = 0.0, v1 = 0.0;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const long long o = static_cast<long long>(b) * a.C * plane + static_cast<long long>(gy) * a.W + gx;
      for (int c = 0; c < a.C; ++c) {
        v0 += static_cast<double>(a.frame[0][o + c * plane]);
        v1 += static_cast<double>(a.frame[1][o + c * plane]);
      }
    }
    g[i] = v0;
    g[LH * LW + i] = v1;
  }
}

// t_0 - t_1 of one offset from the two grey differences and dd = delta_0 - delta_1, with r_k = 1 / sqrt(0.81 + delta_k^2). Where the differences
// have the same sign the ternaries saturate together and t_0 - t_1 would cancel to nothing in fp32 (both round to the
// same float once |delta| passes ~200 grey levels), so there it is formed as (t_0^2 - t_1^2) / (t_0 + t_1) with
// t_0^2 - t_1^2 = 0.81 (delta_0 - delta_1)(delta_0 + delta_1) (r_0 r_1)^2: the same number without the cancellation.
__device__ __forceinline__ float ternary_difference(float d0, float d1, float dd, float& r0, float& r1) {
  r0 = 1.f / sqrtf(0.81f + d0 * d0);
  r1 = 1.f / sqrtf(0.81f + d1 * d1);
  const float t0 = d0 * r0, t1 = d1 * r1, rr = r0 * r1;
  const bool same = (d0 > 0.f && d1 > 0.f) || (d0 < 0.f && d1 < 0.f);
  return same ? (0.81f * dd) * (d0 + d1) * (rr * rr) / (t0 + t1) : t0 - t1;
}

// the scaled differences of one offset from the channel sums of the neighbour (n0, n1) and the centre (c0, c1)
__device__ __forceinline__ void grey_differences(double n0, double n1, double c0, double c1, double scale, float& d0,
                                                 float& d1, float& dd) {
  const double e0 = n0 - c0, e1 = n1 - c1;
  d0 = static_cast<float>(e0 * scale);
  d1 = static_cast<float>(e1 * scale);
  dd = static_cast<float>((e0 - e1) * scale);
}

// s of the pixel at (cy, cx) of the LDS planes g0, g1 (row stride LW); every neighbour is inside the planes
template <int P>
__device__ __forceinline__ float census_s(const double* g0, const double* g1, int LW, int cy, int cx, double scale) {
  constexpr int R = P / 2;
  const double c0 = g0[cy * LW + cx], c1 = g1[cy * LW + cx];
  float s = 0.f;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int o = (cy + dy) * LW + cx + dx;
      float d0, d1, dd, r0, r1;
      grey_differences(g0[o], g1[o], c0, c1, scale, d0, d1, dd);
      const float df = ternary_difference(d0, d1, dd, r0, r1), e = df * df;
      s += e / (0.1f + e);
    }
  }
  return s;
}

__device__ __forceinline__ void tile_of(const CensusArgs& a, int& b, int& y0, int& x0) {
  const int t = blockIdx.x;
  const int per_image = a.tiles_x * a.tiles_y;
  b = t / per_image;
  const int r = t - b * per_image;
  const int ty = r / a.tiles_x;
  y0 = ty * kTileH;
  x0 = (r - ty * a.tiles_x) * kTileW;
}

template <int P, int MK>
__global__ __launch_bounds__(kThreads) void census_forward_kernel(CensusArgs a, float* __restrict__ s_map,
                                                                  double* __restrict__ partials) {
  constexpr int R = P / 2, LH = kTileH + 2 * R, LW = kTileW + 2 * R;
  __shared__ double g[2 * LH * LW];
  int b, y0, x0;
  tile_of(a, b, y0, x0);
  stage_grey<R>(a, b, y0, x0, g);
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  double sum_rho = 0.0, sum_m = 0.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ty = ly + k * (kTileH / 2);
    const int py = y0 + ty, px = x0 + lx;
    if (py < a.H && px < a.W) {
      const bool interior = py >= R && py < a.H - R && px >= R && px < a.W - R;
      const long long o = (static_cast<long long>(b) * a.H + py) * a.W + px;
      float s = 0.f;
      if (interior) {
        s = census_s<P>(g, g + LH * LW, LW, ty + R, lx + R, a.grey_scale);
        const float m = mask_at<MK>(a.mask, o);
        sum_rho += static_cast<double>(m * powf(s + 0.01f, 0.4f));
        sum_m += static_cast<double>(m);
      }
      if (s_map) s_map[o] = s;
    }
  }
  block_sum2_f64(sum_rho, sum_m);
  if (threadIdx.x == 0) {
    partials[2LL * blockIdx.x] = sum_rho;
    partials[2LL * blockIdx.x + 1] = sum_m;
  }
}

// one workgroup: thread t adds the rows t, t + 256, ... in index order, then block_sum2_f64's fixed order
__global__ __launch_bounds__(kThreads) void census_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                   float* __restrict__ loss, double* __restrict__ sum_m_out) {
  double sr = 0.0, sm = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) {
    sr += partials[2LL * i];
    sm += partials[2LL * i + 1];
  }
  block_sum2_f64(sr, sm);
  if (threadIdx.x == 0) {
    loss[0] = static_cast<float>(sr / (sm + 1e-6));
    sum_m_out[0] = sm;
  }
}

// one pair of the backward: with delta_k = the neighbour's grey (n_k) minus the centre's (c_k), the derivatives of e / (0.1 + e)
// with respect to delta_0 and delta_1 (the centre's factor c is applied by the caller)
__device__ __forceinline__ void pair_grad(double n0, double n1, double c0, double c1, double scale, float& a0, float& a1) {
  float d0, d1, dd, r0, r1;
  grey_differences(n0, n1, c0, c1, scale, d0, d1, dd);
  const float df = ternary_difference(d0, d1, dd, r0, r1), e = df * df;
  const float q = 0.1f + e;
  const float w = (0.2f * df) / (q * q);
  a0 = w * (0.81f * (r0 * r0 * r0));
  a1 = -w * (0.81f * (r1 * r1 * r1));
}

template <int P, int MK, bool RECOMPUTE>
__global__ __launch_bounds__(kThreads) void census_backward_kernel(CensusArgs a, const float* __restrict__ grad_loss,
                                                                   const double* __restrict__ sum_m,
                                                                   const float* __restrict__ s_map, float* __restrict__ grad0,
                                                                   float* __restrict__ grad1) {
  constexpr int R = P / 2;
  constexpr int GH = RECOMPUTE ? 2 * R : R;  // the grey planes' halo
  constexpr int LH = kTileH + 2 * GH, LW = kTileW + 2 * GH;
  constexpr int CH = kTileH + 2 * R, CW = kTileW + 2 * R;
  __shared__ double g[2 * LH * LW];
  __shared__ float cs[CH * CW];
  int b, y0, x0;
  tile_of(a, b, y0, x0);
  stage_grey<GH>(a, b, y0, x0, g);
  if (RECOMPUTE) __syncthreads();
  const double* g0 = g;
  const double* g1 = g + LH * LW;
  const float scale = static_cast<float>(static_cast<double>(grad_loss[0]) / (sum_m[0] + 1e-6));
  for (int i = threadIdx.x; i < CH * CW; i += kThreads) {
    const int ly = i / CW, lx = i - ly * CW;
    const int gy = y0 - R + ly, gx = x0 - R + lx;
    float c = 0.f;
    if (gy >= R && gy < a.H - R && gx >= R && gx < a.W - R) {  // interior (so inside the image)
      const long long o = (static_cast<long long>(b) * a.H + gy) * a.W + gx;
      const float s = RECOMPUTE ? census_s<P>(g0, g1, LW, ly + GH - R, lx + GH - R, a.grey_scale) : s_map[o];
      c = (scale * mask_at<MK>(a.mask, o)) * (0.4f * powf(s + 0.01f, -0.6f));
    }
    cs[i] = c;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const long long plane = static_cast<long long>(a.H) * a.W;
  for (int k = 0; k < 2; ++k) {
    const int ty = ly + k * (kTileH / 2);
    const int py = y0 + ty, px = x0 + lx;
    if (py >= a.H || px >= a.W) continue;
    const int gq = (ty + GH) * LW + lx + GH, cq = (ty + R) * CW + lx + R;
    const double q0 = g0[gq], q1 = g1[gq];
    const float c_here = cs[cq];
    float gg0 = 0.f, gg1 = 0.f;
#pragma unroll 1  // (rows rolled: fully unrolled, the hoisted LDS reads take all 256 VGPRs and leave one wave per SIMD)
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        if (dy == 0 && dx == 0) continue;
        float a0, a1;
        // A(q, d): q is the centre, q + d the neighbour
        const int on = gq + dy * LW + dx;
        pair_grad(g0[on], g1[on], q0, q1, a.grey_scale, a0, a1);
        gg0 -= c_here * a0;
        gg1 -= c_here * a1;
        // A(q - d, d): q - d is the centre, q the neighbour
        const int oc = gq - dy * LW - dx;
        pair_grad(q0, q1, g0[oc], g1[oc], a.grey_scale, a0, a1);
        const float c_there = cs[cq - dy * CW - dx];
        gg0 += c_there * a0;
        gg1 += c_there * a1;
      }
    }
    gg0 *= static_cast<float>(a.grey_scale);
    gg1 *= static_cast<float>(a.grey_scale);
    const long long o = static_cast<long long>(b) * a.C * plane + static_cast<long long>(py) * a.W + px;
    for (int c = 0; c < a.C; ++c) {
      if (grad0) grad0[o + c * plane] = gg0;
      if (grad1) grad1[o + c * plane] = gg1;
    }
  }
}

// tiles of one launch, 0 when the shape is outside the kernels' range
long long census_tiles(int B, int H, int W, int& tiles_x, int& tiles_y) {
  if (B < 1 || H < 1 || W < 1 || B > 65535 || static_cast<long long>(H) * W > (1LL << 28)) return 0;
  tiles_x = (W + kTileW - 1) / kTileW;
  tiles_y = (H + kTileH - 1) / kTileH;
  const long long n = static_cast<long long>(B) * tiles_x * tiles_y;
  return n <= INT_MAX ? n : 0;
}

int census_args(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B, int C, int H,
                int W, int patch, float image_range, CensusArgs& a, long long& tiles) {
  if (!d_frame0 || !d_frame1) return OFLOW_E_NULL;
  if (mask_kind < OFLOW_VALID_NONE || mask_kind > OFLOW_VALID_U8) return OFLOW_E_MODE;
  if (mask_kind != OFLOW_VALID_NONE && !d_mask) return OFLOW_E_NULL;
  if (patch != 3 && patch != 5 && patch != 7) return OFLOW_E_MODE;
  tiles = census_tiles(B, H, W, a.tiles_x, a.tiles_y);
  if (tiles == 0 || C < 1 || !(image_range > 0.f) || !std::isfinite(image_range)) return OFLOW_E_SHAPE;
  if (!aligned_to(d_frame0, 4) || !aligned_to(d_frame1, 4) ||
      (mask_kind == OFLOW_VALID_F32 && !aligned_to(d_mask, 4)))
    return OFLOW_E_ALIGN;
  a.frame[0] = d_frame0, a.frame[1] = d_frame1;
  a.mask = mask_kind != OFLOW_VALID_NONE ? d_mask : nullptr;
  a.B = B, a.C = C, a.H = H, a.W = W;
  a.grey_scale = 255.0 / (static_cast<double>(image_range) * C);
  return OFLOW_OK;
}

// kernel instances by (patch, mask kind)
template <int P>
auto forward_kernel_of(int kind) {
  return kind == OFLOW_VALID_F32  ? census_forward_kernel<P, OFLOW_VALID_F32>
         : kind == OFLOW_VALID_U8 ? census_forward_kernel<P, OFLOW_VALID_U8>
                                  : census_forward_kernel<P, OFLOW_VALID_NONE>;
}
template <int P, bool RECOMPUTE>
auto backward_kernel_of(int kind) {
  return kind == OFLOW_VALID_F32  ? census_backward_kernel<P, OFLOW_VALID_F32, RECOMPUTE>
         : kind == OFLOW_VALID_U8 ? census_backward_kernel<P, OFLOW_VALID_U8, RECOMPUTE>
                                  : census_backward_kernel<P, OFLOW_VALID_NONE, RECOMPUTE>;
}
template <bool RECOMPUTE>
auto backward_kernel_of(int patch, int kind) {
  return patch == 7   ? backward_kernel_of<7, RECOMPUTE>(kind)
         : patch == 5 ? backward_kernel_of<5, RECOMPUTE>(kind)
                      : backward_kernel_of<3, RECOMPUTE>(kind);
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" long long oflow_census_loss_workspace_bytes(int B, int H, int W) {
  int tx, ty;
  return 16 * census_tiles(B, H, W, tx, ty);
}

extern "C" int oflow_census_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind,
                                     int B, int C, int H, int W, int patch, float image_range, float* d_s_map,
                                     double* d_workspace, float* d_loss, double* d_sum_m, void* stream) {
  if (!d_workspace || !d_loss || !d_sum_m) return OFLOW_E_NULL;
  CensusArgs a;
  long long tiles;
  const int st0 = census_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, patch, image_range, a, tiles);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_s_map, 4) || !aligned_to(d_workspace, 8) || !aligned_to(d_loss, 4) || !aligned_to(d_sum_m, 8))
    return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto kernel = patch == 7   ? forward_kernel_of<7>(mask_kind)
                : patch == 5 ? forward_kernel_of<5>(mask_kind)
                             : forward_kernel_of<3>(mask_kind);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, st, a, d_s_map, d_workspace);
  const int status = launch_status();
  if (status != OFLOW_OK) return status;
  hipLaunchKernelGGL(census_finalize_kernel, dim3(1), dim3(kThreads), 0, st, d_workspace, static_cast<int>(tiles), d_loss,
                     d_sum_m);
  return launch_status();
}

extern "C" int oflow_census_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                              const void* d_mask, int mask_kind, const float* d_s_map,
                                              const double* d_sum_m, int B, int C, int H, int W, int patch,
                                              float image_range, float* d_grad_frame0, float* d_grad_frame1,
                                              void* stream) {
  if (!d_grad_loss || !d_sum_m || (!d_grad_frame0 && !d_grad_frame1)) return OFLOW_E_NULL;
  CensusArgs a;
  long long tiles;
  const int st0 = census_args(d_frame0, d_frame1, d_mask, mask_kind, B, C, H, W, patch, image_range, a, tiles);
  if (st0 != OFLOW_OK) return st0;
  if (!aligned_to(d_grad_loss, 4) || !aligned_to(d_s_map, 4) || !aligned_to(d_sum_m, 8) ||
      !aligned_to(d_grad_frame0, 4) || !aligned_to(d_grad_frame1, 4))
    return OFLOW_E_ALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto kernel = d_s_map ? backward_kernel_of<false>(patch, mask_kind) : backward_kernel_of<true>(patch, mask_kind);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, st, a,
                     d_grad_loss, d_sum_m, d_s_map, d_grad_frame0, d_grad_frame1);
  return launch_status();
}
