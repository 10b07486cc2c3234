// fb_consistency (gfx950): the forward-backward consistency check of two optical flows -- the occlusion mask of both
// frames, optionally with the squared residual -- as one streaming launch. The criterion is UnFlow's (Meister et al.,
// AAAI 2018): a pixel is occluded when the other direction's flow, sampled where this pixel lands, does not cancel this
// pixel's own flow: |a + o(p + a)|^2 > alpha * (|a|^2 + |o(p + a)|^2) + beta. include/oflow.h states the contract.
//
// Structure: both directions in one grid (blockIdx.z: 0 checks fw against bw, 1 the reverse), blockIdx.y the image. A
// thread owns kPix = 4 consecutive pixels of the image plane (row-major, so 4 consecutive pixels of a row except where
// the run wraps into the next row): its two flow components are one 16-byte load each, its four mask bytes one packed
// 32-bit store and its four residuals one 16-byte store, whenever the run is whole and its address is aligned (always
// when H*W is a multiple of 4; otherwise the images whose planes start off the alignment, and the last partial run of
// every plane, take scalar loads and byte stores). The eight taps per pixel are plain gathers from the other flow,
// which is L2-resident at these sizes and mostly hit in the same or a neighbouring line (flows are smooth). No LDS, no
// atomics, every output element written exactly once: the same bits on every run.
//
// Cost per pixel and direction: 8 B of own flow + 8 gathered taps read, 1 B (+ 4 B) written; ~40 VALU. The tap rate, not
// HBM, bounds it: measured, the kernel issues gathers at the rate the warp kernel does (DESIGN.md §4 has the times).
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;  // pixels per thread

struct FbArgs {
  const float* flow[2];  // [0] fw, [1] bw
  unsigned char* mask[2];
  float* err[2];  // may be NULL
  int H, W;
  float alpha, beta;
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One pixel of the contract: (u, v) at (i, j) against the other flow's planes ou / ov.
__device__ __forceinline__ void check_pixel(float u, float v, int i, int j, const float* __restrict__ ou,
                                            const float* __restrict__ ov, int H, int W, float alpha, float beta,
                                            unsigned& m, float& e) {
  const float px = static_cast<float>(j) + u, py = static_cast<float>(i) + v;
  const bool inside = px >= 0.f && px <= static_cast<float>(W - 1) && py >= 0.f && py <= static_cast<float>(H - 1);
  m = 1u;
  e = __builtin_inff();
  if (inside) {  // 0 <= floor(px) <= W - 1 and 0 <= floor(py) <= H - 1: every tap index is inside the plane
    const float fx = floorf(px), fy = floorf(py);
    const float wx = px - fx, wy = py - fy;
    const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const int r0 = y0 * W, r1 = y1 * W;
    const float a00 = ou[r0 + x0], a01 = ou[r0 + x1], a10 = ou[r1 + x0], a11 = ou[r1 + x1];
    const float b00 = ov[r0 + x0], b01 = ov[r0 + x1], b10 = ov[r1 + x0], b11 = ov[r1 + x1];
    const float at = a00 + wx * (a01 - a00), ab = a10 + wx * (a11 - a10);
    const float bt = b00 + wx * (b01 - b00), bb = b10 + wx * (b11 - b10);
    const float s0 = at + wy * (ab - at), s1 = bt + wy * (bb - bt);
    const float du = u + s0, dv = v + s1;
    e = du * du + dv * dv;
    const float thr = alpha * (u * u + v * v + s0 * s0 + s1 * s1) + beta;
    m = (e <= thr) ? 0u : 1u;  // NaN / inf in a tap: not <=, occluded
  }
}

__global__ __launch_bounds__(kThreads) void fb_consistency_kernel(FbArgs a) {
  const int H = a.H, W = a.W;
  const int HW = H * W;
  const int n0 = (blockIdx.x * kThreads + threadIdx.x) * kPix;  // first pixel of this thread's run (host: no overflow)
  if (n0 >= HW) return;
  const int d = blockIdx.z;
  const long long plane = static_cast<long long>(blockIdx.y) * HW;
  const float* au = a.flow[d] + 2 * plane;
  const float* av = au + HW;
  const float* ou = a.flow[1 - d] + 2 * plane;
  const float* ov = ou + HW;
  unsigned char* mk = a.mask[d] + plane;
  float* er = a.err[d] ? a.err[d] + plane : nullptr;
  const bool whole = n0 + kPix <= HW;

  float u[kPix], v[kPix];
  if (whole && aligned16(au + n0) && aligned16(av + n0)) {
    const float4 u4 = *reinterpret_cast<const float4*>(au + n0);
    const float4 v4 = *reinterpret_cast<const float4*>(av + n0);
    u[0] = u4.x, u[1] = u4.y, u[2] = u4.z, u[3] = u4.w;
    v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const bool in = n0 + k < HW;
      u[k] = in ? au[n0 + k] : 0.f;
      v[k] = in ? av[n0 + k] : 0.f;
    }
  }

  int i = n0 / W, j = n0 - i * W;
  unsigned m[kPix];
  float e[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    m[k] = 0u;
    e[k] = 0.f;
    if (n0 + k < HW) check_pixel(u[k], v[k], i, j, ou, ov, H, W, a.alpha, a.beta, m[k], e[k]);
    if (++j == W) {
      j = 0;
      ++i;
    }
  }

  if (whole && (reinterpret_cast<uintptr_t>(mk + n0) & 3) == 0) {
    *reinterpret_cast<unsigned*>(mk + n0) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k)
      if (n0 + k < HW) mk[n0 + k] = static_cast<unsigned char>(m[k]);
  }
  if (er) {
    if (whole && aligned16(er + n0)) {
      *reinterpret_cast<float4*>(er + n0) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int k = 0; k < kPix; ++k)
        if (n0 + k < HW) er[n0 + k] = e[k];
    }
  }
}

// [p, p + n) and [q, q + m) share a byte
inline bool overlaps(const void* p, long long n, const void* q, long long m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + static_cast<uintptr_t>(m) && b < a + static_cast<uintptr_t>(n);
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_fb_consistency_f32(const float* d_fw, const float* d_bw, int B, int H, int W, float alpha,
                                        float beta, unsigned char* d_mask_fw, unsigned char* d_mask_bw, float* d_err_fw,
                                        float* d_err_bw, void* stream) {
  if (!d_fw || !d_bw || !d_mask_fw) return OFLOW_E_NULL;
  if (d_err_bw && !d_mask_bw) return OFLOW_E_NULL;  // the reverse direction runs iff its mask is asked for
  if (B < 1 || H < 1 || W < 1 || B > 65535 || (long long)H * W > (1LL << 30)) return OFLOW_E_SHAPE;
  const long long px = (long long)B * H * W;
  const void* ins[2] = {d_fw, d_bw};
  const void* outs[4] = {d_mask_fw, d_mask_bw, d_err_fw, d_err_bw};
  const long long out_bytes[4] = {px, px, 4 * px, 4 * px};
  for (int o = 0; o < 4; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 2; ++i)
      if (overlaps(outs[o], out_bytes[o], ins[i], 8 * px)) return OFLOW_E_SHAPE;  // an output aliases an input
    for (int p = 0; p < o; ++p)
      if (outs[p] && overlaps(outs[o], out_bytes[o], outs[p], out_bytes[p])) return OFLOW_E_SHAPE;
  }
  if ((reinterpret_cast<uintptr_t>(d_fw) | reinterpret_cast<uintptr_t>(d_bw) | reinterpret_cast<uintptr_t>(d_err_fw) |
       reinterpret_cast<uintptr_t>(d_err_bw)) & 3)
    return OFLOW_E_ALIGN;
  FbArgs a;
  a.flow[0] = d_fw, a.flow[1] = d_bw;
  a.mask[0] = d_mask_fw, a.mask[1] = d_mask_bw;
  a.err[0] = d_err_fw, a.err[1] = d_err_bw;
  a.H = H, a.W = W;
  a.alpha = alpha, a.beta = beta;
  const int per_block = kThreads * kPix;
  const unsigned blocks = static_cast<unsigned>(((long long)H * W + per_block - 1) / per_block);
  hipLaunchKernelGGL(fb_consistency_kernel, dim3(blocks, B, d_mask_bw ? 2 : 1), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  return launch_status();
}
