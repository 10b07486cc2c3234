// The two building blocks of the norm-layer kernels (norm_backward.hip, batch_norm.hip): a workgroup-wide fixed-order
// sum of two fp64 values and the float4 / scalar sweep over a contiguous run of fp32 elements.
#pragma once

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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace oflow
