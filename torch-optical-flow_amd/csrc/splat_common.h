// What csrc/splat.hip and csrc/splat_backward.hip share: the per-image words at the end of the workspace and the kernels
// that fill them. Every reduction here ends in an integer atomicMax on a bit pattern, so it is order-independent.
#pragma once

#include "oflow_internal.h"

namespace oflow {

// the argument checks the forward and the backward share; OFLOW_OK or the first error (splat.hip)
int splat_check_shape(int B, int C, int H, int W, int mode);

namespace {

constexpr int kSplatThreads = 256;
constexpr int kHdrWords = 4;       // per image: [0] max |frame| bits, [1] metric maximum, [2] eN, [3] eD
constexpr int kRangeBlocks = 128;  // blocks per image of the range kernel, at most

inline long long splat_acc_bytes(int B, int C, int H, int W) { return 8LL * B * (C + 1) * H * W; }

// monotone map float -> unsigned (larger float, larger key), and back
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, 64)));
  return v;
}

// max over the block, then one integer atomicMax
__device__ __forceinline__ void block_max_to(unsigned v, unsigned* dst, unsigned* lds) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = lds[0];
    for (int k = 1; k < kSplatThreads / 64; ++k) m = max(m, lds[k]);
    atomicMax(dst, m);
  }
  __syncthreads();
}

// grid (blocks, B); hdr zeroed beforehand. frame: chw floats per image, or NULL (word 0 stays 0); metric: hw floats per
// image, or NULL. Word 1 becomes the order key of the metric's maximum (SOFT) or the bits of max |metric| (LINEAR).
__global__ __launch_bounds__(kSplatThreads) void splat_range_kernel(const float* __restrict__ frame,
                                                                    const float* __restrict__ metric, long long chw,
                                                                    int hw, int mode, unsigned* __restrict__ hdr) {
  __shared__ unsigned lds[kSplatThreads / 64];
  const int b = blockIdx.y;
  if (frame != nullptr) {
    const float* f = frame + static_cast<long long>(b) * chw;
    unsigned mf = 0u;  // the bits of a non-negative float order as the float does (NaN above everything)
    for (long long e = static_cast<long long>(blockIdx.x) * kSplatThreads + threadIdx.x; e < chw;
         e += static_cast<long long>(gridDim.x) * kSplatThreads)
      mf = max(mf, __float_as_uint(fabsf(f[e])));
    block_max_to(mf, hdr + b * kHdrWords, lds);
  }
  if (metric != nullptr) {
    const float* mt = metric + static_cast<long long>(b) * hw;
    unsigned mm = 0u;
    for (long long e = static_cast<long long>(blockIdx.x) * kSplatThreads + threadIdx.x; e < hw;
         e += static_cast<long long>(gridDim.x) * kSplatThreads)
      mm = max(mm, mode == OFLOW_SPLAT_SOFT ? order_key(mt[e]) : __float_as_uint(fabsf(mt[e])));
    block_max_to(mm, hdr + b * kHdrWords + 1, lds);
  }
}

// frexp exponent of a non-negative float (x < 2^e); 0 for zero, 129 for inf / NaN (unspecified outputs, a finite scale)
__device__ __forceinline__ int exponent_of(float x) {
  if (!(x < __builtin_inff())) return 129;
  int e = 0;
  frexpf(x, &e);
  return x == 0.f ? 0 : e;
}

// one thread per image: the exponents eN = eF + eM and eD = eM; for SOFT word 1 becomes the maximum as a float
__global__ void splat_exponent_kernel(unsigned* __restrict__ hdr, int B, int mode) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  unsigned* h = hdr + b * kHdrWords;
  const int eF = exponent_of(__uint_as_float(h[0]));
  int eM = 1;  // m <= 1 < 2^1: SUM, AVG, and SOFT (expf of a non-positive number)
  if (mode == OFLOW_SPLAT_LINEAR) eM = exponent_of(__uint_as_float(h[1]));
  if (mode == OFLOW_SPLAT_SOFT) h[1] = __float_as_uint(order_value(h[1]));
  h[2] = static_cast<unsigned>(eF + eM);
  h[3] = static_cast<unsigned>(eM);
}

// enqueue both on `s`: hdr (kHdrWords * B words, zeroed) -> maxima and exponents
inline void splat_launch_range(const float* d_frame, const float* d_metric, int B, long long chw, int hw, int mode,
                               unsigned* hdr, hipStream_t s) {
  const long long n = d_frame ? chw : hw;
  const long long want = (n + 8LL * kSplatThreads - 1) / (8LL * kSplatThreads);
  const unsigned blocks = static_cast<unsigned>(want < kRangeBlocks ? want : kRangeBlocks);
  hipLaunchKernelGGL(splat_range_kernel, dim3(blocks, B), dim3(kSplatThreads), 0, s, d_frame, d_metric, chw, hw, mode, hdr);
  hipLaunchKernelGGL(splat_exponent_kernel, dim3((B + kSplatThreads - 1) / kSplatThreads), dim3(kSplatThreads), 0, s,
                     hdr, B, mode);
}

}  // namespace
}  // namespace oflow
