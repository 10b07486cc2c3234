// Backward of the convex upsampling (gfx950): the autograd transpose of csrc/upsample.hip, so that a training step
// (raft.py:149-175) differentiates RAFT.upsample_flow (raft.py:73-85) through one streaming pass instead of the ATen
// composition's softmax / unfold / broadcast-multiply / sum backward passes over the 576-channel mask.
//
// With F_k(c, y, x) = 8 * flow[n, c, y + k/3 - 1, x + k%3 - 1] (zero outside the grid),
// w_k(i, j, y, x) = softmax_k(mask[n, k*64 + i*8 + j, y, x]), g_c = grad_out[n, c, 8y + i, 8x + j] and
// a_k = sum_c g_c * F_k(c):
//   grad_mask[n, k*64 + i*8 + j, y, x] = w_k * (a_k - sum_k' w_k' * a_k')
//   S_k(c, y, x)                       = sum_{i, j} w_k * g_c
//   grad_flow[n, c, y', x']            = 8 * sum_k S_k(c, y' - (k/3 - 1), x' - (k%3 - 1))   (source pixel inside the grid)
// The softmax is recomputed from the mask; nothing but flow and mask is kept from the forward.
//
// Kernel 1 has the forward's shape: one workgroup = one low-res row segment of 32 pixels, looping over the 8 sub-pixel
// rows i. The 9 x 8 x 32 mask values of row i come in as 72 coalesced 128-B rows (lanes along x) through LDS and are
// consumed with lanes along (x, j), the mapping in which grad_out's rows (256 consecutive floats per channel) are read
// directly; the mask gradients go back through the same LDS tile and leave as 72 coalesced rows. Each lane keeps the 18
// sums S_k(c) of its (x, j) over i; the 8 j lanes of a pixel are then folded by a fixed xor tree and the segment's
// 18 x 32 sums are staged as rows of the (B, 18, H, W) scratch (row c*9 + k). Kernel 2 gathers the nine taps of every
// flow gradient from the scratch in the fixed order k = 0..8: no atomics, every output element written exactly once.
// Bound: HBM, (576 read + 576 written + 2*64) * 4 B per low-res pixel + 18 floats of scratch written and read.
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kUX = 32;       // low-res pixels per workgroup
constexpr int kMP = kUX + 4;  // mask tile pitch: the (x, j) lanes of a 32-lane group (4 x, 8 j) fall on 32 distinct banks

template <bool MASK, bool FLOW>
__global__ __launch_bounds__(256) void convex_upsample_backward_kernel(const float* __restrict__ gout,
                                                                       const float* __restrict__ flow,
                                                                       const float* __restrict__ mask, int H, int W,
                                                                       float* __restrict__ gmask,
                                                                       float* __restrict__ scratch) {
  __shared__ float sM[9][8][kMP];
  __shared__ float sF[2][3][kUX + 2];
  __shared__ float sS[18][kUX];
  const int tid = threadIdx.x;
  const int xb = blockIdx.x, y = blockIdx.y, n = blockIdx.z;
  const int x0 = xb * kUX;
  const long long HW = (long long)H * W;
  const float* fl = flow + (long long)n * 2 * HW;
  const long long mrow = (long long)n * 576 * HW + (long long)y * W;
  const float* mk = mask + mrow;
  // 8 * flow on the 3 x (32 + 2) neighbourhood, zeros outside (unfold's padding)
  for (int e = tid; e < 2 * 3 * (kUX + 2); e += 256) {
    const int c = e / (3 * (kUX + 2)), rem = e - c * 3 * (kUX + 2);
    const int dy = rem / (kUX + 2), dx = rem - dy * (kUX + 2);
    const int yy = y + dy - 1, xx = x0 + dx - 1;
    float v = 0.f;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = 8.0f * fl[c * HW + (long long)yy * W + xx];
    sF[c][dy][dx] = v;
  }
  // sub-pixel mapping: lane -> (x, j) with j fastest: 256 consecutive grad_out floats per channel row
  const int xo = tid >> 3, j = tid & 7;
  const bool live = x0 + xo < W;
  const long long W8 = 8LL * W, H8W8 = 64LL * HW;
  float acc[9][2];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k][0] = acc[k][1] = 0.f;
  for (int i = 0; i < 8; ++i) {
    __syncthreads();  // sF ready (i = 0) / row i-1's gradient rows have left the tile
    // 9 k x 8 j rows of 32 x: lanes along x
    for (int e = tid; e < 9 * 8 * kUX; e += 256) {
      const int row = e / kUX, xl = e - row * kUX;
      const int k = row >> 3, jj = row & 7;
      float v = 0.f;
      if (x0 + xl < W) v = mk[(long long)(k * 64 + i * 8 + jj) * HW + x0 + xl];
      sM[k][jj][xl] = v;
    }
    float g0 = 0.f, g1 = 0.f;  // (a lane past W: zero gradient, so it adds nothing below)
    if (live) {
      const float* gp = gout + (long long)n * 2 * H8W8 + (long long)(8 * y + i) * W8 + 8LL * (x0 + xo) + j;
      g0 = gp[0];
      g1 = gp[H8W8];
    }
    __syncthreads();
    float m[9], a[9];
    float mx = sM[0][j][xo];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      m[k] = sM[k][j][xo];
      mx = fmaxf(mx, m[k]);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      m[k] = expf(m[k] - mx);
      s += m[k];
    }
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float w = m[k] / s;
      const int dy = k / 3, dx = k % 3;
      a[k] = g0 * sF[0][dy][xo + dx] + g1 * sF[1][dy][xo + dx];
      dot += w * a[k];
      m[k] = w;
      if (FLOW) {
        acc[k][0] += w * g0;
        acc[k][1] += w * g1;
      }
    }
    if (MASK) {
      // each (k, j, x) element of the tile is read and rewritten by the one lane that owns it
#pragma unroll
      for (int k = 0; k < 9; ++k) sM[k][j][xo] = m[k] * (a[k] - dot);
      __syncthreads();
      for (int e = tid; e < 9 * 8 * kUX; e += 256) {
        const int row = e / kUX, xl = e - row * kUX;
        const int k = row >> 3, jj = row & 7;
        if (x0 + xl < W) gmask[mrow + (long long)(k * 64 + i * 8 + jj) * HW + x0 + xl] = sM[k][jj][xl];
      }
    }
  }
  if (FLOW) {
    // fold the 8 j lanes of each pixel (lanes 8 x .. 8 x + 7 of one wave): fixed xor tree, the same in every run
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float v = acc[k][c];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        if (j == 0) sS[c * 9 + k][xo] = v;
      }
    }
    __syncthreads();
    float* sc = scratch + (long long)n * 18 * HW + (long long)y * W;
    for (int e = tid; e < 18 * kUX; e += 256) {
      const int row = e / kUX, xl = e - row * kUX;
      if (x0 + xl < W) sc[(long long)row * HW + x0 + xl] = sS[row][xl];
    }
  }
}

// grad_flow[n, c, y, x] = 8 * sum_k S[n, c*9 + k, y - (k/3 - 1), x - (k%3 - 1)] over the source pixels inside the grid
__global__ __launch_bounds__(64) void convex_upsample_flow_grad_kernel(const float* __restrict__ scratch, int H, int W,
                                                                       float* __restrict__ gflow) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= W) return;
  const long long HW = (long long)H * W;
  const float* sc = scratch + (long long)n * 18 * HW;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int ys = y - (k / 3 - 1), xs = x - (k % 3 - 1);
      if (ys >= 0 && ys < H && xs >= 0 && xs < W) s += sc[(long long)(c * 9 + k) * HW + (long long)ys * W + xs];
    }
    gflow[((long long)n * 2 + c) * HW + (long long)y * W + x] = 8.0f * s;
  }
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_convex_upsample_backward_f32(const float* d_grad_out, const float* d_flow, const float* d_mask, int B,
                                                  int H, int W, float* d_grad_flow, float* d_grad_mask, float* d_scratch,
                                                  void* stream) {
  if (!d_grad_out || !d_flow || !d_mask || (!d_grad_flow && !d_grad_mask) || (d_grad_flow && !d_scratch))
    return OFLOW_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535) return OFLOW_E_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dim3 grid((W + kUX - 1) / kUX, H, B);
  if (d_grad_flow && d_grad_mask)
    hipLaunchKernelGGL((convex_upsample_backward_kernel<true, true>), grid, dim3(256), 0, st, d_grad_out, d_flow, d_mask,
                       H, W, d_grad_mask, d_scratch);
  else if (d_grad_mask)
    hipLaunchKernelGGL((convex_upsample_backward_kernel<true, false>), grid, dim3(256), 0, st, d_grad_out, d_flow, d_mask,
                       H, W, d_grad_mask, d_scratch);
  else
    hipLaunchKernelGGL((convex_upsample_backward_kernel<false, true>), grid, dim3(256), 0, st, d_grad_out, d_flow, d_mask,
                       H, W, d_grad_mask, d_scratch);
  if (d_grad_flow)
    hipLaunchKernelGGL(convex_upsample_flow_grad_kernel, dim3((W + 63) / 64, H, B), dim3(64), 0, st, d_scratch, H, W,
                       d_grad_flow);
  return launch_status();
}
