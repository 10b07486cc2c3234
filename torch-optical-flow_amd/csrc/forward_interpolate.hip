// forward_interpolate (gfx950): RAFT's warm-start initialiser on the device. The previous pair's low-resolution flow is
// forward-projected along itself: every grid pixel takes the flow of the source pixel that LANDS nearest to it. Upstream
// RAFT does this on the host with scipy's griddata(method="nearest") on float64 coordinates; this is the same selection,
// exact, with the tie-break made explicit (include/oflow.h states the contract).
//
// Per image, in fp64: source s = y*W + x lands at (x1, y1) = (x + dx[s], y + dy[s]) (exact); it counts iff
// 0 < x1 < W and 0 < y1 < H (all false for NaN, one false for +-inf). Query (qx, qy) takes the landed source with the
// least (qx - x1)^2 + (qy - y1)^2 -- two products and one sum, each rounded once, no FMA contraction, so every candidate
// is measured by the same arithmetic as a float64 host reference -- and among equal distances the lowest s.
//
// Structure: one launch, no scratch, no atomics. A workgroup of 1024 threads owns kQueries = 32 consecutive queries of
// one image and walks the image's H*W sources in LDS tiles of kTile entries. An entry is (x1, y1) as two doubles, formed
// once per workgroup while the tile is staged; a source that did not land is staged as (+inf, 0), whose distance is +inf
// and never beats `best` under the strict <. Thread t works for query t % 32 on slice t / 32 of every tile (32 slices
// of 64 entries), so the 32 lanes of a half-wave read one LDS address: a broadcast, no bank conflicts. Each thread keeps
// (best_d2, best_s) over its slices, ascending in s with a strict <; the slices of a query are then folded through LDS
// by the lexicographic minimum of (d2, s), which does not depend on the order of the fold: the result is the
// lowest-index nearest source, the same bits on every run. The winner's two fp32 values are copied unchanged; a query
// whose best is still +inf (no source landed in the image) writes zeros.
//
// 32 queries per workgroup, not 64: Sintel's 55x128 grid at 1/8 resolution is then 220 workgroups on the 256 CUs
// instead of 110 (28.7 vs 43.9 us measured), and where the grid fills the chip either way the two differ by 4 % in
// either direction (8 x 55x128: 141 vs 147 us; 135x240: 353 vs 338 us), so there is one kernel.
// Cost: (H*W)^2 candidate evaluations per image, ~11 VALU instructions each (6 of them fp64). Times: DESIGN.md §4.
#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kThreads = 1024;
constexpr int kQueries = 32;                  // queries per workgroup
constexpr int kSlices = kThreads / kQueries;  // threads per query, each on its own slice of a tile
constexpr int kTile = 2048;                   // sources per LDS tile: 32 KiB of (x1, y1)
constexpr int kChunk = kTile / kSlices;       // tile entries per slice

__global__ __launch_bounds__(kThreads) void forward_interpolate_kernel(const float* __restrict__ flow, int H, int W,
                                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double2 sP[kTile];
  __shared__ double sD[kSlices][kQueries];
  __shared__ int sS[kSlices][kQueries];
  const int tid = threadIdx.x;
  const int ql = tid % kQueries, slice = tid / kQueries;
  const int HW = H * W;
  const float* fl = flow + (long long)blockIdx.y * 2 * HW;
  const int q = blockIdx.x * kQueries + ql;
  const double qx = (double)(q % W), qy = (double)(q / W);  // (q >= HW: scanned like any query, never written)
  const double inf = __builtin_inf();
  const double wd = (double)W, hd = (double)H;
  double best = inf;
  int best_s = 0;
  for (int t0 = 0; t0 < HW; t0 += kTile) {
    __syncthreads();  // the previous tile has been scanned
    for (int e = tid; e < kTile; e += kThreads) {
      const int s = t0 + e;
      double2 p = make_double2(inf, 0.0);
      if (s < HW) {
        const double x1 = (double)(s % W) + (double)fl[s];
        const double y1 = (double)(s / W) + (double)fl[HW + s];
        if (x1 > 0.0 && x1 < wd && y1 > 0.0 && y1 < hd) p = make_double2(x1, y1);
      }
      sP[e] = p;
    }
    __syncthreads();
    const int e0 = slice * kChunk;
    const int e1 = min(e0 + kChunk, HW - t0);
#pragma unroll 4
    for (int e = e0; e < e1; ++e) {
      const double2 p = sP[e];
      const double dx = qx - p.x, dy = qy - p.y;
      const double d2 = dx * dx + dy * dy;
      if (d2 < best) {
        best = d2;
        best_s = t0 + e;
      }
    }
  }
  sD[slice][ql] = best;
  sS[slice][ql] = best_s;
  __syncthreads();
  if (tid < kQueries && q < HW) {
    double bd = sD[0][tid];
    int bs = sS[0][tid];
    for (int k = 1; k < kSlices; ++k) {
      const double d = sD[k][tid];
      const int s = sS[k][tid];
      if (d < bd || (d == bd && s < bs)) {
        bd = d;
        bs = s;
      }
    }
    float* o = out + (long long)blockIdx.y * 2 * HW;
    const bool any = bd < inf;
    o[q] = any ? fl[bs] : 0.f;
    o[HW + q] = any ? fl[HW + bs] : 0.f;
  }
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_forward_interpolate_f32(const float* d_flow, int B, int H, int W, float* d_out, void* stream) {
  if (!d_flow || !d_out) return OFLOW_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (long long)H * W > (1LL << 30)) return OFLOW_E_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(forward_interpolate_kernel, dim3((H * W + kQueries - 1) / kQueries, B), dim3(kThreads), 0, st,
                     d_flow, H, W, d_out);
  return launch_status();
}
