// Backward of the on-the-fly ("alternate") correlation lookup (corr_otf.hip), gfx950: what training differentiates
// through AlternateCorrBlock. No (HW)^2 tensor is formed in either direction.
//
// With a = f1h (fp16 copy of fmap1 / sqrt(C)) and F_l = f2h[l] (fp16 floor-pooled fmap2), both taken as exact leaves:
//   dP_l[q][u][v] = nw*g[u][v] + ne*g[u][v-1] + sw*g[u-1][v] + se*g[u-1][v-1]    (corr_backward.hip's patch gradient)
//   gA[b,q,:]     = sum_l sum_{(u,v) inside level l} dP_l[q][u][v] * F_l[b, ys+u, xs+v, :]
//   gF_l[b,y,x,:] = sum_q sum_{(u,v): (ys+u, xs+v) = (y,x)} dP_l[q][u][v] * a[b,q,:]
//   grad_fmap1 = gA / sqrt(C);  grad_fmap2[b,c,y,x] = sum_l gF_l[b, y>>l, x>>l, c] / 4^l  (inside level l)
//
// corr_otf_backward_kernel: a workgroup owns the forward's 2 x 16 query segment and loops over the levels. Per level it
// lists the targets of a pass -- the clipped bounding box of the 32 windows when it holds at most kTMax targets, else
// (divergent flow) the windows of 3 queries per pass, 128 slots each -- and builds dP as an fp32 [target][query] tile
// in LDS (zero where a query's window does not cover the target). Two GEMMs on v_mfma_f32_32x32x2_f32 follow, the fp16
// features converted exactly to fp32 and the gradients kept in fp32 (a mean loss puts them near fp16's subnormals):
//   gA^T[c][q] += F[t][c] * dP[t][q]   accumulated in registers over targets, passes and levels; written once, in a
//                                      fixed order (deterministic, no atomics);
//   gF[t][c]    = dP[t][q] * a[q][c]   the sum over the 32 queries is the MFMA's K dimension; the tile is then added
//                                      to the level's zero-initialised fp32 NHWC scratch with no-return atomicAdd, each
//                                      accumulator register as it stands = two 128-B channel runs (boxes of neighbouring
//                                      workgroups overlap). Arrival order varies: grad_fmap2 is not bit-reproducible.
// otf_fold_kernel: the level scratches -> grad_fmap2 (B, C, H, W), pool transpose + NHWC -> NCHW through an LDS tile, fixed
// order, every element written once.
#include <hip/hip_fp16.h>

#include "oflow_internal.h"

namespace oflow {
namespace {

constexpr int kQR = 2;            // query rows per segment (corr_otf.hip)
constexpr int kQC = 16;           // query cols per segment
constexpr int kQ = kQR * kQC;     // 32 queries = one MFMA tile side
constexpr int kTMax = 384;        // max targets per pass (12 M-tiles)
constexpr int kDS = kQ + 1;       // LDS row stride of the dP tile [target][query]: conflict-free for both GEMMs
constexpr int kSlot = 128;        // fallback: target slots per query ((2r+2)^2 <= 100)
constexpr int kSlotQ = kTMax / kSlot;  // fallback: queries per pass (3)
constexpr int kThreads = 256;
constexpr int kCChunk = 256;      // channels whose gA accumulators a workgroup holds in registers (2 tiles per wave)
constexpr int kNTW = kCChunk / 32 / 4;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct OtfBwdArgs {
  const float* gout;                   // (B, L*K*K, H, W)
  const __half* f1;                    // (B, H, W, C)
  const __half* f2[OFLOW_MAX_LEVELS];  // (B, H_l, W_l, C)
  float* scr[OFLOW_MAX_LEVELS];        // (B, H_l, W_l, C) fp32, zeroed; null when grad_fmap2 is not wanted
  int Hl[OFLOW_MAX_LEVELS], Wl[OFLOW_MAX_LEVELS];
  const float* coords;                 // (B, 2, H, W)
  float* g1;                           // (B, C, H, W) or null
  int B, C, H, W, segx, segy, cout, nlev, want2;
  float scale;                         // 1 / sqrt(C)
};

template <int R>
__global__ __launch_bounds__(kThreads) void corr_otf_backward_kernel(OtfBwdArgs a) {
  constexpr int PK = 2 * R + 2, K = 2 * R + 1, KK = K * K, GS = KK + 1;
  __shared__ float sD[kTMax * kDS];     // dP tile: [target][query]
  __shared__ float sG[kQ * GS];         // the segment's output gradients of this level: [query][channel]
  __shared__ int sTp[kTMax];            // target -> pixel index (b*Hl + y)*Wl + x of the level, -1 when dead
  __shared__ short sTy[kTMax], sTx[kTMax], sTo[kTMax];  // target row / column / owning query (-1: every query)
  __shared__ int sXs[kQ], sYs[kQ];
  __shared__ float4 sW[kQ];

  const int seg = blockIdx.x;
  const int b = seg / (a.segx * a.segy);
  const int sr = seg - b * a.segx * a.segy;
  const int qy0 = (sr / a.segx) * kQR, qx0 = (sr % a.segx) * kQC;
  const int N = a.H * a.W;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const bool want1 = a.g1 != nullptr, want2 = a.want2 != 0;

  for (int cs = 0; cs < a.C; cs += kCChunk) {  // one trip for C <= 256
    const int ntc = min((a.C - cs) >> 5, kCChunk / 32);  // 32-channel tiles of this chunk
    f32x16 acc1[kNTW];
#pragma unroll
    for (int j = 0; j < kNTW; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc1[j][e] = 0.f;

    for (int lvl = 0; lvl < a.nlev; ++lvl) {
      const int Hl = a.Hl[lvl], Wl = a.Wl[lvl];
      const __half* __restrict__ F2 = a.f2[lvl];
      float* __restrict__ scr = a.scr[lvl];
      __syncthreads();  // the previous level's readers of sXs.. / sG / sD are done
      if (threadIdx.x < kQ) {
        const int qy = qy0 + threadIdx.x / kQC, qx = qx0 + threadIdx.x % kQC;
        int xs = 1 << 28, ys = 1 << 28;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qy < a.H && qx < a.W) {
          const float inv = 1.0f / static_cast<float>(1 << lvl);
          const float cx = a.coords[((size_t)(2 * b) * a.H + qy) * a.W + qx] * inv;
          const float cy = a.coords[((size_t)(2 * b + 1) * a.H + qy) * a.W + qx] * inv;
          if (fabsf(cx) < 4194304.0f && fabsf(cy) < 4194304.0f) {
            const float fx = floorf(cx), fy = floorf(cy);
            const float wx = cx - fx, wy = cy - fy, ex = 1.0f - wx, ey = 1.0f - wy;
            xs = static_cast<int>(fx) - R;
            ys = static_cast<int>(fy) - R;
            w = make_float4(ey * ex, ey * wx, wy * ex, wy * wx);
          }
        }
        sXs[threadIdx.x] = xs;
        sYs[threadIdx.x] = ys;
        sW[threadIdx.x] = w;
      }
      for (int e = threadIdx.x; e < kQ * KK; e += kThreads) {
        const int c = e / kQ, qi = e - c * kQ;
        const int qy = qy0 + qi / kQC, qx = qx0 + qi % kQC;
        float g = 0.f;
        if (qy < a.H && qx < a.W) g = a.gout[(((size_t)b * a.cout + lvl * KK + c) * a.H + qy) * a.W + qx];
        sG[qi * GS + c] = g;
      }
      __syncthreads();

      // Box of the whole segment, clipped to the level (corr_otf_kernel's)
      int by0 = 1 << 29, bx0 = 1 << 29, by1 = -(1 << 29), bx1 = -(1 << 29);
      for (int q = 0; q < kQ; ++q) {
        const int ys = sYs[q], xs = sXs[q];
        if (ys < (1 << 27) && ys + PK > 0 && ys < Hl && xs + PK > 0 && xs < Wl) {
          by0 = min(by0, ys);
          bx0 = min(bx0, xs);
          by1 = max(by1, ys + PK - 1);
          bx1 = max(bx1, xs + PK - 1);
        }
      }
      by0 = max(by0, 0);
      bx0 = max(bx0, 0);
      by1 = min(by1, Hl - 1);
      bx1 = min(bx1, Wl - 1);
      const bool any = by1 >= by0 && bx1 >= bx0;
      const int bh = by1 - by0 + 1, bw = bx1 - bx0 + 1;
      const bool fits = any && bh * bw <= kTMax;
      const int passes = !any ? 0 : (fits ? 1 : (kQ + kSlotQ - 1) / kSlotQ);

      for (int pass = 0; pass < passes; ++pass) {
        const int T = fits ? bh * bw : kTMax;
        const int Tp = (T + 31) & ~31;  // <= kTMax
        if (pass) __syncthreads();      // the previous pass's GEMMs have read sD / sT*
        // ---- targets of this pass ----
        for (int t = threadIdx.x; t < Tp; t += kThreads) {
          int p = -1, ty = 0, tx = 0, own = -1;
          if (fits) {
            if (t < T) {
              ty = by0 + t / bw;
              tx = bx0 + t % bw;
              p = (b * Hl + ty) * Wl + tx;
            }
          } else {
            own = pass * kSlotQ + t / kSlot;
            const int tt = t % kSlot;
            if (own < kQ) {
              const int ys = sYs[own], xs = sXs[own];
              if (ys < (1 << 27) && ys + PK > 0 && ys < Hl && xs + PK > 0 && xs < Wl) {
                const int y0 = max(ys, 0), x0 = max(xs, 0);
                const int h = min(ys + PK - 1, Hl - 1) - y0 + 1, w = min(xs + PK - 1, Wl - 1) - x0 + 1;
                if (tt < h * w) {
                  ty = y0 + tt / w;
                  tx = x0 + tt % w;
                  p = (b * Hl + ty) * Wl + tx;
                }
              }
            }
          }
          sTp[t] = p;
          sTy[t] = static_cast<short>(ty);  // levels are at most 32767 px a side (checked by the host entry)
          sTx[t] = static_cast<short>(tx);
          sTo[t] = static_cast<short>(own);
        }
        __syncthreads();
        // ---- dP tile: [target][query] ----
        for (int e = threadIdx.x; e < Tp * kQ; e += kThreads) {
          const int t = e >> 5, qi = e & 31;
          float d = 0.f;
          const int own = sTo[t];
          if (sTp[t] >= 0 && (own < 0 || own == qi)) {
            const int ys = sYs[qi], xs = sXs[qi];
            if (ys < (1 << 27)) {
              const int u = sTy[t] - ys, v = sTx[t] - xs;  // patch row (y) / column (x)
              if (static_cast<unsigned>(u) < static_cast<unsigned>(PK) && static_cast<unsigned>(v) < static_cast<unsigned>(PK)) {
                const float4 w = sW[qi];
                const float* g = &sG[qi * GS];
                // channel k = i*K + j samples (x: i, y: j); g[j][i] = g[i*K + j]
                if (u < K && v < K) d += w.x * g[v * K + u];
                if (u < K && v >= 1) d += w.y * g[(v - 1) * K + u];
                if (u >= 1 && v < K) d += w.z * g[v * K + (u - 1)];
                if (u >= 1 && v >= 1) d += w.w * g[(v - 1) * K + (u - 1)];
              }
            }
          }
          sD[t * kDS + qi] = d;
        }
        __syncthreads();

        // ---- gA^T[c][q] += sum_t F[t][c] dP[t][q]: wave w holds channel tiles w, w + 4 ----
        if (want1) {
          for (int k0 = 0; k0 < Tp; k0 += 2) {
            const int t = k0 + lh;
            const int p = sTp[t];
            const float bv = sD[t * kDS + l31];
#pragma unroll
            for (int j = 0; j < kNTW; ++j) {
              const int nt = wave + 4 * j;
              if (nt < ntc) {  // wave-uniform
                float av = 0.f;
                if (p >= 0) av = __half2float(F2[(size_t)p * a.C + cs + nt * 32 + l31]);
                acc1[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc1[j], 0, 0, 0);
              }
            }
          }
        }
        // ---- gF[t][c] = sum_q dP[t][q] a[q][c], added to the level scratch ----
        if (want2) {
          for (int nt = wave; nt < ntc; nt += 4) {
            float bq[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
              const int qi = 2 * kk + lh;
              const int qy = qy0 + qi / kQC, qx = qx0 + qi % kQC;
              bq[kk] = 0.f;
              if (qy < a.H && qx < a.W)
                bq[kk] = __half2float(a.f1[((size_t)b * N + (size_t)qy * a.W + qx) * a.C + cs + nt * 32 + l31]);
            }
            for (int mt = 0; mt < (Tp >> 5); ++mt) {
              f32x16 acc;
#pragma unroll
              for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
              for (int kk = 0; kk < 16; ++kk) {
                const float av = sD[(mt * 32 + l31) * kDS + 2 * kk + lh];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[kk], acc, 0, 0, 0);
              }
              // C/D map: acc[e] <-> row 4 * (lane >> 5) + (e & 3) + 8 * (e >> 2), column lane & 31
#pragma unroll
              for (int e = 0; e < 16; ++e) {
                const int t = mt * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);
                const int p = sTp[t];
                if (p >= 0) atomicAdd(scr + (size_t)p * a.C + cs + nt * 32 + l31, acc[e]);
              }
            }
          }
        }
      }
    }

    // ---- grad_fmap1 (B, C, H, W): every element of the segment once ----
    if (want1) {
      const int qy = qy0 + l31 / kQC, qx = qx0 + l31 % kQC;
      if (qy < a.H && qx < a.W) {
#pragma unroll
        for (int j = 0; j < kNTW; ++j) {
          const int nt = wave + 4 * j;
          if (nt < ntc) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int c = cs + nt * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);
              a.g1[(((size_t)b * a.C + c) * a.H + qy) * a.W + qx] = acc1[j][e] * a.scale;
            }
          }
        }
      }
    }
  }
}

struct FoldArgs {
  const float* scr[OFLOW_MAX_LEVELS];
  int Hl[OFLOW_MAX_LEVELS], Wl[OFLOW_MAX_LEVELS];
  float* g2;  // (B, C, H, W)
  int C, H, W, nlev;
};

// 64 pixels x 64 channels per block: reads along channels (NHWC rows of every level), writes along pixels
__global__ __launch_bounds__(256) void otf_fold_kernel(FoldArgs a) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z;
  const int HW = a.H * a.W;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int p = p0 + r, c = c0 + tx;
    float acc = 0.f;
    if (p < HW && c < a.C) {
      const int y = p / a.W, x = p - y * a.W;
      acc = a.scr[0][((size_t)b * HW + p) * a.C + c];
      float s = 1.0f;
      for (int l = 1; l < a.nlev; ++l) {
        s *= 0.25f;  // exact
        const int yl = y >> l, xl = x >> l;
        if (yl < a.Hl[l] && xl < a.Wl[l]) acc += a.scr[l][(((size_t)b * a.Hl[l] + yl) * a.Wl[l] + xl) * a.C + c] * s;
      }
    }
    tile[r][tx] = acc;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int c = c0 + r, p = p0 + tx;
    if (c < a.C && p < HW) a.g2[((size_t)b * a.C + c) * HW + p] = tile[tx][r];
  }
}

template <int R>
int launch_otf_backward(const OtfBwdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(corr_otf_backward_kernel<R>, dim3(a.B * a.segx * a.segy), dim3(kThreads), 0, s, a);
  return launch_status();
}

}  // namespace
}  // namespace oflow

using namespace oflow;

extern "C" int oflow_corr_lookup_otf_backward_f32(const float* d_grad_out, const void* d_f1h, const void* const* d_f2h,
                                                  const int* level_h, const int* level_w, int num_levels,
                                                  const float* d_coords, int B, int C, int H, int W, int radius,
                                                  float* d_grad_fmap1, float* d_grad_fmap2, float* d_scratch,
                                                  void* stream) {
  if (!d_grad_out || !d_f1h || !d_f2h || !level_h || !level_w || !d_coords) return OFLOW_E_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32 != 0) return OFLOW_E_SHAPE;
  if (num_levels < 1 || num_levels > OFLOW_MAX_LEVELS) return OFLOW_E_LEVELS;
  if (radius < 0 || radius > 4) return OFLOW_E_RADIUS;
  if (d_grad_fmap2 && !d_scratch) return OFLOW_E_NULL;
  if ((long long)B * H * W >= (1ll << 31) || B > 65535) return OFLOW_E_SHAPE;  // level pixel indices are 32-bit
  OtfBwdArgs a{};
  FoldArgs f{};
  a.gout = d_grad_out;
  a.f1 = static_cast<const __half*>(d_f1h);
  size_t off = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (!d_f2h[l]) return OFLOW_E_NULL;
    if (level_h[l] < 2 || level_w[l] < 2) return OFLOW_E_TINY;
    if (level_h[l] > 32767 || level_w[l] > 32767) return OFLOW_E_SHAPE;  // target rows / columns are 16-bit
    a.f2[l] = static_cast<const __half*>(d_f2h[l]);
    a.Hl[l] = f.Hl[l] = level_h[l];
    a.Wl[l] = f.Wl[l] = level_w[l];
    a.scr[l] = d_grad_fmap2 ? d_scratch + off : nullptr;
    f.scr[l] = a.scr[l];
    off += (size_t)B * C * level_h[l] * level_w[l];
  }
  if (level_h[0] != H || level_w[0] != W) return OFLOW_E_SHAPE;  // the fold maps level 0 onto grad_fmap2 one to one
  if (!d_grad_fmap1 && !d_grad_fmap2) return OFLOW_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_grad_fmap2 && hipMemsetAsync(d_scratch, 0, off * sizeof(float), s) != hipSuccess) return launch_status();
  a.coords = d_coords;
  a.g1 = d_grad_fmap1;
  a.B = B;
  a.C = C;
  a.H = H;
  a.W = W;
  a.segx = (W + kQC - 1) / kQC;
  a.segy = (H + kQR - 1) / kQR;
  const int K = 2 * radius + 1;
  a.cout = num_levels * K * K;
  a.nlev = num_levels;
  a.want2 = d_grad_fmap2 ? 1 : 0;
  a.scale = 1.0f / sqrtf(static_cast<float>(C));
  int st;
  switch (radius) {
    case 0: st = launch_otf_backward<0>(a, s); break;
    case 1: st = launch_otf_backward<1>(a, s); break;
    case 2: st = launch_otf_backward<2>(a, s); break;
    case 3: st = launch_otf_backward<3>(a, s); break;
    case 4: st = launch_otf_backward<4>(a, s); break;
    default: return OFLOW_E_RADIUS;
  }
  if (st != OFLOW_OK || !d_grad_fmap2) return st;
  f.g2 = d_grad_fmap2;
  f.C = C;
  f.H = H;
  f.W = W;
  f.nlev = num_levels;
  hipLaunchKernelGGL(otf_fold_kernel, dim3((H * W + 63) / 64, (C + 63) / 64, B), dim3(256), 0, s, f);
  return launch_status();
}
