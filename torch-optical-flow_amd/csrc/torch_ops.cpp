// PyTorch operator registration of the correlation / warp path: TORCH_LIBRARY(oflow) -> torch.ops.oflow.*.
//
// Each op's HIP-key (PyTorch-ROCm's "CUDA" dispatch key) kernel validates its tensors and calls the C ABI of
// liboflow_hip.so (include/oflow.h) on PyTorch's current HIP stream; the Meta kernel computes output shapes only,
// which is what torch.compile's fake-tensor tracing runs. Autograd formulas are registered from Python
// (optical_flow/_ops.py) on top of these ops, so CorrBlock / warp trace into a single graph with no breaks.
//
// Each op is one function `R op(bool run, Args...)`: with run == false it checks its arguments and returns outputs of
// the right shape without touching a data pointer (the Meta kernel); with run == true it goes on to the launch (the
// HIP kernel, and the CPU key's, so that a CPU tensor reaches the "no CPU fallback" check). bind<&op>(m, "name") at
// the end of the file registers all three from that one function.
//
// Ops (reference interface each one implements):
//   corr_pyramid(fmap1, fmap2, num_levels) -> Tensor[]            CorrBlock.__init__  (corr.py:38-54, 79-87)
//   corr_pyramid_tiled(fmap1, fmap2, num_levels) -> Tensor[]      same values, tiled lookup layout
//   corr_lookup(levels, coords, radius) -> Tensor                 CorrBlock.__call__  (corr.py:56-77)
//   corr_lookup_tiled(levels, coords, radius) -> Tensor           same, over the tiled levels
//   corr_lookup_tiled_nhwc(levels, coords, radius, out!) -> ()    same, fp32 NHWC rows (convc1 input)
//   corr_otf_prepare(fmap1, fmap2, num_levels) -> (Tensor, Tensor[])  AlternateCorrBlock.__init__ (fp16 features)
//   corr_lookup_otf(f1h, f2h, coords, radius) -> Tensor           AlternateCorrBlock.__call__ (corr.py:90-110)
//   corr_lookup_alt(fmap1, fmap2, f1h, f2h, coords, radius) -> Tensor   corr_lookup_otf with the fp32 fmaps autograd tracks
//   corr_lookup_alt_backward(grad_out, f1h, f2h, coords, radius, mask) -> (grad_fmap1, grad_fmap2)   its autograd
//   grid_warp(frame, flow, mode, padding_mode, align_corners)     optical_flow.warp   (operator.py:8-33)
//   grid_sample(input, grid, mode, padding_mode, align_corners)   bilinear_sampler    (utils.py:64-80)
//   corr_lookup_backward(grad_out, coords, radius, H0, W0, L)     transpose of corr_lookup (training, §8(f) row 3)
//   corr_pyramid_backward(level_grads, fmap1, fmap2) -> (g1, g2)  pool transpose + two fp32-MFMA GEMMs
//   grid_warp_backward(grad_out, frame, flow, mode, pad, ac, mask) -> (grad_frame, grad_flow)     warp's autograd
//   grid_sample_backward(grad_out, input, grid, mode, pad, ac, mask) -> (grad_input, grad_grid)   grid_sample's autograd
//   flow_error_stats(pred, target, valid?, abs, rel, max_flow, accum!, epe_map) -> Tensor   metrics/epe.py:24-65, f1.py:34-55
//   sequence_loss(flow_preds, flow_gt, valid, weights, max_flow) -> (loss, stats)           raft.py:231-260 (forward)
//   sequence_loss_backward(grad_out, flow_preds, flow_gt, valid, weights, max_flow, need) -> Tensor[]   its autograd
//   convex_upsample(flow, mask) -> Tensor                                                   RAFT.upsample_flow (raft.py:73-85)
//   convex_upsample_backward(grad_out, flow, mask, mask2) -> (grad_flow, grad_mask)         its autograd
//   conv2d_same(x, weight, bias?) -> Tensor                       nn.Conv2d, stride 1, "same" zero padding (update.py:31-161)
//   conv2d_same_backward(grad_out, x, weight, mask3) -> (grad_x, grad_weight, grad_bias)    its autograd (conv_backward.hip)
//   conv2d_strided(x, weight, bias?, stride) / conv2d_strided_backward(..., stride, mask3)   the encoders' nn.Conv2d, stride 1 / 2
//   instance_norm_act(x, eps, relu) / instance_norm_act_backward(grad_out, x, eps, relu)      InstanceNorm2d [+ ReLU] (norm_backward.hip)
//   frozen_batch_norm_act(x, weight, bias, running_mean, running_var, eps, relu) / _backward(..., mask3)   eval BatchNorm2d [+ ReLU]
//   batch_norm_act(x, weight, bias, eps, relu) -> (y, mean, var) / batch_norm_act_backward(..., mean, var, eps, relu, mask3)
//                                                                 train-mode BatchNorm2d [+ ReLU], native both ways (batch_norm.hip)
//   forward_interpolate(flow) -> Tensor                           warm-start flow_init (upstream RAFT's forward_interpolate)
//   augment_batch(img1, img2, flow, valid?, params, crop_h, crop_w) -> (img1, img2, flow, valid)   data/augmentor.py:43-324
//   fb_consistency(flow_fw, flow_bw, alpha, beta, both, with_error) -> (mask_fw, mask_bw, err_fw, err_bw)
//                                                                 forward-backward occlusion masks (not in the reference)
//   splat(frame, flow, metric?, mode) -> (out, weight)           forward warping: sum / average / linear / softmax splatting
//   splat_backward(grad_out, frame, flow, metric?, out, weight, mode, mask3) -> (grad_frame, grad_flow, grad_metric)
//                                                                 its autograd (splat.hip, splat_backward.hip; not in the reference)
//   census_loss(frame0, frame1, mask?, patch, image_range) -> (loss, sum_m, s_map)   the ternary census loss (census_loss.hip)
//   census_loss_backward(grad_loss, frame0, frame1, mask?, sum_m, s_map, patch, image_range, mask2) -> (grad_frame0, grad_frame1)
//   smoothness_loss(flow, image, order, edge_weight, image_range) -> loss             edge-aware smoothness (smoothness_loss.hip)
//   smoothness_loss_backward(grad_loss, flow, image, order, edge_weight, image_range) -> grad_flow
//   ssim_loss(frame0, frame1, mask?, window, c1, c2, with_map) -> (loss, sum_m, ssim_map)   SSIM loss (photometric_loss.hip)
//   ssim_loss_backward(grad_loss, frame0, frame1, mask?, sum_m, window, c1, c2, mask2) -> (grad_frame0, grad_frame1)
//   charbonnier_loss(frame0, frame1, mask?, eps, alpha, image_range) -> (loss, sum_m)        robust L1 (photometric_loss.hip)
//   charbonnier_loss_backward(grad_loss, frame0, frame1, mask?, sum_m, eps, alpha, image_range, mask2) -> (grad_frame0, grad_frame1)
#include <array>
#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <climits>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <utility>
#include <vector>

#include "oflow.h"

namespace {

using at::Tensor;
using Tensor3 = std::tuple<Tensor, Tensor, Tensor>;
using Tensor4 = std::tuple<Tensor, Tensor, Tensor, Tensor>;

void check_status(int st, const char* what) {
  if (st == OFLOW_OK) return;
  // Q3 (a level under 2 px): the reference returns NaN; this build raises ValueError, as the Python layer did
  TORCH_CHECK_VALUE(st != OFLOW_E_TINY, what, ": ", oflow_status_string(st));
  TORCH_CHECK(false, what, " failed (", st, "): ", oflow_status_string(st));
}

void* cur_stream() { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

// the one refusal of a tensor that is not on a ROCm GPU (there is no CPU path)
const char* kNoCpu = "; this MI355X build runs only on ROCm GPU tensors (no CPU fallback)";

void check_on_gpu(const Tensor& t, const char* name, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, ": ", name, " is on ", t.device(), kNoCpu);
}

Tensor gpu_f32(const Tensor& t, const char* name, const char* what) {
  check_on_gpu(t, name, what);
  return t.to(at::kFloat).contiguous();
}

// a gradient output by its output_mask entry: the given shape where wanted, an empty (0-element) tensor where not
Tensor wanted(bool want, at::IntArrayRef sizes, const at::TensorOptions& opt) {
  return at::empty(want ? sizes : at::IntArrayRef{0}, opt);
}

std::vector<std::pair<int, int>> dims_of(int64_t h, int64_t w, int64_t nl, const char* what) {
  TORCH_CHECK(nl >= 1 && nl <= OFLOW_MAX_LEVELS, what, ": number of pyramid levels ", nl, " outside [1, ",
              OFLOW_MAX_LEVELS, "]");
  int hs[OFLOW_MAX_LEVELS], ws[OFLOW_MAX_LEVELS];
  check_status(oflow_corr_pyramid_dims((int)h, (int)w, (int)nl, hs, ws), what);
  std::vector<std::pair<int, int>> d;
  for (int l = 0; l < nl; ++l) d.emplace_back(hs[l], ws[l]);
  return d;
}

void check_fmaps(const Tensor& f1, const Tensor& f2, const char* what) {
  TORCH_CHECK(f1.dim() == 4 && f1.sizes() == f2.sizes(), what, ": fmap1 ", f1.sizes(), " and fmap2 ", f2.sizes(),
              " must be equal (B, C, H, W)");
  TORCH_CHECK(f1.device() == f2.device(), what, ": fmap1 and fmap2 are on different devices");
}

void check_pool_dims(const std::vector<std::pair<int, int>>& d, int64_t nl, const char* what) {
  for (auto& p : d)
    TORCH_CHECK(p.first >= 1 && p.second >= 1, what, ": ", nl, " levels of 2x2 pooling need H, W >= ",
                1 << (nl - 1));
}

void check_radius(int64_t r, int64_t rmax, const char* what) {
  TORCH_CHECK(r >= 0 && r <= rmax, what, ": radius ", r, " outside [0, ", rmax, "]");
}

void check_coords(const Tensor& co, const char* what) {
  TORCH_CHECK(co.dim() == 4 && co.size(1) == 2, what, ": coords must be (B, 2, H, W), got ", co.sizes());
}

// ---------------------------------------------------------------- pyramid
// (check_fmaps has put fmap2 on fmap1's device, so the refusal of a CPU tensor names fmap1)
std::vector<Tensor> corr_pyramid(bool run, const Tensor& fmap1, const Tensor& fmap2, int64_t num_levels) {
  const char* what = "corr_pyramid";
  check_fmaps(fmap1, fmap2, what);
  if (run) check_on_gpu(fmap1, "fmap1", what);
  const int64_t b = fmap1.size(0), c = fmap1.size(1), h = fmap1.size(2), w = fmap1.size(3);
  auto d = dims_of(h, w, num_levels, what);
  std::vector<Tensor> levels;
  for (auto& p : d) levels.push_back(at::empty({b * h * w, 1, p.first, p.second}, fmap1.options().dtype(at::kFloat)));
  if (!run || b == 0) return levels;
  check_pool_dims(d, num_levels, what);
  Tensor f1 = gpu_f32(fmap1, "fmap1", what), f2 = gpu_f32(fmap2, "fmap2", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f1.device());
  float* ptrs[OFLOW_MAX_LEVELS];
  for (int l = 0; l < num_levels; ++l) ptrs[l] = levels[l].data_ptr<float>();
  check_status(oflow_corr_pyramid_f32(f1.data_ptr<float>(), f2.data_ptr<float>(), (int)b, (int)c, (int)h, (int)w,
                                      (int)num_levels, ptrs, cur_stream()),
               what);
  return levels;
}

std::vector<Tensor> corr_pyramid_tiled(bool run, const Tensor& fmap1, const Tensor& fmap2, int64_t num_levels) {
  const char* what = "corr_pyramid";
  check_fmaps(fmap1, fmap2, what);
  if (run) check_on_gpu(fmap1, "fmap1", what);
  const int64_t b = fmap1.size(0), c = fmap1.size(1), h = fmap1.size(2), w = fmap1.size(3), q = b * h * w;
  auto d = dims_of(h, w, num_levels, what);
  if (run) check_pool_dims(d, num_levels, what);
  std::vector<Tensor> levels;
  for (auto& p : d)
    levels.push_back(at::empty({q, oflow_corr_tiled_level_floats(p.first, p.second)}, fmap1.options().dtype(at::kFloat)));
  if (!run || q == 0) return levels;
  Tensor f1 = gpu_f32(fmap1, "fmap1", what), f2 = gpu_f32(fmap2, "fmap2", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f1.device());
  float* ptrs[OFLOW_MAX_LEVELS];
  for (int l = 0; l < num_levels; ++l) ptrs[l] = levels[l].data_ptr<float>();
  check_status(oflow_corr_pyramid_tiled_f32(f1.data_ptr<float>(), f2.data_ptr<float>(), (int)b, (int)c, (int)h,
                                            (int)w, (int)num_levels, ptrs, cur_stream()),
               what);
  return levels;
}

// ---------------------------------------------------------------- lookups
struct LevelArgs {
  const float* ptr[OFLOW_MAX_LEVELS];
  int h[OFLOW_MAX_LEVELS], w[OFLOW_MAX_LEVELS];
  int n = 0;
};

// canonical levels: (B*H*W, 1, H_l, W_l)
LevelArgs canonical_levels(const std::vector<Tensor>& lv, std::vector<Tensor>& keep, const Tensor& co,
                           const char* what) {
  const int64_t n = (int64_t)lv.size();
  TORCH_CHECK(n >= 1 && n <= OFLOW_MAX_LEVELS, what, ": number of pyramid levels ", n, " outside [1, ",
              OFLOW_MAX_LEVELS, "]");
  const int64_t q = co.size(0) * co.size(2) * co.size(3);
  LevelArgs a;
  a.n = (int)n;
  for (int64_t i = 0; i < n; ++i) {
    Tensor t = gpu_f32(lv[i], "corr_pyramid level", what);
    TORCH_CHECK(t.device() == co.device(), what, ": corr_pyramid[", i, "] and coords are on different devices");
    TORCH_CHECK(t.dim() == 4 && t.size(0) == q && t.size(1) == 1, what, ": corr_pyramid[", i, "] shape ", t.sizes(),
                " != (", q, ", 1, H_l, W_l)");
    keep.push_back(t);
    a.ptr[i] = t.data_ptr<float>();
    a.h[i] = (int)t.size(2);
    a.w[i] = (int)t.size(3);
  }
  return a;
}

// tiled levels: (B*H*W, floats_l), level dims from the query grid
LevelArgs tiled_levels(const std::vector<Tensor>& lv, const Tensor& co, const char* what) {
  const int64_t n = (int64_t)lv.size();
  auto d = dims_of(co.size(2), co.size(3), n, what);
  const int64_t q = co.size(0) * co.size(2) * co.size(3);
  LevelArgs a;
  a.n = (int)n;
  for (int64_t i = 0; i < n; ++i) {
    const Tensor& t = lv[i];
    TORCH_CHECK(t.is_cuda() && t.device() == co.device(), what, ": tiled level ", i, " and coords are on different devices");
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() && t.dim() == 2 && t.size(0) == q &&
                    t.size(1) == oflow_corr_tiled_level_floats(d[i].first, d[i].second),
                what, ": tiled level ", i, " ", t.sizes(), " does not match coords ", co.sizes(),
                " (expected a contiguous fp32 (", q, ", ", oflow_corr_tiled_level_floats(d[i].first, d[i].second), "))");
    a.ptr[i] = t.data_ptr<float>();
    a.h[i] = d[i].first;
    a.w[i] = d[i].second;
  }
  return a;
}

Tensor lookup_out(const Tensor& co, int64_t nl, int64_t radius) {
  const int64_t k = 2 * radius + 1;
  return at::empty({co.size(0), nl * k * k, co.size(2), co.size(3)}, co.options().dtype(at::kFloat));
}

// The three lookups over a stored pyramid validate only coords and the radius without run: the levels are checked
// against the device (tiled_levels asks is_cuda(), which a fake tensor fails) and through their data on the way to
// the launch.
Tensor corr_lookup(bool run, const std::vector<Tensor>& levels, const Tensor& coords, int64_t radius) {
  const char* what = "corr_lookup";
  check_coords(coords, what);
  check_radius(radius, OFLOW_MAX_RADIUS, what);
  if (!run) return lookup_out(coords, (int64_t)levels.size(), radius);
  Tensor co = gpu_f32(coords, "coords", what);
  std::vector<Tensor> keep;
  LevelArgs a = canonical_levels(levels, keep, co, what);
  Tensor out = lookup_out(co, a.n, radius);
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  check_status(oflow_corr_lookup_f32(a.ptr, a.h, a.w, a.n, co.data_ptr<float>(), (int)co.size(0), (int)co.size(2),
                                     (int)co.size(3), (int)radius, out.data_ptr<float>(), cur_stream()),
               what);
  return out;
}

Tensor corr_lookup_tiled(bool run, const std::vector<Tensor>& levels, const Tensor& coords, int64_t radius) {
  const char* what = "corr_lookup";
  check_coords(coords, what);
  check_radius(radius, OFLOW_MAX_RADIUS, what);
  if (!run) return lookup_out(coords, (int64_t)levels.size(), radius);
  Tensor co = gpu_f32(coords, "coords", what);
  LevelArgs a = tiled_levels(levels, co, what);
  Tensor out = lookup_out(co, a.n, radius);
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  check_status(oflow_corr_lookup_tiled_f32(a.ptr, a.h, a.w, a.n, co.data_ptr<float>(), (int)co.size(0),
                                           (int)co.size(2), (int)co.size(3), (int)radius, out.data_ptr<float>(),
                                           cur_stream()),
               what);
  return out;
}

void corr_lookup_tiled_nhwc(bool run, const std::vector<Tensor>& levels, const Tensor& coords, int64_t radius,
                            const Tensor& out) {
  const char* what = "corr_lookup";
  check_coords(coords, what);
  check_radius(radius, OFLOW_MAX_RADIUS, what);
  if (!run) return;
  Tensor co = gpu_f32(coords, "coords", what);
  LevelArgs a = tiled_levels(levels, co, what);
  const int64_t q = co.size(0) * co.size(2) * co.size(3);
  TORCH_CHECK(out.is_cuda() && out.device() == co.device() && out.scalar_type() == at::kFloat && out.is_contiguous() &&
                  out.dim() == 2 && out.size(0) == q,
              what, ": NHWC output must be a contiguous fp32 [B*H*W, row] on the coords' device, got ", out.sizes());
  if (q == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  check_status(oflow_corr_lookup_tiled_nhwc_f32(a.ptr, a.h, a.w, a.n, co.data_ptr<float>(), (int)co.size(0),
                                                (int)co.size(2), (int)co.size(3), (int)radius, out.data_ptr<float>(),
                                                (int)out.size(1), cur_stream()),
               what);
}

// ---------------------------------------------------------------- on-the-fly (fp16 feature) correlation
std::tuple<Tensor, std::vector<Tensor>> corr_otf_prepare(bool run, const Tensor& fmap1, const Tensor& fmap2,
                                                         int64_t num_levels) {
  const char* what = "corr_otf_prepare";
  check_fmaps(fmap1, fmap2, what);
  if (run) check_on_gpu(fmap1, "fmap1", what);
  const int64_t b = fmap1.size(0), c = fmap1.size(1), h = fmap1.size(2), w = fmap1.size(3);
  TORCH_CHECK(c % 32 == 0, what, ": the fp16 MFMA path needs C % 32 == 0, got C=", c);
  auto d = dims_of(h, w, num_levels, what);
  check_pool_dims(d, num_levels, what);
  auto o16 = fmap1.options().dtype(at::kHalf);
  Tensor f1h = at::empty({b, h, w, c}, o16);
  std::vector<Tensor> f2h;
  int64_t pooled = 0;
  for (int l = 0; l < num_levels; ++l) {
    f2h.push_back(at::empty({b, d[l].first, d[l].second, c}, o16));
    if (l) pooled += (int64_t)d[l].first * d[l].second;
  }
  if (!run || b == 0) return {f1h, f2h};
  Tensor f1 = gpu_f32(fmap1, "fmap1", what), f2 = gpu_f32(fmap2, "fmap2", what);
  Tensor scratch = at::empty({std::max<int64_t>(1, b * c * pooled)}, f1.options());
  c10::hip::HIPGuardMasqueradingAsCUDA g(f1.device());
  void* ptrs[OFLOW_MAX_LEVELS];
  for (int l = 0; l < num_levels; ++l) ptrs[l] = f2h[l].data_ptr();
  check_status(oflow_corr_otf_prepare_f16(f1.data_ptr<float>(), f2.data_ptr<float>(), (int)b, (int)c, (int)h, (int)w,
                                          (int)num_levels, f1h.data_ptr(), ptrs, scratch.data_ptr<float>(),
                                          cur_stream()),
               what);
  return {f1h, f2h};
}

// f1h (B, H, W, C) fp16 against coords (B, 2, H, W), and the number of fmap2 levels: returns C
int64_t check_f1h(const Tensor& f1h, int64_t nl, const Tensor& coords, const char* what) {
  const int64_t b = coords.size(0), h = coords.size(2), w = coords.size(3);
  TORCH_CHECK(f1h.scalar_type() == at::kHalf && f1h.dim() == 4 && f1h.size(0) == b && f1h.size(1) == h &&
                  f1h.size(2) == w && f1h.is_contiguous(),
              what, ": f1h ", f1h.sizes(), " must be contiguous fp16 (", b, ", ", h, ", ", w, ", C)");
  TORCH_CHECK(nl >= 1 && nl <= OFLOW_MAX_LEVELS, what, ": number of pyramid levels ", nl, " outside [1, ",
              OFLOW_MAX_LEVELS, "]");
  return f1h.size(3);
}

// every fp16 fmap2 level (B, H_l, W_l, C) on the coords' device: fills hs / ws and returns the levels' pixel sum
int64_t check_f2h_levels(const std::vector<Tensor>& f2h, const Tensor& coords, int64_t c, int* hs, int* ws,
                         const char* what) {
  const int64_t b = coords.size(0);
  int64_t pix = 0;
  for (int64_t i = 0; i < (int64_t)f2h.size(); ++i) {
    const Tensor& t = f2h[i];
    TORCH_CHECK(t.scalar_type() == at::kHalf && t.dim() == 4 && t.size(0) == b && t.size(3) == c && t.is_contiguous(),
                what, ": fmap2 level ", i, " ", t.sizes(), " must be contiguous fp16 (", b, ", H_l, W_l, ", c, ")");
    TORCH_CHECK(t.device() == coords.device(), what, ": fmap2 level ", i, " and coords are on different devices");
    hs[i] = (int)t.size(1);
    ws[i] = (int)t.size(2);
    pix += t.size(1) * t.size(2);
  }
  return pix;
}

Tensor corr_lookup_otf(bool run, const Tensor& f1h, const std::vector<Tensor>& f2h, const Tensor& coords,
                       int64_t radius) {
  const char* what = "corr_lookup_otf";
  check_coords(coords, what);
  if (run) check_on_gpu(coords, "coords", what);
  check_radius(radius, 4, what);
  const int64_t b = coords.size(0), h = coords.size(2), w = coords.size(3), nl = (int64_t)f2h.size();
  const int64_t c = check_f1h(f1h, nl, coords, what);
  int hs[OFLOW_MAX_LEVELS], ws[OFLOW_MAX_LEVELS];
  check_f2h_levels(f2h, coords, c, hs, ws, what);
  Tensor out = lookup_out(coords, nl, radius);
  if (!run || out.numel() == 0) return out;
  const void* ptrs[OFLOW_MAX_LEVELS];
  for (int64_t i = 0; i < nl; ++i) ptrs[i] = f2h[i].data_ptr();  // (fake tensors of a trace have no data pointer)
  Tensor co = gpu_f32(coords, "coords", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  check_status(oflow_corr_lookup_otf_f16(f1h.data_ptr(), ptrs, hs, ws, (int)nl, co.data_ptr<float>(), (int)b, (int)c,
                                         (int)h, (int)w, (int)radius, out.data_ptr<float>(), cur_stream()),
               what);
  return out;
}

// corr_lookup_alt: corr_lookup_otf's forward on (f1h, f2h), with the fp32 feature maps those were prepared from as the
// arguments autograd tracks (their values are not read: the fp16 roundings count as identity, _ops.py).
Tensor corr_lookup_alt(bool run, const Tensor& fmap1, const Tensor& fmap2, const Tensor& f1h,
                       const std::vector<Tensor>& f2h, const Tensor& coords, int64_t radius) {
  const char* what = "corr_lookup_alt";
  check_fmaps(fmap1, fmap2, what);
  TORCH_CHECK(f1h.dim() == 4 && fmap1.size(0) == f1h.size(0) && fmap1.size(1) == f1h.size(3) &&
                  fmap1.size(2) == f1h.size(1) && fmap1.size(3) == f1h.size(2),
              what, ": fmap1 ", fmap1.sizes(), " is not the (B, C, H, W) that f1h ", f1h.sizes(), " (B, H, W, C) was prepared from");
  return corr_lookup_otf(run, f1h, f2h, coords, radius);
}

// (grad_fmap1, grad_fmap2) as (B, C, H, W) fp32; an output not wanted is an empty (0-element) tensor and the kernel gets
// a null pointer for it (no GEMM / no scratch, no atomics). The per-level NHWC scratch of grad_fmap2 is allocated here:
// B*C*sum_l H_l*W_l floats, nothing that scales with (HW)^2.
std::tuple<Tensor, Tensor> corr_lookup_alt_backward(bool run, const Tensor& gout, const Tensor& f1h,
                                                    const std::vector<Tensor>& f2h, const Tensor& coords,
                                                    int64_t radius, std::array<bool, 2> om) {
  const char* what = "corr_lookup_alt backward";
  check_coords(coords, what);
  if (run) TORCH_CHECK(coords.is_cuda() && gout.is_cuda(), what, ": coords is on ", coords.device(), ", grad_out on ",
                       gout.device(), kNoCpu);
  check_radius(radius, 4, what);
  const int64_t b = coords.size(0), h = coords.size(2), w = coords.size(3), nl = (int64_t)f2h.size();
  const int64_t c = check_f1h(f1h, nl, coords, what);
  const int64_t k = 2 * radius + 1;
  TORCH_CHECK(gout.dim() == 4 && gout.size(0) == b && gout.size(1) == nl * k * k && gout.size(2) == h && gout.size(3) == w,
              what, ": grad_out ", gout.sizes(), " must be (", b, ", ", nl * k * k, ", ", h, ", ", w, ")");
  TORCH_CHECK(gout.device() == coords.device() && f1h.device() == coords.device(), what,
              ": grad_out, f1h and coords are on different devices");
  int hs[OFLOW_MAX_LEVELS], ws[OFLOW_MAX_LEVELS];
  const int64_t pix = check_f2h_levels(f2h, coords, c, hs, ws, what);
  TORCH_CHECK(hs[0] == h && ws[0] == w, what, ": fmap2 level 0 ", f2h[0].sizes(), " must be (", b, ", ", h, ", ", w, ", C)");
  const auto opt = coords.options().dtype(at::kFloat);
  Tensor g1 = wanted(om[0], {b, c, h, w}, opt), g2 = wanted(om[1], {b, c, h, w}, opt);
  if (!run || b * c * h * w == 0 || (!om[0] && !om[1])) return {g1, g2};
  Tensor go = gpu_f32(gout, "grad_out", what), co = gpu_f32(coords, "coords", what);
  const void* ptrs[OFLOW_MAX_LEVELS];
  for (int64_t i = 0; i < nl; ++i) ptrs[i] = f2h[i].data_ptr();
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  Tensor scratch = om[1] ? at::empty({b * c * pix}, opt) : at::empty({0}, opt);
  check_status(oflow_corr_lookup_otf_backward_f32(go.data_ptr<float>(), f1h.data_ptr(), ptrs, hs, ws, (int)nl,
                                                  co.data_ptr<float>(), (int)b, (int)c, (int)h, (int)w, (int)radius,
                                                  om[0] ? g1.data_ptr<float>() : nullptr,
                                                  om[1] ? g2.data_ptr<float>() : nullptr,
                                                  om[1] ? scratch.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {g1, g2};
}

// ---------------------------------------------------------------- warp / grid_sample
void check_modes(int64_t mode, int64_t pad, const char* what) {
  TORCH_CHECK_VALUE(mode >= 0 && mode <= 2, what, ": interpolation mode ", mode, " is not 0 (bilinear), 1 (nearest) or 2 (bicubic)");
  TORCH_CHECK_VALUE(pad >= 0 && pad <= 2, what, ": padding mode ", pad, " is not 0 (zeros), 1 (border) or 2 (reflection)");
}

void check_warp(const Tensor& fr, const Tensor& fl, const char* what) {
  TORCH_CHECK(fr.dim() == 4 && fl.dim() == 4 && fl.size(1) == 2 && fl.size(0) == fr.size(0) && fl.size(2) == fr.size(2) &&
                  fl.size(3) == fr.size(3),
              what, ": frame ", fr.sizes(), " must be (B, C, H, W) and flow ", fl.sizes(), " (B, 2, H, W)");
  TORCH_CHECK(fr.device() == fl.device(), what, ": frame and flow are on different devices");
}

Tensor grid_warp(bool run, const Tensor& frame, const Tensor& flow, int64_t mode, int64_t pad, bool align_corners) {
  const char* what = "warp";
  check_modes(mode, pad, what);
  check_warp(frame, flow, what);
  if (!run) return at::empty(frame.sizes(), frame.options().dtype(at::kFloat));
  Tensor fr = gpu_f32(frame, "frame", what), fl = gpu_f32(flow, "flow", what);
  Tensor out = at::empty_like(fr);
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(fr.device());
  check_status(oflow_grid_warp_f32(fr.data_ptr<float>(), fl.data_ptr<float>(), (int)fr.size(0), (int)fr.size(1),
                                   (int)fr.size(2), (int)fr.size(3), (int)mode, (int)pad, align_corners ? 1 : 0,
                                   out.data_ptr<float>(), cur_stream()),
               what);
  return out;
}

void check_sample(const Tensor& x, const Tensor& g, const char* what) {
  TORCH_CHECK(x.dim() == 4 && g.dim() == 4 && g.size(3) == 2 && g.size(0) == x.size(0), what, ": input ", x.sizes(),
              " must be (B, C, H, W) and grid ", g.sizes(), " (B, Ho, Wo, 2)");
  TORCH_CHECK(x.device() == g.device(), what, ": input and grid are on different devices");
}

Tensor grid_sample(bool run, const Tensor& input, const Tensor& grid, int64_t mode, int64_t pad, bool align_corners) {
  const char* what = "grid_sample";
  check_modes(mode, pad, what);
  check_sample(input, grid, what);
  if (!run)
    return at::empty({input.size(0), input.size(1), grid.size(1), grid.size(2)}, input.options().dtype(at::kFloat));
  Tensor x = gpu_f32(input, "input", what), gr = gpu_f32(grid, "grid", what);
  Tensor out = at::empty({x.size(0), x.size(1), gr.size(1), gr.size(2)}, x.options());
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  check_status(oflow_grid_sample_f32(x.data_ptr<float>(), gr.data_ptr<float>(), (int)x.size(0), (int)x.size(1),
                                     (int)x.size(2), (int)x.size(3), (int)gr.size(1), (int)gr.size(2), (int)mode,
                                     (int)pad, align_corners ? 1 : 0, out.data_ptr<float>(), cur_stream()),
               what);
  return out;
}

// warp / grid_sample backward (warp_backward.hip): (grad_frame, grad_flow) / (grad_input, grad_grid)
// output_mask (ATen grid_sampler_2d_backward's): an output not wanted is returned as an empty (0-element) tensor and
// the kernel gets a null pointer for it (no zero fill, no atomics for grad_frame)
std::tuple<Tensor, Tensor> grid_warp_backward(bool run, const Tensor& gout, const Tensor& frame, const Tensor& flow,
                                              int64_t mode, int64_t pad, bool ac, std::array<bool, 2> mask) {
  const char* what = "warp backward";
  check_modes(mode, pad, what);
  check_warp(frame, flow, what);
  TORCH_CHECK(gout.sizes() == frame.sizes(), what, ": grad_out ", gout.sizes(), " must match the frame ", frame.sizes());
  const auto fopt = frame.options().dtype(at::kFloat), lopt = flow.options().dtype(at::kFloat);
  if (!run) return {wanted(mask[0], frame.sizes(), fopt), wanted(mask[1], flow.sizes(), lopt)};
  Tensor go = gpu_f32(gout, "grad_out", what), fr = gpu_f32(frame, "frame", what), fl = gpu_f32(flow, "flow", what);
  Tensor gfr = mask[0] ? at::zeros_like(fr) : at::empty({0}, fopt), gfl = mask[1] ? at::empty_like(fl) : at::empty({0}, lopt);
  if (fr.numel() == 0) return {gfr, gfl.zero_()};
  if (!mask[0] && !mask[1]) return {gfr, gfl};
  c10::hip::HIPGuardMasqueradingAsCUDA g(fr.device());
  check_status(oflow_grid_warp_backward_f32(go.data_ptr<float>(), fr.data_ptr<float>(), fl.data_ptr<float>(), (int)fr.size(0),
                                            (int)fr.size(1), (int)fr.size(2), (int)fr.size(3), (int)mode, (int)pad, ac ? 1 : 0,
                                            mask[0] ? gfr.data_ptr<float>() : nullptr,
                                            mask[1] ? gfl.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {gfr, gfl};
}

std::tuple<Tensor, Tensor> grid_sample_backward(bool run, const Tensor& gout, const Tensor& input, const Tensor& grid,
                                                int64_t mode, int64_t pad, bool ac, std::array<bool, 2> mask) {
  const char* what = "grid_sample backward";
  check_modes(mode, pad, what);
  check_sample(input, grid, what);
  TORCH_CHECK(gout.dim() == 4 && gout.size(0) == input.size(0) && gout.size(1) == input.size(1) &&
                  gout.size(2) == grid.size(1) && gout.size(3) == grid.size(2),
              what, ": grad_out ", gout.sizes(), " must be (B, C, Ho, Wo)");
  const auto xopt = input.options().dtype(at::kFloat), gopt = grid.options().dtype(at::kFloat);
  if (!run) return {wanted(mask[0], input.sizes(), xopt), wanted(mask[1], grid.sizes(), gopt)};
  Tensor go = gpu_f32(gout, "grad_out", what), x = gpu_f32(input, "input", what), gr = gpu_f32(grid, "grid", what);
  Tensor gx = mask[0] ? at::zeros_like(x) : at::empty({0}, xopt), gg = mask[1] ? at::empty_like(gr) : at::empty({0}, gopt);
  if (go.numel() == 0) return {gx, gg.zero_()};
  if (!mask[0] && !mask[1]) return {gx, gg};
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  check_status(oflow_grid_sample_backward_f32(go.data_ptr<float>(), x.data_ptr<float>(), gr.data_ptr<float>(), (int)x.size(0),
                                              (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)gr.size(1), (int)gr.size(2),
                                              (int)mode, (int)pad, ac ? 1 : 0, mask[0] ? gx.data_ptr<float>() : nullptr,
                                              mask[1] ? gg.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {gx, gg};
}

// ---------------------------------------------------------------- backward (training path, §8(f) row 3)
std::vector<Tensor> corr_lookup_backward(bool run, const Tensor& grad_out, const Tensor& coords, int64_t radius,
                                         int64_t h0, int64_t w0, int64_t nl) {
  const char* what = "corr_lookup_backward";
  check_coords(coords, what);
  check_radius(radius, OFLOW_MAX_RADIUS, what);
  const int64_t b = coords.size(0), h = coords.size(2), w = coords.size(3), k = 2 * radius + 1;
  TORCH_CHECK(grad_out.dim() == 4 && grad_out.size(0) == b && grad_out.size(1) == nl * k * k && grad_out.size(2) == h &&
                  grad_out.size(3) == w,
              what, ": grad_out ", grad_out.sizes(), " does not match coords / levels");
  auto d = dims_of(h0, w0, nl, what);
  if (run) check_on_gpu(coords, "coords", what);
  std::vector<Tensor> grads;
  auto opt = coords.options().dtype(at::kFloat);
  for (auto& p : d) grads.push_back(run ? at::zeros({b * h * w, 1, p.first, p.second}, opt)
                                        : at::empty({b * h * w, 1, p.first, p.second}, opt));
  if (!run || b * h * w == 0) return grads;
  Tensor go = gpu_f32(grad_out, "grad_out", what), co = gpu_f32(coords, "coords", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(co.device());
  float* ptrs[OFLOW_MAX_LEVELS];
  int hs[OFLOW_MAX_LEVELS], ws[OFLOW_MAX_LEVELS];
  for (int64_t l = 0; l < nl; ++l) {
    ptrs[l] = grads[l].data_ptr<float>();
    hs[l] = d[l].first;
    ws[l] = d[l].second;
  }
  check_status(oflow_corr_lookup_backward_f32(go.data_ptr<float>(), co.data_ptr<float>(), (int)b, (int)h, (int)w,
                                              (int)radius, ptrs, hs, ws, (int)nl, cur_stream()),
               what);
  return grads;
}

// grads[0] += every coarser level's gradient pushed back through the floor 2x2 pools (native kernel), then
// grad_f1 = f2 . G^T / sqrt(C), grad_f2 = f1 . G / sqrt(C) as batched GEMMs on the fp32 matrix cores
// (oflow_corr_fmap_grad_f32, csrc/corr_backward.hip)
std::tuple<Tensor, Tensor> corr_pyramid_backward(bool run, const std::vector<Tensor>& level_grads, const Tensor& fmap1,
                                                 const Tensor& fmap2) {
  const char* what = "corr_pyramid_backward";
  check_fmaps(fmap1, fmap2, what);
  const int64_t b = fmap1.size(0), c = fmap1.size(1), h = fmap1.size(2), w = fmap1.size(3), n = h * w;
  const int64_t nl = (int64_t)level_grads.size();
  auto d = dims_of(h, w, nl, what);
  if (!run) return {at::empty_like(fmap1), at::empty_like(fmap2)};
  std::vector<Tensor> gl;
  for (int64_t l = 0; l < nl; ++l) {
    Tensor t = gpu_f32(level_grads[l], "level gradient", what);
    TORCH_CHECK(t.numel() == b * n * d[l].first * d[l].second, what, ": level ", l, " gradient ", t.sizes(),
                " does not match the pyramid");
    gl.push_back(l == 0 ? t.clone() : t);  // level 0 is accumulated in place
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(fmap1.device());
  if (b * n > 0) {
    float* ptrs[OFLOW_MAX_LEVELS];
    int hs[OFLOW_MAX_LEVELS], ws[OFLOW_MAX_LEVELS];
    for (int64_t l = 0; l < nl; ++l) {
      ptrs[l] = gl[l].data_ptr<float>();
      hs[l] = d[l].first;
      ws[l] = d[l].second;
    }
    check_status(oflow_corr_pyramid_grad_combine_f32(ptrs, hs, ws, (int)nl, b * n, cur_stream()), what);
  }
  // the fmap gradients on the fp32 matrix cores (corr_backward.hip): scale as the forward, 1/sqrt(float(C))
  const float s = 1.0f / std::sqrt(static_cast<float>(c));
  Tensor f1m = fmap1.to(at::kFloat).contiguous(), f2m = fmap2.to(at::kFloat).contiguous();
  Tensor g1 = at::empty({b, c, h, w}, f1m.options()), g2 = at::empty({b, c, h, w}, f2m.options());
  check_status(oflow_corr_fmap_grad_f32(f1m.data_ptr<float>(), f2m.data_ptr<float>(), gl[0].data_ptr<float>(), (int)b,
                                        (int)c, (int)n, s, g1.data_ptr<float>(), g2.data_ptr<float>(), cur_stream()),
               what);
  return {g1.to(fmap1.scalar_type()), g2.to(fmap2.scalar_type())};
}

// ---------------------------------------------------------------- metrics / sequence loss (flow_metrics.hip)
void check_flow_pair(const Tensor& pred, const Tensor& target, const char* what) {
  TORCH_CHECK(pred.dim() == 4 && pred.size(1) == 2 && pred.sizes() == target.sizes(), what, ": pred ", pred.sizes(),
              " and target ", target.sizes(), " must be equal (B, 2, H, W)");
  TORCH_CHECK(pred.device() == target.device(), what, ": pred and target are on different devices");
  TORCH_CHECK(pred.size(0) <= INT_MAX && pred.size(2) <= INT_MAX && pred.size(3) <= INT_MAX, what, ": a size exceeds 2^31");
}

// fp32 with unit stride along W; batch / channel / row strides stay as they are (a cropped view is read in place)
Tensor strided_f32(const Tensor& t) {
  Tensor f = t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
  return (f.size(3) > 1 && f.stride(3) != 1) ? f.contiguous() : f;
}

struct ValidArg {
  Tensor t;
  int kind = OFLOW_VALID_NONE;
  int64_t sb = 0, sh = 0;
  const void* ptr() const { return kind == OFLOW_VALID_NONE ? nullptr : t.data_ptr(); }
};

void check_valid(const Tensor& v, const Tensor& flow, const char* what) {
  TORCH_CHECK(v.numel() == flow.size(0) * flow.size(2) * flow.size(3), what, ": valid ", v.sizes(),
              " must have one element per pixel of ", flow.sizes());
  TORCH_CHECK(v.device() == flow.device(), what, ": valid is on another device than the flow");
}

// valid as (B, H, W) with unit W stride: bool / uint8 as they are (1 byte), anything else as fp32
ValidArg valid_arg(const Tensor& valid, const Tensor& flow, bool need_contiguous) {
  ValidArg a;
  const int64_t b = flow.size(0), h = flow.size(2), w = flow.size(3);
  const bool bytes = valid.scalar_type() == at::kBool || valid.scalar_type() == at::kByte;
  Tensor v = (bytes || valid.scalar_type() == at::kFloat) ? valid : valid.to(at::kFloat);
  if (v.dim() == 4 && v.size(1) == 1) v = v.select(1, 0);
  const bool shaped = v.dim() == 3 && v.size(0) == b && v.size(1) == h && v.size(2) == w && (w == 1 || v.stride(2) == 1);
  if (!shaped || need_contiguous) v = v.reshape({b, h, w}).contiguous();
  a.t = v;
  a.kind = bytes ? OFLOW_VALID_U8 : OFLOW_VALID_F32;
  a.sb = v.stride(0);
  a.sh = v.stride(1);
  return a;
}

Tensor flow_error_stats(bool run, const Tensor& pred, const Tensor& target, const c10::optional<Tensor>& valid,
                        double abs_t, double rel_t, double max_flow, const Tensor& accum, bool epe_map) {
  const char* what = "flow_error_stats";
  check_flow_pair(pred, target, what);
  if (valid.has_value()) check_valid(*valid, pred, what);
  TORCH_CHECK(accum.scalar_type() == at::kDouble && accum.dim() == 1 && accum.size(0) == 8 && accum.is_contiguous() &&
                  accum.device() == pred.device(),
              what, ": the accumulator must be a contiguous float64 [8] on the flow's device, got ", accum.sizes());
  const int64_t b = pred.size(0), h = pred.size(2), w = pred.size(3);
  if (run) check_on_gpu(pred, "pred", what);
  Tensor map = wanted(epe_map, {b, h, w}, pred.options().dtype(at::kFloat));
  if (!run || b * h * w == 0) return map;
  Tensor pr = strided_f32(pred), tg = strided_f32(target);
  ValidArg va;
  if (valid.has_value()) va = valid_arg(*valid, pr, false);
  c10::hip::HIPGuardMasqueradingAsCUDA g(pr.device());
  Tensor ws = at::empty({OFLOW_FLOW_METRICS_PARTIALS * 8}, pr.options().dtype(at::kDouble));
  check_status(oflow_flow_error_stats_f32(pr.data_ptr<float>(), pr.stride(0), pr.stride(1), pr.stride(2),
                                          tg.data_ptr<float>(), tg.stride(0), tg.stride(1), tg.stride(2), va.ptr(), va.kind,
                                          va.sb, va.sh, (int)b, (int)h, (int)w, (float)abs_t, (float)rel_t, (float)max_flow,
                                          epe_map ? map.data_ptr<float>() : nullptr, ws.data_ptr<double>(),
                                          accum.data_ptr<double>(), cur_stream()),
               what);
  return map;
}

void check_loss_args(const std::vector<Tensor>& preds, const Tensor& gt, const Tensor& valid, at::ArrayRef<double> weights,
                     const char* what) {
  const int64_t n = (int64_t)preds.size();
  TORCH_CHECK(n >= 1 && n <= OFLOW_MAX_PREDS, what, ": number of flow predictions ", n, " outside [1, ", OFLOW_MAX_PREDS, "]");
  TORCH_CHECK((int64_t)weights.size() == n, what, ": ", weights.size(), " weights for ", n, " predictions");
  for (int64_t i = 0; i < n; ++i) check_flow_pair(preds[i], gt, what);
  check_valid(valid, gt, what);
}

std::tuple<Tensor, Tensor> sequence_loss(bool run, const std::vector<Tensor>& preds, const Tensor& gt,
                                         const Tensor& valid, at::ArrayRef<double> weights, double max_flow) {
  const char* what = "sequence_loss";
  check_loss_args(preds, gt, valid, weights, what);
  Tensor loss = at::empty({}, gt.options().dtype(at::kFloat)), stats = at::empty({8}, gt.options().dtype(at::kDouble));
  if (!run) return {loss, stats};
  check_on_gpu(gt, "flow_gt", what);
  const int64_t b = gt.size(0), h = gt.size(2), w = gt.size(3), n = (int64_t)preds.size();
  if (b * h * w == 0)  // the mean of no elements
    return {loss.fill_(std::numeric_limits<float>::quiet_NaN()), stats.zero_()};
  Tensor g32 = gpu_f32(gt, "flow_gt", what);
  ValidArg va = valid_arg(valid, g32, true);
  std::vector<Tensor> keep;
  const float* ptrs[OFLOW_MAX_PREDS];
  float wts[OFLOW_MAX_PREDS];
  for (int64_t i = 0; i < n; ++i) {
    keep.push_back(gpu_f32(preds[i], "flow_preds", what));
    ptrs[i] = keep.back().data_ptr<float>();
    wts[i] = (float)weights[i];
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(g32.device());
  Tensor ws = at::empty({OFLOW_FLOW_METRICS_PARTIALS * 8}, stats.options());
  check_status(oflow_sequence_loss_f32(ptrs, (int)n, wts, g32.data_ptr<float>(), va.ptr(), va.kind, (int)b, (int)h, (int)w,
                                       (float)max_flow, ws.data_ptr<double>(), loss.data_ptr<float>(),
                                       stats.data_ptr<double>(), cur_stream()),
               what);
  return {loss, stats};
}

// one gradient per prediction; a prediction with need[i] == 0 gets an empty (0-element) tensor and the kernel a null
// pointer for it (nothing read or written for that prediction)
std::vector<Tensor> sequence_loss_backward(bool run, const Tensor& gout, const std::vector<Tensor>& preds,
                                           const Tensor& gt, const Tensor& valid, at::ArrayRef<double> weights,
                                           double max_flow, at::IntArrayRef need) {
  const char* what = "sequence_loss backward";
  check_loss_args(preds, gt, valid, weights, what);
  const int64_t n = (int64_t)preds.size();
  TORCH_CHECK((int64_t)need.size() == n, what, ": ", need.size(), " gradient flags for ", n, " predictions");
  TORCH_CHECK(gout.numel() == 1 && gout.device() == gt.device(), what, ": grad_out must be one element on the flow's device");
  std::vector<Tensor> grads;
  for (int64_t i = 0; i < n; ++i) grads.push_back(wanted(need[i] != 0, gt.sizes(), gt.options().dtype(at::kFloat)));
  if (!run) return grads;
  check_on_gpu(gt, "flow_gt", what);
  const int64_t b = gt.size(0), h = gt.size(2), w = gt.size(3);
  if (b * h * w == 0) return grads;
  Tensor g32 = gpu_f32(gt, "flow_gt", what), go = gpu_f32(gout, "grad_out", what).reshape({1});
  ValidArg va = valid_arg(valid, g32, true);
  std::vector<Tensor> keep;
  const float* ptrs[OFLOW_MAX_PREDS];
  float* gptrs[OFLOW_MAX_PREDS];
  float wts[OFLOW_MAX_PREDS];
  for (int64_t i = 0; i < n; ++i) {
    keep.push_back(gpu_f32(preds[i], "flow_preds", what));
    ptrs[i] = keep.back().data_ptr<float>();
    gptrs[i] = need[i] ? grads[i].data_ptr<float>() : nullptr;
    wts[i] = (float)weights[i];
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(g32.device());
  check_status(oflow_sequence_loss_backward_f32(go.data_ptr<float>(), ptrs, gptrs, (int)n, wts, g32.data_ptr<float>(),
                                                va.ptr(), va.kind, (int)b, (int)h, (int)w, (float)max_flow, cur_stream()),
               what);
  return grads;
}

// ---------------------------------------------------------------- convex upsampling (upsample.hip, upsample_backward.hip)
void check_upsample(const Tensor& flow, const Tensor& mask, const char* what) {
  TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2 && mask.dim() == 4 && mask.size(1) == 576 &&
                  mask.size(0) == flow.size(0) && mask.size(2) == flow.size(2) && mask.size(3) == flow.size(3),
              what, ": flow ", flow.sizes(), " must be (B, 2, H, W) and mask ", mask.sizes(), " (B, 576, H, W)");
  TORCH_CHECK(flow.device() == mask.device(), what, ": flow and mask are on different devices");
  TORCH_CHECK(flow.size(0) <= 65535 && flow.size(2) <= 65535 && flow.size(3) <= INT_MAX / 8, what, ": flow ", flow.sizes(),
              " is past the kernel's grid (B, H <= 65535, 8 W < 2^31)");
}

Tensor convex_upsample(bool run, const Tensor& flow, const Tensor& mask) {
  const char* what = "upsample_flow";
  if (run) check_on_gpu(flow, "flow", what), check_on_gpu(mask, "mask", what);
  check_upsample(flow, mask, what);
  const int64_t b = flow.size(0), h = flow.size(2), w = flow.size(3);
  if (!run) return at::empty({b, 2, 8 * h, 8 * w}, flow.options().dtype(at::kFloat));
  Tensor fl = gpu_f32(flow, "flow", what), mk = gpu_f32(mask, "mask", what);
  Tensor out = at::empty({b, 2, 8 * h, 8 * w}, fl.options());
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(fl.device());
  check_status(oflow_convex_upsample_f32(fl.data_ptr<float>(), mk.data_ptr<float>(), (int)b, (int)h, (int)w,
                                         out.data_ptr<float>(), cur_stream()),
               what);
  return out;
}

// (grad_flow, grad_mask); an output not wanted is an empty (0-element) tensor and the kernel gets a null pointer for it
// (no grad_mask stores / no flow phase). The (B, 18, H, W) tap-sum scratch of the flow gradient is allocated here.
std::tuple<Tensor, Tensor> convex_upsample_backward(bool run, const Tensor& gout, const Tensor& flow, const Tensor& mask,
                                                    std::array<bool, 2> om) {
  const char* what = "upsample_flow backward";
  if (run) check_on_gpu(gout, "grad_out", what), check_on_gpu(flow, "flow", what), check_on_gpu(mask, "mask", what);
  check_upsample(flow, mask, what);
  const int64_t b = flow.size(0), h = flow.size(2), w = flow.size(3);
  TORCH_CHECK(gout.dim() == 4 && gout.size(0) == b && gout.size(1) == 2 && gout.size(2) == 8 * h && gout.size(3) == 8 * w,
              what, ": grad_out ", gout.sizes(), " must be (B, 2, 8H, 8W) of flow ", flow.sizes());
  TORCH_CHECK(gout.device() == flow.device(), what, ": grad_out and flow are on different devices");
  const auto fopt = flow.options().dtype(at::kFloat), mopt = mask.options().dtype(at::kFloat);
  if (!run) return {wanted(om[0], flow.sizes(), fopt), wanted(om[1], mask.sizes(), mopt)};
  Tensor go = gpu_f32(gout, "grad_out", what), fl = gpu_f32(flow, "flow", what), mk = gpu_f32(mask, "mask", what);
  Tensor gf = om[0] ? at::empty_like(fl) : at::empty({0}, fopt), gm = om[1] ? at::empty_like(mk) : at::empty({0}, mopt);
  if (fl.numel() == 0 || (!om[0] && !om[1])) return {gf, gm};
  c10::hip::HIPGuardMasqueradingAsCUDA g(fl.device());
  Tensor scratch = om[0] ? at::empty({b, 18, h, w}, fopt) : at::empty({0}, fopt);
  check_status(oflow_convex_upsample_backward_f32(go.data_ptr<float>(), fl.data_ptr<float>(), mk.data_ptr<float>(), (int)b,
                                                  (int)h, (int)w, om[0] ? gf.data_ptr<float>() : nullptr,
                                                  om[1] ? gm.data_ptr<float>() : nullptr,
                                                  om[0] ? scratch.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {gf, gm};
}

// (grad_x, grad_weight, grad_bias) of the conv and norm layers: an output not wanted is an empty (0-element) tensor and
// is not formed. With no pixels the parameter gradients are empty sums:
Tensor3 zero_param_grads(Tensor gx, Tensor gw, Tensor gb, std::array<bool, 3> om) {
  if (om[1]) gw.zero_();
  if (om[2]) gb.zero_();
  return Tensor3(gx, gw, gb);
}

// ---------------------------------------------------------------- convolutions under autograd (conv_backward.hip)
// conv2d_same (the update block's layers: stride 1) and conv2d_strided (the encoders': stride 1 or 2) are one forward
// and one backward. The geometry the native backward covers: dilation 1, groups 1, odd kernel <= 7, zero padding
// (kh/2, kw/2); the output is ((H + s - 1) / s, (W + s - 1) / s). No stride means conv2d_same: its own messages and the
// stride-1 entry points of conv_backward.hip, which differ from the strided ones at stride 1 in the summation order of
// the weight gradient (those fold (channel, tap) for a small Cin).
using Stride = c10::optional<int64_t>;
void check_conv(const Tensor& x, const Tensor& weight, Stride stride, const char* what) {
  TORCH_CHECK(x.dim() == 4 && weight.dim() == 4 && weight.size(1) == x.size(1), what, ": x ", x.sizes(),
              " must be (B, Cin, H, W) and weight ", weight.sizes(), " (Cout, Cin, kh, kw) (groups = 1)");
  const int64_t kh = weight.size(2), kw = weight.size(3);
  TORCH_CHECK(kh % 2 == 1 && kw % 2 == 1 && kh <= 7 && kw <= 7, what, ": kernel ", kh, " x ", kw,
              " is not supported (odd sizes up to 7, stride 1, zero padding (kh/2, kw/2))");
  TORCH_CHECK(x.scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat, what, ": x and weight must be float32, got ",
              x.scalar_type(), " and ", weight.scalar_type());
  TORCH_CHECK(x.device() == weight.device(), what, ": x and weight are on different devices");
  TORCH_CHECK(weight.size(0) >= 1 && weight.size(1) >= 1, what, ": weight ", weight.sizes(), " has no channels");
  if (stride) TORCH_CHECK(*stride == 1 || *stride == 2, what, ": stride ", *stride, " is not supported (1 or 2, the same in y and x)");
}

Tensor conv2d_forward(bool run, const Tensor& x, const Tensor& weight, const c10::optional<Tensor>& bias, Stride strided) {
  const char* what = strided ? "conv2d_strided" : "conv2d_same";
  if (run) check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_conv(x, weight, strided, what);
  const int64_t stride = strided.value_or(1);
  if (bias.has_value())
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == weight.size(0) && bias->scalar_type() == at::kFloat &&
                    bias->device() == x.device(),
                what, ": bias must be float32 (Cout) on x's device, got ", bias->scalar_type(), " ", bias->sizes());
  if (!run)
    return at::empty({x.size(0), weight.size(0), (x.size(2) + stride - 1) / stride, (x.size(3) + stride - 1) / stride},
                     x.options());
  // the forward is the nn.Conv2d's own call (ATen / MIOpen): the same bits; only the backward is replaced
  return at::conv2d(x, weight, bias, {stride, stride}, {weight.size(2) / 2, weight.size(3) / 2}, {1, 1}, 1);
}

// The K-slab workspace of the weight / bias gradient is allocated here (uninitialised: the kernels write all of it they
// read).
Tensor3 conv2d_backward(bool run, const Tensor& gout, const Tensor& x, const Tensor& weight, Stride strided,
                        std::array<bool, 3> om) {
  const char* what = strided ? "conv2d_strided backward" : "conv2d_same backward";
  if (run) check_on_gpu(gout, "grad_out", what), check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_conv(x, weight, strided, what);
  const int64_t stride = strided.value_or(1);
  const int64_t b = x.size(0), cin = x.size(1), h = x.size(2), w = x.size(3);
  const int64_t cout = weight.size(0), kh = weight.size(2), kw = weight.size(3);
  const int64_t ho = (h + stride - 1) / stride, wo = (w + stride - 1) / stride;
  TORCH_CHECK(gout.dim() == 4 && gout.size(0) == b && gout.size(1) == cout && gout.size(2) == ho && gout.size(3) == wo &&
                  gout.scalar_type() == at::kFloat,
              what, ": grad_out ", gout.sizes(), " must be float32 (B, Cout, ", strided ? "H', W'" : "H, W", ") = (", b, ", ",
              cout, ", ", ho, ", ", wo, ")");
  TORCH_CHECK(gout.device() == x.device(), what, ": grad_out and x are on different devices");
  const auto opt = x.options();
  Tensor gx = wanted(om[0], x.sizes(), opt), gw = wanted(om[1], weight.sizes(), opt), gb = wanted(om[2], {cout}, opt);
  if (!run || !(om[0] || om[1] || om[2])) return Tensor3(gx, gw, gb);
  if (x.numel() == 0) return zero_param_grads(gx, gw, gb, om);
  TORCH_CHECK(b <= INT_MAX && h <= INT_MAX && w <= INT_MAX && cout <= INT_MAX && cin <= INT_MAX, what, ": x ", x.sizes(),
              " is past the kernels' index range");
  Tensor go = gout.contiguous(), xc = x.contiguous(), wc = weight.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA g(xc.device());
  const int B = (int)b, Co = (int)cout, Ci = (int)cin, H = (int)h, W = (int)w, KH = (int)kh, KW = (int)kw, S = (int)stride;
  if (om[0])
    check_status(strided ? oflow_conv2d_strided_backward_input_f32(go.data_ptr<float>(), wc.data_ptr<float>(), B, Co, Ci, H,
                                                                   W, KH, KW, S, gx.data_ptr<float>(), cur_stream())
                         : oflow_conv2d_backward_input_f32(go.data_ptr<float>(), wc.data_ptr<float>(), B, Co, Ci, H, W, KH,
                                                           KW, gx.data_ptr<float>(), cur_stream()),
                 what);
  if (om[1] || om[2]) {
    const long long n = strided ? oflow_conv2d_strided_backward_weight_workspace_floats(B, Co, Ci, H, W, KH, KW, S)
                                : oflow_conv2d_backward_weight_workspace_floats(B, Co, Ci, H, W, KH, KW);
    Tensor ws = at::empty({(int64_t)n}, opt);
    float* pgw = om[1] ? gw.data_ptr<float>() : nullptr;
    float* pgb = om[2] ? gb.data_ptr<float>() : nullptr;
    check_status(strided ? oflow_conv2d_strided_backward_weight_f32(go.data_ptr<float>(), xc.data_ptr<float>(), B, Co, Ci, H,
                                                                    W, KH, KW, S, pgw, pgb, ws.data_ptr<float>(), cur_stream())
                         : oflow_conv2d_backward_weight_f32(go.data_ptr<float>(), xc.data_ptr<float>(), B, Co, Ci, H, W, KH,
                                                            KW, pgw, pgb, ws.data_ptr<float>(), cur_stream()),
                 what);
  }
  return Tensor3(gx, gw, gb);
}

Tensor conv2d_same(bool run, const Tensor& x, const Tensor& weight, const c10::optional<Tensor>& bias) {
  return conv2d_forward(run, x, weight, bias, c10::nullopt);
}
Tensor conv2d_strided(bool run, const Tensor& x, const Tensor& weight, const c10::optional<Tensor>& bias, int64_t stride) {
  return conv2d_forward(run, x, weight, bias, stride);
}
Tensor3 conv2d_same_backward(bool run, const Tensor& gout, const Tensor& x, const Tensor& weight, std::array<bool, 3> om) {
  return conv2d_backward(run, gout, x, weight, c10::nullopt, om);
}
Tensor3 conv2d_strided_backward(bool run, const Tensor& gout, const Tensor& x, const Tensor& weight, int64_t stride,
                                std::array<bool, 3> om) {
  return conv2d_backward(run, gout, x, weight, stride, om);
}

// ---------------------------------------------------------------- encoder norm layers under autograd (norm_backward.hip)
void check_norm_input(const Tensor& x, const char* what) {
  TORCH_CHECK(x.dim() == 4 && x.scalar_type() == at::kFloat, what, ": x must be float32 (B, C, H, W), got ", x.scalar_type(),
              " ", x.sizes());
  TORCH_CHECK(x.size(1) >= 1, what, ": x ", x.sizes(), " has no channels");
}
void check_norm_grad(const Tensor& gout, const Tensor& x, const char* what) {
  TORCH_CHECK(gout.sizes() == x.sizes() && gout.scalar_type() == at::kFloat, what, ": grad_out ", gout.sizes(),
              " must be float32 of x's shape ", x.sizes());
  TORCH_CHECK(gout.device() == x.device(), what, ": grad_out and x are on different devices");
  TORCH_CHECK(x.size(0) * x.size(1) <= INT_MAX && x.size(2) * x.size(3) <= INT_MAX, what, ": x ", x.sizes(),
              " is past the kernels' index range");
}

// the per-channel vectors of a batch norm, each float32 (C) on x's device
using NamedTensors = std::initializer_list<std::pair<const char*, const Tensor*>>;
void check_channel_vectors(const Tensor& x, NamedTensors params, const char* what) {
  for (auto& p : params)
    TORCH_CHECK(p.second->dim() == 1 && p.second->size(0) == x.size(1) && p.second->scalar_type() == at::kFloat &&
                    p.second->device() == x.device(),
                what, ": ", p.first, " must be float32 (C) on x's device, got ", p.second->scalar_type(), " ",
                p.second->sizes());
}

// relu(instance_norm(x)) / instance_norm(x) of an nn.InstanceNorm2d without affine parameters or running statistics
Tensor instance_norm_act(bool run, const Tensor& x, double eps, bool relu) {
  const char* what = "instance_norm_act";
  if (run) check_on_gpu(x, "x", what);
  check_norm_input(x, what);
  if (!run) return at::empty(x.sizes(), x.options());
  // the module's own ATen call (F.instance_norm with use_input_stats) and nn.ReLU's: the same bits
  Tensor y = at::instance_norm(x, {}, {}, {}, {}, true, 0.1, eps, at::globalContext().userEnabledCuDNN());
  return relu ? at::relu_(y) : y;
}

Tensor instance_norm_act_backward(bool run, const Tensor& gout, const Tensor& x, double eps, bool relu) {
  const char* what = "instance_norm_act backward";
  if (run) check_on_gpu(gout, "grad_out", what), check_on_gpu(x, "x", what);
  check_norm_input(x, what);
  check_norm_grad(gout, x, what);
  Tensor gx = at::empty(x.sizes(), x.options());
  if (!run || x.numel() == 0) return gx;
  Tensor go = gout.contiguous(), xc = x.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA g(xc.device());
  check_status(oflow_instance_norm_backward_f32(go.data_ptr<float>(), xc.data_ptr<float>(), (int)(x.size(0) * x.size(1)),
                                                (int)(x.size(2) * x.size(3)), eps, relu ? 1 : 0, gx.data_ptr<float>(),
                                                cur_stream()),
               what);
  return gx;
}

// relu(batch_norm(x)) / batch_norm(x) of an nn.BatchNorm2d on its running statistics (eval mode)
Tensor frozen_batch_norm_act(bool run, const Tensor& x, const Tensor& weight, const Tensor& bias, const Tensor& rm,
                             const Tensor& rv, double eps, bool relu) {
  const char* what = "frozen_batch_norm_act";
  if (run) check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_norm_input(x, what);
  check_channel_vectors(x, {{"weight", &weight}, {"bias", &bias}, {"running_mean", &rm}, {"running_var", &rv}}, what);
  if (!run) return at::empty(x.sizes(), x.options());
  // the module's own ATen call (F.batch_norm, training = False) and nn.ReLU's: the same bits
  Tensor y = at::batch_norm(x, weight, bias, rm, rv, false, 0.1, eps, at::globalContext().userEnabledCuDNN());
  return relu ? at::relu_(y) : y;
}

Tensor3 frozen_batch_norm_act_backward(bool run, const Tensor& gout, const Tensor& x, const Tensor& weight,
                                       const Tensor& bias, const Tensor& rm, const Tensor& rv, double eps, bool relu,
                                       std::array<bool, 3> om) {
  const char* what = "frozen_batch_norm_act backward";
  if (run) check_on_gpu(gout, "grad_out", what), check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_norm_input(x, what);
  check_channel_vectors(x, {{"weight", &weight}, {"bias", &bias}, {"running_mean", &rm}, {"running_var", &rv}}, what);
  check_norm_grad(gout, x, what);
  const int64_t b = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
  const auto opt = x.options();
  Tensor gx = wanted(om[0], x.sizes(), opt), gw = wanted(om[1], {c}, opt), gb = wanted(om[2], {c}, opt);
  if (!run || !(om[0] || om[1] || om[2])) return Tensor3(gx, gw, gb);
  if (x.numel() == 0) return zero_param_grads(gx, gw, gb, om);
  Tensor go = gout.contiguous(), xc = x.contiguous();
  Tensor wc = weight.contiguous(), bc = bias.contiguous(), rmc = rm.contiguous(), rvc = rv.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA g(xc.device());
  Tensor ws;
  if (om[1] || om[2]) ws = at::empty({(int64_t)oflow_frozen_batch_norm_backward_workspace_floats((int)b, (int)c, (int)hw)}, opt);
  check_status(oflow_frozen_batch_norm_backward_f32(
                   go.data_ptr<float>(), xc.data_ptr<float>(), wc.data_ptr<float>(), bc.data_ptr<float>(),
                   rmc.data_ptr<float>(), rvc.data_ptr<float>(), (int)b, (int)c, (int)hw, eps, relu ? 1 : 0,
                   om[0] ? gx.data_ptr<float>() : nullptr, om[1] ? gw.data_ptr<float>() : nullptr,
                   om[2] ? gb.data_ptr<float>() : nullptr, ws.defined() ? ws.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return Tensor3(gx, gw, gb);
}

// ---------------------------------------------------------------- batch norm on batch statistics (batch_norm.hip)
void check_bn_batch(const Tensor& x, NamedTensors params, const char* what) {
  check_channel_vectors(x, params, what);
  TORCH_CHECK(x.size(0) <= INT_MAX && x.size(1) <= INT_MAX && x.size(2) * x.size(3) <= INT_MAX, what, ": x ", x.sizes(),
              " is past the kernels' index range");
}

// relu(batch_norm(x)) / batch_norm(x) of an nn.BatchNorm2d on batch statistics -> (y, mean, biased var); the running
// statistics are the caller's to update (extractor.py: enc_norm_act)
Tensor3 batch_norm_act(bool run, const Tensor& x, const Tensor& weight, const Tensor& bias, double eps, bool relu) {
  const char* what = "batch_norm_act";
  if (run) check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_norm_input(x, what);
  check_bn_batch(x, {{"weight", &weight}, {"bias", &bias}}, what);
  const int64_t b = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
  const auto opt = x.options();
  Tensor y = at::empty(x.sizes(), opt), mean = at::empty({c}, opt), var = at::empty({c}, opt);
  if (!run) return Tensor3(y, mean, var);
  if (x.numel() == 0) {  // no elements: no statistics
    mean.zero_();
    var.zero_();
    return Tensor3(y, mean, var);
  }
  Tensor xc = x.contiguous(), wc = weight.contiguous(), bc = bias.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA g(xc.device());
  Tensor ws = at::empty({(int64_t)oflow_batch_norm_workspace_floats((int)b, (int)c, (int)hw)}, opt);
  check_status(oflow_batch_norm_forward_f32(xc.data_ptr<float>(), wc.data_ptr<float>(), bc.data_ptr<float>(), (int)b, (int)c,
                                            (int)hw, eps, relu ? 1 : 0, y.data_ptr<float>(), mean.data_ptr<float>(),
                                            var.data_ptr<float>(), ws.data_ptr<float>(), cur_stream()),
               what);
  return Tensor3(y, mean, var);
}

Tensor3 batch_norm_act_backward(bool run, const Tensor& gout, const Tensor& x, const Tensor& weight, const Tensor& bias,
                                const Tensor& mean, const Tensor& var, double eps, bool relu, std::array<bool, 3> om) {
  const char* what = "batch_norm_act backward";
  if (run) check_on_gpu(gout, "grad_out", what), check_on_gpu(x, "x", what), check_on_gpu(weight, "weight", what);
  check_norm_input(x, what);
  check_bn_batch(x, {{"weight", &weight}, {"bias", &bias}, {"mean", &mean}, {"var", &var}}, what);
  check_norm_grad(gout, x, what);
  const int64_t b = x.size(0), c = x.size(1), hw = x.size(2) * x.size(3);
  const auto opt = x.options();
  Tensor gx = wanted(om[0], x.sizes(), opt), gw = wanted(om[1], {c}, opt), gb = wanted(om[2], {c}, opt);
  if (!run || !(om[0] || om[1] || om[2])) return Tensor3(gx, gw, gb);
  if (x.numel() == 0) return zero_param_grads(gx, gw, gb, om);
  Tensor go = gout.contiguous(), xc = x.contiguous();
  Tensor wc = weight.contiguous(), bc = bias.contiguous(), mc = mean.contiguous(), vc = var.contiguous();
  c10::hip::HIPGuardMasqueradingAsCUDA g(xc.device());
  Tensor ws = at::empty({(int64_t)oflow_batch_norm_workspace_floats((int)b, (int)c, (int)hw)}, opt);
  check_status(oflow_batch_norm_backward_f32(go.data_ptr<float>(), xc.data_ptr<float>(), wc.data_ptr<float>(),
                                             bc.data_ptr<float>(), mc.data_ptr<float>(), vc.data_ptr<float>(), (int)b, (int)c,
                                             (int)hw, eps, relu ? 1 : 0, om[0] ? gx.data_ptr<float>() : nullptr,
                                             om[1] ? gw.data_ptr<float>() : nullptr, om[2] ? gb.data_ptr<float>() : nullptr,
                                             ws.data_ptr<float>(), cur_stream()),
               what);
  return Tensor3(gx, gw, gb);
}

// ---------------------------------------------------------------- warm start (forward_interpolate.hip)
Tensor forward_interpolate(bool run, const Tensor& flow) {
  const char* what = "forward_interpolate";
  if (run) check_on_gpu(flow, "flow", what);
  TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2, what, ": flow must be (B, 2, H, W), got ", flow.sizes());
  TORCH_CHECK(flow.scalar_type() == at::kFloat, what, ": flow must be float32, got ", flow.scalar_type());
  const int64_t b = flow.size(0), h = flow.size(2), w = flow.size(3);
  TORCH_CHECK(b <= 65535 && h * w <= (int64_t(1) << 30), what, ": flow ", flow.sizes(),
              " is past the kernel's grid (B <= 65535, H*W <= 2^30)");
  if (!run) return at::empty(flow.sizes(), flow.options());
  Tensor fl = flow.contiguous();
  Tensor out = at::empty(fl.sizes(), fl.options());
  if (out.numel() == 0) return out;
  c10::hip::HIPGuardMasqueradingAsCUDA g(fl.device());
  check_status(oflow_forward_interpolate_f32(fl.data_ptr<float>(), (int)b, (int)h, (int)w, out.data_ptr<float>(),
                                             cur_stream()),
               what);
  return out;
}

// ---------------------------------------------------------------- forward-backward consistency (fb_consistency.hip)
Tensor4 fb_consistency(bool run, const Tensor& fw, const Tensor& bw, double alpha, double beta, bool both,
                       bool with_error) {
  const char* what = "fb_consistency";
  if (run) check_on_gpu(fw, "flow_fw", what), check_on_gpu(bw, "flow_bw", what);
  TORCH_CHECK(fw.dim() == 4 && fw.size(1) == 2 && fw.sizes() == bw.sizes(), what, ": flow_fw ", fw.sizes(),
              " and flow_bw ", bw.sizes(), " must be equal (B, 2, H, W)");
  TORCH_CHECK(fw.device() == bw.device(), what, ": flow_fw and flow_bw are on different devices");
  const int64_t b = fw.size(0), h = fw.size(2), w = fw.size(3);
  TORCH_CHECK(b <= 65535 && h * w <= (int64_t(1) << 30), what, ": flows ", fw.sizes(),
              " are past the kernel's grid (B <= 65535, H*W <= 2^30)");
  auto mo = fw.options().dtype(at::kBool), eo = fw.options().dtype(at::kFloat);
  Tensor none_m = at::empty({0}, mo), none_e = at::empty({0}, eo);
  Tensor m_fw = at::empty({b, 1, h, w}, mo), m_bw = both ? at::empty({b, 1, h, w}, mo) : none_m;
  Tensor e_fw = with_error ? at::empty({b, 1, h, w}, eo) : none_e;
  Tensor e_bw = with_error && both ? at::empty({b, 1, h, w}, eo) : none_e;
  if (!run || m_fw.numel() == 0) return Tensor4(m_fw, m_bw, e_fw, e_bw);
  Tensor f = gpu_f32(fw, "flow_fw", what), r = gpu_f32(bw, "flow_bw", what);  // (as warp: any float dtype or strides)
  c10::hip::HIPGuardMasqueradingAsCUDA g(f.device());
  check_status(oflow_fb_consistency_f32(f.data_ptr<float>(), r.data_ptr<float>(), (int)b, (int)h, (int)w, (float)alpha,
                                        (float)beta, reinterpret_cast<unsigned char*>(m_fw.data_ptr<bool>()),
                                        both ? reinterpret_cast<unsigned char*>(m_bw.data_ptr<bool>()) : nullptr,
                                        with_error ? e_fw.data_ptr<float>() : nullptr,
                                        with_error && both ? e_bw.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return Tensor4(m_fw, m_bw, e_fw, e_bw);
}

// ---------------------------------------------------------------- forward warping (splat.hip, splat_backward.hip)
void check_splat(const Tensor& frame, const Tensor& flow, const c10::optional<Tensor>& metric, int64_t mode, bool run,
                 const char* what) {
  if (run) {
    check_on_gpu(frame, "frame", what), check_on_gpu(flow, "flow", what);
    if (metric.has_value()) check_on_gpu(*metric, "metric", what);
  }
  TORCH_CHECK(frame.dim() == 4, what, ": frame must be (B, C, H, W), got ", frame.sizes());
  const int64_t b = frame.size(0), c = frame.size(1), h = frame.size(2), w = frame.size(3);
  TORCH_CHECK(flow.dim() == 4 && flow.size(0) == b && flow.size(1) == 2 && flow.size(2) == h && flow.size(3) == w, what,
              ": flow must be (B, 2, H, W) = (", b, ", 2, ", h, ", ", w, "), got ", flow.sizes());
  TORCH_CHECK(flow.device() == frame.device(), what, ": frame and flow are on different devices");
  TORCH_CHECK(mode >= OFLOW_SPLAT_SUM && mode <= OFLOW_SPLAT_SOFT, what, ": mode ", mode, " outside [0, 3]");
  const bool metric_mode = mode == OFLOW_SPLAT_LINEAR || mode == OFLOW_SPLAT_SOFT;
  TORCH_CHECK(metric.has_value() == metric_mode, what, ": mode ", mode,
              metric_mode ? " needs a metric" : " takes no metric");
  if (metric_mode) {
    TORCH_CHECK(metric->dim() == 4 && metric->size(0) == b && metric->size(1) == 1 && metric->size(2) == h &&
                    metric->size(3) == w,
                what, ": metric must be (B, 1, H, W) = (", b, ", 1, ", h, ", ", w, "), got ", metric->sizes());
    TORCH_CHECK(metric->device() == frame.device(), what, ": frame and metric are on different devices");
  }
  TORCH_CHECK(b <= 65535 && c <= INT_MAX && h * w <= OFLOW_SPLAT_MAX_PIXELS, what, ": frame ", frame.sizes(),
              " is past the kernels' range (B <= 65535, H*W <= 2^22)");
}

// (out (B, C, H, W), weight (B, 1, H, W)) fp32; any float dtype or strides, as warp
std::tuple<Tensor, Tensor> splat(bool run, const Tensor& frame, const Tensor& flow, const c10::optional<Tensor>& metric,
                                 int64_t mode) {
  const char* what = "splat";
  check_splat(frame, flow, metric, mode, run, what);
  const int64_t b = frame.size(0), c = frame.size(1), h = frame.size(2), w = frame.size(3);
  const auto opt = frame.options().dtype(at::kFloat);
  Tensor out = at::empty({b, c, h, w}, opt), weight = at::empty({b, 1, h, w}, opt);
  if (!run || out.numel() == 0) {
    if (run) weight.zero_();  // (C = 0 with pixels: nothing lands anywhere)
    return {out, weight};
  }
  Tensor fr = gpu_f32(frame, "frame", what), fl = gpu_f32(flow, "flow", what), me;
  if (metric.has_value()) me = gpu_f32(*metric, "metric", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(fr.device());
  Tensor ws = at::empty({oflow_splat_workspace_bytes((int)b, (int)c, (int)h, (int)w) / 8}, opt.dtype(at::kLong));
  check_status(oflow_splat_f32(fr.data_ptr<float>(), fl.data_ptr<float>(), me.defined() ? me.data_ptr<float>() : nullptr,
                               (int)b, (int)c, (int)h, (int)w, (int)mode, out.data_ptr<float>(),
                               weight.data_ptr<float>(), ws.data_ptr<int64_t>(), cur_stream()),
               what);
  return {out, weight};
}

Tensor3 splat_backward(bool run, const Tensor& gout, const Tensor& frame, const Tensor& flow,
                       const c10::optional<Tensor>& metric, const Tensor& out, const Tensor& weight, int64_t mode,
                       std::array<bool, 3> om) {
  const char* what = "splat backward";
  if (run) check_on_gpu(gout, "grad_out", what);
  check_splat(frame, flow, metric, mode, run, what);
  const int64_t b = frame.size(0), c = frame.size(1), h = frame.size(2), w = frame.size(3);
  TORCH_CHECK(gout.sizes() == frame.sizes() && out.sizes() == frame.sizes(), what, ": grad_out ", gout.sizes(), " and out ",
              out.sizes(), " must have frame's shape ", frame.sizes());
  TORCH_CHECK(weight.dim() == 4 && weight.size(0) == b && weight.size(1) == 1 && weight.size(2) == h && weight.size(3) == w,
              what, ": weight must be (B, 1, H, W), got ", weight.sizes());
  TORCH_CHECK(gout.device() == frame.device() && out.device() == frame.device() && weight.device() == frame.device(), what,
              ": all tensors must be on one device");
  TORCH_CHECK(!om[2] || metric.has_value(), what, ": a metric gradient needs a metric");
  const auto opt = frame.options().dtype(at::kFloat);
  Tensor gfr = wanted(om[0], {b, c, h, w}, opt), gfl = wanted(om[1], {b, 2, h, w}, opt), gme = wanted(om[2], {b, 1, h, w}, opt);
  if (!run || !(om[0] || om[1] || om[2])) return Tensor3(gfr, gfl, gme);
  if (frame.numel() == 0) {
    if (om[1]) gfl.zero_();
    if (om[2]) gme.zero_();
    return Tensor3(gfr, gfl, gme);
  }
  Tensor go = gpu_f32(gout, "grad_out", what), fr = gpu_f32(frame, "frame", what), fl = gpu_f32(flow, "flow", what);
  Tensor ou = gpu_f32(out, "out", what), we = gpu_f32(weight, "weight", what), me;
  if (metric.has_value()) me = gpu_f32(*metric, "metric", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(fr.device());
  Tensor ws = at::empty({oflow_splat_workspace_bytes((int)b, (int)c, (int)h, (int)w) / 8}, opt.dtype(at::kLong));
  check_status(oflow_splat_backward_f32(go.data_ptr<float>(), fr.data_ptr<float>(), fl.data_ptr<float>(),
                                        me.defined() ? me.data_ptr<float>() : nullptr, ou.data_ptr<float>(),
                                        we.data_ptr<float>(), (int)b, (int)c, (int)h, (int)w, (int)mode,
                                        om[0] ? gfr.data_ptr<float>() : nullptr, om[1] ? gfl.data_ptr<float>() : nullptr,
                                        om[2] ? gme.data_ptr<float>() : nullptr, ws.data_ptr<int64_t>(), cur_stream()),
               what);
  return Tensor3(gfr, gfl, gme);
}

// ---------------------------------------------------------------- unsupervised losses (census_loss.hip, smoothness_loss.hip)
// the mask as the C ABI takes it: bool -> bytes, any float dtype -> fp32, none -> OFLOW_VALID_NONE
int loss_mask(const c10::optional<Tensor>& mask, Tensor& keep, const void*& ptr) {
  ptr = nullptr;
  if (!mask.has_value()) return OFLOW_VALID_NONE;
  if (mask->scalar_type() == at::kBool) {
    keep = mask->contiguous();
    ptr = keep.data_ptr<bool>();
    return OFLOW_VALID_U8;
  }
  keep = mask->to(at::kFloat).contiguous();
  ptr = keep.data_ptr<float>();
  return OFLOW_VALID_F32;
}

void check_census(const Tensor& f0, const Tensor& f1, const c10::optional<Tensor>& mask, int64_t patch, double range,
                  bool run, const char* what) {
  if (run) {
    check_on_gpu(f0, "frame0", what), check_on_gpu(f1, "frame1", what);
    if (mask.has_value()) check_on_gpu(*mask, "mask", what);
  }
  TORCH_CHECK(f0.dim() == 4 && f0.sizes() == f1.sizes(), what, ": frame0 ", f0.sizes(), " and frame1 ", f1.sizes(),
              " must be equal (B, C, H, W)");
  TORCH_CHECK(f0.device() == f1.device(), what, ": frame0 and frame1 are on different devices");
  const int64_t b = f0.size(0), h = f0.size(2), w = f0.size(3);
  if (mask.has_value()) {
    TORCH_CHECK(mask->dim() == 4 && mask->size(0) == b && mask->size(1) == 1 && mask->size(2) == h && mask->size(3) == w,
                what, ": mask must be (B, 1, H, W) = (", b, ", 1, ", h, ", ", w, "), got ", mask->sizes());
    TORCH_CHECK(mask->scalar_type() == at::kBool || mask->is_floating_point(), what, ": mask must be float or bool, got ",
                mask->scalar_type());
    TORCH_CHECK(mask->device() == f0.device(), what, ": frame0 and mask are on different devices");
  }
  TORCH_CHECK(patch == 3 || patch == 5 || patch == 7, what, ": patch ", patch, " is not one of 3, 5, 7");
  TORCH_CHECK(range > 0 && std::isfinite(range), what, ": image_range ", range, " must be positive and finite");
  TORCH_CHECK(b <= 65535 && f0.size(1) <= INT_MAX && h * w <= (int64_t(1) << 28), what, ": frames ", f0.sizes(),
              " are past the kernels' range (B <= 65535, H*W <= 2^28)");
}

// (loss fp32 0-dim, sum M fp64 0-dim, s (B, 1, H, W) fp32); any float dtype or strides, as warp
Tensor3 census_loss(bool run, const Tensor& frame0, const Tensor& frame1, const c10::optional<Tensor>& mask, int64_t patch,
                    double range) {
  const char* what = "census_loss";
  check_census(frame0, frame1, mask, patch, range, run, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor loss = at::empty({}, opt), sum_m = at::empty({}, opt.dtype(at::kDouble)), s_map = at::empty({b, 1, h, w}, opt);
  if (!run) return Tensor3(loss, sum_m, s_map);
  if (frame0.numel() == 0) return Tensor3(loss.zero_(), sum_m.zero_(), s_map.zero_());
  Tensor f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  Tensor ws = at::empty({oflow_census_loss_workspace_bytes((int)b, (int)h, (int)w) / 8}, opt.dtype(at::kDouble));
  check_status(oflow_census_loss_f32(f0.data_ptr<float>(), f1.data_ptr<float>(), mp, kind, (int)b, (int)c, (int)h, (int)w,
                                     (int)patch, (float)range, s_map.data_ptr<float>(), ws.data_ptr<double>(),
                                     loss.data_ptr<float>(), sum_m.data_ptr<double>(), cur_stream()),
               what);
  return Tensor3(loss, sum_m, s_map);
}

std::tuple<Tensor, Tensor> census_loss_backward(bool run, const Tensor& gloss, const Tensor& frame0, const Tensor& frame1,
                                                const c10::optional<Tensor>& mask, const Tensor& sum_m,
                                                const Tensor& s_map, int64_t patch, double range, std::array<bool, 2> om) {
  const char* what = "census_loss backward";
  if (run) check_on_gpu(gloss, "grad_loss", what), check_on_gpu(sum_m, "sum_m", what), check_on_gpu(s_map, "s_map", what);
  check_census(frame0, frame1, mask, patch, range, run, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  TORCH_CHECK(gloss.numel() == 1 && sum_m.numel() == 1, what, ": grad_loss and sum_m must hold one element each");
  TORCH_CHECK(s_map.dim() == 4 && s_map.size(0) == b && s_map.size(1) == 1 && s_map.size(2) == h && s_map.size(3) == w,
              what, ": s_map must have the shape (B, 1, H, W) = (", b, ", 1, ", h, ", ", w, "), got ", s_map.sizes());
  TORCH_CHECK(gloss.device() == frame0.device() && sum_m.device() == frame0.device() && s_map.device() == frame0.device(),
              what, ": all tensors must be on one device");
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor g0 = wanted(om[0], {b, c, h, w}, opt), g1 = wanted(om[1], {b, c, h, w}, opt);
  if (!run || !(om[0] || om[1]) || frame0.numel() == 0) return {g0, g1};
  Tensor go = gpu_f32(gloss, "grad_loss", what), f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what);
  Tensor sm = sum_m.to(at::kDouble).contiguous(), sp = gpu_f32(s_map, "s_map", what), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  check_status(oflow_census_loss_backward_f32(go.data_ptr<float>(), f0.data_ptr<float>(), f1.data_ptr<float>(), mp, kind,
                                              sp.data_ptr<float>(), sm.data_ptr<double>(), (int)b, (int)c, (int)h, (int)w,
                                              (int)patch, (float)range, om[0] ? g0.data_ptr<float>() : nullptr,
                                              om[1] ? g1.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {g0, g1};
}

void check_smoothness(const Tensor& flow, const Tensor& image, int64_t order, double edge_weight, double range, bool run,
                      const char* what) {
  if (run) check_on_gpu(flow, "flow", what), check_on_gpu(image, "image", what);
  TORCH_CHECK(image.dim() == 4, what, ": image must be (B, C, H, W), got ", image.sizes());
  const int64_t b = image.size(0), h = image.size(2), w = image.size(3);
  TORCH_CHECK(flow.dim() == 4 && flow.size(0) == b && flow.size(1) == 2 && flow.size(2) == h && flow.size(3) == w, what,
              ": flow must be (B, 2, H, W) = (", b, ", 2, ", h, ", ", w, "), got ", flow.sizes());
  TORCH_CHECK(flow.device() == image.device(), what, ": flow and image are on different devices");
  TORCH_CHECK(order == 1 || order == 2, what, ": order ", order, " is not 1 or 2");
  TORCH_CHECK(range > 0 && std::isfinite(range) && std::isfinite(edge_weight), what, ": image_range ", range,
              " must be positive and finite and edge_weight ", edge_weight, " finite");
  TORCH_CHECK(b <= 65535 && image.size(1) <= INT_MAX && h * w <= (int64_t(1) << 28), what, ": image ", image.sizes(),
              " is past the kernels' range (B <= 65535, H*W <= 2^28)");
}

Tensor smoothness_loss(bool run, const Tensor& flow, const Tensor& image, int64_t order, double edge_weight, double range) {
  const char* what = "smoothness_loss";
  check_smoothness(flow, image, order, edge_weight, range, run, what);
  const int64_t b = image.size(0), c = image.size(1), h = image.size(2), w = image.size(3);
  const auto opt = flow.options().dtype(at::kFloat);
  Tensor loss = at::empty({}, opt);
  if (!run) return loss;
  if (image.numel() == 0) return loss.zero_();
  Tensor fl = gpu_f32(flow, "flow", what), im = gpu_f32(image, "image", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(fl.device());
  Tensor ws = at::empty({oflow_smoothness_loss_workspace_bytes((int)b, (int)h, (int)w) / 8}, opt.dtype(at::kDouble));
  check_status(oflow_smoothness_loss_f32(fl.data_ptr<float>(), im.data_ptr<float>(), (int)b, (int)c, (int)h, (int)w,
                                         (int)order, (float)edge_weight, (float)range, ws.data_ptr<double>(),
                                         loss.data_ptr<float>(), cur_stream()),
               what);
  return loss;
}

Tensor smoothness_loss_backward(bool run, const Tensor& gloss, const Tensor& flow, const Tensor& image, int64_t order,
                                double edge_weight, double range) {
  const char* what = "smoothness_loss backward";
  if (run) check_on_gpu(gloss, "grad_loss", what);
  check_smoothness(flow, image, order, edge_weight, range, run, what);
  TORCH_CHECK(gloss.numel() == 1, what, ": grad_loss must hold one element");
  TORCH_CHECK(gloss.device() == flow.device(), what, ": all tensors must be on one device");
  const int64_t b = image.size(0), c = image.size(1), h = image.size(2), w = image.size(3);
  Tensor gf = at::empty({b, 2, h, w}, flow.options().dtype(at::kFloat));
  if (!run || gf.numel() == 0) return gf;
  if (c == 0) return gf.zero_();
  Tensor go = gpu_f32(gloss, "grad_loss", what), fl = gpu_f32(flow, "flow", what), im = gpu_f32(image, "image", what);
  c10::hip::HIPGuardMasqueradingAsCUDA g(fl.device());
  check_status(oflow_smoothness_loss_backward_f32(go.data_ptr<float>(), fl.data_ptr<float>(), im.data_ptr<float>(), (int)b,
                                                  (int)c, (int)h, (int)w, (int)order, (float)edge_weight, (float)range,
                                                  gf.data_ptr<float>(), cur_stream()),
               what);
  return gf;
}

// ---------------------------------------------------------------- photometric losses (photometric_loss.hip)
// the checks the two losses share: the frames, the mask and the kernels' range
void check_photometric(const Tensor& f0, const Tensor& f1, const c10::optional<Tensor>& mask, bool run, const char* what) {
  if (run) {
    check_on_gpu(f0, "frame0", what), check_on_gpu(f1, "frame1", what);
    if (mask.has_value()) check_on_gpu(*mask, "mask", what);
  }
  TORCH_CHECK(f0.dim() == 4 && f0.sizes() == f1.sizes(), what, ": frame0 ", f0.sizes(), " and frame1 ", f1.sizes(),
              " must be equal (B, C, H, W)");
  TORCH_CHECK(f0.device() == f1.device(), what, ": frame0 and frame1 are on different devices");
  const int64_t b = f0.size(0), h = f0.size(2), w = f0.size(3);
  if (mask.has_value()) {
    TORCH_CHECK(mask->dim() == 4 && mask->size(0) == b && mask->size(1) == 1 && mask->size(2) == h && mask->size(3) == w,
                what, ": mask must be (B, 1, H, W) = (", b, ", 1, ", h, ", ", w, "), got ", mask->sizes());
    TORCH_CHECK(mask->scalar_type() == at::kBool || mask->is_floating_point(), what, ": mask must be float or bool, got ",
                mask->scalar_type());
    TORCH_CHECK(mask->device() == f0.device(), what, ": frame0 and mask are on different devices");
  }
  TORCH_CHECK(b <= 65535 && f0.size(1) <= INT_MAX && h * w <= (int64_t(1) << 28), what, ": frames ", f0.sizes(),
              " are past the kernels' range (B <= 65535, H*W <= 2^28)");
}

// the 1-D window as the C ABI takes it (fp32 in host memory)
std::vector<float> check_ssim(at::ArrayRef<double> window, double c1, double c2, const char* what) {
  const size_t n = window.size();
  TORCH_CHECK(n == 3 || n == 5 || n == 7 || n == 9 || n == 11, what, ": a window of ", n,
              " weights is not one of 3, 5, 7, 9, 11");
  std::vector<float> w(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(std::isfinite(window[i]), what, ": window weight ", i, " is not finite");
    w[i] = (float)window[i];
  }
  TORCH_CHECK(c1 > 0 && c2 > 0 && std::isfinite(c1) && std::isfinite(c2), what, ": c1 ", c1, " and c2 ", c2,
              " must be positive and finite");
  return w;
}

// grad_loss and sum_m of a backward, as the kernels take them
void check_loss_scalars(const Tensor& gloss, const Tensor& sum_m, const Tensor& frame0, bool run, const char* what) {
  if (run) check_on_gpu(gloss, "grad_loss", what), check_on_gpu(sum_m, "sum_m", what);
  TORCH_CHECK(gloss.numel() == 1 && sum_m.numel() == 1, what, ": grad_loss and sum_m must hold one element each");
  TORCH_CHECK(gloss.device() == frame0.device() && sum_m.device() == frame0.device(), what,
              ": all tensors must be on one device");
}

// (loss fp32 0-dim, sum M fp64 0-dim, mean_c SSIM (B, 1, H, W) fp32, empty without with_map); any float dtype or strides
Tensor3 ssim_loss(bool run, const Tensor& frame0, const Tensor& frame1, const c10::optional<Tensor>& mask,
                  at::ArrayRef<double> window, double c1, double c2, bool with_map) {
  const char* what = "ssim_loss";
  check_photometric(frame0, frame1, mask, run, what);
  const std::vector<float> wt = check_ssim(window, c1, c2, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor loss = at::empty({}, opt), sum_m = at::empty({}, opt.dtype(at::kDouble));
  Tensor map = with_map ? at::empty({b, 1, h, w}, opt) : at::empty({0}, opt);
  if (!run) return Tensor3(loss, sum_m, map);
  if (frame0.numel() == 0) return Tensor3(loss.zero_(), sum_m.zero_(), map.zero_());
  Tensor f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  Tensor ws = at::empty({oflow_ssim_loss_workspace_bytes((int)b, (int)h, (int)w) / 8}, opt.dtype(at::kDouble));
  check_status(oflow_ssim_loss_f32(f0.data_ptr<float>(), f1.data_ptr<float>(), mp, kind, (int)b, (int)c, (int)h, (int)w,
                                   (int)wt.size(), wt.data(), (float)c1, (float)c2,
                                   with_map ? map.data_ptr<float>() : nullptr, ws.data_ptr<double>(),
                                   loss.data_ptr<float>(), sum_m.data_ptr<double>(), cur_stream()),
               what);
  return Tensor3(loss, sum_m, map);
}

std::tuple<Tensor, Tensor> ssim_loss_backward(bool run, const Tensor& gloss, const Tensor& frame0, const Tensor& frame1,
                                              const c10::optional<Tensor>& mask, const Tensor& sum_m,
                                              at::ArrayRef<double> window, double c1, double c2, std::array<bool, 2> om) {
  const char* what = "ssim_loss backward";
  check_loss_scalars(gloss, sum_m, frame0, run, what);
  check_photometric(frame0, frame1, mask, run, what);
  const std::vector<float> wt = check_ssim(window, c1, c2, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor g0 = wanted(om[0], {b, c, h, w}, opt), g1 = wanted(om[1], {b, c, h, w}, opt);
  if (!run || !(om[0] || om[1]) || frame0.numel() == 0) return {g0, g1};
  Tensor go = gpu_f32(gloss, "grad_loss", what), f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what);
  Tensor sm = sum_m.to(at::kDouble).contiguous(), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  check_status(oflow_ssim_loss_backward_f32(go.data_ptr<float>(), f0.data_ptr<float>(), f1.data_ptr<float>(), mp, kind,
                                            sm.data_ptr<double>(), (int)b, (int)c, (int)h, (int)w, (int)wt.size(),
                                            wt.data(), (float)c1, (float)c2, om[0] ? g0.data_ptr<float>() : nullptr,
                                            om[1] ? g1.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {g0, g1};
}

void check_charbonnier(double eps, double alpha, double range, const char* what) {
  TORCH_CHECK(eps > 0 && std::isfinite(eps), what, ": eps ", eps, " must be positive and finite");
  TORCH_CHECK(alpha > 0 && alpha <= 1, what, ": alpha ", alpha, " must be in (0, 1]");
  TORCH_CHECK(range > 0 && std::isfinite(range), what, ": image_range ", range, " must be positive and finite");
}

// (loss fp32 0-dim, sum of the mask fp64 0-dim)
std::tuple<Tensor, Tensor> charbonnier_loss(bool run, const Tensor& frame0, const Tensor& frame1,
                                            const c10::optional<Tensor>& mask, double eps, double alpha, double range) {
  const char* what = "charbonnier_loss";
  check_photometric(frame0, frame1, mask, run, what);
  check_charbonnier(eps, alpha, range, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor loss = at::empty({}, opt), sum_m = at::empty({}, opt.dtype(at::kDouble));
  if (!run) return {loss, sum_m};
  if (frame0.numel() == 0) return {loss.zero_(), sum_m.zero_()};
  Tensor f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  Tensor ws = at::empty({oflow_ssim_loss_workspace_bytes((int)b, (int)h, (int)w) / 8}, opt.dtype(at::kDouble));
  check_status(oflow_charbonnier_loss_f32(f0.data_ptr<float>(), f1.data_ptr<float>(), mp, kind, (int)b, (int)c, (int)h,
                                          (int)w, (float)eps, (float)alpha, (float)range, ws.data_ptr<double>(),
                                          loss.data_ptr<float>(), sum_m.data_ptr<double>(), cur_stream()),
               what);
  return {loss, sum_m};
}

std::tuple<Tensor, Tensor> charbonnier_loss_backward(bool run, const Tensor& gloss, const Tensor& frame0,
                                                     const Tensor& frame1, const c10::optional<Tensor>& mask,
                                                     const Tensor& sum_m, double eps, double alpha, double range,
                                                     std::array<bool, 2> om) {
  const char* what = "charbonnier_loss backward";
  check_loss_scalars(gloss, sum_m, frame0, run, what);
  check_photometric(frame0, frame1, mask, run, what);
  check_charbonnier(eps, alpha, range, what);
  const int64_t b = frame0.size(0), c = frame0.size(1), h = frame0.size(2), w = frame0.size(3);
  const auto opt = frame0.options().dtype(at::kFloat);
  Tensor g0 = wanted(om[0], {b, c, h, w}, opt), g1 = wanted(om[1], {b, c, h, w}, opt);
  if (!run || !(om[0] || om[1]) || frame0.numel() == 0) return {g0, g1};
  Tensor go = gpu_f32(gloss, "grad_loss", what), f0 = gpu_f32(frame0, "frame0", what), f1 = gpu_f32(frame1, "frame1", what);
  Tensor sm = sum_m.to(at::kDouble).contiguous(), mk;
  const void* mp;
  const int kind = loss_mask(mask, mk, mp);
  c10::hip::HIPGuardMasqueradingAsCUDA g(f0.device());
  check_status(oflow_charbonnier_loss_backward_f32(go.data_ptr<float>(), f0.data_ptr<float>(), f1.data_ptr<float>(), mp,
                                                   kind, sm.data_ptr<double>(), (int)b, (int)c, (int)h, (int)w, (float)eps,
                                                   (float)alpha, (float)range, om[0] ? g0.data_ptr<float>() : nullptr,
                                                   om[1] ? g1.data_ptr<float>() : nullptr, cur_stream()),
               what);
  return {g0, g1};
}

// ---------------------------------------------------------------- training-batch augmentation (augment.hip)
Tensor4 augment_batch(bool run, const Tensor& img1, const Tensor& img2, const Tensor& flow,
                      const c10::optional<Tensor>& valid, const Tensor& params, int64_t ch, int64_t cw) {
  const char* what = "augment_batch";
  const bool sparse = valid.has_value();
  if (run) {
    check_on_gpu(img1, "img1", what), check_on_gpu(img2, "img2", what), check_on_gpu(flow, "flow", what);
    check_on_gpu(params, "params", what);
    if (sparse) check_on_gpu(*valid, "valid", what);
  }
  TORCH_CHECK(img1.dim() == 4 && img1.size(3) == 3 && img1.sizes() == img2.sizes(), what, ": img1 ", img1.sizes(),
              " and img2 ", img2.sizes(), " must be equal (B, H, W, 3)");
  TORCH_CHECK(img1.scalar_type() == at::kByte && img2.scalar_type() == at::kByte, what, ": images must be uint8");
  const int64_t b = img1.size(0), h = img1.size(1), w = img1.size(2);
  TORCH_CHECK(flow.dim() == 4 && flow.size(0) == b && flow.size(1) == 2 && flow.size(2) == h && flow.size(3) == w,
              what, ": flow must be (B, 2, H, W) = (", b, ", 2, ", h, ", ", w, "), got ", flow.sizes());
  TORCH_CHECK(flow.scalar_type() == at::kFloat, what, ": flow must be float32, got ", flow.scalar_type());
  if (sparse)
    TORCH_CHECK(valid->dim() == 3 && valid->size(0) == b && valid->size(1) == h && valid->size(2) == w &&
                    valid->scalar_type() == at::kFloat,
                what, ": valid must be float32 (B, H, W), got ", valid->scalar_type(), " ", valid->sizes());
  TORCH_CHECK(params.dim() == 2 && params.size(0) == b && params.size(1) == OFLOW_AUG_PARAM_DOUBLES &&
                  params.scalar_type() == at::kDouble,
              what, ": params must be float64 (B, ", OFLOW_AUG_PARAM_DOUBLES, "), got ", params.scalar_type(), " ",
              params.sizes());
  TORCH_CHECK(ch >= 1 && cw >= 1 && ch * cw <= (int64_t(1) << 28), what, ": crop ", ch, " x ", cw, " out of range");
  TORCH_CHECK(b <= 65535 && h * w <= (int64_t(1) << 28), what, ": source ", img1.sizes(),
              " is past the kernels' grid (B <= 65535, H*W <= 2^28)");
  for (const Tensor* t : {&img2, &flow, &params})
    TORCH_CHECK(t->device() == img1.device(), what, ": all tensors must be on one device");
  if (sparse) TORCH_CHECK(valid->device() == img1.device(), what, ": all tensors must be on one device");
  auto fo = flow.options();
  Tensor o1 = at::empty({b, 3, ch, cw}, fo), o2 = at::empty({b, 3, ch, cw}, fo);
  Tensor of = at::empty({b, 2, ch, cw}, fo), ov = at::empty({b, ch, cw}, fo);
  if (!run || b == 0) return Tensor4(o1, o2, of, ov);
  TORCH_CHECK(h >= 1 && w >= 1, what, ": empty source frames");
  Tensor i1 = img1.contiguous(), i2 = img2.contiguous(), fl = flow.contiguous(), pa = params.contiguous();
  Tensor stats = at::zeros({b, OFLOW_AUG_STATS_WORDS}, fo.dtype(at::kLong));
  c10::hip::HIPGuardMasqueradingAsCUDA g(i1.device());
  void* st = cur_stream();
  const auto* p1 = i1.data_ptr<uint8_t>();
  const auto* p2 = i2.data_ptr<uint8_t>();
  auto* ps = reinterpret_cast<long long*>(stats.data_ptr<int64_t>());
  for (int stage = 0; stage < 2; ++stage)
    check_status(oflow_augment_stats_u8(p1, p2, pa.data_ptr<double>(), (int)b, (int)h, (int)w, stage, ps, st), what);
  check_status(oflow_augment_dense_f32(p1, p2, sparse ? nullptr : fl.data_ptr<float>(), pa.data_ptr<double>(), ps,
                                       (int)b, (int)h, (int)w, (int)ch, (int)cw, o1.data_ptr<float>(),
                                       o2.data_ptr<float>(), sparse ? nullptr : of.data_ptr<float>(),
                                       sparse ? nullptr : ov.data_ptr<float>(), st),
               what);
  if (sparse) {
    Tensor va = valid->contiguous();
    check_status(oflow_augment_sparse_flow_f32(fl.data_ptr<float>(), va.data_ptr<float>(), pa.data_ptr<double>(),
                                               (int)b, (int)h, (int)w, (int)ch, (int)cw, of.data_ptr<float>(),
                                               ov.data_ptr<float>(), st),
                 what);
  }
  return Tensor4(o1, o2, of, ov);
}

// ---------------------------------------------------------------- registration
// The two kernels the dispatcher gets from one op function R op(bool run, Args...): Args... is deduced from the
// function pointer (a leading `run` keeps the pack deducible).
template <auto F>
struct Kernels;
template <class R, class... A, R (*F)(bool, A...)>
struct Kernels<F> {
  static R launch(A... a) { return F(true, std::forward<A>(a)...); }
  static R shapes(A... a) { return F(false, std::forward<A>(a)...); }
};

// One row per op registers its three kernels, so none can be left out of a table. CPU tensors reach the launching
// kernel, whose first device check raises "no CPU fallback" (there is no CPU path); a missing CPU kernel would turn
// that into PyTorch's generic "could not run ... with arguments from the 'CPU' backend".
template <auto F>
void bind(torch::Library& m, const char* name) {
  m.impl(name, c10::DispatchKey::CUDA, &Kernels<F>::launch);
  m.impl(name, c10::DispatchKey::CPU, &Kernels<F>::launch);
  m.impl(name, c10::DispatchKey::Meta, &Kernels<F>::shapes);
}

}  // namespace

TORCH_LIBRARY(oflow, m) {
  m.def("corr_pyramid(Tensor fmap1, Tensor fmap2, int num_levels) -> Tensor[]");
  m.def("corr_pyramid_tiled(Tensor fmap1, Tensor fmap2, int num_levels) -> Tensor[]");
  m.def("corr_lookup(Tensor[] levels, Tensor coords, int radius) -> Tensor");
  m.def("corr_lookup_tiled(Tensor[] levels, Tensor coords, int radius) -> Tensor");
  m.def("corr_lookup_tiled_nhwc(Tensor[] levels, Tensor coords, int radius, Tensor(a!) out) -> ()");
  m.def("corr_otf_prepare(Tensor fmap1, Tensor fmap2, int num_levels) -> (Tensor, Tensor[])");
  m.def("corr_lookup_otf(Tensor f1h, Tensor[] f2h, Tensor coords, int radius) -> Tensor");
  m.def("corr_lookup_alt(Tensor fmap1, Tensor fmap2, Tensor f1h, Tensor[] f2h, Tensor coords, int radius) -> Tensor");
  m.def("corr_lookup_alt_backward(Tensor grad_out, Tensor f1h, Tensor[] f2h, Tensor coords, int radius, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("grid_warp(Tensor frame, Tensor flow, int mode, int padding_mode, bool align_corners) -> Tensor");
  m.def("grid_sample(Tensor input, Tensor grid, int mode, int padding_mode, bool align_corners) -> Tensor");
  m.def("corr_lookup_backward(Tensor grad_out, Tensor coords, int radius, int H, int W, int num_levels) -> Tensor[]");
  m.def("corr_pyramid_backward(Tensor[] level_grads, Tensor fmap1, Tensor fmap2) -> (Tensor, Tensor)");
  m.def("grid_warp_backward(Tensor grad_out, Tensor frame, Tensor flow, int mode, int padding_mode, bool align_corners, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("grid_sample_backward(Tensor grad_out, Tensor input, Tensor grid, int mode, int padding_mode, bool align_corners, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("flow_error_stats(Tensor pred, Tensor target, Tensor? valid, float abs_threshold, float rel_threshold, float max_flow, Tensor(a!) accum, bool epe_map) -> Tensor");
  m.def("sequence_loss(Tensor[] flow_preds, Tensor flow_gt, Tensor valid, float[] weights, float max_flow) -> (Tensor, Tensor)");
  m.def("sequence_loss_backward(Tensor grad_out, Tensor[] flow_preds, Tensor flow_gt, Tensor valid, float[] weights, float max_flow, int[] need) -> Tensor[]");
  m.def("convex_upsample(Tensor flow, Tensor mask) -> Tensor");
  m.def("convex_upsample_backward(Tensor grad_out, Tensor flow, Tensor mask, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("conv2d_same(Tensor x, Tensor weight, Tensor? bias) -> Tensor");
  m.def("conv2d_same_backward(Tensor grad_out, Tensor x, Tensor weight, bool[3] output_mask) -> (Tensor, Tensor, Tensor)");
  m.def("conv2d_strided(Tensor x, Tensor weight, Tensor? bias, int stride) -> Tensor");
  m.def("conv2d_strided_backward(Tensor grad_out, Tensor x, Tensor weight, int stride, bool[3] output_mask) -> (Tensor, Tensor, Tensor)");
  m.def("instance_norm_act(Tensor x, float eps, bool relu) -> Tensor");
  m.def("instance_norm_act_backward(Tensor grad_out, Tensor x, float eps, bool relu) -> Tensor");
  m.def("frozen_batch_norm_act(Tensor x, Tensor weight, Tensor bias, Tensor running_mean, Tensor running_var, float eps, bool relu) -> Tensor");
  m.def("frozen_batch_norm_act_backward(Tensor grad_out, Tensor x, Tensor weight, Tensor bias, Tensor running_mean, Tensor running_var, float eps, bool relu, bool[3] output_mask) -> (Tensor, Tensor, Tensor)");
  m.def("batch_norm_act(Tensor x, Tensor weight, Tensor bias, float eps, bool relu) -> (Tensor y, Tensor mean, Tensor var)");
  m.def("batch_norm_act_backward(Tensor grad_out, Tensor x, Tensor weight, Tensor bias, Tensor mean, Tensor var, float eps, bool relu, bool[3] output_mask) -> (Tensor, Tensor, Tensor)");
  m.def("forward_interpolate(Tensor flow) -> Tensor");
  m.def("augment_batch(Tensor img1, Tensor img2, Tensor flow, Tensor? valid, Tensor params, int crop_h, int crop_w) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("fb_consistency(Tensor flow_fw, Tensor flow_bw, float alpha, float beta, bool both, bool with_error) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("splat(Tensor frame, Tensor flow, Tensor? metric, int mode) -> (Tensor out, Tensor weight)");
  m.def("splat_backward(Tensor grad_out, Tensor frame, Tensor flow, Tensor? metric, Tensor out, Tensor weight, int mode, bool[3] output_mask) -> (Tensor, Tensor, Tensor)");
  m.def("census_loss(Tensor frame0, Tensor frame1, Tensor? mask, int patch, float image_range) -> (Tensor loss, Tensor sum_m, Tensor s_map)");
  m.def("census_loss_backward(Tensor grad_loss, Tensor frame0, Tensor frame1, Tensor? mask, Tensor sum_m, Tensor s_map, int patch, float image_range, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("smoothness_loss(Tensor flow, Tensor image, int order, float edge_weight, float image_range) -> Tensor");
  m.def("smoothness_loss_backward(Tensor grad_loss, Tensor flow, Tensor image, int order, float edge_weight, float image_range) -> Tensor");
  m.def("ssim_loss(Tensor frame0, Tensor frame1, Tensor? mask, float[] window, float c1, float c2, bool with_map) -> (Tensor loss, Tensor sum_m, Tensor ssim_map)");
  m.def("ssim_loss_backward(Tensor grad_loss, Tensor frame0, Tensor frame1, Tensor? mask, Tensor sum_m, float[] window, float c1, float c2, bool[2] output_mask) -> (Tensor, Tensor)");
  m.def("charbonnier_loss(Tensor frame0, Tensor frame1, Tensor? mask, float eps, float alpha, float image_range) -> (Tensor loss, Tensor sum_m)");
  m.def("charbonnier_loss_backward(Tensor grad_loss, Tensor frame0, Tensor frame1, Tensor? mask, Tensor sum_m, float eps, float alpha, float image_range, bool[2] output_mask) -> (Tensor, Tensor)");

  bind<&corr_pyramid>(m, "corr_pyramid");
  bind<&corr_pyramid_tiled>(m, "corr_pyramid_tiled");
  bind<&corr_lookup>(m, "corr_lookup");
  bind<&corr_lookup_tiled>(m, "corr_lookup_tiled");
  bind<&corr_lookup_tiled_nhwc>(m, "corr_lookup_tiled_nhwc");
  bind<&corr_otf_prepare>(m, "corr_otf_prepare");
  bind<&corr_lookup_otf>(m, "corr_lookup_otf");
  bind<&corr_lookup_alt>(m, "corr_lookup_alt");
  bind<&corr_lookup_alt_backward>(m, "corr_lookup_alt_backward");
  bind<&grid_warp>(m, "grid_warp");
  bind<&grid_sample>(m, "grid_sample");
  bind<&corr_lookup_backward>(m, "corr_lookup_backward");
  bind<&corr_pyramid_backward>(m, "corr_pyramid_backward");
  bind<&grid_warp_backward>(m, "grid_warp_backward");
  bind<&grid_sample_backward>(m, "grid_sample_backward");
  bind<&flow_error_stats>(m, "flow_error_stats");
  bind<&sequence_loss>(m, "sequence_loss");
  bind<&sequence_loss_backward>(m, "sequence_loss_backward");
  bind<&convex_upsample>(m, "convex_upsample");
  bind<&convex_upsample_backward>(m, "convex_upsample_backward");
  bind<&conv2d_same>(m, "conv2d_same");
  bind<&conv2d_same_backward>(m, "conv2d_same_backward");
  bind<&conv2d_strided>(m, "conv2d_strided");
  bind<&conv2d_strided_backward>(m, "conv2d_strided_backward");
  bind<&instance_norm_act>(m, "instance_norm_act");
  bind<&instance_norm_act_backward>(m, "instance_norm_act_backward");
  bind<&frozen_batch_norm_act>(m, "frozen_batch_norm_act");
  bind<&frozen_batch_norm_act_backward>(m, "frozen_batch_norm_act_backward");
  bind<&batch_norm_act>(m, "batch_norm_act");
  bind<&batch_norm_act_backward>(m, "batch_norm_act_backward");
  bind<&forward_interpolate>(m, "forward_interpolate");
  bind<&augment_batch>(m, "augment_batch");
  bind<&fb_consistency>(m, "fb_consistency");
  bind<&splat>(m, "splat");
  bind<&splat_backward>(m, "splat_backward");
  bind<&census_loss>(m, "census_loss");
  bind<&census_loss_backward>(m, "census_loss_backward");
  bind<&smoothness_loss>(m, "smoothness_loss");
  bind<&smoothness_loss_backward>(m, "smoothness_loss_backward");
  bind<&ssim_loss>(m, "ssim_loss");
  bind<&ssim_loss_backward>(m, "ssim_loss_backward");
  bind<&charbonnier_loss>(m, "charbonnier_loss");
  bind<&charbonnier_loss_backward>(m, "charbonnier_loss_backward");
}
