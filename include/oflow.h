/*
 * oflow.h — C ABI of liboflow_hip.so, the MI355X (gfx950) implementation of the RAFT inference hot path of
 * awaelchli/torch-optical-flow. Plain pointers and sizes only: no torch or C++ types cross this boundary.
 *
 * All pointers named d_* are DEVICE pointers (HBM), contiguous, fp32 unless stated. Every entry point only
 * ENQUEUES work on `stream` (hipStream_t passed as void*; NULL = the null stream of the current device) and
 * returns without synchronising; it never allocates. Callers set the current device to the one owning the
 * buffers (the Python host layer does this with a torch device guard).
 *
 * Return value: OFLOW_OK (0), a negative OFLOW_E_* argument error (nothing was enqueued), or a positive
 * hipError_t from the launch. oflow_status_string() turns either into text; the Python layer raises
 * RuntimeError/ValueError with it, the exception types the reference's ATen ops raise.
 *
 * Replaces (reference file:line, /root/reference):
 *   oflow_corr_pyramid_f32  <- methods/raft/model/corr.py:38-54 (CorrBlock.__init__) + 79-87 (CorrBlock.corr)
 *   oflow_corr_lookup_f32   <- methods/raft/model/corr.py:56-77 (CorrBlock.__call__)
 *                              + methods/raft/model/utils.py:64-80 (bilinear_sampler)
 *   oflow_grid_warp_f32     <- optical_flow/operator/operator.py:8-56 (warp, warp_grid -> F.grid_sample)
 *   oflow_conv_s32 & co.    <- methods/raft/model/update.py:40-161 (update-block convolutions)
 *   oflow_stem_patches_s32, oflow_norm_*, oflow_conv_s32 <- methods/raft/model/extractor.py:35-231 (encoders)
 *   oflow_convex_upsample_f32 <- methods/raft/model/raft.py:73-85 (RAFT.upsample_flow)
 *   oflow_convex_upsample_backward_f32 <- the same lines under autograd (the training step, raft.py:149-175)
 *   oflow_conv2d_backward_input_f32, oflow_conv2d_backward_weight_f32 <- methods/raft/model/update.py:31-161 under
 *                              autograd (the update block's nn.Conv2d layers in the training step, raft.py:149-175)
 *   oflow_conv2d_strided_backward_*_f32, oflow_instance_norm_backward_f32, oflow_frozen_batch_norm_backward_f32
 *                           <- methods/raft/model/extractor.py:35-231 under autograd (the encoders in the training step)
 *   oflow_batch_norm_forward_f32, oflow_batch_norm_backward_f32 <- the same file's BatchNorm2d layers on batch statistics
 *                              (cnet in train mode: the Chairs stage), forward and backward, + the ReLU after them
 *   oflow_flow_stats_f32, oflow_flow2rgb_f32 <- optical_flow/visualization/flow2rgb.py:19-73 (+ visualization/methods/)
 *   oflow_flow_pack_f32     <- optical_flow/io/middlebury.py:43-71, optical_flow/io/pfm.py:79-104 (file payloads)
 *   oflow_flow_error_stats_f32 <- optical_flow/metrics/epe.py:24-65 (AverageEndPointError.update, end_point_error)
 *                              + optical_flow/metrics/f1.py:34-55 (OutlierRatio.update)
 *   oflow_sequence_loss_f32, oflow_sequence_loss_backward_f32 <- methods/raft/model/raft.py:231-260 (sequence_loss
 *                              and its autograd)
 *   oflow_forward_interpolate_f32 <- nothing in the reference: it produces the flow_init that
 *                              methods/raft/model/raft.py:122-123 consumes (upstream RAFT's forward_interpolate)
 *   oflow_fb_consistency_f32 <- nothing in the reference (csrc/fb_consistency.hip): the forward-backward occlusion
 *                              mask of a flow pair, UnFlow's criterion (Meister et al., whom the reference cites for
 *                              optical_flow/visualization/methods/meister.py)
 *   oflow_splat_f32, oflow_splat_backward_f32 <- nothing in the reference (csrc/splat.hip, csrc/splat_backward.hip):
 *                              forward warping, the sum / average / linear / softmax splatting of Niklaus and Liu
 *   oflow_census_loss_f32, oflow_smoothness_loss_f32 and their backwards <- nothing in the reference
 *                              (csrc/census_loss.hip, csrc/smoothness_loss.hip): the unsupervised training losses of
 *                              UnFlow / UFlow, scoring a flow against the images alone
 *   oflow_ssim_loss_f32, oflow_charbonnier_loss_f32 and their backwards <- nothing in the reference
 *                              (csrc/photometric_loss.hip): the SSIM and robust L1 photometric terms of the same methods
 *   oflow_augment_stats_u8, oflow_augment_dense_f32, oflow_augment_sparse_flow_f32 <- methods/raft/data/augmentor.py:43-324
 *                              (FlowAugmentor, SparseFlowAugmentor: PIL ColorJitter, cv2.resize, eraser, flips, crop)
 *                              + methods/raft/data/dataset.py:114-119 (fp32 flow, the dense valid mask)
 */
#ifndef OFLOW_H_
#define OFLOW_H_

#ifdef __cplusplus
extern "C" {
#endif

#define OFLOW_ABI_VERSION 3

#define OFLOW_OK 0
#define OFLOW_E_NULL (-1)      /* a required pointer is NULL */
#define OFLOW_E_SHAPE (-2)     /* a size is <= 0 or inconsistent */
#define OFLOW_E_LEVELS (-3)    /* num_levels outside [1, OFLOW_MAX_LEVELS] */
#define OFLOW_E_TINY (-4)      /* a pyramid level is < 2 pixels in H or W (reference divides by 0: Q3) */
#define OFLOW_E_RADIUS (-5)    /* radius outside [0, OFLOW_MAX_RADIUS] */
#define OFLOW_E_MODE (-6)      /* unknown interpolation or padding mode */
#define OFLOW_E_ALIGN (-7)     /* a pointer is not 4-byte aligned */

#define OFLOW_MAX_LEVELS 8
#define OFLOW_MAX_RADIUS 7

/* grid_sample modes (torch.nn.functional.grid_sample names) */
#define OFLOW_INTERP_BILINEAR 0
#define OFLOW_INTERP_NEAREST 1
#define OFLOW_INTERP_BICUBIC 2
#define OFLOW_PAD_ZEROS 0
#define OFLOW_PAD_BORDER 1
#define OFLOW_PAD_REFLECTION 2

/* oflow_conv_s32_desc.in_format */
#define OFLOW_IN_S32 0
#define OFLOW_IN_F32_NORM 1
#define OFLOW_IN_F32 2
#define OFLOW_IN_IMG7S2 3
#define OFLOW_IN_FLOW7 4
/* oflow_conv_s32_desc.epilogue: the flow-head epilogue (epilogues 0-2: plain numbers) */
#define OFLOW_EPI_FLOW_HEAD 3

int oflow_abi_version(void);
const char* oflow_status_string(int status);

/*
 * Pyramid level sizes for a (H, W) query grid: level 0 = (H, W), level l = floor-halves of level l-1
 * (avg_pool2d(2, stride=2) semantics, corr.py:53). Writes num_levels entries to level_h / level_w (host).
 */
int oflow_corr_pyramid_dims(int H, int W, int num_levels, int* level_h, int* level_w);

/*
 * All-pairs correlation pyramid (CorrBlock.__init__).
 *   d_fmap1, d_fmap2 : (B, C, H, W) fp32
 *   d_levels[l]      : host array of num_levels device pointers; level l is (B*H*W, H_l, W_l) fp32,
 *                      i.e. the reference's corr_pyramid[l] of shape (B*H*W, 1, H_l, W_l).
 *   level 0 = (fmap1^T fmap2) / sqrt(C) on fp32 MFMA (v_mfma_f32_32x32x2f32); levels 1.. are the floor
 *   2x2 average pools of the level above, fused in the GEMM epilogue (level 0 is never re-read).
 */
int oflow_corr_pyramid_f32(const float* d_fmap1, const float* d_fmap2, int B, int C, int H, int W,
                           int num_levels, float* const* d_levels, void* stream);

/*
 * Windowed multi-level bilinear lookup (CorrBlock.__call__).
 *   d_levels[l] : as produced above (H_l, W_l from oflow_corr_pyramid_dims)
 *   d_coords    : (B, 2, H, W) fp32 pixel coordinates, channel 0 = x, 1 = y
 *   d_out       : (B, num_levels*(2r+1)^2, H, W) fp32; channel l*(2r+1)^2 + i*(2r+1) + j samples level l
 *                 at (x/2^l + i - r, y/2^l + j - r), bilinear, zero outside the level (grid_sample
 *                 align_corners=True, padding_mode='zeros').
 */
int oflow_corr_lookup_f32(const float* const* d_levels, const int* level_h, const int* level_w,
                          int num_levels, const float* d_coords, int B, int H, int W, int radius,
                          float* d_out, void* stream);

/*
 * Tiled pyramid storage (what CorrBlock uses internally): level l of each query is stored as
 * [ceil(H_l/4)][ceil(W_l/8)][4][8] fp32 tiles, one 4x8 tile = one 128-B line, so a (2r+2)^2 lookup window
 * touches ~7 lines instead of ~13 with canonical rows. oflow_corr_tiled_level_floats(H_l, W_l) = floats per query
 * of a level; levels are otherwise produced and read exactly like the canonical ones above, and
 * oflow_corr_untile_f32 rebuilds the canonical (Q, H_l, W_l) view bit-for-bit.
 */
long long oflow_corr_tiled_level_floats(int H_l, int W_l);
int oflow_corr_pyramid_tiled_f32(const float* d_fmap1, const float* d_fmap2, int B, int C, int H, int W,
                                 int num_levels, float* const* d_levels, void* stream);
/* oflow_corr_pyramid_tiled_s32: oflow_corr_pyramid_tiled_f32's levels (same tiled layout) from feature maps given as
 * S32 rows (B, H, W, C/32 groups of hi[32] | lo[32] fp16; C % 32 == 0; 16-B aligned) -- the RAFT forward's pyramid,
 * fed by the feature encoder's last convolution: products as three fp16 MFMAs on the hi/lo split (22-bit operands,
 * fp32 accumulation), not fp32 MFMAs. Within SURVEY §8(c)'s pyramid tolerance of the fp32 result (tested). */
int oflow_corr_pyramid_tiled_s32(const void* d_fmap1_s32, const void* d_fmap2_s32, int B, int C, int H, int W,
                                 int num_levels, float* const* d_levels, void* stream);
int oflow_corr_lookup_tiled_f32(const float* const* d_levels, const int* level_h, const int* level_w,
                                int num_levels, const float* d_coords, int B, int H, int W, int radius,
                                float* d_out, void* stream);
int oflow_corr_untile_f32(const float* d_tiled, float* d_out, long long Q, int H_l, int W_l, void* stream);

/*
 * Inverse warp (optical_flow.warp): out = grid_sample(frame, linspace-grid + flow, mode, padding_mode,
 * align_corners). d_frame, d_out: (B, C, H, W); d_flow: (B, 2, H, W) already normalized to [-1, 1] units.
 */
int oflow_grid_warp_f32(const float* d_frame, const float* d_flow, int B, int C, int H, int W, int mode,
                        int padding_mode, int align_corners, float* d_out, void* stream);

/*
 * Explicit-grid sampling (F.grid_sample): d_input (B, C, H, W), d_grid (B, Ho, Wo, 2) in [-1, 1] units
 * (x, y), d_out (B, C, Ho, Wo). Replaces the grid_sample inside methods/raft/model/utils.py:64-80
 * (bilinear_sampler, called there with align_corners=True, zeros padding) for callers outside CorrBlock.
 */
int oflow_grid_sample_f32(const float* d_input, const float* d_grid, int B, int C, int H, int W, int Ho, int Wo,
                          int mode, int padding_mode, int align_corners, float* d_out, void* stream);

/*
 * On-the-fly fp16 correlation (memory-efficient path for large frames; BASELINE configs[4], no volume).
 * Same output as oflow_corr_lookup_f32 on the dense pyramid of (fmap1, fmap2), by linearity of the pooling:
 * level-l correlations are dot products of fmap1 with the floor 2^l-pooled fmap2 (corr.py:38-54, 79-87).
 *   prepare: d_f1h = fmap1 / sqrt(C) as (B, H, W, C) fp16; d_f2h[l] = pool_l(fmap2) as (B, H_l, W_l, C) fp16,
 *            pooled in fp32 (d_scratch: B*C*sum_{l>=1} H_l*W_l floats) then rounded. C % 32 == 0.
 *   lookup:  d_out (B, L*(2r+1)^2, H, W) fp32, radius <= 4; window dot products on v_mfma_f32_16x16x32_f16.
 */
int oflow_corr_otf_prepare_f16(const float* d_fmap1, const float* d_fmap2, int B, int C, int H, int W,
                               int num_levels, void* d_f1h, void* const* d_f2h, float* d_scratch, void* stream);
int oflow_corr_lookup_otf_f16(const void* d_f1h, const void* const* d_f2h, const int* level_h, const int* level_w,
                              int num_levels, const float* d_coords, int B, int C, int H, int W, int radius,
                              float* d_out, void* stream);

/*
 * Backward of oflow_corr_lookup_otf_f16 (training with AlternateCorrBlock; csrc/corr_otf_backward.hip). The fp16
 * roundings of the stored features are taken as identity: the derivative is evaluated at d_f1h / d_f2h as they are.
 *   d_grad_out    (B, L*(2r+1)^2, H, W) fp32, the gradient of the lookup output (kept in fp32 throughout).
 *   d_grad_fmap1  (B, C, H, W) fp32 or NULL: gradient of fmap1 (1/sqrt(C) included); every element written once in a
 *                 fixed order (bit-reproducible).
 *   d_grad_fmap2  (B, C, H, W) fp32 or NULL: gradient of fmap2 through the floor 2x2 pools; every element written once,
 *                 from per-level sums formed with fp32 atomic adds (last bits depend on arrival order).
 *   d_scratch     B*C*sum_l H_l*W_l floats, needed only when d_grad_fmap2 is not NULL (may be NULL otherwise); the call
 *                 zeroes it itself.
 * Coordinates get no gradient; queries with NaN / inf / |c / 2^l| >= 2^22 coordinates contribute nothing at level l.
 * level_h[0] x level_w[0] must be H x W. Same status codes as the forward: radius 0-4, C % 32 == 0, levels >= 2 px.
 * With both outputs NULL the call checks its arguments and does nothing.
 */
int oflow_corr_lookup_otf_backward_f32(const float* d_grad_out, const void* d_f1h, const void* const* d_f2h,
                                       const int* level_h, const int* level_w, int num_levels, const float* d_coords,
                                       int B, int C, int H, int W, int radius, float* d_grad_fmap1,
                                       float* d_grad_fmap2, float* d_scratch, void* stream);

/*
 * Fused elementwise stages of the update block around its (bias-free) MIOpen convolutions
 * (methods/raft/model/update.py:69-161). Tensors are (B, C, P) with contiguous (C, P)
 * parts and an explicit batch stride in floats, so they can be channel slices of concatenated buffers.
 *   bias_act : y0[b,c,p] (and y1 if not NULL) = act(x[b,c,p] + bias[c]) * scale; act 0 none, 1 relu,
 *              2 sigmoid, 3 tanh; bias may be NULL; y0 may alias x.
 *   gru_reset: rh = sigmoid(zr[:, CH + c] + br[c]) * h          (zr = [z | r] pre-bias gate convolution)
 *   gru_blend: h = (1 - z) * h + z * tanh(q + bq[c]), z = sigmoid(zr[:, c] + bz[c]); h updated in place
 */
int oflow_bias_act_f32(const float* d_x, long long sx, const float* d_bias, float* d_y0, long long sy0, float* d_y1,
                       long long sy1, int B, int C, int P, int activation, float scale, void* stream);
int oflow_gru_reset_f32(const float* d_zr, long long szr, const float* d_br, const float* d_h, long long sh,
                        float* d_rh, long long srh, int B, int CH, int P, void* stream);
int oflow_gru_blend_f32(const float* d_zr, long long szr, const float* d_bz, const float* d_q, long long sq,
                        const float* d_bq, float* d_h, long long sh, int B, int CH, int P, void* stream);

/*
 * Split-fp16 ("S32") update-block path: fp32-accurate convolutions on the fp16 matrix cores
 * (methods/raft/model/update.py:40-161; csrc/conv_s32.hip).
 *
 * S32 activation format: NHWC by groups of 32 channels; element (pixel p, channel c) of a buffer with G groups
 * is hi = fp16(v) at byte p*G*128 + (c/32)*128 + (c%32)*2 and lo = fp16(v - hi) 64 bytes further (v ~ hi + lo,
 * 22 significant bits). A channel slice starting at group g0 is (base + g0*128, pixel stride G*128).
 * Padding channels (beyond the real ones, up to a multiple of 32) must hold zeros.
 *
 * oflow_conv_s32: the convolution itself; see its descriptor, oflow_conv_s32_desc, below.
 * oflow_pack_s32_f32: d_x (B, C, H, W) fp32 with batch stride x_batch_stride -> act -> S32 d_y0 (and d_y1) channels
 *   dst_channel + c (dst_channel % 8 == 0; the last 8-channel chunk is zero-filled past C), and optionally a
 *   [P][nhwc_pixel_stride] fp32 copy.                                     (raft.py:115-118: tanh / relu of cnet)
 * oflow_flow_prep_s32: flow = coords1 - pixel grid (raft.py:129) as the 7x7 patch matrix of convf1
 *   (d_patches: S32 with 4 groups; channel t*2 + c = flow c at tap t = ky*7 + kx, zero padded) and, if not NULL,
 *   the 2 flow channels at d_flow0 / d_flow1 (byte address of the hi half of the x channel; y follows).
 */
int oflow_pack_s32_f32(const float* d_x, long long x_batch_stride, int C, int B, int H, int W, int activation,
                       int dst_channel, void* d_y0, long long y0_pixel_stride, void* d_y1, long long y1_pixel_stride,
                       float* d_nhwc, int nhwc_pixel_stride, void* stream);
int oflow_flow_prep_s32(const float* d_coords, int B, int H, int W, void* d_patches, void* d_flow0,
                        long long flow0_pixel_stride, void* d_flow1, long long flow1_pixel_stride, void* stream);

/*
 * oflow_conv_s32: the split-fp16 convolution of the update block (update.py:40-161) and the encoders
 * (extractor.py:35-231), described by one oflow_conv_s32_desc. A zero-filled descriptor has every optional feature off
 * (S32 input, epilogue 0, no activation, every optional pointer NULL); the caller sets struct_size =
 * sizeof(oflow_conv_s32_desc) and the fields it needs. A stride, count or flag that belongs to a NULL pointer is
 * ignored. desc NULL: OFLOW_E_NULL; struct_size != sizeof(oflow_conv_s32_desc): OFLOW_E_MODE, before any other field
 * is read (a caller built against another layout of this struct).
 */
typedef struct oflow_conv_s32_desc {
  unsigned int struct_size;
  /* Input: OFLOW_IN_S32, d_x an S32 slice of in_groups groups (16-B aligned, x_pixel_stride % 128 == 0). The other
   * formats split fp32 values into hi + lo while the kernel stages them (epilogue 0 only):
   *   OFLOW_IN_F32_NORM: the raw fp32 NHWC output [P][in_groups*32] of the previous convolution (x_pixel_stride =
   *     in_groups*128), normalised and ReLU'd while staged, x = max(0, raw * d_in_scale[b, c] + d_in_shift[b, c])
   *     ([B][in_groups*32] each) -- the instance norm + ReLU between a residual block's two 3x3 convs
   *     (extractor.py:75-76) never materialises (3x3, in_groups <= 4);
   *   OFLOW_IN_F32: an fp32 NHWC input of cin = x_pixel_stride/4 channels per pixel ((in_groups-1)*32 < cin <=
   *     in_groups*32, x_pixel_stride % 16 == 0; channels past cin stage as zeros) (1x1, block_n 128: convc1 reading
   *     oflow_corr_lookup_tiled_nhwc_f32's rows);
   *   OFLOW_IN_IMG7S2: the encoders' stem (extractor.py:186, 7x7 / stride 2 / pad 3 on a 3-channel image) straight from
   *     the fp32 NCHW image d_x (B, 3, 2H, 2W) for an output of H x W (x_pixel_stride ignored): each output tile builds
   *     its patch-matrix operand (channel t*3 + c, t = ky*7 + kx; in_groups 5, weights packed as for
   *     oflow_stem_patches_s32's matrix) from an LDS window, so no patch matrix is written (1x1 geometry, block_n 64);
   *   OFLOW_IN_FLOW7: the motion encoder's convf1 (update.py:116, 7x7 / pad 3 on the 2-channel flow) straight from
   *     coords1 d_x (B, 2, H, W) fp32 (x_pixel_stride ignored): flow = coords1 - the pixel grid (raft.py:129) and its
   *     patch operand (channel t*2 + c; in_groups 4, weights packed as for oflow_flow_prep_s32's matrix) are built per
   *     output tile: bit for bit the conv of that matrix, which is then not written (1x1 geometry, block_n 128). */
  int in_format, in_groups;
  const void* d_x;
  long long x_pixel_stride;
  const float *d_in_scale, *d_in_shift;
  /* Weights: d_wpack = [in_groups][kh*kw][n_pad][hi[32] | lo[32]] fp16 after scaling output channel n by 2^s_n
   * (|w| <= 2^14), 16-B aligned; d_wscale[n] = 2^-s_n ([n_pad]); d_bias [N] or NULL; N real output channels.
   * d_wfrag: an optional fragment-major copy of d_wpack (same bytes, reordered [group][tap][n/32][slice][hi|lo][k half]
   * [row][8]: one wave's 32x16 MFMA B fragment is 1 KB contiguous and goes straight into registers, skipping the LDS
   * staging of B; 16-B aligned, n_pad % 32 == 0). Used, on S32 input without d_stats outside the small-grid tiles, by
   * every multi-tap convolution with block_n 128 and by 3x3 convolutions with block_n 64 or 32 (these two measured
   * slower in the RAFT step, DESIGN.md §4 r04: pass NULL for them unless comparing); other shapes ignore it. */
  const void *d_wpack, *d_wfrag;
  const float *d_wscale, *d_bias;
  int n_pad, N;
  /* Geometry: a stride-1 'same' convolution of B images of H x W pixels, kernel kh x kw in {1x1, 3x3, 1x5, 5x1} or 2x2
   * (taps at offsets -1, 0); block_n in {32, 64, 96, 128} output channels per workgroup divides n_pad. */
  int B, H, W, kh, kw, block_n;
  /* Epilogue, activation and scale: value = act(acc * d_wscale[n] + d_bias[n]) * out_scale, activation 0 none, 1 relu,
   * 2 sigmoid, 3 tanh, which epilogue 0 stores to any of the S32, fp32 and encoder destinations below; epilogues 1 and 2
   * are the GRU's, OFLOW_EPI_FLOW_HEAD the flow head's (both below; the GRU epilogues ignore activation). */
  int epilogue, activation;
  float out_scale;
  /* S32 and fp32 destinations (epilogue 0; at least one destination of this or the encoder group): S32 d_y0 (and d_y1)
   * for channels n < N (16-B aligned, pixel strides % 128 == 0), and / or fp32 NCHW d_f32 (batch / channel strides in
   * floats; f32_accumulate = 1 adds to it). */
  void *d_y0, *d_y1;
  long long y0_pixel_stride, y1_pixel_stride;
  float* d_f32;
  long long f32_batch_stride, f32_channel_stride;
  int f32_accumulate;
  /* GRU (block_n 128, 1x5 / 5x1; d_gru_h, d_gru_z [P][CH] fp32, CH = gru_channels, CH % 8 == 0, read / written as
   * 16-B vectors: both 16-byte aligned, else OFLOW_E_ALIGN):
   *   epilogue 1 (gates, N = 2*CH): n < CH -> z = sigmoid(.) into d_gru_z;
   *     n >= CH -> sigmoid(.) * d_gru_h[p][n-CH] into S32 d_y0 channel n-CH                      (update.py:91-96)
   *   epilogue 2 (candidate, N = CH): h = (1 - z) * h + z * tanh(.), in place in d_gru_h and into S32 d_y0
   *     (update.py:96-97). */
  float *d_gru_h, *d_gru_z;
  int gru_channels;
  /* Encoder options (epilogue 0 only):
   *   d_nhwc : fp32 [P][nhwc_pixel_stride] copy of the value (after activation / residual); 16-B aligned,
   *            nhwc_pixel_stride >= N, a multiple of 4;
   *   d_stats: per-tile instance-norm partials (count, mean, M2) of the pre-activation conv output, layout
   *            [B][ceil(H/4)*ceil(W/32)][n_pad][3] floats (reduced by oflow_norm_stats_finalize);
   *   d_res  : S32 residual added after the activation, then res_activation (relu(x + y), extractor.py:90);
   *   s2d    : S32 destinations in space-to-depth layout (pixel (y/2, x/2), channel + ((y%2)*2 + x%2) * N), the input
   *            form of the next stage's stride-2 convolutions (a 3x3/2 conv = a 2x2/1 conv on s2d input, a 1x1/2 conv =
   *            a 1x1 conv over the first N channels of it); H, W even, N % 8 == 0. */
  float *d_nhwc, *d_stats;
  const void* d_res;
  long long res_pixel_stride;
  int nhwc_pixel_stride, res_activation, s2d;
  /* Addend (GRU epilogues only): fp32 NHWC d_addend[P * addend_pixel_stride + n] added to the pre-activation value
   * after the scale and bias (16-B aligned, addend_pixel_stride >= N, a multiple of 4, N % 8 == 0). It carries the
   * GRU's loop-invariant context term: x = [inp | motion] (update.py:153-154) and inp never changes across iterations
   * (raft.py:115-118), so W_inp * inp + bias is computed once per forward and the per-iteration z / r / q convolutions
   * (update.py:92-105) run over [h | motion | flow] only. */
  const float* d_addend;
  long long addend_pixel_stride;
  /* Flow head (epilogue OFLOW_EPI_FLOW_HEAD): update.py:31-37, conv2(relu(conv1(x))), with its 256 -> 2 output conv
   * folded into conv1's epilogue. The call is conv1 (3x3, S32 input, N = n_pad = 256, activation 1 = ReLU, out_scale 1,
   * block_n 64 or 128; 128 needs d_wfrag); relu(conv1) is never stored. Per pixel and 64-channel slab the epilogue
   * forms the 18 per-tap products of conv2 at that INPUT pixel,
   *   d_fh_partial[slab][b][t*2 + c][y][x] = sum_{ch in slab} relu(conv1)[b][slab*64 + ch][y][x] * W2[c][slab*64 + ch][ky][kx],
   *   t = ky*3 + kx   (fp32, [fh_slabs][B][18][H][W], every in-image element written on every call),
   * as fp32 FMAs on the fp32 values (nothing is re-split to fp16) in an order that depends on the channel's index
   * within the slab only -- two fmaf chains over the slab's even and odd channels, each ascending, then even + odd --
   * so every block_n and weight staging gives the same bits. oflow_flow_head_finish_f32 gathers the taps and slabs.
   *   d_fh_weights: conv2's weight (2, 256, 3, 3) repacked [slab 4][channel 64][t*2 + c] fp32;
   *   fh_slabs    : N / 64 = 4 (else OFLOW_E_SHAPE).
   * Every destination of the other epilogues and d_addend must be NULL (OFLOW_E_MODE). Always the default 4 x 32 tiles,
   * small grids included. Any other epilogue ignores these three fields. */
  const float* d_fh_weights;
  float* d_fh_partial;
  int fh_slabs;
} oflow_conv_s32_desc;
int oflow_conv_s32(const oflow_conv_s32_desc* desc, void* stream);

/* oflow_flow_head_col2im_f32: d_coords (B, 2, H, W) += d_bias[c] + sum_{ky,kx} d_y[b][(ky*3+kx)*2 + c][y+ky-1][x+kx-1]
 * (zero outside the image): the flow head's output conv (update.py:35-36, conv2 3x3 C -> 2, raft.py:133 coords1 +=
 * delta_flow) as a 1x1 conv C -> 18 per-tap products (oflow_conv_s32 with an fp32 NCHW destination d_y (B, 18, H, W))
 * followed by this gather. */
int oflow_flow_head_col2im_f32(const float* d_y, const float* d_bias, int B, int H, int W, float* d_coords, void* stream);
/* oflow_flow_head_finish_f32: the second half of the flow head folded into conv1 (oflow_conv_s32,
 * OFLOW_EPI_FLOW_HEAD) and the next iteration's flow channels. Per pixel and output channel c, in this order:
 *   s = 0; for t = 0..8 (ky = t / 3, kx = t % 3), for slab = 0..slabs-1:
 *     s += d_partial[slab][b][t*2 + c][y + ky - 1][x + kx - 1]   (neighbours outside the image contribute nothing);
 *   d_coords[b][c][y][x] += s + d_bias[c]      (raft.py:133 coords1 = coords1 + delta_flow; d_coords contiguous)
 * then flow = coords1 - coords0 of the UPDATED coords1 (raft.py:129; coords0 the pixel grid) goes, split into fp16
 * hi + lo, into the two flow channels of the GRU input buffers d_flow0 / d_flow1 (NULL: not written) -- the bytes, and
 * the range-flag behaviour, of oflow_flow_prep_s32 called on the updated coords1 with the same destinations.
 * d_partial: [slabs][B][18][H][W] fp32, slabs = 4. */
int oflow_flow_head_finish_f32(const float* d_partial, int slabs, const float* d_bias, int B, int H, int W,
                               float* d_coords, void* d_flow0, long long flow0_pixel_stride, void* d_flow1,
                               long long flow1_pixel_stride, void* stream);

/* oflow_normalize_images_f32: y = 2 * (x / 255) - 1 for two frames of n fp32 values each (4-B aligned; vector loads
 * when n % 4 == 0 and 16-B aligned): RAFT.forward's input scaling (methods/raft/model/raft.py:104-105), the reference's
 * fp32 operations (a correctly rounded division) in one pass -- bit-identical to the reference on the CPU. */
int oflow_normalize_images_f32(const float* d_x0, const float* d_x1, long long n, float* d_y0, float* d_y1, void* stream);

/* oflow_replicate_pad_f32: InputPadder.pad (methods/raft/model/utils.py:38-61, F.pad(x, [left, right, top, bottom],
 * mode="replicate")) of `count` (1..4) tensors of `planes` x H x W fp32 values each (host arrays of device pointers),
 * into planes x (H + top + bottom) x (W + left + right): a copy, bit-exact, one launch. */
int oflow_replicate_pad_f32(const float* const* d_src, float* const* d_dst, int count, long long planes, int H, int W,
                            int top, int bottom, int left, int right, void* stream);

/* oflow_set_range_flag: register d_flag (one unsigned int in device memory of the current device; NULL: off) as the
 * range flag of the split-fp16 operands. Every kernel that writes or stages S32 values (the conv epilogues and staging,
 * norm_apply, pack / flow_prep, the fused lookup + convc1) sets it to 1 (atomic or) when a value's hi half overflows
 * fp16 (|x| >= 65520 or inf); it is never cleared by the library. Synchronous (a copy to each kernel module's symbol). */
int oflow_set_range_flag(unsigned int* d_flag);

/* oflow_range_flag_exchange: *d_out = the range flag's value, and the flag cleared, in one device atomic exchange on
 * `stream` (enqueued after a forward's kernels: that forward's snapshot; an overflow set concurrently by a forward on
 * another stream lands in this snapshot or the next one, never lost). d_flag: the pointer given to
 * oflow_set_range_flag; d_out: one unsigned int of device memory. Replaces nothing in the reference (the split-fp16
 * range guard of RAFT.forward, methods/raft/model/raft.py:87-147, is this build's addition). */
int oflow_range_flag_exchange(unsigned int* d_flag, unsigned int* d_out, void* stream);

/* Instrumentation (bench.py's per-kernel timings; replaces nothing in the reference): HIP timing events that can be
 * recorded inside a stream capture as external event-record nodes (external != 0), so every replay of the graph
 * re-records them; oflow_timing_event_elapsed_ms = hipEventElapsedTime(end - start). Status OFLOW_OK or a HIP error. */
int oflow_timing_event_create(void** ev);
int oflow_timing_event_destroy(void* ev);
int oflow_timing_event_record(void* ev, void* stream, int external);
int oflow_timing_event_elapsed_ms(void* start, void* end, float* ms);

/* oflow_flow_head2_s32: the flow head's output conv (update.py:35-36 conv2: 3x3, C -> 2, zero padding) added into
 * coords (B, 2, H, W) fp32 in place (raft.py:133 `coords1 = coords1 + delta_flow`), from an S32 input of in_groups
 * groups (1..8): fp32 FMAs on the exact S32 values; d_weight (2, C, 3, 3) fp32 as the nn.Conv2d stores it, d_bias [2].
 * Built for small grids (one image at 1/8 resolution); larger ones run faster as oflow_conv_s32 with n_pad 32. */
int oflow_flow_head2_s32(const void* d_x, long long x_pixel_stride, int in_groups, const float* d_weight,
                         const float* d_bias, int B, int H, int W, float* d_coords, void* stream);
/* oflow_flow_head2_tiled_s32: oflow_flow_head2_s32 for large grids (update.py:36 FlowHead.conv2 + raft.py:133): each
 * workgroup stages a 4 x 32 output tile's 6 x 34 halo per 32-channel group in LDS as fp32 (hi + lo) and runs the
 * 3x3 x C -> 2 products as fp32 FMAs. d_wr: the weight (2, C, 3, 3) repacked [group][4-channel chunk][tap][output][4]
 * (16-B aligned); coords1 (B, 2, H, W) += conv + bias. */
int oflow_flow_head2_tiled_s32(const void* d_x, long long x_pixel_stride, int in_groups, const float* d_wr,
                               const float* d_bias, int B, int H, int W, float* d_coords, void* stream);
/* oflow_corr_lookup_tiled_nhwc_f32: the tiled lookup as fp32 NHWC rows [B*H*W][row_floats] (d_out 16-B aligned) in the
 * reference's channel order: row q, channel l*(2r+1)^2 + k = oflow_corr_lookup_tiled_f32's (b, l*(2r+1)^2 + k, y, x) bit for
 * bit; row_floats >= num_levels*(2r+1)^2, channels past that are not written. With row_floats = num_levels*(2r+1)^2 (324)
 * it is the RAFT forward's convc1 input (oflow_conv_s32, OFLOW_IN_F32). Replaces corr.py:56-77 + the permute feeding
 * update.py:120-121. */
int oflow_corr_lookup_tiled_nhwc_f32(const float* const* d_levels, const int* level_h, const int* level_w, int num_levels,
                                     const float* d_coords, int B, int H, int W, int radius, float* d_out, int row_floats,
                                     void* stream);
/* oflow_corr_lookup_convc1_s32: the tiled lookup fused into the motion encoder's first convolution -- S32 output
 * y = relu(convc1(corr_fn(coords))) (256 channels: d_y + P * y_pixel_stride, 8 groups), the lookup volume never
 * written. Replaces raft.py:128 (corr.py:56-77) + update.py:120-121 (`F.relu(self.convc1(corr))`) in the forward.
 * Weights: oflow_conv_s32's packing (1x1, n_pad 256) of convc1 with its input channels regrouped per level -- level l's
 * tap k at channel l*G*32 + k, G = ceil((2r+1)^2/32), zeros elsewhere (num_levels*G k32 groups) -- stored
 * fragment-major: [group][wave 4][n tile 2][sub 2][hi, lo][lane 64][8 fp16], where lane = hh*32 + r holds output channel
 * wave*64 + ntile*32 + r, inputs k = 16*sub + 8*hh .. +7 of the group (the same bytes as the conv packing
 * [group][256][hi 32 | lo 32], permuted); d_wscale [256], d_bias [256] or NULL. radius 3 or 4 (else OFLOW_E_RADIUS),
 * y_pixel_stride % 128 == 0. */
int oflow_corr_lookup_convc1_s32(const float* const* d_levels, const int* level_h, const int* level_w, int num_levels,
                                 const float* d_coords, int B, int H, int W, int radius, const void* d_wpack,
                                 const float* d_wscale, const float* d_bias, void* d_y, long long y_pixel_stride,
                                 void* stream);

/*
 * Encoders on the split-fp16 path (methods/raft/model/extractor.py:35-231; csrc/encoder_s32.hip).
 *
 * oflow_stem_patches_s32: 7x7/2 pad-3 patch matrix of a (B, C, H, W) fp32 image: S32 (B, ceil(H/2), ceil(W/2),
 *   out_groups) with channel t*C + c (t = ky*7 + kx), zeros past 49*C.
 * oflow_norm_stats_finalize: merge the partials (fp64 sums) -> alpha = 1/sqrt(var + eps), beta = -mean * alpha, [B][C].
 * oflow_norm_apply_s32: y = act(x*alpha + beta) for x [P][C] fp32 (C % 8 == 0); res_mode 1: y = res_act(y + S32 res),
 *   res_mode 2: y = res_act((x2*alpha2 + beta2) + y); res_mode 3: y = res_act(relu(x2*alpha2 + beta2) + y) (a block
 *   input kept as raw fp32 + its norm); written as S32 (s2d: space-to-depth as above).
 */
int oflow_stem_patches_s32(const float* d_img, int B, int C, int H, int W, void* d_out, int out_groups, void* stream);
int oflow_norm_stats_finalize(const float* d_partials, int B, int tiles, int n_pad, int C, double eps, float* d_alpha,
                              float* d_beta, void* stream);
int oflow_norm_apply_s32(const float* d_x, int C, int B, int H, int W, const float* d_alpha, const float* d_beta,
                         int activation, int res_mode, const void* d_res, long long res_pixel_stride, const float* d_x2,
                         const float* d_alpha2, const float* d_beta2, int res_activation, int s2d, void* d_y,
                         long long y_pixel_stride, void* stream);

/*
 * Convex upsampling (methods/raft/model/raft.py:73-85, RAFT.upsample_flow; csrc/upsample.hip).
 * oflow_convex_upsample_f32: flow (B, 2, H, W), mask (B, 576, H, W) (the mask head output, already x0.25) ->
 *   out (B, 2, 8H, 8W): softmax over the 9 neighbours of each 8x8 sub-pixel, convex combination of 8*flow over the
 *   zero-padded 3x3 neighbourhood. B, H <= 65535.
 */
int oflow_convex_upsample_f32(const float* d_flow, const float* d_mask, int B, int H, int W, float* d_out, void* stream);
/*
 * oflow_convex_upsample_backward_f32 (csrc/upsample_backward.hip): its autograd transpose for a training step
 *   (raft.py:149-175). d_grad_out (B, 2, 8H, 8W), the forward's flow and mask -> d_grad_flow (B, 2, H, W) and
 *   d_grad_mask (B, 576, H, W). The softmax is recomputed from the mask; nothing else is kept from the forward.
 *   Either output may be NULL (that gradient is not formed: no stores of d_grad_mask, or no flow phase); both NULL is
 *   OFLOW_E_NULL. Every element of a requested output is written (the caller zeroes nothing), with no atomics: two
 *   calls give the same bits.
 *   d_scratch: B * 18 * H * W floats, required when d_grad_flow is not NULL (else ignored, may be NULL); it holds the
 *   per-pixel tap sums (B, 18, H, W) between the main pass and the nine-tap gather and needs no initialisation.
 *   B, H <= 65535.
 */
int oflow_convex_upsample_backward_f32(const float* d_grad_out, const float* d_flow, const float* d_mask, int B, int H,
                                       int W, float* d_grad_flow, float* d_grad_mask, float* d_scratch, void* stream);

/*
 * Backward of the update block's convolutions (methods/raft/model/update.py:31-161 under autograd, the training step
 * raft.py:149-175; csrc/conv_backward.hip). Stride 1, dilation 1, groups 1, odd kh, kw <= 7 with zero padding
 * (kh/2, kw/2), contiguous fp32 NCHW: d_grad_out (B, Cout, H, W), d_x (B, Cin, H, W), d_weight (Cout, Cin, kh, kw).
 * With oy = ky - kh/2, ox = kx - kw/2 and out-of-image terms zero:
 *   d_grad_input[b, c, y, x]    = sum_{ky, kx, n} grad_out[b, n, y - oy, x - ox] * weight[n, c, ky, kx]
 *   d_grad_weight[n, c, ky, kx] = sum_{b, y, x}   grad_out[b, n, y, x] * x[b, c, y + oy, x + ox]
 *   d_grad_bias[n]              = sum_{b, y, x}   grad_out[b, n, y, x]
 * on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 fma chains). Every element of a requested output is
 * written (the caller zeroes nothing), in a fixed summation order and with no atomics: two calls give the same bits.
 * Sizes: Cout, Cin <= 65535, B*H*W <= 65535 * oflow_conv2d_backward_weight_slab_pixels(), Cout*Cin*kh*kw < 2^31; a
 * non-positive size, an even or > 7 kernel size or a size past these limits is OFLOW_E_SHAPE.
 *
 * oflow_conv2d_backward_weight_f32 splits the pixel sum into slabs of oflow_conv2d_backward_weight_slab_pixels()
 * flattened (b, y, x) pixels; each slab's partial goes to d_workspace and a second kernel adds the slabs in ascending
 * order. d_workspace: oflow_conv2d_backward_weight_workspace_floats(...) floats (0 for a shape the call would refuse),
 * no initialisation needed. d_grad_weight or d_grad_bias may be NULL (that gradient is not formed; both NULL is
 * OFLOW_E_NULL); d_x may be NULL when d_grad_weight is.
 */
int oflow_conv2d_backward_input_f32(const float* d_grad_out, const float* d_weight, int B, int Cout, int Cin, int H, int W,
                                    int kh, int kw, float* d_grad_input, void* stream);
int oflow_conv2d_backward_weight_slab_pixels(void);
long long oflow_conv2d_backward_weight_workspace_floats(int B, int Cout, int Cin, int H, int W, int kh, int kw);
int oflow_conv2d_backward_weight_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin, int H, int W,
                                     int kh, int kw, float* d_grad_weight, float* d_grad_bias, float* d_workspace,
                                     void* stream);

/*
 * The same gradients for stride 1 or 2 (the same in y and x): the encoders' convolutions
 * (methods/raft/model/extractor.py:35-231 under autograd; csrc/conv_backward.hip). H, W are the input's; d_grad_out is
 * (B, Cout, H', W') with H' = (H + stride - 1) / stride, W' likewise (odd sizes are legal). With py = kh/2, px = kw/2:
 *   d_grad_input[b, c, y, x]    = sum grad_out[b, n, Y, X] * weight[n, c, ky, kx]
 *                                 over (ky, kx, n) with stride*Y = y + py - ky, stride*X = x + px - kx inside the output
 *   d_grad_weight[n, c, ky, kx] = sum_{b, Y, X} grad_out[b, n, Y, X] * x[b, c, stride*Y + ky - py, stride*X + kx - px]
 *   d_grad_bias[n]              = sum_{b, Y, X} grad_out[b, n, Y, X]
 * Every element of d_grad_input is written (at stride 2 under a 1x1 kernel three of four are exact zeros). The slabs of
 * the weight gradient are oflow_conv2d_backward_weight_slab_pixels() flattened OUTPUT pixels. The NULL conventions, the
 * workspace rule and the size limits are those of the stride-1 calls, with B*H'*W' in the pixel limit and B*H*W < 2^31;
 * a stride other than 1 or 2 is OFLOW_E_SHAPE. With stride 1 the results are bit-identical to the stride-1 calls',
 * except the weight gradient with Cin <= 4: there the (channel, tap) pairs are folded into one tile dimension (the
 * 3 -> 64 7x7 stem: 3 tiles of 64 columns instead of 49 tap slices with 3 columns filled).
 * oflow_conv2d_strided_backward_weight_generic_f32 is that call without the folding (what the folded path is measured
 * and tested against).
 */
int oflow_conv2d_strided_backward_input_f32(const float* d_grad_out, const float* d_weight, int B, int Cout, int Cin, int H,
                                            int W, int kh, int kw, int stride, float* d_grad_input, void* stream);
long long oflow_conv2d_strided_backward_weight_workspace_floats(int B, int Cout, int Cin, int H, int W, int kh, int kw,
                                                                int stride);
int oflow_conv2d_strided_backward_weight_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin, int H,
                                             int W, int kh, int kw, int stride, float* d_grad_weight, float* d_grad_bias,
                                             float* d_workspace, void* stream);
int oflow_conv2d_strided_backward_weight_generic_f32(const float* d_grad_out, const float* d_x, int B, int Cout, int Cin,
                                                     int H, int W, int kh, int kw, int stride, float* d_grad_weight,
                                                     float* d_grad_bias, float* d_workspace, void* stream);

/*
 * Backward of the encoders' norm layers with the ReLU that follows them folded in (extractor.py:35-231 under autograd;
 * csrc/norm_backward.hip). Contiguous fp32 planes of HW elements; relu != 0: the layer's output went through a ReLU,
 * whose mask is recomputed from x (nothing but x is kept from the forward). Per plane mu, r = 1/sqrt(var_biased + eps),
 * xh = (x - mu) * r, g = grad_out * [output > 0] (relu) or grad_out.
 *   oflow_instance_norm_backward_f32 (InstanceNorm2d without affine parameters; planes = B * C):
 *     d_grad_input = r * (g - mean(g) - xh * mean(g * xh)), the statistics recomputed in fp64.
 *   oflow_frozen_batch_norm_backward_f32 (BatchNorm2d on its running statistics: eval mode / RAFT.freeze_bn()):
 *     y = (x - running_mean) * weight / sqrt(running_var + eps) + bias;  d_grad_input = g * weight / sqrt(running_var + eps),
 *     d_grad_weight[c] = sum_{b, pixels} g * (x - running_mean) / sqrt(running_var + eps), d_grad_bias[c] = sum g.
 *     A NULL output is not formed (all three NULL: OFLOW_E_NULL). d_workspace:
 *     oflow_frozen_batch_norm_backward_workspace_floats(B, C, HW) floats, needed (and fully written) when a parameter
 *     gradient is asked for; it holds one partial per plane, added over b in ascending order by a second kernel.
 * No atomics, a fixed summation order: two calls give the same bits. Non-positive sizes or eps < 0: OFLOW_E_SHAPE.
 */
int oflow_instance_norm_backward_f32(const float* d_grad_out, const float* d_x, int planes, int HW, double eps, int relu,
                                     float* d_grad_input, void* stream);
long long oflow_frozen_batch_norm_backward_workspace_floats(int B, int C, int HW);
int oflow_frozen_batch_norm_backward_f32(const float* d_grad_out, const float* d_x, const float* d_weight, const float* d_bias,
                                         const float* d_running_mean, const float* d_running_var, int B, int C, int HW,
                                         double eps, int relu, float* d_grad_input, float* d_grad_weight, float* d_grad_bias,
                                         float* d_workspace, void* stream);

/*
 * Batch norm on batch statistics with the ReLU that follows it folded in (relu != 0): nn.BatchNorm2d in train mode,
 * cnet in the Chairs stage (extractor.py:35-231; csrc/batch_norm.hip). Contiguous fp32 NCHW, HW = H * W, n = B * HW.
 *   forward:  d_mean[c], d_var[c] (biased) over (B, H, W), formed from fp64 sums shifted by x[0, c, 0, 0] (a constant
 *             channel has var = 0 exactly); r = 1 / sqrt(var + eps); d_y = (x - mean) * r * weight + bias [ReLU].
 *             d_y == NULL: statistics only (d_weight, d_bias may then be NULL too). d_mean, d_var (C floats each) and the
 *             workspace are required. Running statistics are the caller's business (var * n / (n - 1) is the unbiased one).
 *   backward: takes d_mean and d_var as the forward returned them (it does not recompute them) and recomputes the ReLU
 *             mask from x with the forward's own arithmetic. g = grad_out * [y > 0] (relu) or grad_out, xh = (x - mean) * r:
 *             d_grad_bias = sum g, d_grad_weight = sum g * xh,
 *             d_grad_input = weight * r * (g - d_grad_bias / n - xh * d_grad_weight / n).
 *             A NULL output is not formed (all three NULL: OFLOW_E_NULL); the others are the same bits whichever are asked
 *             for. d_grad_input needs both channel sums, so the workspace is required by every backward call.
 * d_workspace: oflow_batch_norm_workspace_floats(B, C, HW) floats, a function of the shape alone (0 for a shape the calls
 * refuse), required by both calls and fully written by each; nothing needs zeroing. It holds fp64 partial sums (two per
 * plane and chunk of oflow_batch_norm_chunk_elements() elements, two per channel), so the pointer must be 8-byte
 * aligned: otherwise OFLOW_E_ALIGN. Non-positive sizes, eps < 0 or NaN, or B * C * chunks past 2^31 - 1: OFLOW_E_SHAPE.
 * Nothing is written on an error. No atomics, a fixed summation order: bit-reproducible for a given shape and
 * alignment (16-byte aligned tensors move as float4, others as scalars).
 */
int oflow_batch_norm_chunk_elements(void);
long long oflow_batch_norm_workspace_floats(int B, int C, int HW);
int oflow_batch_norm_forward_f32(const float* d_x, const float* d_weight, const float* d_bias, int B, int C, int HW,
                                 double eps, int relu, float* d_y, float* d_mean, float* d_var, float* d_workspace,
                                 void* stream);
int oflow_batch_norm_backward_f32(const float* d_grad_out, const float* d_x, const float* d_weight, const float* d_bias,
                                  const float* d_mean, const float* d_var, int B, int C, int HW, double eps, int relu,
                                  float* d_grad_input, float* d_grad_weight, float* d_grad_bias, float* d_workspace,
                                  void* stream);

/*
 * Backward of the correlation (methods/raft/model/corr.py:38-87 + utils.py:64-80 under autograd, the training step
 * raft.py:149-175; csrc/corr_backward.hip). Canonical levels (B*H*W, H_l, W_l) fp32.
 * oflow_corr_lookup_backward_f32: d_grad_out (B, L*(2r+1)^2, H, W) -> d_grad_levels[l] += its gradient (same window
 *   and weights as the forward; coordinates get none: the reference detaches them, raft.py:127).
 * oflow_corr_pyramid_grad_combine_f32: d_grad_levels[0] += sum_{l>0} of level l's gradient pushed back through the
 *   floor 2x2 average pools (value / 4^l on every level-0 cell it averaged).
 */
int oflow_corr_lookup_backward_f32(const float* d_grad_out, const float* d_coords, int B, int H, int W, int radius,
                                   float* const* d_grad_levels, const int* level_h, const int* level_w, int num_levels,
                                   void* stream);
int oflow_corr_pyramid_grad_combine_f32(float* const* d_grad_levels, const int* level_h, const int* level_w,
                                        int num_levels, long long Q, void* stream);
/* oflow_corr_fmap_grad_f32: the feature-map gradients of corr.py:85 (corr = f1^T f2 / sqrt(C)) from the level-0-folded
 *   gradient g0 (B, N, N) (query-major): d_grad_f1 (B, C, N) = scale * f2 . g0^T, d_grad_f2 (B, C, N) = scale * f1 . g0
 *   (scale = 1/sqrt(C)), fmaps (B, C, N) fp32; fp32 MFMA GEMMs, deterministic. Either output may be NULL. */
int oflow_corr_fmap_grad_f32(const float* d_fmap1, const float* d_fmap2, const float* d_g0, int B, int C, int N,
                             float scale, float* d_grad_f1, float* d_grad_f2, void* stream);

/*
 * Backward of the warp / grid_sample (optical_flow/operator/operator.py:8-56, utils.py:64-80 under autograd; SURVEY
 * §8(f) row 3; csrc/warp_backward.hip): ATen grid_sampler_2d_backward's formulas for every mode / padding /
 * align_corners. d_grad_frame / d_grad_input must be zero-filled by the caller (taps are added with fp32 atomics);
 * either output may be NULL.
 * oflow_grid_warp_backward_f32: d_grad_out (B, C, H, W), frame (B, C, H, W), normalized flow (B, 2, H, W) ->
 *   d_grad_frame (B, C, H, W) += ..., d_grad_flow (B, 2, H, W) = dL/d(grid) (grid = linspace base + flow).
 * oflow_grid_sample_backward_f32: d_grad_out (B, C, Ho, Wo), input (B, C, H, W), grid (B, Ho, Wo, 2) ->
 *   d_grad_input += ..., d_grad_grid (B, Ho, Wo, 2).
 */
int oflow_grid_warp_backward_f32(const float* d_grad_out, const float* d_frame, const float* d_flow, int B, int C, int H,
                                 int W, int mode, int padding_mode, int align_corners, float* d_grad_frame,
                                 float* d_grad_flow, void* stream);
int oflow_grid_sample_backward_f32(const float* d_grad_out, const float* d_input, const float* d_grid, int B, int C,
                                   int H, int W, int Ho, int Wo, int mode, int padding_mode, int align_corners,
                                   float* d_grad_input, float* d_grad_grid, void* stream);

/*
 * Inference I/O (csrc/flow_io.hip).
 * oflow_flow_stats_f32: flow (B, 2, H, W) -> d_partials (B, OFLOW_FLOW_STATS_CHUNKS, 2): per-chunk maxima of |flow|
 *   and of the flow values, after clip to [clip_lo, clip_hi] (when clip != 0) and y negation (when invert_y != 0).
 * oflow_flow2rgb_f32: flow (B, 2, H, W) -> d_rgb (B, 3, H, W) in [0, 1], the reference's flow2rgb
 *   (optical_flow/visualization/flow2rgb.py:19-73). method OFLOW_FLOW2RGB_{BAKER,HSV,MEISTER}. The flow is divided
 *   by denom (= max_norm + 1e-5, the caller's max_norm) when have_denom != 0, else by max|flow| + 1e-5 taken from
 *   d_partials (which oflow_flow_stats_f32 must have filled with the same clip / invert_y, earlier on the stream).
 *   d_partials is also required for MEISTER (its max_flow). Same clip / invert_y semantics as above.
 * oflow_flow_pack_f32: planar flow (B, 2, H, W) -> per image the file payload (H, W, channels) fp32:
 *   channels 2 = Middlebury .flo rows (io/middlebury.py:64-71); channels 3 = PFM rows with a zero third channel,
 *   written bottom row first when flip_rows != 0 (io/pfm.py:95-98). B, H <= 65535.
 */
#define OFLOW_FLOW_STATS_CHUNKS 128
#define OFLOW_FLOW2RGB_BAKER 0
#define OFLOW_FLOW2RGB_HSV 1
#define OFLOW_FLOW2RGB_MEISTER 2
int oflow_flow_stats_f32(const float* d_flow, int B, int H, int W, int clip, float clip_lo, float clip_hi,
                         int invert_y, float* d_partials, void* stream);
int oflow_flow2rgb_f32(const float* d_flow, int B, int H, int W, int method, int clip, float clip_lo, float clip_hi,
                       int invert_y, int have_denom, float denom, const float* d_partials, float* d_rgb, void* stream);
int oflow_flow_pack_f32(const float* d_flow, int B, int H, int W, int channels, int flip_rows, float* d_out,
                        void* stream);

/*
 * Evaluation metrics and the training loss as fused streaming reductions (optical_flow/metrics/epe.py:24-65,
 * optical_flow/metrics/f1.py:34-55, methods/raft/model/raft.py:231-260; csrc/flow_metrics.hip). Each is a partial
 * kernel of at most OFLOW_FLOW_METRICS_PARTIALS workgroups, one row of 8 doubles each in d_workspace
 * (>= OFLOW_FLOW_METRICS_PARTIALS * 8 doubles, 8-B aligned, any contents), and a one-workgroup finalize kernel that sums
 * the rows in a fixed order: no float atomics, results bit-reproducible from run to run, no host synchronisation.
 *
 * oflow_flow_error_stats_f32: d_pred, d_target (B, 2, H, W) fp32 views with batch / channel / row strides in elements
 *   (W stride 1; a cropped view such as InputPadder.unpad's is read in place). d_valid: (B, H, W) with batch / row
 *   strides, valid_kind OFLOW_VALID_NONE (d_valid ignored), _F32 or _U8 (1-byte bool / uint8, non-zero = 1). Per pixel
 *   in fp32, no contraction: dx = p0 - t0, dy = p1 - t1, epe = sqrt(dx*dx + dy*dy), mag = sqrt(t0*t0 + t1*t1),
 *   keep = (valid >= 0.5) && (mag < max_flow, only when max_flow is positive and finite),
 *   outlier = (epe > abs_threshold) && (epe / mag > rel_threshold) with a true division (mag == 0: an outlier when
 *   epe > abs_threshold; 0 / 0 and a NaN prediction are not). Over the kept pixels
 *     d_accum[0..5] += {sum epe, n, n_outlier, n(epe < 1), n(epe < 3), n(epe < 5)}   (fp64; d_accum[6..7] untouched)
 *   so one accumulator serves any number of calls; d_epe_map (NULL: none): contiguous (B, H, W) fp32, epe of EVERY pixel.
 *   16-B loads when every base and stride allows, coalesced dword loads otherwise.
 * oflow_sequence_loss_f32: d_preds: host array of n_preds (1..OFLOW_MAX_PREDS) device pointers to contiguous
 *   (B, 2, H, W) fp32 predictions, weights: n_preds HOST floats (gamma^(n - i - 1)), d_flow_gt (B, 2, H, W), d_valid
 *   (B, H, W) of kind _F32 or _U8, all contiguous. mask = (valid >= 0.5) && (mag_gt < max_flow);
 *   d_loss[0] = fp32(sum_i w_i * sum mask * (|dx_i| + |dy_i|) / (2 B H W)) (the mask multiplies: NaN under it propagates);
 *   d_stats[0..7] = {n_valid, n(epe < 1), n(epe < 3), n(epe < 5), sum epe, the fp64 loss sum, 0, 0} of the LAST prediction
 *   over the masked pixels (written, not added).
 * oflow_sequence_loss_backward_f32: d_grads[i] (NULL: prediction i needs none) = (gout * w_i / (2 B H W)) * mask *
 *   sgn(pred_i - gt), sgn(0) = sgn(NaN) = 0 (ATen's abs backward); gout = d_grad_out[0], a device scalar. One launch.
 */
#define OFLOW_FLOW_METRICS_PARTIALS 1024
#define OFLOW_MAX_PREDS 32
#define OFLOW_VALID_NONE 0
#define OFLOW_VALID_F32 1
#define OFLOW_VALID_U8 2
int oflow_flow_error_stats_f32(const float* d_pred, long long pred_sb, long long pred_sc, long long pred_sh,
                               const float* d_target, long long target_sb, long long target_sc, long long target_sh,
                               const void* d_valid, int valid_kind, long long valid_sb, long long valid_sh, int B, int H,
                               int W, float abs_threshold, float rel_threshold, float max_flow, float* d_epe_map,
                               double* d_workspace, double* d_accum, void* stream);
int oflow_sequence_loss_f32(const float* const* d_preds, int n_preds, const float* weights, const float* d_flow_gt,
                            const void* d_valid, int valid_kind, int B, int H, int W, float max_flow,
                            double* d_workspace, float* d_loss, double* d_stats, void* stream);
int oflow_sequence_loss_backward_f32(const float* d_grad_out, const float* const* d_preds, float* const* d_grads,
                                     int n_preds, const float* weights, const float* d_flow_gt, const void* d_valid,
                                     int valid_kind, int B, int H, int W, float max_flow, void* stream);

/*
 * Warm-start initialiser (RAFT's video mode; csrc/forward_interpolate.hip): the flow of one pair, forward-projected
 * along itself, as `flow_init` of the next pair -- upstream RAFT's forward_interpolate (scipy griddata(method="nearest")
 * on float64 coordinates) with the tie-break made explicit, on the device. The reference has no such function;
 * it only consumes the result (methods/raft/model/raft.py:122-123).
 * oflow_forward_interpolate_f32: d_flow, d_out contiguous (B, 2, H, W) fp32, channel 0 = dx, 1 = dy; d_out must not
 *   alias d_flow. Per image, with all selection arithmetic in float64:
 *     source s = y*W + x lands at x1 = x + (double)dx[s], y1 = y + (double)dy[s] (exact) and is LANDED iff
 *     x1 > 0 && x1 < W && y1 > 0 && y1 < H (so a NaN or +-inf flow never lands);
 *     out[:, qy, qx] = flow[:, s*], s* the landed source with the least (qx - x1)^2 + (qy - y1)^2 (two products and
 *     one sum, each rounded once to float64, no FMA contraction), ties to the LOWEST s; the selected fp32 values are
 *     copied unchanged; an image with no landed source gives all zeros (a cold start).
 *   Images are independent; no atomics and a fixed reduction order: bit-identical from run to run. One launch, no
 *   scratch, O((H*W)^2) candidate evaluations per image. B <= 65535, H*W <= 2^30.
 */
int oflow_forward_interpolate_f32(const float* d_flow, int B, int H, int W, float* d_out, void* stream);

/*
 * Forward-backward consistency (csrc/fb_consistency.hip): the occlusion masks of a pair of flows in pixel units, and
 * optionally the squared residuals, in one launch. The criterion is UnFlow's (Meister et al., AAAI 2018; their defaults
 * alpha = 0.01, beta = 0.5). The reference has no such function.
 * oflow_fb_consistency_f32: d_fw, d_bw contiguous (B, 2, H, W) fp32, channel 0 = dx, 1 = dy, 4-byte aligned (else
 *   OFLOW_E_ALIGN); d_mask_* (B, 1, H, W) bytes, written 0 or 1; d_err_* (B, 1, H, W) fp32. For image b, direction d
 *   (0: a = fw, o = bw, outputs *_fw; 1: a = bw, o = fw, outputs *_bw) and pixel (i, j):
 *     u = a[b,0,i,j], v = a[b,1,i,j] (fp32);
 *     px = float(j) + u, py = float(i) + v (fp32 sums, each rounded once);
 *     inside = px >= 0 && px <= W-1 && py >= 0 && py <= H-1 (false for NaN);
 *     not inside: mask = 1, err = +inf (the target left the frame, nothing is sampled);
 *     inside: x0 = floorf(px), x1 = min(x0+1, W-1), wx = px - x0, the same in y; s0, s1 the bilinear values of o[b,0],
 *       o[b,1] at those four taps in fp32, as top = t00 + wx*(t01 - t00), bot = t10 + wx*(t11 - t10),
 *       s = top + wy*(bot - top) (products and sums may be contracted into FMAs; a non-finite tap gives NaN in this
 *       form even under a zero weight);
 *       err = (u+s0)^2 + (v+s1)^2;  thr = alpha*(u^2 + v^2 + s0^2 + s1^2) + beta;
 *       mask = !(err <= thr), so non-finite values count as occluded.
 *   d_mask_fw is required. Direction 1 runs iff d_mask_bw != NULL (d_err_bw without it: OFLOW_E_NULL); d_err_fw and
 *   d_err_bw may be NULL, and the other outputs are the same bits whichever are asked for. NULL d_fw / d_bw / d_mask_fw:
 *   OFLOW_E_NULL. B, H or W < 1, B > 65535 or H*W > 2^30: OFLOW_E_SHAPE. An output that overlaps an input or another
 *   output: OFLOW_E_SHAPE. Every output element is written exactly once, no atomics: bit-identical from run to run.
 */
int oflow_fb_consistency_f32(const float* d_fw, const float* d_bw, int B, int H, int W, float alpha, float beta,
                             unsigned char* d_mask_fw, unsigned char* d_mask_bw, float* d_err_fw, float* d_err_bw,
                             void* stream);

/*
 * Forward warping / splatting (csrc/splat.hip, csrc/splat_backward.hip): summation, average, linear and softmax
 * splatting (Niklaus and Liu, CVPR 2020) of a frame along a flow in pixel units, deterministic in both directions. The
 * reference has no such function.
 * oflow_splat_f32: d_frame (B, C, H, W), d_flow (B, 2, H, W) (channel 0 = dx, 1 = dy), d_metric (B, 1, H, W) or NULL,
 *   all contiguous fp32; outputs d_out (B, C, H, W) and d_weight (B, 1, H, W) fp32, both required. mode:
 *     OFLOW_SPLAT_SUM     m = 1, out = N            (d_metric must be NULL, else OFLOW_E_MODE)
 *     OFLOW_SPLAT_AVG     m = 1, out = N / (D + EPS) (d_metric must be NULL, else OFLOW_E_MODE)
 *     OFLOW_SPLAT_LINEAR  m = metric (expected >= 0), out = N / (D + EPS)   (d_metric required, else OFLOW_E_NULL)
 *     OFLOW_SPLAT_SOFT    m = expf(fp32(metric - M_b)), M_b the maximum of image b's metric, out = N / (D + EPS)
 *   with EPS = OFLOW_SPLAT_EPS = 1e-7. For image b and source pixel s = (i, j) with u = flow[b,0,i,j], v = flow[b,1,i,j]:
 *     px = float(j) + u, py = float(i) + v (fp32 sums, each rounded once, as oflow_fb_consistency_f32 forms them);
 *     skipped unless px > -1 && px < W && py > -1 && py < H (false for NaN; tested before any float-to-int
 *       conversion, so +-inf and 1e30 are skipped too): a skipped source contributes nothing;
 *     x0 = floorf(px), fx = px - x0 in fp64 (exact), the same in y; the four taps (x0 + dx, y0 + dy), dx, dy in {0, 1},
 *       have the weights w = ax[dx] * ay[dy] with ax = (1 - fx, fx), ay = (1 - fy, fy), also in fp64; a tap outside
 *       the frame is dropped on its own;
 *     N_c(t) = sum of w * m * frame[b,c,s] and D(t) = sum of w * m over every source and tap that meets target t.
 *   A target that nothing reaches has out = 0 and weight = 0 exactly; d_weight = D marks the holes (for SOFT, D is
 *   relative to the image's largest weight, which is 1: the shift by M_b keeps expf from overflowing, counts as a
 *   constant in the gradient, and makes EPS act relative to the image's largest weight -- the paper's form is unshifted).
 *   Sums are 64-bit fixed point: per image, with F = max |frame[b]| and Mx = max |metric[b]| (LINEAR; 1 otherwise), the
 *   exponents are eF = frexp exponent of F (F < 2^eF; 0 for F = 0), eM likewise of Mx, eN = eF + eM, eD = eM; every
 *   contribution is formed in fp64 ((w * m) * frame), multiplied by 2^(K - eN) (N) or 2^(K - eD) (D), rounded to the
 *   nearest integer (ties to even) and added with a 64-bit integer atomic; K = oflow_splat_frac_bits(H, W) =
 *   62 - ceil(log2(4 * H * W)) fractional bits (60 for one pixel, OFLOW_SPLAT_MIN_FRAC_BITS = 38 at the largest frame).
 *   Integer addition is associative: the same bits on every run, and an image's bits do not depend on the rest of the
 *   batch (its scale is its own). Overflow is impossible: a target receives at most 4 * H * W contributions, each at
 *   most 2^K in magnitude after scaling, so |sum| <= 4 * H * W * 2^K <= 2^62 < 2^63 (H * W <= OFLOW_SPLAT_MAX_PIXELS
 *   = 2^22). The finish pass converts each sum to fp64, multiplies by the quantum 2^(eN - K) / 2^(eD - K), divides
 *   in fp64 and rounds once to fp32. A non-finite frame or metric value makes that image's outputs unspecified (no
 *   address depends on it; other images are unaffected).
 *   d_workspace: oflow_splat_workspace_bytes(B, C, H, W) bytes, 8-byte aligned (else OFLOW_E_ALIGN): the planar int64
 *   accumulators (B, C + 1, H, W) and 4 words per image (range maxima and the two exponents). The library zeroes it
 *   on the stream; the caller initialises nothing. Every element of both outputs is written.
 *   NULL d_frame / d_flow / d_out / d_weight / d_workspace: OFLOW_E_NULL. B, C, H or W < 1, B > 65535 or H * W >
 *   2^22: OFLOW_E_SHAPE (oflow_splat_workspace_bytes and oflow_splat_frac_bits return 0 for these). mode outside
 *   0..3: OFLOW_E_MODE.
 * oflow_splat_backward_f32: the gradients of a scalar loss with d_grad_out = dL/dout (B, C, H, W); d_out and d_weight
 *   are the forward's outputs (not read for SUM). A pure gather, no atomics, every element of a requested output written
 *   exactly once: bit-identical from run to run, and each output has the same bits whichever others are asked for.
 *   With r_t = 1 / (D(t) + EPS) and gd_t = -r_t * sum_c g_c(t) * out_c(t) (SUM: r = 1, gd = 0), per source s and its
 *   taps t (dropped taps contribute nothing, a skipped source gets zeros):
 *     G_c = sum_t w_t r_t g_c(t);  GD = sum_t w_t gd_t;  grad_frame[c] = m * G_c;  g_m = sum_c frame_c G_c + GD;
 *     grad_metric = g_m (LINEAR), m * g_m (SOFT; M_b counts as a constant);
 *     grad_flow[x] = m * sum_t (dw_t/dpx) q_t, q_t = sum_c frame_c r_t g_c(t) + gd_t, dw_t/dpx = -ay[dy] (dx = 0),
 *     +ay[dy] (dx = 1); the same in y. The floor convention fixes the one-sided derivative at integer positions, as
 *     grid_sample's backward does. fp32 arithmetic.
 *   d_grad_frame (B, C, H, W), d_grad_flow (B, 2, H, W), d_grad_metric (B, 1, H, W): a NULL output is not formed (all
 *   three NULL, or d_grad_metric given for SUM / AVG: OFLOW_E_NULL / OFLOW_E_MODE). d_workspace: the same size as the
 *   forward's (its first 8 * B * H * W bytes hold the r and gd planes), not zeroed by anyone; may be NULL for SUM.
 *   The other argument errors are the forward's.
 */
#define OFLOW_SPLAT_SUM 0
#define OFLOW_SPLAT_AVG 1
#define OFLOW_SPLAT_LINEAR 2
#define OFLOW_SPLAT_SOFT 3
#define OFLOW_SPLAT_EPS 1e-7
#define OFLOW_SPLAT_MIN_FRAC_BITS 38
#define OFLOW_SPLAT_MAX_PIXELS (1 << 22)
int oflow_splat_frac_bits(int H, int W);
long long oflow_splat_workspace_bytes(int B, int C, int H, int W);
int oflow_splat_f32(const float* d_frame, const float* d_flow, const float* d_metric, int B, int C, int H, int W,
                    int mode, float* d_out, float* d_weight, void* d_workspace, void* stream);
int oflow_splat_backward_f32(const float* d_grad_out, const float* d_frame, const float* d_flow, const float* d_metric,
                             const float* d_out, const float* d_weight, int B, int C, int H, int W, int mode,
                             float* d_grad_frame, float* d_grad_flow, float* d_grad_metric, void* d_workspace,
                             void* stream);

/*
 * Unsupervised training losses (csrc/census_loss.hip, csrc/smoothness_loss.hip): the ternary census loss over a
 * patch x patch neighbourhood and the edge-aware smoothness term of UnFlow (Meister et al., AAAI 2018) and UFlow
 * (Jonschkowski et al., ECCV 2020). The constants (0.81, 0.1, 0.01, 0.4, 0.001; callers default edge_weight to 150) are
 * the published ones, not tuned here. The reference has no such functions. All tensors contiguous, fp32 4-byte aligned
 * (else OFLOW_E_ALIGN), fp64 8-byte aligned. No atomics, fixed-order fp64 reductions, grids that depend on the shapes
 * only: both directions of both losses are bit-identical from run to run.
 * oflow_census_loss_f32: d_frame0, d_frame1 (B, C, H, W); in a training loss frame1 is the second image already warped
 *   back. d_mask (B, 1, H, W): fp32 (OFLOW_VALID_F32), bytes with non-zero = 1 (OFLOW_VALID_U8), or ignored, meaning 1
 *   (OFLOW_VALID_NONE).
 *     Grey value: g = (sum_c frame_c) * 255 / (image_range * C).
 *     r = patch / 2; interior pixels are those with r <= y < H - r and r <= x < W - r.
 *     For an interior pixel p and each of the patch^2 - 1 offsets d != 0:
 *       delta_k = g_k(p + d) - g_k(p);  t_k = delta_k / sqrt(0.81 + delta_k^2);  e = (t_0 - t_1)^2;
 *       s(p) = sum_d e / (0.1 + e).
 *     Robust term: rho(p) = (s(p) + 0.01)^0.4.
 *     M(p) = mask(p) on interior pixels and 0 elsewhere.
 *     loss = sum M rho / (sum M + 1e-6), summed over the whole batch; the reductions are fp64 in a fixed order.
 *   d_loss: 1 float; d_sum_m: 1 double (sum M, which the backward takes); d_s_map: s as (B, 1, H, W) fp32, 0 outside the
 *   interior, or NULL. If H or W is smaller than patch, or the mask is all zero, the loss is exactly 0. Non-finite frame
 *   values make the result unspecified. Arithmetic: the channel sums and the differences delta_0, delta_1 and
 *   delta_0 - delta_1 are formed in fp64 (exact for fp32 frames), scaled and rounded once to fp32; the rest is fp32
 *   with IEEE sqrt and division, and where delta_0 and delta_1 have the same sign t_0 - t_1 is formed as
 *   0.81 (delta_0 - delta_1)(delta_0 + delta_1) / ((n_0 n_1)^2 (t_0 + t_1)), n_k = sqrt(0.81 + delta_k^2): the same
 *   number without the cancellation of two saturated ternaries.
 *   d_workspace: oflow_census_loss_workspace_bytes(B, H, W) bytes (one row of 2 doubles per 64 x 8 tile), any
 *   contents. patch outside {3, 5, 7} or a mask kind outside 0..2: OFLOW_E_MODE. B, C, H or W < 1, B > 65535, H * W >
 *   2^28, image_range not a positive finite number: OFLOW_E_SHAPE (the workspace query returns 0).
 * oflow_census_loss_backward_f32: the gradients of a scalar with d_grad_loss = dL/dloss (1 float on the device). A
 *   gather, no atomics of any kind: the gradient of g_k(q) is -sum_d A_k(q, d) + sum_d A_k(q - d, d) with
 *     A_k(p, d) = c(p) * d[e / (0.1 + e)]/dt_k * dt_k/ddelta_k,
 *     c(p) = grad_loss * M(p) / (sum M + 1e-6) * 0.4 (s(p) + 0.01)^-0.6,
 *   and each channel's gradient is the grey gradient times 255 / (image_range * C). d_s_map: the forward's map, or NULL
 *   to recompute s in the kernel. d_sum_m: the forward's. d_grad_frame0 / d_grad_frame1 (B, C, H, W): a NULL output is
 *   not formed (both NULL: OFLOW_E_NULL), and the other has the same bits either way. Every element of a requested
 *   output is written, zeros where nothing contributes (all of it when H or W < patch or the mask is all zero): callers
 *   need no memset. The mask gets no gradient. An image's gradient bits depend on the rest of the batch only through
 *   the scalar grad_loss / (sum M + 1e-6). The other argument errors are the forward's.
 * oflow_smoothness_loss_f32: d_flow (B, 2, H, W) in pixel units, d_image (B, C, H, W).
 *     Order 1: Dx f = f(x+1) - f(x);  wx = exp(-(edge_weight / image_range) * mean_c |I_c(x+1) - I_c(x)|);
 *       Lx = mean over (B, 2, H, W-1) of wx * sqrt((Dx f)^2 + 0.001^2); Ly is the mirror image in y;
 *       loss = (Lx + Ly) / 2.
 *     Order 2: Dxx f = f(x+2) - 2 f(x+1) + f(x); wx is formed from I(x+2) - I(x); the mean is over (B, 2, H, W-2).
 *     A direction whose domain is empty contributes 0.
 *   The flow stencil is formed in fp64 (exact for fp32 flows) and rounded once; the rest is fp32 with expf.
 *   d_loss: 1 float. d_workspace: oflow_smoothness_loss_workspace_bytes(B, H, W) bytes (one row of 2 doubles per 256
 *   pixels), any contents. order outside {1, 2}: OFLOW_E_MODE; sizes as the census loss; edge_weight must be finite.
 * oflow_smoothness_loss_backward_f32: d_grad_flow (B, 2, H, W), every element written; a flow pixel gathers from the 2
 *   (order 1) or 3 (order 2) differences it takes part in, in each direction. The image is data and gets no gradient.
 */
long long oflow_census_loss_workspace_bytes(int B, int H, int W);
int oflow_census_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B,
                          int C, int H, int W, int patch, float image_range, float* d_s_map, double* d_workspace,
                          float* d_loss, double* d_sum_m, void* stream);
int oflow_census_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                   const void* d_mask, int mask_kind, const float* d_s_map, const double* d_sum_m,
                                   int B, int C, int H, int W, int patch, float image_range, float* d_grad_frame0,
                                   float* d_grad_frame1, void* stream);
long long oflow_smoothness_loss_workspace_bytes(int B, int H, int W);
int oflow_smoothness_loss_f32(const float* d_flow, const float* d_image, int B, int C, int H, int W, int order,
                              float edge_weight, float image_range, double* d_workspace, float* d_loss, void* stream);
int oflow_smoothness_loss_backward_f32(const float* d_grad_loss, const float* d_flow, const float* d_image, int B,
                                       int C, int H, int W, int order, float edge_weight, float image_range,
                                       float* d_grad_flow, void* stream);

/*
 * Photometric losses (csrc/photometric_loss.hip): SSIM and Charbonnier (robust L1), the terms the unsupervised methods
 * use beside or instead of the census loss (UnFlow and UFlow ablate between the three; ARFlow's default is
 * L1 + SSIM + ternary). The reference has no such functions. Frames d_frame0, d_frame1 (B, C, H, W); in a training loss
 * frame1 is the second image already warped back. d_mask (B, 1, H, W) and mask_kind as for the census loss. All tensors
 * contiguous, fp32 4-byte aligned (else OFLOW_E_ALIGN), fp64 8-byte aligned. No atomics, fixed-order fp64 reductions,
 * grids that depend on the shapes only: both directions of both losses are bit-identical from run to run.
 * oflow_ssim_loss_f32: window in {3, 5, 7, 9, 11}, r = window / 2. weights: window floats in HOST memory, the 1-D
 *   weights w[i] of the separable window w(dy, dx) = w[dy] w[dx] (the product of the two fp32 values as a real number).
 *   Callers normalise a box (1 / window) or a Gaussian (exp(-(i - r)^2 / (2 sigma^2))) in float64 and round to fp32;
 *   the fp32 values are the contract's weights, so S = (sum_i w[i])^2 is 1 only to rounding, and k = 1 - S.
 *   c1 = (k1 image_range)^2 and c2 = (k2 image_range)^2, likewise formed in float64 and rounded to fp32 by the caller;
 *   the frames are used as they are (no division of the input).
 *     Interior pixels: r <= y < H - r and r <= x < W - r (a "valid" filter, as the census loss).
 *     For an interior pixel p and channel c, sums over the window offsets d:
 *       mu_x = sum w(d) x(p + d),  mu_y likewise;
 *       v_x = sum w(d) (x(p + d) - mu_x)^2,  v_y likewise;  c_xy = sum w(d) (x(p + d) - mu_x)(y(p + d) - mu_y);
 *       SSIM_c = (2 mu_x mu_y + c1)(2 c_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(v_x + v_y + c2)).
 *     d(p) = mean_c (1 - SSIM_c) / 2, not clamped (with c1, c2 > 0 it lies in [0, 1] already).
 *     M(p) = mask(p) on interior pixels and 0 elsewhere.
 *     loss = sum M d / (sum M + 1e-6), summed over the whole batch; the reductions are fp64 in a fixed order.
 *   Arithmetic: 1 - SSIM from the quotient above loses everything on near-identical frames, so it is formed as
 *       A1 = 2 mu_x mu_y + c1,  B2 = v_x + v_y + c2,  dm = mu_x - mu_y = sum w(d) e(p + d),  e = x - y,
 *       v_d = sum w(d) (e(p + d) - dm)^2  (= v_x + v_y - 2 c_xy),
 *       1 - SSIM_c = (A1 v_d + dm^2 B2) / ((A1 + dm^2) B2),
 *   every term non-negative on non-negative frames; e is formed in fp64 (exact for fp32 frames) and rounded once, the
 *   rest is fp32 with IEEE division. The window sums run row by row (columns first) with fused multiply-adds over the
 *   values less the centre pixel's, so that a flat neighbourhood keeps its small deviations: for t in (x, y, e)
 *       o_t = sum w(d) (t(p + d) - t(p)) - k t(p)  (= mu_t - t(p)),  mu_t = t(p) + o_t,
 *       v_t = sum w(d) ((t(p + d) - t(p)) - o_t)^2.
 *   d_loss: 1 float; d_sum_m: 1 double (sum M, which the backward takes); d_ssim_map: mean_c SSIM_c = 1 - (sum_c (1 -
 *   SSIM_c)) / C as (B, 1, H, W) fp32, 0 outside the interior, or NULL. If H or W is smaller than window, or the mask is
 *   all zero, the loss is exactly 0; on identical non-negative frames it is exactly 0 too. Non-finite frame values
 *   make the result unspecified. d_workspace: oflow_ssim_loss_workspace_bytes(B, H, W) bytes (one row of 2 doubles per
 *   64 x 8 tile), any contents. A window outside the set or a mask kind outside 0..2: OFLOW_E_MODE. B, C, H or W < 1,
 *   B > 65535, H * W > 2^28, c1 or c2 not a positive finite number, a non-finite weight: OFLOW_E_SHAPE (the workspace
 *   query returns 0). NULL frames, weights, workspace or outputs (the map excepted): OFLOW_E_NULL. Nothing is launched
 *   on an error.
 * oflow_ssim_loss_backward_f32: the gradients of a scalar with d_grad_loss = dL/dloss (1 float on the device), from the
 *   cancellation-free form as well. With F = 1 - SSIM_c of pixel p, l = A1 / T, T = A1 + dm^2, csl = v_d / B2,
 *   cs = 1 - csl:
 *       dF/dmu_x = Fx = 2 cs dm (mu_y (mu_x + mu_y) + c1) / T^2,   dF/dmu_y = Fy = -2 cs dm (mu_x (mu_x + mu_y) + c1) / T^2,
 *       dF/dv_x = dF/dv_y = l cs / B2,   dF/dc_xy = -2 l / B2 = -G,
 *       dmu_x/dx(q) = w(d),  dv_x/dx(q) = 2 w(d) (x(q) - mu_x - k mu_x),  dc_xy/dx(q) = w(d) (y(q) - mu_y - k mu_y),
 *   d = q - p, with G = 2 l / B2, so that
 *       dF(p)/dx(q) = w(q - p) (Fx' + G (cs (x(q) - mu_x) - (y(q) - mu_y))),   Fx' = Fx - k G (dm - csl mu_x),
 *       dF(p)/dy(q) = w(q - p) (Fy' + G (cs (y(q) - mu_y) - (x(q) - mu_x))),   Fy' = Fy + k G (dm + csl mu_y).
 *   cs (x - mu_x) - (y - mu_y) = (e(q) - dm) - csl (x(q) - mu_x): the kernel takes the left side, with
 *   cs = (2 c_xy + c2) / B2, where v_d > B2 / 2 (dissimilar frames, cs near 0) and the right side, with cs = 1 - csl,
 *   elsewhere (similar frames, where x - mu_x and y - mu_y nearly cancel); and it takes every t(q) - mu_t as
 *   (t(q) - t(p)) - o_t, the o_t above. In either case
 *       dF(p)/dx(q) = w(q - p) (Px(p) + al(p) (x(q) - x(p)) + be(p) (y(q) - y(p)) + ga(p) (e(q) - e(p))),
 *       dF(p)/dy(q) = w(q - p) (Py(p) + al(p) (y(q) - y(p)) + be(p) (x(q) - x(p)) - ga(p) (e(q) - e(p))),
 *   (al, be, ga) = (G cs, -G, 0) or (-G csl, 0, G), Px = Fx' - (al o_x + be o_y + ga o_e), Py = Fy' - (al o_y + be o_x -
 *   ga o_e), and the gradient of x_c(q) is the window-weighted gather of these per-pixel coefficient planes over the
 *   pixels p whose window holds q, each scaled by g(p) = grad_loss * M(p) / (sum M + 1e-6) / (2 C). The statistics
 *   are recomputed from the frames. d_grad_frame0 / d_grad_frame1 (B, C, H, W): a NULL output is not formed (both
 *   NULL: OFLOW_E_NULL), and the other has the same bits either way. Every element of a requested output is written,
 *   zeros where nothing contributes (all of it when H or W < window or the mask is all zero): callers need no memset.
 *   The mask gets no gradient. The other argument errors are the forward's.
 * oflow_charbonnier_loss_f32: on every pixel (no interior),
 *     rho(p) = mean_c (((x - y) / image_range)^2 + eps^2)^alpha,  loss = sum mask rho / (sum mask + 1e-6).
 *   x - y is formed in fp64 and rounded once; the rest is fp32 with IEEE division, sqrtf when alpha is 0.5 and powf
 *   otherwise. eps, alpha and image_range are the fp32 values passed. d_workspace: oflow_ssim_loss_workspace_bytes(B, H,
 *   W) bytes are enough (one row of 2 doubles per 1024 pixels, never more than one per tile). eps not positive and
 *   finite, alpha outside (0, 1], image_range not positive and finite: OFLOW_E_SHAPE; the rest as the SSIM loss.
 * oflow_charbonnier_loss_backward_f32: elementwise, with z = (x - y) / image_range and q = z^2 + eps^2,
 *     dL/dx_c(p) = grad_loss * mask(p) / (sum mask + 1e-6) * (2 alpha / (C image_range)) * z * q^(alpha - 1)
 *   and dL/dy_c(p) its negative. Outputs as for the SSIM backward.
 */
long long oflow_ssim_loss_workspace_bytes(int B, int H, int W);
int oflow_ssim_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B, int C,
                        int H, int W, int window, const float* weights, float c1, float c2, float* d_ssim_map,
                        double* d_workspace, float* d_loss, double* d_sum_m, void* stream);
int oflow_ssim_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                 const void* d_mask, int mask_kind, const double* d_sum_m, int B, int C, int H, int W,
                                 int window, const float* weights, float c1, float c2, float* d_grad_frame0,
                                 float* d_grad_frame1, void* stream);
int oflow_charbonnier_loss_f32(const float* d_frame0, const float* d_frame1, const void* d_mask, int mask_kind, int B,
                               int C, int H, int W, float eps, float alpha, float image_range, double* d_workspace,
                               float* d_loss, double* d_sum_m, void* stream);
int oflow_charbonnier_loss_backward_f32(const float* d_grad_loss, const float* d_frame0, const float* d_frame1,
                                        const void* d_mask, int mask_kind, const double* d_sum_m, int B, int C, int H,
                                        int W, float eps, float alpha, float image_range, float* d_grad_frame0,
                                        float* d_grad_frame1, void* stream);

/*
 * Training-batch augmentation (csrc/augment.hip): the reference's FlowAugmentor / SparseFlowAugmentor
 * (methods/raft/data/augmentor.py) for a batch of B samples of one source size, on the device. The random decisions are
 * made on the host (data.augmentor.*.sample) and arrive as d_params, a (B, OFLOW_AUG_PARAM_DOUBLES) float64 array; row:
 *    [0]      asymmetric (0 / 1)
 *    [1..8]   frame 1: the op order (4 entries, 0 brightness, 1 contrast, 2 saturation, 3 hue: torchvision's fn_idx),
 *             then the brightness, contrast, saturation and hue factors
 *    [9..16]  frame 2, the same (a symmetric draw repeats frame 1's)
 *    [17]     number of eraser rectangles (0..2);  [18..25] two rectangles (x0, y0, dx, dy) in source pixels
 *    [26]     do_resize;  [27] scale_x;  [28] scale_y;  [29] hflip;  [30] vflip;  [31] crop y0;  [32] crop x0
 *    [33..]   reserved, zero
 * d_img1, d_img2: (B, H, W, 3) uint8, HWC. d_flow: (B, 2, H, W) fp32. d_stats: (B, OFLOW_AUG_STATS_WORDS) int64, ZEROED
 * by the caller before stage 0: [0], [1] the grey sums of frame 1 / 2 in front of the contrast op, [2..4] the R, G, B
 * sums of the jittered frame 2. Outputs: (B, 3, crop_h, crop_w), (B, 2, crop_h, crop_w), (B, crop_h, crop_w) fp32.
 *
 * Arithmetic (the contract; tests/augment_cases.py restates it in NumPy and the kernels equal it bit for bit):
 *   colour jitter as Pillow computes it -- L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; blend(d, x, f) =
 *   (float)d + f * ((float)x - (float)d) in fp32 (one product, one sum, no FMA), truncated for 0 <= f <= 1, else clamped
 *   to [0, 255] and truncated; brightness d = 0, saturation d = L of the pixel, contrast d = int(mean(L) + 0.5) with the
 *   mean the exact integer sum over the image as it stands at contrast's turn, divided in float64, over BOTH frames for
 *   a symmetric draw (the reference jitters them stacked) and per frame for an asymmetric one; hue through Pillow's
 *   RGB -> HSV -> RGB with H += trunc(hue * 255) mod 256, also for hue 0. The eraser fills its rectangles (clipped at
 *   the frame edge) of frame 2 with trunc(channel sum / (H*W)) of the jittered frame 2. Resize follows OpenCV's
 *   documented INTER_LINEAR mapping: size round_half_even(n * s); f = fp32((d + 0.5) * (1 / s) - 0.5) (float64, rounded
 *   once), i = floor(f), a = f - i, i < 0 -> (0, 0), i >= n - 1 -> (n - 1, 0); S0 * (1 - a) + S1 * a in fp32 (two
 *   products, one sum), horizontally then vertically; image levels are then rounded half-even and clamped (OpenCV's own
 *   8-bit path blends in fixed point: agreement with it is not measured); the flow is then multiplied by
 *   (scale_x, scale_y) and the flips' signs in float64 and rounded once. Flips, then the crop at (y0, x0).
 *   Dense valid = (|u| < 1000) & (|v| < 1000) of the output flow.
 *   Sparse flow / valid under resize (resize_sparse_flow_map): source (x, y) with valid >= 1 lands at xx =
 *   round_half_even((double)(float)x * scale_x), yy likewise, kept iff 0 < xx < wd1 and 0 < yy < ht1, value
 *   fp32((double)flow * scale); of several sources on one pixel the LAST in row-major source order stays; unreached
 *   pixels are 0 / 0. Without resize flow and valid pass through. The sparse class flips only horizontally.
 * oflow_augment_stats_u8: stage 0 accumulates [0], [1]; stage 1 (after stage 0 on the same stream) accumulates [2..4]
 *   for the samples that erase. 64-bit integer atomics: exact, the same bits on every run.
 * oflow_augment_dense_f32: images, and with d_flow != NULL the dense flow and valid (NULL: images only, d_out_flow and
 *   d_out_valid are not touched). Needs both stats stages. One thread per output pixel; only the crop's taps are read.
 * oflow_augment_sparse_flow_f32: the sparse flow and valid (d_valid: (B, H, W) fp32), a gather without atomics.
 * The kernels clamp every source index into the frame, but a crop outside the resized frame, a scale <= 0 or an op
 * order that is no permutation gives meaningless values: callers validate the rows first (data.augmentor does).
 * B <= 65535, H*W <= 2^28, crop_h*crop_w <= 2^28; stage 0 or 1. OFLOW_E_NULL / OFLOW_E_SHAPE before any launch.
 */
#define OFLOW_AUG_PARAM_DOUBLES 36
#define OFLOW_AUG_STATS_WORDS 8
int oflow_augment_stats_u8(const unsigned char* d_img1, const unsigned char* d_img2, const double* d_params, int B,
                           int H, int W, int stage, long long* d_stats, void* stream);
int oflow_augment_dense_f32(const unsigned char* d_img1, const unsigned char* d_img2, const float* d_flow,
                            const double* d_params, const long long* d_stats, int B, int H, int W, int crop_h,
                            int crop_w, float* d_out1, float* d_out2, float* d_out_flow, float* d_out_valid,
                            void* stream);
int oflow_augment_sparse_flow_f32(const float* d_flow, const float* d_valid, const double* d_params, int B, int H,
                                  int W, int crop_h, int crop_w, float* d_out_flow, float* d_out_valid, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OFLOW_H_ */
