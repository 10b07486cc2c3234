"""``torch.ops.oflow``: the correlation / warp path as PyTorch operators (csrc/torch_ops.cpp -> liboflow_torch.so).

The library registers, per op, a HIP-key kernel that calls the C ABI of liboflow_hip.so on PyTorch's current stream
and a Meta kernel (output shapes only, what torch.compile's fake-tensor tracing runs). This module loads it and
registers the autograd formulas on top, so ``CorrBlock`` and ``optical_flow.warp`` are ordinary traceable ops:
``torch.compile(fullgraph=True)`` captures them without graph breaks, and training differentiates through them.

Autograd:
  * ``corr_pyramid``: the level gradients go back through the floor 2x2 pools (native kernel) and two batched GEMMs
    (``corr_pyramid_backward``, fp32 MFMA): grad_f1 = f2 . G^T / sqrt(C), grad_f2 = f1 . G / sqrt(C).
  * ``corr_lookup``: the native transpose of the bilinear window gather (``corr_lookup_backward``); coords get no
    gradient -- the reference detaches them before every lookup (methods/raft/model/raft.py:127).
  * ``grid_warp`` / ``grid_sample``: the native transpose (``grid_warp_backward`` / ``grid_sample_backward``,
    csrc/warp_backward.hip: ATen grid_sampler_2d_backward's formulas, tap gradients added with fp32 atomics); the
    warp's base grid is constant, so the flow gradient is the grid gradient.
  * ``sequence_loss``: one native pass writes the gradient of every prediction that needs one
    (``sequence_loss_backward``, csrc/flow_metrics.hip); flow_gt and valid get none, and the statistics output is not
    differentiable. ``register_autograd`` handles the ``Tensor[]`` argument (a list of per-prediction gradients, None
    where ``needs_input_grad`` is False).
  * ``convex_upsample`` (RAFT.upsample_flow): the native transpose (``convex_upsample_backward``,
    csrc/upsample_backward.hip): one streaming pass recomputes the softmax from the saved flow and mask, writes the mask
    gradient as whole rows and stages the tap sums of the flow gradient, which a small second kernel gathers in a fixed
    order (no atomics, deterministic); only the wanted gradients are formed.
  * ``corr_lookup_alt`` (AlternateCorrBlock under autograd): ``corr_lookup_otf``'s forward on the fp16 features, with
    the fp32 feature maps they were prepared from as the tracked arguments. The fp16 roundings count as identity; the
    native transpose (``corr_lookup_alt_backward``, csrc/corr_otf_backward.hip) evaluates the derivative at the stored
    fp16 values with the gradients kept in fp32 (fp32 MFMA). Only f1h, f2h and coords are saved: nothing that scales with
    (HW)^2 exists in either direction. grad_fmap1 is written in a fixed order (bit-reproducible); grad_fmap2 sums
    overlapping windows with fp32 atomics (last bits vary from run to run). coords get no gradient.
  * ``conv2d_same`` (the update block's ``nn.Conv2d`` layers with ``RAFT.conv_backward_impl = "native"``): the forward
    is ATen's convolution with the module's own arguments (stride 1, zero padding (kh // 2, kw // 2): the same bits);
    the backward (``conv2d_same_backward``, csrc/conv_backward.hip) forms the input gradient as a gather-form GEMM and
    the weight / bias gradients as pixel-slab partial sums added in a fixed order, all on the fp32 matrix cores: no
    atomics, no MIOpen find step or workspace, bit-reproducible. Only the gradients ``needs_input_grad`` asks for are
    formed (convf1's input, the detached flow, gets none).
  * ``conv2d_strided`` (the encoders' ``nn.Conv2d`` layers with ``RAFT.encoder_backward_impl = "native"``): as
    ``conv2d_same`` with stride 1 or 2 (``conv2d_strided_backward``: at stride 2 the input gradient is tiled by the
    input pixels' parity class, so no matrix-core step is spent on a tap a pixel never meets; with Cin <= 4, the stem,
    the weight gradient folds (channel, tap) into one tile dimension). The stem's input, the images, gets no gradient.
  * ``instance_norm_act`` / ``frozen_batch_norm_act`` (the encoders' norm layers with the ReLU that follows them): the
    forward is the module's own ATen call plus ``relu``; only ``x`` (and the batch norm's parameters and running
    statistics) are saved, and the backward (csrc/norm_backward.hip) recomputes the statistics and the ReLU mask from
    it, one workgroup per plane, fixed-order sums in fp64: no atomics, bit-reproducible.
  * ``batch_norm_act`` (cnet's ``BatchNorm2d`` layers on batch statistics, with the ReLU that follows them, under
    ``RAFT.batch_norm_impl = "native"``): forward and backward are both native (csrc/batch_norm.hip), because ATen's
    batch-statistics forward cannot be reproduced bit for bit. It returns (y, mean, biased var); x, the parameters and
    the two statistics are saved, mean and var are not differentiable, and the backward (``batch_norm_act_backward``)
    takes the statistics as saved and recomputes the ReLU mask with the forward's arithmetic. One workgroup per
    (plane, chunk), fp64 partials added in a fixed order: no atomics, bit-reproducible. The op is functional: the
    module's running statistics are updated by the caller (``model.extractor.enc_norm_act``).
The tiled / NHWC lookups and the raw fp16 on-the-fly ops (``corr_otf_prepare`` / ``corr_lookup_otf``) are the inference
layouts and have no autograd formula; ``flow_error_stats`` (the metrics' accumulating reduction) has none either, nor
has ``forward_interpolate`` (the warm-start initialiser, csrc/forward_interpolate.hip: a nearest-landed-source selection
in float64, piecewise constant in its input; callers detach the input, ``model.utils.forward_interpolate``), nor has
``augment_batch`` (the training-batch augmentation, csrc/augment.hip: integer image levels and a resampled ground truth),
nor has ``fb_consistency`` (the forward-backward occlusion masks, csrc/fb_consistency.hip): a mask is piecewise constant
in the flows and has no gradient, and the residual is returned for inspection and thresholding, not for a loss, so
``optical_flow.fb_consistency`` detaches its inputs.
  * ``splat`` (``optical_flow.splat``, forward warping): the forward (csrc/splat.hip) scatters 64-bit fixed-point
    contributions with integer atomics and returns (out, weight); frame, flow, the metric, out and weight are saved, the
    weight is not differentiable, and the backward (``splat_backward``, csrc/splat_backward.hip) is a pure gather over
    each source's four taps: no float atomics in either direction, bit-reproducible. Only the gradients
    ``needs_input_grad`` asks for are formed; the softmax mode's shift by the image's metric maximum counts as a
    constant. ``splat`` and ``splat_backward`` are listed in ``OPS_SPLAT``, not in ``OPS``.
  * ``census_loss`` / ``smoothness_loss`` (``optical_flow.losses``, the unsupervised training losses): the census
    forward (csrc/census_loss.hip) returns (loss, sum M, s map); the frames, the mask and the last two are saved, sum M
    and the map are not differentiable, and the backward (``census_loss_backward``) is a tiled gather that takes s from
    the saved map instead of recomputing it. Only the frame gradients ``needs_input_grad`` asks for are formed; the mask
    gets none. ``smoothness_loss`` saves the flow and the image; its backward (``smoothness_loss_backward``,
    csrc/smoothness_loss.hip) gathers each flow pixel's two or three differences per direction, and the image, which
    is data, gets none. No atomics and fixed-order fp64 sums in both directions: bit-reproducible. The four ops are
    listed in ``OPS_LOSSES``, not in ``OPS`` or ``OPS_SPLAT``.
  * ``ssim_loss`` / ``charbonnier_loss`` (``optical_flow.losses``, the other photometric terms): the forwards
    (csrc/photometric_loss.hip) return (loss, sum M[, mean_c SSIM map]); the frames, the mask and sum M are saved, sum M
    and the map are not differentiable, and the backwards (``ssim_loss_backward``, a tiled gather that recomputes the
    window statistics from the frames; ``charbonnier_loss_backward``, elementwise) form only the frame gradients
    ``needs_input_grad`` asks for; the mask gets none. No atomics and fixed-order fp64 sums: bit-reproducible. The four
    ops are listed in ``OPS_PHOTOMETRIC``.
"""
from __future__ import annotations

import os

import torch

_OPS_PATH = os.environ.get(
    "OFLOW_OPS_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "liboflow_torch.so")
)
OPS = (
    "corr_pyramid",
    "corr_pyramid_tiled",
    "corr_lookup",
    "corr_lookup_tiled",
    "corr_lookup_tiled_nhwc",
    "corr_otf_prepare",
    "corr_lookup_otf",
    "grid_warp",
    "grid_sample",
    "corr_lookup_backward",
    "corr_pyramid_backward",
    "grid_warp_backward",
    "grid_sample_backward",
    "flow_error_stats",
    "sequence_loss",
    "sequence_loss_backward",
    "convex_upsample",
    "convex_upsample_backward",
    "corr_lookup_alt",
    "corr_lookup_alt_backward",
    "forward_interpolate",
    "augment_batch",
    "conv2d_same",
    "conv2d_same_backward",
    "conv2d_strided",
    "conv2d_strided_backward",
    "instance_norm_act",
    "instance_norm_act_backward",
    "frozen_batch_norm_act",
    "frozen_batch_norm_act_backward",
    "batch_norm_act",
    "batch_norm_act_backward",
    "fb_consistency",
)
# the forward-warping ops, kept apart from OPS (tests/golden/op_schemas.txt records that tuple as it stood); their
# schemas are recorded in tests/golden/op_schemas_splat.txt
OPS_SPLAT = (
    "splat",
    "splat_backward",
)
# the unsupervised training losses, kept apart likewise; their schemas are recorded in
# tests/golden/op_schemas_losses.txt
OPS_LOSSES = (
    "census_loss",
    "census_loss_backward",
    "smoothness_loss",
    "smoothness_loss_backward",
)
# the SSIM and Charbonnier losses, kept apart likewise (tests/test_losses_host.py records OPS_LOSSES as it stood); their
# schemas are recorded in tests/golden/op_schemas_photometric.txt
OPS_PHOTOMETRIC = (
    "ssim_loss",
    "ssim_loss_backward",
    "charbonnier_loss",
    "charbonnier_loss_backward",
)
_loaded = False


def library_path() -> str:
    return _OPS_PATH


def load() -> None:
    """Load liboflow_torch.so once and register the autograd formulas. Raises RuntimeError if it is missing."""
    global _loaded
    if _loaded:
        return
    if not os.path.exists(_OPS_PATH):
        raise RuntimeError(
            f"liboflow_torch.so not found at {_OPS_PATH}: build it with `make -C torch-optical-flow_amd/csrc` "
            "(or __graft_entry__.build()); the MI355X path has no CPU fallback"
        )
    torch.ops.load_library(_OPS_PATH)
    _register_autograd()
    _loaded = True


# ---------------------------------------------------------------------------------------------- autograd formulas
def _pyramid_setup(ctx, inputs, output):
    fmap1, fmap2, _ = inputs
    ctx.save_for_backward(fmap1, fmap2)
    ctx.shapes = [tuple(t.shape) for t in output]


def _pyramid_backward(ctx, grads):
    fmap1, fmap2 = ctx.saved_tensors
    levels = [
        g.contiguous() if g is not None else torch.zeros(sh, device=fmap1.device, dtype=torch.float32)
        for g, sh in zip(grads, ctx.shapes)
    ]
    g1, g2 = torch.ops.oflow.corr_pyramid_backward(levels, fmap1, fmap2)
    return g1, g2, None


def _lookup_setup(ctx, inputs, output):
    levels, coords, radius = inputs
    # the native transpose rebuilds every level's size from level 0 by floor 2x2 pooling (corr.py:53): levels of any
    # other size are refused here, in the forward, instead of failing with a gradient-shape error in the backward
    h, w = (int(v) for v in levels[0].shape[-2:])
    for lv in levels:
        if tuple(int(v) for v in lv.shape[-2:]) != (h, w):
            raise RuntimeError(
                f"corr_lookup backward: level sizes must be the floor 2x2 pools of level 0 (expected {(h, w)}, got "
                f"{tuple(lv.shape[-2:])})")
        h, w = h // 2, w // 2
    ctx.save_for_backward(coords)
    ctx.radius = radius
    ctx.level0 = tuple(levels[0].shape[-2:])
    ctx.nl = len(levels)


def _lookup_backward(ctx, grad_out):
    (coords,) = ctx.saved_tensors
    h0, w0 = ctx.level0
    grads = torch.ops.oflow.corr_lookup_backward(grad_out.contiguous(), coords, ctx.radius, h0, w0, ctx.nl)
    return list(grads), None, None


def _sampler_formula(backward_op):
    """(setup_context, backward) of ``grid_warp`` (frame, flow) and ``grid_sample`` (input, grid): the same formula over
    (source, field, mode, padding_mode, align_corners), with the op's own native transpose."""

    def setup(ctx, inputs, output):
        src, field, mode, pad, ac = inputs
        ctx.save_for_backward(src, field)
        ctx.args = (mode, pad, ac)

    def backward(ctx, grad_out):
        src, field = ctx.saved_tensors
        # the native transpose (warp_backward.hip): a warp's grid = linspace base + flow, so its flow gradient is the
        # grid gradient. Only the wanted outputs are formed (no zero fill / atomics for a source that needs no gradient)
        need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
        g_src, g_field = backward_op(grad_out.contiguous(), src, field, *ctx.args, need)
        return (g_src.to(src.dtype) if need[0] else None), (g_field.to(field.dtype) if need[1] else None), None, None, None

    return setup, backward


def _seqloss_setup(ctx, inputs, output):
    preds, flow_gt, valid, weights, max_flow = inputs
    ctx.save_for_backward(flow_gt, valid, *preds)
    ctx.args = (list(weights), max_flow)
    ctx.mark_non_differentiable(output[1])


def _seqloss_backward(ctx, grad_loss, _grad_stats):
    flow_gt, valid, *preds = ctx.saved_tensors
    weights, max_flow = ctx.args
    need = [bool(n) for n in ctx.needs_input_grad[0]]
    grads = torch.ops.oflow.sequence_loss_backward(grad_loss, preds, flow_gt, valid, weights, max_flow,
                                                   [int(n) for n in need])
    return [g.to(p.dtype) if n else None for g, p, n in zip(grads, preds, need)], None, None, None, None


def _upsample_setup(ctx, inputs, output):
    flow, mask = inputs
    ctx.save_for_backward(flow, mask)  # the softmax is recomputed in the backward: nothing else is kept


def _upsample_backward(ctx, grad_out):
    flow, mask = ctx.saved_tensors
    need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
    g_flow, g_mask = torch.ops.oflow.convex_upsample_backward(grad_out.contiguous(), flow, mask, need)
    return (g_flow.to(flow.dtype) if need[0] else None), (g_mask.to(mask.dtype) if need[1] else None)


def _param_layer_formula(backward_op, n_saved, n_plain, saves_statistics=False):
    """(setup_context, backward) of the layers with an (x, weight, bias) gradient: ``conv2d_same`` / ``conv2d_strided``
    and ``frozen_batch_norm_act`` / ``batch_norm_act``. Their inputs are (x, weight, bias, further tensors..., then
    ``n_plain`` non-tensor arguments) and their backward op takes (grad_out, saved tensors..., non-tensor arguments...,
    output_mask) -> (grad_x, grad_weight, grad_bias).

    ``n_saved``: how many leading inputs are saved: 2 for the convolutions (x and weight; of the bias only whether there
    is one), all the tensors for the norms. ``saves_statistics``: the outputs after the first (``batch_norm_act``'s mean
    and var, as the forward returned them: C floats each) are saved too and are not differentiable."""

    def setup(ctx, inputs, output):
        saved = tuple(inputs[:n_saved])
        if saves_statistics:
            saved += tuple(output[1:])
            ctx.mark_non_differentiable(*output[1:])
        ctx.save_for_backward(*saved)
        ctx.has_bias = inputs[2] is not None
        ctx.plain = tuple(inputs[len(inputs) - n_plain:])
        ctx.n_inputs = len(inputs)

    def backward(ctx, grad_out, *_grad_statistics):
        need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]), ctx.has_bias and bool(ctx.needs_input_grad[2])]
        # (a stride-0 expanded gradient, what .sum() hands over, becomes a real tensor here)
        grads = backward_op(grad_out.contiguous(), *ctx.saved_tensors, *ctx.plain, need)
        return tuple(g if n else None for g, n in zip(grads, need)) + (None,) * (ctx.n_inputs - 3)

    return setup, backward


def _inorm_setup(ctx, inputs, output):
    x, eps, relu = inputs
    ctx.save_for_backward(x)  # the statistics and the ReLU mask are recomputed in the backward: nothing else is kept
    ctx.args = (eps, relu)


def _inorm_backward(ctx, grad_out):
    (x,) = ctx.saved_tensors
    eps, relu = ctx.args
    return torch.ops.oflow.instance_norm_act_backward(grad_out.contiguous(), x, eps, relu), None, None


def _alt_setup(ctx, inputs, output):
    _fmap1, _fmap2, f1h, f2h, coords, radius = inputs
    ctx.save_for_backward(f1h, coords, *f2h)  # O(B*C*H*W): the fp32 fmaps are not kept, no volume exists
    ctx.radius = radius
    ctx.dtypes = (_fmap1.dtype, _fmap2.dtype)


def _alt_backward(ctx, grad_out):
    f1h, coords, *f2h = ctx.saved_tensors
    need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
    g1, g2 = torch.ops.oflow.corr_lookup_alt_backward(grad_out.contiguous(), f1h, f2h, coords, ctx.radius, need)
    d1, d2 = ctx.dtypes  # fp32 in AlternateCorrBlock: the casts are no-ops there
    # (a Tensor[] argument takes a list of its own length)
    return (g1.to(d1) if need[0] else None), (g2.to(d2) if need[1] else None), None, [None] * len(f2h), None, None


def _splat_setup(ctx, inputs, output):
    frame, flow, metric, mode = inputs
    out, weight = output
    ctx.save_for_backward(frame, flow, metric, out, weight)
    ctx.mode = mode
    ctx.mark_non_differentiable(weight)


def _splat_backward(ctx, grad_out, _grad_weight):
    frame, flow, metric, out, weight = ctx.saved_tensors
    need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]),
            metric is not None and bool(ctx.needs_input_grad[2])]
    g_frame, g_flow, g_metric = torch.ops.oflow.splat_backward(grad_out.contiguous(), frame, flow, metric, out, weight,
                                                               ctx.mode, need)
    return (g_frame.to(frame.dtype) if need[0] else None), (g_flow.to(flow.dtype) if need[1] else None), \
        (g_metric.to(metric.dtype) if need[2] else None), None


def _census_setup(ctx, inputs, output):
    frame0, frame1, mask, patch, image_range = inputs
    _loss, sum_m, s_map = output
    ctx.save_for_backward(frame0, frame1, mask, sum_m, s_map)  # s is taken from the map, not recomputed
    ctx.args = (patch, image_range)
    ctx.mark_non_differentiable(sum_m, s_map)


def _census_backward(ctx, grad_loss, _grad_sum_m, _grad_s_map):
    frame0, frame1, mask, sum_m, s_map = ctx.saved_tensors
    need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
    g0, g1 = torch.ops.oflow.census_loss_backward(grad_loss.contiguous(), frame0, frame1, mask, sum_m, s_map, *ctx.args,
                                                  need)
    return (g0.to(frame0.dtype) if need[0] else None), (g1.to(frame1.dtype) if need[1] else None), None, None, None


def _smoothness_setup(ctx, inputs, output):
    flow, image, order, edge_weight, image_range = inputs
    ctx.save_for_backward(flow, image)
    ctx.args = (order, edge_weight, image_range)


def _smoothness_backward(ctx, grad_loss):
    flow, image = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    g = torch.ops.oflow.smoothness_loss_backward(grad_loss.contiguous(), flow, image, *ctx.args)
    return g.to(flow.dtype), None, None, None, None


def _photometric_formula(backward_op, n_outputs):
    """(setup_context, backward) of ``ssim_loss`` and ``charbonnier_loss``: inputs (frame0, frame1, mask, plain
    arguments...), outputs (loss, sum M, ...), backward op (grad_loss, frame0, frame1, mask, sum M, plain arguments...,
    output_mask) -> (grad_frame0, grad_frame1). ``ssim_loss``'s last plain argument, ``with_map``, is not the
    backward's."""
    n_plain = 3

    def setup(ctx, inputs, output):
        frame0, frame1, mask = inputs[:3]
        ctx.save_for_backward(frame0, frame1, mask, output[1])
        ctx.args = tuple(inputs[3:3 + n_plain])
        ctx.n_inputs = len(inputs)
        ctx.mark_non_differentiable(*output[1:])

    def backward(ctx, grad_loss, *_grads):
        frame0, frame1, mask, sum_m = ctx.saved_tensors
        need = [bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])]
        g0, g1 = backward_op(grad_loss.contiguous(), frame0, frame1, mask, sum_m, *ctx.args, need)
        return ((g0.to(frame0.dtype) if need[0] else None), (g1.to(frame1.dtype) if need[1] else None)) + \
            (None,) * (ctx.n_inputs - 2)

    assert n_outputs in (2, 3)
    return setup, backward


def _register_autograd() -> None:
    ops = torch.ops.oflow

    def reg(name, setup, backward):
        torch.library.register_autograd(name, backward, setup_context=setup)

    reg("oflow::corr_pyramid", _pyramid_setup, _pyramid_backward)
    reg("oflow::corr_lookup", _lookup_setup, _lookup_backward)
    reg("oflow::grid_warp", *_sampler_formula(ops.grid_warp_backward))
    reg("oflow::grid_sample", *_sampler_formula(ops.grid_sample_backward))
    reg("oflow::sequence_loss", _seqloss_setup, _seqloss_backward)
    reg("oflow::convex_upsample", _upsample_setup, _upsample_backward)
    reg("oflow::corr_lookup_alt", _alt_setup, _alt_backward)
    reg("oflow::conv2d_same", *_param_layer_formula(ops.conv2d_same_backward, n_saved=2, n_plain=0))
    reg("oflow::conv2d_strided", *_param_layer_formula(ops.conv2d_strided_backward, n_saved=2, n_plain=1))
    reg("oflow::instance_norm_act", _inorm_setup, _inorm_backward)
    reg("oflow::frozen_batch_norm_act", *_param_layer_formula(ops.frozen_batch_norm_act_backward, n_saved=5, n_plain=2))
    reg("oflow::batch_norm_act",
        *_param_layer_formula(ops.batch_norm_act_backward, n_saved=3, n_plain=2, saves_statistics=True))
    reg("oflow::splat", _splat_setup, _splat_backward)
    reg("oflow::census_loss", _census_setup, _census_backward)
    reg("oflow::smoothness_loss", _smoothness_setup, _smoothness_backward)
    reg("oflow::ssim_loss", *_photometric_formula(ops.ssim_loss_backward, n_outputs=3))
    reg("oflow::charbonnier_loss", *_photometric_formula(ops.charbonnier_loss_backward, n_outputs=2))
