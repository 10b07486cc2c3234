"""RAFT inference model (reference: methods/raft/model/raft.py:21-147), MI355X-native correlation path.

Same constructor arguments, ``hparams`` attribute, sub-modules and ``state_dict`` keys as the reference's
LightningModule, so its checkpoints load unchanged. Of the training / evaluation half (`raft.py:149-260`) the metrics
(``epe_train`` / ``epe_val`` / ``f1_val``), ``training_step``, ``validation_step`` and the module-level
``sequence_loss`` are here, on the fused reductions of csrc/flow_metrics.hip and, under autograd, the native backward
kernels (correlation, convex upsampling, loss); the Lightning trainer hooks, optimizers and W&B logging stay out of scope
(SURVEY.md §2 row 7). ``forward`` keeps the reference's semantics and return
values; three output-identical changes remove host work from the loop:
  * the correlation pyramid and every lookup run on the gfx950 kernels (``model.corr.CorrBlock``);
    ``alternate_corr=True`` (an addition, default off) swaps in the volume-free fp16 ``AlternateCorrBlock``
    for large frames;
  * coordinate grids are built on the device (no CPU build + H2D copy, `raft.py:68-69`);
  * with ``test_mode=True`` only the last iteration's convex upsampling is computed — the reference computes
    all ``iters`` and returns only the last (Q11, `raft.py:136-145`);
  * without autograd on the GPU the encoders run through ``SplitEncoder`` (split-fp16 convolutions, fp64-merged
    instance-norm statistics, folded eval batch norm; ``encoder_impl = "module"`` keeps the nn.Modules) and the
    update block runs through ``SplitUpdate``: every convolution on the
    split-fp16 matrix-core kernel (fp32-level accuracy) with the GRU gates, activations, concatenations and the
    ``coords1 += delta_flow`` update fused into convolution epilogues (``update_impl = "fused"`` selects the
    MIOpen-based ``FusedUpdate`` instead); in test mode the mask head (two convolutions feeding only the
    upsampling) runs at the last iteration only.
``forward_bidirectional`` (an addition) gives the flows of both directions from one forward, the stacked forward
``self(cat([image0, image1]), cat([image1, image0]))`` with the feature encoder run once per image; both entry points
share the encoder stage (``_encode``).
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from optical_flow import _native
from optical_flow.metrics import AverageEndPointError, OutlierRatio

from .corr import AlternateCorrBlock, CorrBlock
from .extractor import BasicEncoder, SplitEncoder
from .update import BasicUpdateBlock, FusedUpdate, SplitUpdate, _side_stream, capture_active
from .utils import InputPadder, coords_grid, upflow8

# RAFT.forward's input scaling (raft.py:104-105) through oflow_normalize_images_f32 on GPU inference: one kernel for
# both frames, bit-identical to the reference's CPU arithmetic (ATen on the GPU divides by multiplying with fl(1/255),
# 1 ulp off for ~74 % of values); in-process step 18.56 -> 18.48 ms (profiles/r04/s35_ab.log). False: the ATen form.
NATIVE_NORMALIZE = True
# the pair lanes' SplitUpdate state (cnet output packed into the GRU state, the hoisted context terms) built on the cnet
# stream right after cnet, beside fnet's tail and the correlation pyramid, instead of on the lanes after the pyramid
EARLY_LANE_INIT = True


class HParams(dict):
    """Attribute access to the constructor arguments (Lightning's ``self.hparams`` as used in `raft.py`)."""

    def __getattr__(self, key: str) -> Any:
        try:
            return self[key]
        except KeyError as e:
            raise AttributeError(key) from e


def strip_module(state_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """Drop the ``module.`` prefix of DataParallel checkpoints (reference `pretrained/convert.py:4-11`)."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def _drop_weight_cache(module: nn.Module, _incompatible) -> None:
    module.__dict__.pop("_split_weights", None)


class RAFT(nn.Module):
    def __init__(
        self,
        hidden_dim: int = 128,
        context_dim: int = 128,
        corr_levels: int = 4,
        corr_radius: int = 4,
        iters: int = 12,
        iters_val: int = 24,
        gamma: float = 0.8,
        dropout: float = 0.0,
        lr: float = 0.00002,
        wdecay: float = 0.00005,
        epsilon: float = 1e-8,
        alternate_corr: bool = False,
    ) -> None:
        super().__init__()
        self.hparams = HParams(
            hidden_dim=hidden_dim,
            context_dim=context_dim,
            corr_levels=corr_levels,
            corr_radius=corr_radius,
            iters=iters,
            iters_val=iters_val,
            gamma=gamma,
            dropout=dropout,
            lr=lr,
            wdecay=wdecay,
            epsilon=epsilon,
            alternate_corr=alternate_corr,
        )
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=dropout)
        self.cnet = BasicEncoder(output_dim=hidden_dim + context_dim, norm_fn="batch", dropout=dropout)
        self.update_block = BasicUpdateBlock(corr_levels=corr_levels, corr_radius=corr_radius, hidden_dim=hidden_dim)
        # metrics (raft.py:55-57): modules without parameters or buffers, so the state_dict keys are the reference's
        # without its torchmetrics states (load_from_checkpoint drops those)
        self.epe_train = AverageEndPointError()
        self.epe_val = AverageEndPointError()
        self.f1_val = OutlierRatio(abs_threshold=3.0, rel_threshold=0.05)
        self.last_train_metrics: Dict[str, float] = {}  # the last training_step's {"1px", "3px", "5px"}
        # plain attributes (not hparams): how GPU inference runs the update block. "split": split-fp16 matrix-core
        # convolutions with fused epilogues (SplitUpdate, default); "fused": MIOpen fp32 convolutions + fused
        # elementwise kernels (FusedUpdate); "module": the nn.Module as written. fused_update=False forces "module".
        self.update_impl = "split"
        self.fused_update = True
        # "split": encoders on the split-fp16 kernels (SplitEncoder) in GPU inference; "module": nn.Module (MIOpen)
        self.encoder_impl = "split"
        # how autograd on the GPU differentiates the convex upsampling: "native": torch.ops.oflow.convex_upsample (the
        # forward's fused kernel, backward csrc/upsample_backward.hip); "aten": the reference's composition (softmax,
        # unfold, broadcast product, sum). Without autograd the fused kernel runs either way.
        self.upsample_impl = "native"
        # how autograd on the GPU differentiates the update block's convolutions: "aten" (default): the nn.Conv2d
        # modules (MIOpen); "native": torch.ops.oflow.conv2d_same, the same forward with the dgrad / wgrad kernels of
        # csrc/conv_backward.hip (fp32 MFMA, no atomics, bit-reproducible). The encoders have their own switch.
        self.conv_backward_impl = "aten"
        # how autograd on the GPU differentiates the two encoders, independent of conv_backward_impl: "aten" (default):
        # the modules (MIOpen); "native": their 32 convolutions as torch.ops.oflow.conv2d_strided and their norm layers
        # (+ ReLU) as instance_norm_act / frozen_batch_norm_act (extractor.py; csrc/conv_backward.hip,
        # csrc/norm_backward.hip). cnet's batch norm in train mode (batch statistics) has its own switch, below.
        self.encoder_backward_impl = "aten"
        # cnet's 15 BatchNorm2d layers on batch statistics (train mode without freeze_bn(): the Chairs stage) under
        # autograd on the GPU, independent of the two switches above: "aten" (default): the modules (MIOpen);
        # "native": torch.ops.oflow.batch_norm_act (+ ReLU), forward and backward both csrc/batch_norm.hip. Opt-in
        # because its forward is not ATen's bit for bit (another summation order for the statistics).
        self.batch_norm_impl = "aten"
        self.encoder_streams = True  # cnet beside fnet + the corr pyramid (inference, split encoders)
        self.fnet_streams = True  # with encoder_streams: fnet's image0 and image1 halves on two streams
        # split update loop over >= 2 pairs (CorrBlock): the pairs' two halves run on two streams so that one half's
        # convolutions fill the CUs the other half's leave idle at a wave tail. pair_lookup "joined": one full-batch
        # lookup per iteration on the main stream (both halves joined around it); "lane": each half looks up its own.
        self.pair_lanes = 2
        self.pair_lookup = "joined"
        # lookup fused into convc1 (csrc/corr_convc1.hip; CorrBlock, radius 3 / 4): each lane runs
        # relu(convc1(lookup)) as one kernel and the lookup volume never reaches HBM (pair_lookup then does not apply)
        self.lookup_fusion = True
        # with the split encoders, fnet writes its features as S32 rows and the pyramid is built from split-fp16
        # products (oflow_corr_pyramid_tiled_s32); False: fp32 features and the fp32-MFMA pyramid
        self.split_corr = True
        # split encoders: the stem convolution builds its 7x7 patch operand from the image tile by tile
        # (OFLOW_IN_IMG7S2) instead of reading a patch matrix written beforehand (fnet's image0 rows shared with cnet)
        self.stem_from_image = True
        # the split-fp16 range guard (csrc: a sticky device flag set when an operand's hi half overflows fp16). After
        # each GPU inference forward the flag is read and cleared in one device-side exchange on the forward's stream
        # (``_native.RangeSnapshot``: that forward's own status, copied to pinned memory behind an event).
        # "deferred" (default): no host sync in the forward; the snapshot is ``last_range_snapshot`` (callers that
        # consume the output asynchronously check it before using it, as predict.py's writer does), a later forward
        # raises once the GPU is past an overflowing one, and check_range() waits and raises. "sync": the forward
        # waits for its snapshot and raises (one host sync per forward: -2.5 % on the 8-pair bench step,
        # profiles/r04/s1_bench*.log). "off": never read (the flag then stays set until another model reads it).
        self.range_guard = "deferred"
        self._range_pending = []  # deferred snapshots not yet checked, in issue order
        self.last_range_snapshot = None
        # the split paths cache packed fp16 hi/lo weights keyed by (storage, version); parameters created under
        # torch.inference_mode() have no version counter, so loading new weights in place drops the caches
        for m in (self.fnet, self.cnet, self.update_block):
            m.register_load_state_dict_post_hook(_drop_weight_cache)

    def invalidate_weight_caches(self) -> None:
        """Drop the packed-weight caches of the split kernels (call after editing parameters in place under
        torch.inference_mode(); load_state_dict does it by itself)."""
        for m in (self.fnet, self.cnet, self.update_block):
            _drop_weight_cache(m, None)

    # -- checkpoints -------------------------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: Union[str, os.PathLike], map_location=None, **kwargs) -> "RAFT":
        """Load a Lightning ``.ckpt`` (``state_dict`` + ``hyper_parameters``) or an official ``.pth``
        (``module.``-prefixed keys) with ``torch.load(weights_only=True)``."""
        ckpt = torch.load(checkpoint_path, map_location=map_location or "cpu", weights_only=True)
        hp = {}
        if isinstance(ckpt, dict) and "state_dict" in ckpt:
            hp = dict(ckpt.get("hyper_parameters", {}) or {})
            sd = ckpt["state_dict"]
        else:
            sd = ckpt
        hp.update(kwargs)
        model = cls(**{k: v for k, v in hp.items() if k in cls.__init__.__code__.co_varnames})
        sd = {k: v for k, v in strip_module(sd).items() if not k.startswith(("epe_", "f1_"))}
        model.load_state_dict(sd)
        return model

    def freeze_bn(self) -> None:
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    # -- training ----------------------------------------------------------------------------------------
    def training_step(self, batch: Tuple[Tensor, Tensor, Tensor, Tensor], batch_idx: int = 0) -> Tensor:
        """One training batch ``(img0, img1, flow_gt, valid)`` (`raft.py:149-175` without Lightning's logging): the
        forward with ``hparams.iters`` refinements, ``sequence_loss`` with ``hparams.gamma``, ``epe_train`` updated with
        the last prediction; returns the loss for the caller's ``backward()`` and optimizer. The 1 / 3 / 5 px shares
        the reference logs are kept on ``last_train_metrics``. On the GPU every step autograd differentiates outside
        the convolutions is a native kernel: correlation, convex upsampling, sequence loss; with
        ``conv_backward_impl = "native"`` the update block's convolutions are too (csrc/conv_backward.hip), and with
        ``encoder_backward_impl = "native"`` the encoders' convolutions and norm layers (csrc/norm_backward.hip). Batch
        norm on batch statistics (cnet in train mode without ``freeze_bn()``) goes native, forward and backward, with
        ``batch_norm_impl = "native"`` (csrc/batch_norm.hip). With all of them (the third only matters without
        ``freeze_bn()``) and ``alternate_corr=False`` the step's gradients are bit-reproducible; ``alternate_corr=True`` stays outside that
        claim (its feature gradient sums overlapping windows with atomics)."""
        img0, img1, flow, valid = batch
        flow_predictions = self(img0, img1, iters=self.hparams.iters)
        loss, metrics = sequence_loss(flow_predictions, flow, valid, gamma=self.hparams.gamma)
        self.epe_train.update(flow_predictions[-1].detach(), flow, valid)
        self.last_train_metrics = metrics
        return loss

    def unsupervised_step(self, batch: Tuple[Tensor, Tensor], batch_idx: int = 0, w_census: float = 1.0,
                          w_smooth: float = 1.0, smooth_order: int = 1, w_ssim: float = 0.0,
                          w_charbonnier: float = 0.0, ssim_window: int = 3, ssim_sigma: Optional[float] = None) -> Tensor:
        """One training batch ``(img0, img1)`` without ground truth (an addition; the reference has none): both flow
        directions from ``forward_bidirectional`` with ``hparams.iters`` refinements, the occlusion masks of the last
        predictions under ``no_grad`` (``optical_flow.fb_consistency(..., both=True)``), and
        ``unsupervised_sequence_loss`` with ``hparams.gamma`` summed over both directions with ``mask = ~occluded``.
        Returns the loss for the caller's ``backward()``; like ``training_step`` it does no logging and has no
        optimizer, and nothing in it synchronises with the host. The weights are plain keyword defaults and untuned:
        the papers this follows (UnFlow, UFlow) weigh the smoothness term per dataset. ``w_ssim`` and
        ``w_charbonnier`` switch on the two other photometric terms (``unsupervised_sequence_loss``); at 0, the default,
        they are not evaluated at all."""
        from optical_flow import fb_consistency

        img0, img1 = batch
        preds_fw, preds_bw = self.forward_bidirectional(img0, img1, iters=self.hparams.iters)
        with torch.no_grad():
            occ_fw, occ_bw = fb_consistency(preds_fw[-1], preds_bw[-1], both=True)
        kw = dict(gamma=self.hparams.gamma, w_census=w_census, w_smooth=w_smooth, smooth_order=smooth_order,
                  w_ssim=w_ssim, w_charbonnier=w_charbonnier, ssim_window=ssim_window, ssim_sigma=ssim_sigma)
        return (unsupervised_sequence_loss(preds_fw, img0, img1, mask=~occ_fw, **kw)
                + unsupervised_sequence_loss(preds_bw, img1, img0, mask=~occ_bw, **kw))

    # -- evaluation --------------------------------------------------------------------------------------
    def validation_step(self, batch: Tuple[Tensor, Tensor, Tensor, Tensor], batch_idx: int = 0, stage: str = "sintel") -> None:
        """One evaluation batch ``(img0, img1, flow_gt, valid)`` (`raft.py:183-196`): pad for ``stage`` (the reference
        takes it from the trainer's datamodule), run ``hparams.iters_val`` iterations in test mode, unpad, update
        ``epe_val`` and ``f1_val``. The metrics read the unpadded prediction as the cropped view it is (no copy) and
        nothing here synchronises with the host; ``compute()`` on the metrics gives the result."""
        img0, img1, flow_gt, valid = batch
        padder = InputPadder(img0.shape, mode=stage)
        img0, img1 = padder.pad(img0, img1)
        _, flow_pr = self(img0, img1, iters=self.hparams.iters_val, test_mode=True)
        flow_pr = padder.unpad(flow_pr)
        self.epe_val.update(flow_pr, flow_gt, valid)
        self.f1_val.update(flow_pr, flow_gt, valid)

    # -- forward -----------------------------------------------------------------------------------------
    @staticmethod
    def initialize_flow(img: Tensor) -> Tuple[Tensor, Tensor]:
        """coords0 = coords1 = pixel grid at 1/8 resolution; flow = coords1 - coords0 (`raft.py:64-71`)."""
        n, _, h, w = img.shape
        coords0 = coords_grid(n, h // 8, w // 8, device=img.device)
        return coords0, coords0.clone()

    @staticmethod
    def upsample_flow(flow: Tensor, mask: Tensor, impl: str = "native") -> Tensor:
        """[H/8, W/8, 2] -> [H, W, 2] by a softmax-weighted 3x3 convex combination (`raft.py:73-85`). On the GPU one
        fused HIP kernel (csrc/upsample.hip); under autograd the same kernel as ``torch.ops.oflow.convex_upsample``,
        differentiated by its native transpose (csrc/upsample_backward.hip), unless ``impl`` (the model's
        ``upsample_impl``) is "aten": then the reference's composition below is what autograd records."""
        if impl not in ("native", "aten"):
            raise ValueError(f"upsample_impl must be 'native' or 'aten', got {impl!r}")
        grad = torch.is_grad_enabled() and (flow.requires_grad or mask.requires_grad)
        if flow.is_cuda and (not grad or impl == "native"):
            return _native.convex_upsample(flow, mask)
        n, _, h, w = flow.shape
        mask = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
        up_flow = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
        up_flow = torch.sum(mask * up_flow, dim=2).permute(0, 1, 4, 2, 5, 3)
        return up_flow.reshape(n, 2, 8 * h, 8 * w)

    def _lane_cuts(self, b: int):
        n = min(self.pair_lanes, b)
        edges = [(b * i) // n for i in range(n + 1)]
        return list(zip(edges[:-1], edges[1:]))

    def _lane_runners(self, cnet_out: Tensor, hdim: int, lanes, on=None) -> list:
        """One SplitUpdate per lane (its buffers, the cnet output packed into the GRU state, the loop-invariant context
        terms), built on stream ``on`` (default: each lane's own stream)."""
        runners = []
        for i, ((b0, b1), st) in enumerate(zip(self._lane_cuts(cnet_out.shape[0]), lanes)):
            with torch.cuda.stream(on if on is not None else st):
                slot = 0 if i == 0 else 200 + i
                runners.append(SplitUpdate(self.update_block, cnet_out[b0:b1], hdim, side_slot=slot, fuse_c1=self.lookup_fusion,
                                           flow_head_pixels=cnet_out.shape[0] * cnet_out.shape[2] * cnet_out.shape[3],
                                           side_owner=st))
        return runners

    def _lanes_for(self, dev, b: int):
        main = torch.cuda.current_stream(dev)
        return [main] + [_side_stream(dev, 100 + i) for i in range(1, min(self.pair_lanes, b))]

    def _split_update_lanes(self, corr_fn, cnet_out: Tensor, coords0: Tensor, coords1: Tensor, iters: int, hdim: int,
                            test_mode: bool, runners=None) -> List[Tensor]:
        """The split update loop with the pairs in ``pair_lanes`` parts, each on its own stream (lane) with its own side stream;
        coords1 is advanced in place. Per-pixel results are those of the single-lane loop bit for bit (no reduction
        crosses pairs). Returns the upsampled flows (test mode: the last one only). ``runners``: the lanes' SplitUpdates
        when already built (on the cnet stream, beside the correlation pyramid; the current stream has waited for it)."""
        b = cnet_out.shape[0]
        dev = cnet_out.device
        cuts = self._lane_cuts(b)
        main = torch.cuda.current_stream(dev)
        lanes = self._lanes_for(dev, b)
        # the packed weights (built on first use, by kernels on this stream) must exist before the lanes fork: the
        # lanes read them with no later join when the lookup is not joined (fused into convc1, or pair_lookup "lane")
        SplitUpdate._weights(self.update_block)
        # lane_init_on_main: the lanes' buffers are allocated (and their loop-invariant context terms computed) on the
        # main stream before the fork, so that no lane allocates from its own stream
        init_main = getattr(self, "lane_init_on_main", False) or runners is not None
        if not init_main:
            for st in lanes[1:]:
                st.wait_stream(main)
        if runners is None:
            runners = self._lane_runners(cnet_out, hdim, lanes, on=main if init_main else None)
        if init_main:
            for st in lanes[1:]:
                st.wait_stream(main)
        joined = self.pair_lookup == "joined" and not runners[0].fusable(corr_fn)
        hw = cnet_out.shape[2] * cnet_out.shape[3]
        if joined:
            rows = torch.empty((b * hw, runners[0].corr_ch), device=dev, dtype=torch.float32)
            h, w = cnet_out.shape[2:]
            ins = [_native.F32In(rows[b0 * hw : b1 * hw], b1 - b0, h, w) for b0, b1 in cuts]
        else:
            parts = [corr_fn.batch_slice(b0, b1) for b0, b1 in cuts]
        outs = []
        for itr in range(iters):
            last = itr == iters - 1
            need = not test_mode or last
            mask = torch.empty((b, 576, *cnet_out.shape[2:]), device=dev, dtype=torch.float32) if need else None
            if joined:
                for st in lanes[1:]:
                    main.wait_stream(st)
                corr_fn.lookup_nhwc(coords1, rows)
            if joined or need:  # (need: the mask block may still be in use by earlier main-stream work)
                for st in lanes[1:]:
                    st.wait_stream(main)
            for i, ((b0, b1), st) in enumerate(zip(cuts, lanes)):
                with torch.cuda.stream(st):
                    c1 = coords1[b0:b1]
                    corr_in = ins[i] if joined else runners[i].lookup(parts[i], c1)
                    runners[i].update(corr_in, c1, need, mask_out=mask[b0:b1] if need else None)
            if need:
                for st in lanes[1:]:
                    main.wait_stream(st)
                outs.append(self.upsample_flow(coords1 - coords0, mask))
        for st in lanes[1:]:
            main.wait_stream(st)
        return outs

    def check_range(self, device=None) -> None:
        """Raise if a split-fp16 operand overflowed in any forward since the last check (waits for those forwards; with
        ``device`` also reads the flag after every stream of it, e.g. forwards of range_guard "off")."""
        pend, self._range_pending = self._range_pending, []
        bad = False
        for snap in pend:
            bad |= snap.overflowed()
        if bad:
            raise RuntimeError(f"RAFT forward: in an earlier forward {_native.RANGE_ERROR}")
        if device is not None:
            _native.range_flag_raise_if_set(device, all_streams=True)

    def forward(
        self,
        image0: Tensor,
        image1: Tensor,
        iters: int = 12,
        flow_init: Optional[Tensor] = None,
        upsample: bool = True,
        test_mode: bool = False,
    ) -> Union[Tensor, Tuple[Tensor, Tensor], List[Tensor]]:
        """Estimate optical flow between pairs of frames (`raft.py:87-147`). Images (B, 3, H, W) in [0, 255]
        with H, W divisible by 8 (use ``InputPadder``). Returns ``(coords1 - coords0, flow_up)`` in test mode,
        else the list of ``iters`` upsampled predictions. ``flow_init`` (B, 2, H/8, W/8), added to the initial
        coordinates (`raft.py:122-123`), is the warm start of RAFT's video mode: pass
        ``model.forward_interpolate(low)``, where ``low`` is the first value the test-mode forward of the previous
        pair of the sequence returned; ``None`` starts cold (``predict.py --warm_start`` runs a folder this way).
        On the GPU in inference the split-fp16 range guard
        (``range_guard``) reports an operand that left the fp16 range with RuntimeError: "sync" raises from this
        forward; "deferred" (default) does not wait -- this forward's status is ``last_range_snapshot``
        (``.overflowed()`` waits for it), and a later forward or ``check_range()`` raises for it."""
        return self._guarded(image0, lambda: self._forward(image0, image1, iters, flow_init, test_mode))

    def forward_bidirectional(
        self,
        image0: Tensor,
        image1: Tensor,
        iters: int = 12,
        flow_init: Optional[Tuple[Optional[Tensor], Optional[Tensor]]] = None,
        test_mode: bool = False,
    ):
        """The flow 0 -> 1 and the flow 1 -> 0 of every pair in one forward (an addition): the result of
        ``self(cat([image0, image1]), cat([image1, image0]), ...)`` split into its halves, with the feature encoder run
        once per distinct image instead of twice -- fnet's instance norm is per image, so an image's features do not
        depend on which side of a pair it sits; the reverse direction's correlation pyramid is the forward one's kernel
        with its arguments swapped, cnet runs on both images, and the update loop sees 2 B independent pairs. Returns
        ``((low_fw, up_fw), (low_bw, up_bw))`` in test mode, else ``(predictions_fw, predictions_bw)``. ``flow_init``:
        ``None`` or a pair ``(init_fw, init_bw)``, either ``None`` (zeros). Differentiable wherever ``forward`` is, and
        under the same range guard. When fnet applies dropout (train mode, ``dropout > 0``) an image's features do depend
        on its place in the batch, and the stacked forward runs as written above.
        ``optical_flow.fb_consistency(up_fw, up_bw, both=True)`` turns the two flows into occlusion masks."""
        n = image0.shape[0]
        init = None
        if flow_init is not None:
            if not isinstance(flow_init, (tuple, list)) or len(flow_init) != 2:
                raise TypeError("forward_bidirectional: flow_init must be None or a pair (init_fw, init_bw), either of "
                                "which may be None")
            init_fw, init_bw = flow_init
            if init_fw is not None or init_bw is not None:
                ref = init_fw if init_fw is not None else init_bw
                init = torch.cat([torch.zeros_like(ref) if t is None else t for t in (init_fw, init_bw)], dim=0)
        if self.fnet.training and self.fnet.dropout is not None:
            stacked0, stacked1 = torch.cat([image0, image1], dim=0), torch.cat([image1, image0], dim=0)
            out = self._guarded(image0, lambda: self._forward(stacked0, stacked1, iters, init, test_mode))
        else:
            out = self._guarded(image0, lambda: self._forward(image0, image1, iters, init, test_mode, both=True))
        if test_mode:
            low, up = out
            return (low[:n], up[:n]), (low[n:], up[n:])
        return [p[:n] for p in out], [p[n:] for p in out]

    def _guarded(self, image0: Tensor, run):
        """``run()`` under the split-fp16 range guard of ``forward``."""
        guard = self.range_guard in ("sync", "deferred") and image0.is_cuda and not torch.is_grad_enabled()
        capturing = image0.is_cuda and capture_active(image0.device)
        if guard and not capturing:
            self._range_before(image0.device)
        out = run()
        if guard and not capturing:
            self._range_after(image0.device)
        return out

    def _range_before(self, dev) -> None:
        """Register the device's range flag; in deferred mode raise for an earlier forward the GPU has finished."""
        _native.range_flag(dev)  # registered before the first kernel that may set it
        if self.range_guard != "deferred":
            return
        bad = False
        while self._range_pending and self._range_pending[0].done():
            bad |= self._range_pending.pop(0).overflowed()
        if bad:
            raise RuntimeError(f"RAFT forward: in an earlier forward {_native.RANGE_ERROR}")

    def _range_after(self, dev) -> None:
        """After a forward's kernels are enqueued: its snapshot (exchange + copy on the current stream); "sync" waits for
        it and raises."""
        snap = _native.RangeSnapshot(torch.device(dev)).take()  # (a new one per forward: callers may hold the last)
        self.last_range_snapshot = snap
        if self.range_guard == "sync":
            if snap.overflowed():
                raise RuntimeError(f"RAFT forward: {_native.RANGE_ERROR}")
        else:
            self._range_pending.append(snap)

    def _encode(self, image0: Tensor, image1: Tensor, hdim: int, both: bool):
        """The encoder stage of ``forward`` and ``forward_bidirectional``: input scaling, fnet, the correlation block,
        cnet. Returns ``(corr_fn, cnet_out, pre_runners, first)``, ``first`` the pairs' first images (cnet's input).
        ``both``: the pairs are (image0, image1) followed by (image1, image0); fnet still runs once per image, and
        each side of the correlation block is the two images' features concatenated in that side's order."""
        if (NATIVE_NORMALIZE and image0.is_cuda and image1.is_cuda and image0.dtype == image1.dtype == torch.float32
                and image0.shape == image1.shape
                and not (torch.is_grad_enabled() and (image0.requires_grad or image1.requires_grad))):
            # raft.py:104-105 as one kernel for both frames (ATen: three launches per frame)
            image0, image1 = _native.normalize_images(image0, image1)
        else:  # CPU tensors, or frames that need gradients (autograd through the elementwise form)
            image0 = (2 * (image0 / 255.0) - 1.0).contiguous()
            image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
        first = torch.cat([image0, image1], dim=0) if both else image0

        def sides(a, b):  # an image pair's features -> the two sides of the correlation block
            return (torch.cat([a, b], dim=0), torch.cat([b, a], dim=0)) if both else (a, b)

        # the split encoders implement the inference forward: fnet in train mode with dropout > 0 applies Dropout2d in
        # the reference (extractor.py BasicEncoder.forward), so it then runs as the module (cnet likewise: batch norm)
        split_enc = (
            image0.is_cuda
            and not torch.is_grad_enabled()
            and self.encoder_impl == "split"
            and (not self.fnet.training or self.fnet.dropout is None)
        )
        fnet = SplitEncoder(self.fnet) if split_enc else self.fnet
        cnet = SplitEncoder(self.cnet) if split_enc and not self.cnet.training else self.cnet
        block = AlternateCorrBlock if self.hparams.get("alternate_corr", False) else CorrBlock
        pre_runners = None
        if split_enc and isinstance(cnet, SplitEncoder):
            # image0's stem patches are the first rows of fnet's (raft.py:109, 115 feed both the same image0); cnet
            # runs on a side stream beside fnet and the correlation pyramid, joined before the update loop
            main = torch.cuda.current_stream(image0.device)
            side = _side_stream(image0.device) if self.encoder_streams else None
            ni = image0.shape[0]
            nb = first.shape[0]  # pairs
            side2 = (_side_stream(image0.device, 1) if side is not None and self.fnet_streams
                     and block is CorrBlock and self.split_corr else None)
            sfi = self.stem_from_image
            # both directions without stem_from_image: cnet reads the patch rows of both images, so one patch matrix
            # of both is built first and each of fnet's halves reads its rows of it
            patches = None if sfi or not both else fnet.stem_patches(first)
            if side2 is not None:
                # fnet's two images on two streams (instance norm is per image: the same values as one batch), so
                # three 8-image encoders share the chip and finish together
                side2.wait_stream(main)
                with torch.cuda.stream(side2):
                    f2s = fnet(image1, patches=None if patches is None else patches[ni:], split_out=True,
                               stem_from_image=sfi)
                if not both:
                    patches = None if sfi else fnet.stem_patches(image0)
            elif not both:
                patches = None if sfi else fnet.stem_patches(torch.cat([image0, image1], dim=0))
            cpatches = None if patches is None else patches[:nb]
            early = (EARLY_LANE_INIT and side is not None and self.fused_update and self.update_impl == "split"
                     and self.pair_lanes > 1 and nb > 1 and block is CorrBlock and self.split_corr)
            lanes = self._lanes_for(image0.device, nb) if early else None  # (main = the current stream, not cnet's)
            if side is not None:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    cnet_out = cnet(first, patches=cpatches, stem_from_image=sfi)
                    if early:
                        # the lanes' GRU state and context terms depend on cnet only: built here, beside fnet's tail
                        # and the correlation pyramid, instead of after the pyramid on the lanes
                        SplitUpdate._weights(self.update_block)
                        pre_runners = self._lane_runners(cnet_out, hdim, lanes, on=side)
            if block is CorrBlock and self.split_corr:
                # features as S32 rows straight from fnet's head conv -> split-fp16 pyramid (no fp32 fmaps)
                if side2 is not None:
                    f1s = fnet(image0, patches=patches[:ni] if both and patches is not None else patches, split_out=True,
                               stem_from_image=sfi)
                    main.wait_stream(side2)
                else:
                    f1s, f2s = fnet([image0, image1], patches=patches, split_out=True, stem_from_image=sfi)
                corr_fn = CorrBlock.from_split_features(*sides(f1s, f2s), radius=self.hparams.corr_radius)
            else:
                fmap1, fmap2 = fnet([image0, image1], patches=patches, stem_from_image=sfi)
                corr_fn = block(*sides(fmap1.float(), fmap2.float()), radius=self.hparams.corr_radius)
            if side is not None:
                main.wait_stream(side)
            else:
                cnet_out = cnet(first, patches=cpatches, stem_from_image=sfi)
        else:
            fmap1, fmap2 = fnet([image0, image1])
            corr_fn = block(*sides(fmap1.float(), fmap2.float()), radius=self.hparams.corr_radius)
            cnet_out = cnet(first)
        return corr_fn, cnet_out, pre_runners, first

    def _forward(self, image0: Tensor, image1: Tensor, iters: int, flow_init: Optional[Tensor], test_mode: bool,
                 both: bool = False):
        """``forward`` without the range guard. ``both``: the pairs are (image0, image1) followed by (image1, image0),
        ``forward_bidirectional``'s 2 B pairs, with fnet run once per image; ``flow_init`` then covers the 2 B pairs."""
        if self.conv_backward_impl not in ("aten", "native"):
            raise ValueError(f"conv_backward_impl must be 'aten' or 'native', got {self.conv_backward_impl!r}")
        if self.encoder_backward_impl not in ("aten", "native"):
            raise ValueError(f"encoder_backward_impl must be 'aten' or 'native', got {self.encoder_backward_impl!r}")
        if self.batch_norm_impl not in ("aten", "native"):
            raise ValueError(f"batch_norm_impl must be 'aten' or 'native', got {self.batch_norm_impl!r}")
        self.fnet.encoder_backward_impl = self.cnet.encoder_backward_impl = self.encoder_backward_impl
        self.fnet.batch_norm_impl = self.cnet.batch_norm_impl = self.batch_norm_impl
        hdim, cdim = self.hparams.hidden_dim, self.hparams.context_dim
        corr_fn, cnet_out, pre_runners, first = self._encode(image0, image1, hdim, both)
        coords0, coords1 = self.initialize_flow(first)
        if flow_init is not None:
            coords1 = coords1 + flow_init

        gpu_inference = cnet_out.is_cuda and not torch.is_grad_enabled() and self.fused_update
        impl = self.update_impl if gpu_inference else "module"
        flow_predictions = []
        flow_up = None
        if impl == "split" and self.pair_lanes > 1 and cnet_out.shape[0] > 1 and hasattr(corr_fn, "lookup_nhwc"):
            coords1 = coords1.contiguous()
            flow_predictions = self._split_update_lanes(corr_fn, cnet_out, coords0, coords1, iters, hdim, test_mode,
                                                        runners=pre_runners)
            if test_mode:
                return coords1 - coords0, flow_predictions[-1]
            return flow_predictions
        if impl == "split":
            # coords1 is advanced in place by the flow head's epilogue (raft.py:133)
            runner = SplitUpdate(self.update_block, cnet_out, hdim, fuse_c1=self.lookup_fusion)
            coords1 = coords1.contiguous()
            for itr in range(iters):
                last = itr == iters - 1
                up_mask = runner.step(corr_fn, coords1, need_mask=not test_mode or last)
                if test_mode and not last:
                    continue  # Q11: intermediate upsamplings are never returned in test mode
                flow_up = self.upsample_flow(coords1 - coords0, up_mask)
                flow_predictions.append(flow_up)
            if test_mode:
                return coords1 - coords0, flow_up
            return flow_predictions

        self.update_block.conv_backward_impl = self.conv_backward_impl
        net, inp = torch.split(cnet_out, [hdim, cdim], dim=1)
        net = torch.tanh(net)
        inp = torch.relu(inp)
        runner = FusedUpdate(self.update_block, net, inp) if impl == "fused" else None
        for itr in range(iters):
            coords1 = coords1.detach()
            corr = corr_fn(coords1)
            flow = coords1 - coords0
            last = itr == iters - 1
            if runner is not None:
                # Q11: in test mode only the last iteration's mask (upsampling) is ever used
                net, up_mask, delta_flow = runner.step(corr, flow, need_mask=not test_mode or last)
            else:
                net, up_mask, delta_flow = self.update_block(net, inp, corr, flow)
            coords1 = coords1 + delta_flow
            if test_mode and not last:
                continue  # Q11: intermediate upsamplings are never returned in test mode
            if up_mask is None:
                flow_up = upflow8(coords1 - coords0)
            else:
                flow_up = self.upsample_flow(coords1 - coords0, up_mask, self.upsample_impl)
            flow_predictions.append(flow_up)

        if test_mode:
            return coords1 - coords0, flow_up
        return flow_predictions


def sequence_loss(
    flow_preds: List[Tensor],
    flow_gt: Tensor,
    valid: Tensor,
    gamma: float = 0.8,
    max_flow: float = 400.0,
) -> Tuple[Tensor, Dict[str, float]]:
    """Loss function defined over a sequence of flow predictions (`raft.py:231-260`): the L1 error of every
    prediction over the pixels with ``valid >= 0.5`` and ``|flow_gt| < max_flow``, weighted by
    ``gamma ** (n - i - 1)``, and the shares of the last prediction's valid pixels with an end-point error under
    1 / 3 / 5 px as Python floats.

    On the GPU this is ``torch.ops.oflow.sequence_loss``: one pass over all predictions for the forward, one for
    every gradient (differentiable in the predictions), and one 64-byte device-to-host copy for the three metrics
    where the reference makes three ``.item()`` calls. CPU tensors run the reference's torch composition."""
    n = len(flow_preds)
    weights = [gamma ** (n - i - 1) for i in range(n)]
    if flow_gt.is_cuda:
        loss, stats = _native.ops().sequence_loss(list(flow_preds), flow_gt, valid, weights, float(max_flow))
        s = stats.cpu()  # the one D2H copy: {n_valid, n<1, n<3, n<5, ...} as float64
        px = (s[1:4] / s[0]).float().tolist()  # (fp32, as the reference's `.float().mean()`; NaN when nothing is valid)
        return loss, {"1px": px[0], "3px": px[1], "5px": px[2]}
    return sequence_loss_torch(flow_preds, flow_gt, valid, weights, max_flow)


def sequence_loss_torch(flow_preds, flow_gt: Tensor, valid: Tensor, weights, max_flow: float):
    """``sequence_loss`` as the reference's torch composition (`raft.py:239-258`) under autograd: the CPU path."""
    mag = torch.sum(flow_gt**2, dim=1).sqrt()
    mask = (valid.reshape(mag.shape) >= 0.5) & (mag < max_flow)
    loss = 0.0
    for w, pred in zip(weights, flow_preds):
        loss = loss + w * (mask[:, None] * (pred - flow_gt).abs()).mean()
    epe = torch.sum((flow_preds[-1].detach() - flow_gt) ** 2, dim=1).sqrt()[mask]
    px = torch.stack([(epe < t).float().mean() for t in (1, 3, 5)]).tolist()
    return loss, {"1px": px[0], "3px": px[1], "5px": px[2]}


def unsupervised_sequence_loss(
    flow_preds: List[Tensor],
    image0: Tensor,
    image1: Tensor,
    mask: Optional[Tensor] = None,
    gamma: float = 0.8,
    w_census: float = 1.0,
    w_smooth: float = 1.0,
    smooth_order: int = 1,
    w_ssim: float = 0.0,
    w_charbonnier: float = 0.0,
    ssim_window: int = 3,
    ssim_sigma: Optional[float] = None,
) -> Tensor:
    """``sequence_loss`` without ground truth (an addition; the reference has none): every prediction is scored against
    the images alone,

        ``sum_i gamma^(n-1-i) [w_census * census_loss(image0, warp(image1, normalize(flow_i), align_corners=True), mask)
        + w_smooth * smoothness_loss(flow_i, image0, order=smooth_order)]``

    with ``optical_flow.census_loss`` / ``smoothness_loss`` (native kernels on the GPU, forward and backward) and the
    differentiable ``optical_flow.warp``. ``mask`` (B, 1, H, W), float or bool, is the census term's: in the intended
    use ``~occluded`` from ``optical_flow.fb_consistency``. ``align_corners=True`` is deliberate: it is the convention
    ``normalize`` uses, and with ``False`` ``warp`` is not the identity at zero flow (quirk Q8 in
    optical_flow/operator/operator.py). The weights are plain defaults, untuned. Images in [0, 255].

    ``w_ssim`` and ``w_charbonnier`` add ``w_ssim * ssim_loss(image0, warped, mask, window=ssim_window,
    sigma=ssim_sigma) + w_charbonnier * charbonnier_loss(image0, warped, mask)`` to each prediction's term, on the same
    warped image and the same mask as the census term (ARFlow's mix is L1 + SSIM + ternary). A weight of exactly 0, the
    default, skips its term entirely -- no kernel, no graph node -- so the defaults give the value they always gave."""
    from optical_flow import census_loss, charbonnier_loss, normalize, smoothness_loss, ssim_loss, warp, warp_grid

    n = len(flow_preds)
    loss = 0.0
    for i, flow in enumerate(flow_preds):
        if flow.is_cuda:
            warped = warp(image1, normalize(flow), align_corners=True)
        else:  # (``warp`` has no CPU path: the same sampling through ATen, as the reference's ``warp`` is written)
            grid = warp_grid(normalize(flow).permute(0, 2, 3, 1))
            warped = F.grid_sample(image1, grid.to(image1.dtype), mode="bilinear", padding_mode="border", align_corners=True)
        term = w_census * census_loss(image0, warped, mask) + w_smooth * smoothness_loss(flow, image0, order=smooth_order)
        if w_ssim != 0:
            term = term + w_ssim * ssim_loss(image0, warped, mask, window=ssim_window, sigma=ssim_sigma)
        if w_charbonnier != 0:
            term = term + w_charbonnier * charbonnier_loss(image0, warped, mask)
        loss = loss + gamma ** (n - 1 - i) * term
    return loss
