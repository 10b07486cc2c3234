"""MI355X-native ``optical_flow`` (drop-in for awaelchli/torch-optical-flow's ``optical_flow`` package).

Re-exports the operator API of the reference (`optical_flow/__init__.py:2`). ``warp`` runs on a hand-written
gfx950 HIP kernel through the C ABI of ``liboflow_hip.so`` (include/oflow.h). The inference I/O of the reference
 is here too: ``flow2rgb``/``colorwheel`` on a fused colour-map kernel and ``read``/``write``
(Middlebury, PFM, KITTI) with the file payload laid out on the device. ``fb_consistency`` (an addition) gives the
forward-backward occlusion masks of a flow pair in one kernel launch; ``splat`` (an addition) warps a frame forwards
along a flow (sum / average / linear / softmax splatting, bit-reproducible, differentiable) and ``interpolate_frame``
blends two such warps into an in-between frame. ``census_loss`` and ``smoothness_loss`` (``optical_flow.losses``, an
addition) score a flow against the images alone: the unsupervised training losses of UnFlow / UFlow on fused kernels;
``ssim_loss`` (which also gives the SSIM map of two frames) and ``charbonnier_loss`` are the other photometric terms
those methods mix with the census loss.
"""
from .io.read_write import read, write
from .losses import census_loss, charbonnier_loss, smoothness_loss, ssim_loss
from .operator.operator import (denormalize, fb_consistency, integrate, interpolate_frame, normalize, resize, scale, splat,
                                warp, warp_grid)
from .visualization.flow2rgb import colorwheel, flow2rgb

__all__ = ["census_loss", "charbonnier_loss", "colorwheel", "denormalize", "fb_consistency", "flow2rgb", "integrate", "interpolate_frame", "normalize", "read",
           "resize", "scale", "smoothness_loss", "splat", "ssim_loss", "warp", "warp_grid", "write"]
