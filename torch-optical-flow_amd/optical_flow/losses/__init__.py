"""``optical_flow.losses`` (an addition; the reference has none): the losses that score a flow against the images
alone, for fine-tuning on unlabelled video -- the ternary census loss and the edge-aware smoothness term of UnFlow
(Meister et al., AAAI 2018) and UFlow (Jonschkowski et al., ECCV 2020), and the two other photometric terms those
methods and ARFlow mix with it, SSIM (box or Gaussian window, with the SSIM map for scoring a warped frame) and
Charbonnier. GPU tensors run the native ops (csrc/census_loss.hip, csrc/smoothness_loss.hip,
csrc/photometric_loss.hip) on the current stream; CPU tensors run the same arithmetic as a differentiable torch
composition, the arrangement ``splat`` and ``fb_consistency`` use.
"""
from .census import census_loss, census_loss_torch
from .photometric import charbonnier_loss, charbonnier_loss_torch, ssim_loss, ssim_loss_torch, ssim_window
from .smoothness import smoothness_loss, smoothness_loss_torch

__all__ = ["census_loss", "charbonnier_loss", "smoothness_loss", "ssim_loss"]
