"""``optical_flow.losses`` (an addition; the reference has none): the losses that score a flow against the images
alone, for fine-tuning on unlabelled video -- the ternary census loss and the edge-aware smoothness term of UnFlow
(Meister et al., AAAI 2018) and UFlow (Jonschkowski et al., ECCV 2020). GPU tensors run the native ops
(csrc/census_loss.hip, csrc/smoothness_loss.hip) on the current stream; CPU tensors run the same arithmetic as a
differentiable torch composition, the arrangement ``splat`` and ``fb_consistency`` use.
"""
from .census import census_loss, census_loss_torch
from .smoothness import smoothness_loss, smoothness_loss_torch

__all__ = ["census_loss", "smoothness_loss"]
