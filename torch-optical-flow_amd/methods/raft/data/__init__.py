"""``data`` drop-in (reference: methods/raft/data/): the augmentors, with a device path for whole batches
(``FlowAugmentor.augment_batch``, csrc/augment.hip). The datasets, the data module and file decoding are not part of
this package."""
from .augmentor import AugmentParams, FlowAugmentor, SparseFlowAugmentor

__all__ = ["AugmentParams", "FlowAugmentor", "SparseFlowAugmentor"]
