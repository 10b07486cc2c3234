from .operator import (denormalize, fb_consistency, integrate, interpolate_frame, normalize, resize, scale, splat, warp,
                       warp_grid)

__all__ = ["denormalize", "fb_consistency", "integrate", "interpolate_frame", "normalize", "resize", "scale", "splat", "warp",
           "warp_grid"]
