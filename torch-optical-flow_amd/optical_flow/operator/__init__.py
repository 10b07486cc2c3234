from .operator import denormalize, fb_consistency, integrate, normalize, resize, scale, warp, warp_grid

__all__ = ["denormalize", "fb_consistency", "integrate", "normalize", "resize", "scale", "warp", "warp_grid"]
