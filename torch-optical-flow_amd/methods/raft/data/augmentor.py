"""``data.augmentor`` drop-in (reference: methods/raft/data/augmentor.py:43-324): ``FlowAugmentor`` and
``SparseFlowAugmentor`` with the reference's constructor arguments, defaults and attributes, split into

* ``sample(ht, wd)``: the random decisions of one sample, drawn on the host in the reference's order, as a plain
  ``AugmentParams``; no pixel is touched;
* ``augment_batch(img1, img2, flow, valid=None, params=None)``: the pixels of a whole batch. CUDA tensors run the
  kernels of csrc/augment.hip (``torch.ops.oflow.augment_batch``: two small statistics launches, one fused pass that
  computes only the crop); CPU tensors run the NumPy composition below, the same arithmetic. The result is what
  ``RAFT.training_step`` takes: fp32 ``(B, 3, ch, cw)`` x 2, ``(B, 2, ch, cw)``, ``(B, ch, cw)``;
* ``__call__``: the reference's per-sample NumPy signature, ``sample()`` plus the CPU path.

The arithmetic is stated in include/oflow.h (oflow_augment_*). Two things about it are NOT verified, because neither
torchvision nor OpenCV was available to compare with:

* the colour draws follow torchvision's *documented* ``ColorJitter.get_params`` order -- ``torch.randperm(4)``, then one
  ``torch.empty(1).uniform_(lo, hi)`` each for brightness, contrast, saturation and hue -- so that the same torch seed
  should make the same decisions as the reference; that order has not been compared with torchvision itself;
* the resize follows OpenCV's documented ``INTER_LINEAR`` coordinate mapping with an fp32 blend; ``cv2``'s own 8-bit
  path blends in 11-bit fixed point, and agreement with it (expected within one level) has not been measured. The
  colour jitter, by contrast, equals Pillow bit for bit (tests/test_augment_host.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

PARAM_DOUBLES = 36  # include/oflow.h OFLOW_AUG_PARAM_DOUBLES
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3  # op ids: torchvision's fn_idx

Rect = Tuple[int, int, int, int]


@dataclass
class AugmentParams:
    """One sample's decisions. ``order*``: the permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE) the frame's ops
    run in; ``factors*``: (brightness, contrast, saturation, hue); frame 2's equal frame 1's unless ``asymmetric``
    (a symmetric draw also takes the contrast mean over both frames, as the reference's stacked image does).
    ``rects``: 0-2 eraser rectangles (x0, y0, dx, dy) in source pixels, frame 2 only. ``scale_x`` / ``scale_y`` are
    float64 and apply when ``do_resize``; the flips act on the resized frame, then the crop starts at (y0, x0)."""

    order1: Tuple[int, int, int, int] = (0, 1, 2, 3)
    factors1: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 0.0)
    order2: Tuple[int, int, int, int] = (0, 1, 2, 3)
    factors2: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 0.0)
    asymmetric: bool = False
    rects: Tuple[Rect, ...] = field(default_factory=tuple)
    do_resize: bool = False
    scale_x: float = 1.0
    scale_y: float = 1.0
    hflip: bool = False
    vflip: bool = False
    y0: int = 0
    x0: int = 0

    @staticmethod
    def to_tensor(params: Sequence["AugmentParams"]) -> torch.Tensor:
        """The rows of include/oflow.h's parameter array: one CPU float64 (len(params), PARAM_DOUBLES) tensor, one
        host-to-device copy for the batch."""
        rows = np.zeros((len(params), PARAM_DOUBLES), np.float64)
        for row, p in zip(rows, params):
            row[0] = float(p.asymmetric)
            row[1:5], row[5:9] = p.order1, p.factors1
            # a symmetric draw jitters both frames as one image: frame 2's own fields are not consulted
            row[9:13], row[13:17] = (p.order2, p.factors2) if p.asymmetric else (p.order1, p.factors1)
            row[17] = len(p.rects)
            for k, r in enumerate(p.rects):
                row[18 + 4 * k : 22 + 4 * k] = r
            row[26:33] = (p.do_resize, p.scale_x, p.scale_y, p.hflip, p.vflip, p.y0, p.x0)
        return torch.from_numpy(rows)


def resized_size(ht: int, wd: int, p: AugmentParams) -> Tuple[int, int]:
    """The frame size the flips and the crop act on: round-half-even of size * scale under resize."""
    if not p.do_resize:
        return ht, wd
    return int(round(ht * p.scale_y)), int(round(wd * p.scale_x))


# ---------------------------------------------------------------------------------------------- colour (Pillow's)
def _luma(img: np.ndarray) -> np.ndarray:
    c = img.astype(np.int32)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16


def _blend(d, img: np.ndarray, f: float) -> np.ndarray:
    f32 = np.float32(f)
    d32 = np.asarray(d, np.float32)
    v = d32 + f32 * (img.astype(np.float32) - d32)
    if not 0.0 <= f32 <= 1.0:
        v = np.clip(v, 0.0, 255.0)
    return v.astype(np.uint8)


def _hue(img: np.ndarray, hue: float) -> np.ndarray:
    shift = int(hue * 255.0) % 256
    f32, f64 = np.float32, np.float64
    c = img.reshape(-1, 3).astype(np.int32)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    mx, mn = c.max(1), c.min(1)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = (mx - r).astype(f32) / cr, (mx - g).astype(f32) / cr, (mx - b).astype(f32) / cr
        h = np.where(r == mx, bc - gc,
                     np.where(g == mx, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                              (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        h = np.where(grey, f32(0), h)
        s = np.where(grey, f32(0), s)
    hh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    ss = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    hh = (hh + shift) & 255
    v = mx.astype(f64)
    hf = hh.astype(f64) * 6.0 / 255.0
    fi = np.floor(hf)
    f = (hf - fi).astype(f32).astype(f64)
    fs = (ss.astype(f64) / 255.0).astype(f32).astype(f64)

    def rnd(x):
        return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)

    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    vi = mx
    sext = fi.astype(np.int64) % 6
    table = ((vi, t, p), (q, vi, p), (p, vi, t), (p, q, vi), (t, p, vi), (vi, p, q))
    out = np.empty_like(c)
    for ch in range(3):
        out[:, ch] = np.choose(sext, [table[k][ch] for k in range(6)])
    out[ss == 0] = vi[ss == 0, None]
    return out.astype(np.uint8).reshape(img.shape)


def _jitter(frames: List[np.ndarray], order, factors) -> List[np.ndarray]:
    """The four ops in ``order`` on ``frames`` as ONE image: the contrast mean runs over all of them."""
    frames = [f.copy() for f in frames]
    for op in order:
        if op == BRIGHTNESS:
            frames = [_blend(0, f, factors[0]) for f in frames]
        elif op == CONTRAST:
            total = sum(int(_luma(f).sum(dtype=np.int64)) for f in frames)
            count = sum(f.shape[0] * f.shape[1] for f in frames)
            d = int(total / count + 0.5)
            frames = [_blend(d, f, factors[1]) for f in frames]
        elif op == SATURATION:
            frames = [_blend(_luma(f)[..., None], f, factors[2]) for f in frames]
        elif op == HUE:
            frames = [_hue(f, factors[3]) for f in frames]
    return frames


# ---------------------------------------------------------------------------------------------- geometry
def _linear_coords(d: np.ndarray, scale: float, n: int):
    """OpenCV's INTER_LINEAR taps of output indices ``d``: (i, i + 1 clamped, a)."""
    f = ((d.astype(np.float64) + 0.5) * (1.0 / scale) - 0.5).astype(np.float32)
    fl = np.floor(f)
    i = fl.astype(np.int64)
    a = f - fl
    lo, hi = i < 0, i >= n - 1
    i = np.where(lo, 0, np.where(hi, n - 1, i))
    a = np.where(lo | hi, np.float32(0), a).astype(np.float32)
    return i, np.minimum(i + 1, n - 1), a


def _lerp(s0, s1, a):
    return s0 * (np.float32(1) - a) + s1 * a


def _resized_coords(p: AugmentParams, ht: int, wd: int, ch: int, cw: int):
    """Rows / columns of the resized frame the crop reads, flips undone."""
    ht1, wd1 = resized_size(ht, wd, p)
    ry = np.arange(ch, dtype=np.int64) + p.y0
    rx = np.arange(cw, dtype=np.int64) + p.x0
    if p.vflip:
        ry = ht1 - 1 - ry
    if p.hflip:
        rx = wd1 - 1 - rx
    return ry, rx, ht1, wd1


def _sample_bilinear(planes: np.ndarray, p: AugmentParams, ry, rx) -> np.ndarray:
    """(C, H, W) fp32 planes at the crop's positions: the horizontal then vertical fp32 blend, or a plain gather."""
    _, ht, wd = planes.shape
    if not p.do_resize:
        return planes[:, ry][:, :, rx]
    iy, iy1, ay = _linear_coords(ry, p.scale_y, ht)
    ix, ix1, ax = _linear_coords(rx, p.scale_x, wd)
    top = _lerp(planes[:, iy][:, :, ix], planes[:, iy][:, :, ix1], ax[None, None, :])
    bot = _lerp(planes[:, iy1][:, :, ix], planes[:, iy1][:, :, ix1], ax[None, None, :])
    return _lerp(top, bot, ay[None, :, None])


def _sparse_flow(flow: np.ndarray, valid: np.ndarray, p: AugmentParams, ry, rx, ht1: int, wd1: int):
    """resize_sparse_flow_map at the crop's positions; the last source in row-major order wins a shared pixel."""
    _, ht, wd = flow.shape
    ys, xs = np.nonzero(valid >= 1)
    xx = np.rint(xs.astype(np.float32).astype(np.float64) * p.scale_x).astype(np.int64)
    yy = np.rint(ys.astype(np.float32).astype(np.float64) * p.scale_y).astype(np.int64)
    keep = (xx > 0) & (xx < wd1) & (yy > 0) & (yy < ht1)
    src = (ys * wd + xs)[keep]
    winner = np.full(ht1 * wd1, -1, np.int64)
    np.maximum.at(winner, (yy * wd1 + xx)[keep], src)
    win = winner.reshape(ht1, wd1)[ry][:, rx]
    hit = win >= 0
    w = np.where(hit, win, 0)
    scale = np.array([p.scale_x, p.scale_y], np.float64)[:, None, None]
    out = (flow.reshape(2, -1)[:, w].astype(np.float64) * scale).astype(np.float32)
    return np.where(hit[None], out, np.float32(0)), hit.astype(np.float32)


class _AugmentorBase:
    sparse = False
    crop_size: Tuple[int, int]

    # -- drawing ---------------------------------------------------------------------------------------
    def _draw_color(self) -> Tuple[Tuple[int, ...], Tuple[float, ...]]:
        """One ColorJitter.get_params draw from torch's global generator (documented order; see the module docstring)."""
        b, c, s, h = self._jitter
        order = tuple(int(v) for v in torch.randperm(4))
        factors = tuple(float(torch.empty(1).uniform_(lo, hi))
                        for lo, hi in ((max(0.0, 1 - b), 1 + b), (max(0.0, 1 - c), 1 + c), (max(0.0, 1 - s), 1 + s), (-h, h)))
        return order, factors

    def _draw_eraser(self, ht: int, wd: int) -> Tuple[Rect, ...]:
        rects = []
        if np.random.rand() < self.eraser_aug_prob:
            for _ in range(np.random.randint(1, 3)):
                x0 = np.random.randint(0, wd)
                y0 = np.random.randint(0, ht)
                dx = np.random.randint(50, 100)
                dy = np.random.randint(50, 100)
                rects.append((int(x0), int(y0), int(dx), int(dy)))
        return tuple(rects)

    # -- checks ----------------------------------------------------------------------------------------
    def _validate(self, p: AugmentParams, ht: int, wd: int) -> None:
        if not isinstance(p, AugmentParams):
            raise TypeError(f"augment_batch: params must hold AugmentParams, got {type(p).__name__}")
        for order in (p.order1, p.order2):
            if sorted(int(v) for v in order) != [0, 1, 2, 3] or len(order) != 4:
                raise ValueError(f"augment_batch: op order {tuple(order)} is not a permutation of (0, 1, 2, 3)")
        for fac in (p.factors1, p.factors2):
            if len(fac) != 4 or not all(math.isfinite(float(v)) for v in fac):
                raise ValueError(f"augment_batch: jitter factors {tuple(fac)} must be four finite numbers")
        if len(p.rects) > 2:
            raise ValueError(f"augment_batch: {len(p.rects)} eraser rectangles (at most 2)")
        for r in p.rects:
            if len(r) != 4 or any(int(v) != v or not 0 <= v < 2 ** 30 for v in r):
                raise ValueError(f"augment_batch: eraser rectangle {tuple(r)} must be non-negative integers (x0, y0, dx, dy)")
        if p.do_resize and not (math.isfinite(p.scale_x) and math.isfinite(p.scale_y) and p.scale_x > 0 and p.scale_y > 0):
            raise ValueError(f"augment_batch: scale ({p.scale_x}, {p.scale_y}) must be positive")
        if p.vflip and self.sparse:
            raise ValueError("augment_batch: the sparse augmentor never flips vertically")
        ht1, wd1 = resized_size(ht, wd, p)
        ch, cw = self.crop_size
        if int(p.y0) != p.y0 or int(p.x0) != p.x0 or p.y0 < 0 or p.x0 < 0 or p.y0 + ch > ht1 or p.x0 + cw > wd1:
            raise ValueError(f"augment_batch: crop {ch}x{cw} at (y0, x0) = ({p.y0}, {p.x0}) leaves the {ht1}x{wd1} "
                             f"resized frame")

    def _check_inputs(self, img1, img2, flow, valid):
        what = "augment_batch"
        for name, t in (("img1", img1), ("img2", img2), ("flow", flow)) + ((("valid", valid),) if self.sparse else ()):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if valid is not None and not self.sparse:
            raise ValueError(f"{what}: the dense augmentor takes no valid mask (it derives one from the flow)")
        if img1.dim() != 4 or img1.shape[3] != 3 or img1.shape != img2.shape:
            raise ValueError(f"{what}: img1 {tuple(img1.shape)} and img2 {tuple(img2.shape)} must be equal (B, H, W, 3)")
        if img1.dtype != torch.uint8 or img2.dtype != torch.uint8:
            raise TypeError(f"{what}: images must be uint8, got {img1.dtype} and {img2.dtype}")
        b, ht, wd, _ = img1.shape
        if tuple(flow.shape) != (b, 2, ht, wd):
            raise ValueError(f"{what}: flow {tuple(flow.shape)} must be (B, 2, H, W) = {(b, 2, ht, wd)}")
        if flow.dtype != torch.float32:
            raise TypeError(f"{what}: flow must be float32, got {flow.dtype}")
        if self.sparse:
            if tuple(valid.shape) != (b, ht, wd):
                raise ValueError(f"{what}: valid {tuple(valid.shape)} must be (B, H, W) = {(b, ht, wd)}")
            if valid.dtype != torch.float32:
                raise TypeError(f"{what}: valid must be float32, got {valid.dtype}")
        devices = {t.device for t in (img1, img2, flow) + ((valid,) if self.sparse else ())}
        if len(devices) != 1:
            raise ValueError(f"{what}: all tensors must be on one device, got {sorted(str(d) for d in devices)}")
        return b, ht, wd

    # -- the pixels ------------------------------------------------------------------------------------
    def augment_batch(self, img1: torch.Tensor, img2: torch.Tensor, flow: torch.Tensor,
                      valid: Optional[torch.Tensor] = None, params: Optional[Sequence[AugmentParams]] = None):
        """Augment a batch: ``img*`` uint8 (B, H, W, 3), ``flow`` fp32 (B, 2, H, W), for the sparse class ``valid`` fp32
        (B, H, W), all on one device and of one source size; ``params``: B ``AugmentParams`` (default: ``sample()`` once
        per sample). Returns fp32 ``(img1, img2, flow, valid)`` of shapes (B, 3, ch, cw), (B, 3, ch, cw), (B, 2, ch, cw),
        (B, ch, cw) on the inputs' device, contiguous -- ``RAFT.training_step``'s batch. The dense ``valid`` is
        ``(|u| < 1000) & (|v| < 1000)`` of the augmented flow. Malformed input or parameters raise before any launch."""
        b, ht, wd = self._check_inputs(img1, img2, flow, valid)
        if params is None:
            params = [self.sample(ht, wd) for _ in range(b)]
        params = list(params)
        if len(params) != b:
            raise ValueError(f"augment_batch: {len(params)} parameter sets for a batch of {b}")
        for p in params:
            self._validate(p, ht, wd)
        ch, cw = self.crop_size
        if img1.is_cuda:
            from optical_flow import _native

            rows = AugmentParams.to_tensor(params).to(img1.device, non_blocking=True)
            return tuple(_native.augment_batch(img1, img2, flow, valid if self.sparse else None, rows, ch, cw))
        outs = [self._augment_numpy(img1[i].numpy(), img2[i].numpy(), flow[i].numpy(),
                                    valid[i].numpy() if self.sparse else None, p) for i, p in enumerate(params)]
        shapes = ((3, ch, cw), (3, ch, cw), (2, ch, cw), (ch, cw))
        return tuple(torch.from_numpy(np.ascontiguousarray(np.stack([o[k] for o in outs]).reshape((b,) + sh), np.float32))
                     for k, sh in enumerate(shapes))

    def _augment_numpy(self, img1, img2, flow, valid, p: AugmentParams):
        """One sample on the host: HWC uint8 frames, (2, H, W) fp32 flow[, (H, W) fp32 valid] -> CHW fp32 crops."""
        ht, wd = img1.shape[:2]
        ch, cw = self.crop_size
        if p.asymmetric:
            (j1,) = _jitter([img1], p.order1, p.factors1)
            (j2,) = _jitter([img2], p.order2, p.factors2)
        else:
            j1, j2 = _jitter([img1, img2], p.order1, p.factors1)
        if p.rects:
            mean = (j2.reshape(-1, 3).sum(0, dtype=np.int64) / float(ht * wd)).astype(np.uint8)
            for x0, y0, dx, dy in p.rects:
                j2[y0 : y0 + dy, x0 : x0 + dx] = mean
        ry, rx, ht1, wd1 = _resized_coords(p, ht, wd, ch, cw)
        outs = []
        for j in (j1, j2):
            v = _sample_bilinear(np.ascontiguousarray(j.transpose(2, 0, 1)).astype(np.float32), p, ry, rx)
            outs.append(np.clip(np.rint(v), 0, 255).astype(np.float32) if p.do_resize else v)
        if self.sparse and p.do_resize:
            fl, va = _sparse_flow(flow, valid, p, ry, rx, ht1, wd1)
        elif self.sparse:
            fl, va = flow[:, ry][:, :, rx], valid[ry][:, rx]
        else:
            fl = _sample_bilinear(flow, p, ry, rx)
            if p.do_resize:  # the reference's flow * [sx, sy] is a float64 product, rounded once afterwards
                fl = (fl.astype(np.float64) * np.array([p.scale_x, p.scale_y])[:, None, None]).astype(np.float32)
        fl = np.array(fl, np.float32)
        if p.hflip:
            fl[0] = -fl[0]
        if p.vflip:
            fl[1] = -fl[1]
        if not self.sparse:
            va = ((np.abs(fl[0]) < 1000) & (np.abs(fl[1]) < 1000)).astype(np.float32)
        return outs[0], outs[1], fl, np.asarray(va, np.float32)

    def _call(self, img1, img2, flow, valid):
        img1, img2 = np.ascontiguousarray(img1), np.ascontiguousarray(img2)
        if img1.dtype != np.uint8 or img2.dtype != np.uint8 or img1.ndim != 3 or img1.shape != img2.shape:
            raise ValueError("augmentor: img1 and img2 must be equal (H, W, 3) uint8 arrays")
        ht, wd = img1.shape[:2]
        p = self.sample(ht, wd)
        self._validate(p, ht, wd)
        fl = np.ascontiguousarray(np.asarray(flow, np.float32).transpose(2, 0, 1))
        va = np.asarray(valid, np.float32) if self.sparse else None
        o1, o2, of, ov = self._augment_numpy(img1, img2, fl, va, p)
        hwc = lambda a, dt: np.ascontiguousarray(a.transpose(1, 2, 0)).astype(dt)  # noqa: E731
        return hwc(o1, np.uint8), hwc(o2, np.uint8), hwc(of, np.float32), ov


class FlowAugmentor(_AugmentorBase):
    """The dense augmentor (reference augmentor.py:43-172). ``__call__(img1, img2, flow)`` takes HWC uint8 frames and
    an (H, W, 2) fp32 flow and returns the crops as (ch, cw, 3) uint8 x 2 and (ch, cw, 2) float32 (the reference's
    float64 product already rounded to the fp32 its dataset casts it to, dataset.py:114)."""

    sparse = False

    def __init__(self, crop_size: Tuple[int, int], min_scale: float = -0.2, max_scale: float = 0.5,
                 do_flip: bool = True) -> None:
        # spatial augmentation params
        self.crop_size = crop_size
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        # flip augmentation params
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        # photometric augmentation params: (brightness, contrast, saturation, hue) of the reference's ColorJitter
        self._jitter = (0.4, 0.4, 0.4, 0.5 / 3.14)
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = 0.5

    def sample(self, ht: int, wd: int) -> AugmentParams:
        """One sample's decisions for an (ht, wd) source. ``np.random`` draws, in the reference's order
        (augmentor.py:78, 98-104, 118-128, 142-153): rand (asymmetric); rand (eraser), then if it erases randint(1, 3)
        and per rectangle randint(0, wd), randint(0, ht), randint(50, 100) x 2; uniform (scale); rand (stretch), then if
        it stretches uniform x 2; rand (resize); with ``do_flip`` rand (h-flip), rand (v-flip); randint (y0), randint
        (x0). Colour draws (torch's global generator): one ``ColorJitter.get_params`` draw, two when asymmetric, in
        torchvision's documented order -- unverified, see the module docstring."""
        asym = bool(np.random.rand() < self.asymmetric_color_aug_prob)
        order1, factors1 = self._draw_color()
        order2, factors2 = self._draw_color() if asym else (order1, factors1)
        rects = self._draw_eraser(ht, wd)
        ch, cw = self.crop_size
        min_scale = np.maximum((ch + 8) / float(ht), (cw + 8) / float(wd))
        scale = 2 ** np.random.uniform(self.min_scale, self.max_scale)
        scale_x = scale_y = scale
        if np.random.rand() < self.stretch_prob:
            scale_x *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
            scale_y *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
        scale_x = float(np.clip(scale_x, min_scale, None))
        scale_y = float(np.clip(scale_y, min_scale, None))
        p = AugmentParams(order1, factors1, order2, factors2, asym, rects,
                          do_resize=bool(np.random.rand() < self.spatial_aug_prob), scale_x=scale_x, scale_y=scale_y)
        if self.do_flip:
            p.hflip = bool(np.random.rand() < self.h_flip_prob)
            p.vflip = bool(np.random.rand() < self.v_flip_prob)
        ht1, wd1 = resized_size(ht, wd, p)
        p.y0 = int(np.random.randint(0, ht1 - ch))
        p.x0 = int(np.random.randint(0, wd1 - cw))
        return p

    def __call__(self, img1: np.ndarray, img2: np.ndarray, flow: np.ndarray):
        return self._call(img1, img2, flow, None)[:3]


class SparseFlowAugmentor(_AugmentorBase):
    """The sparse augmentor (reference augmentor.py:175-324): always a symmetric colour draw, one scale, a horizontal
    flip only with ``do_flip``, the flow and valid maps resampled by nearest landing (``resize_sparse_flow_map``).
    ``__call__(img1, img2, flow, valid)`` returns (ch, cw, 3) uint8 x 2, (ch, cw, 2) float32 and (ch, cw) float32."""

    sparse = True

    def __init__(self, crop_size: Tuple[int, int], min_scale: float = -0.2, max_scale: float = 0.5,
                 do_flip: bool = False) -> None:
        # spatial augmentation params
        self.crop_size = crop_size
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        # flip augmentation params
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        # photometric augmentation params
        self._jitter = (0.3, 0.3, 0.3, 0.3 / 3.14)
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = 0.5

    def sample(self, ht: int, wd: int) -> AugmentParams:
        """One sample's decisions. ``np.random`` draws, in the reference's order (augmentor.py:217-223, 274-301): rand
        (eraser), then if it erases randint(1, 3) and four randints per rectangle; uniform (scale); rand (resize); with
        ``do_flip`` rand (h-flip); randint (y0, margin 20), randint (x0, margin 50), both clipped into the frame. One
        symmetric colour draw from torch's generator (documented torchvision order, unverified)."""
        order, factors = self._draw_color()
        rects = self._draw_eraser(ht, wd)
        ch, cw = self.crop_size
        min_scale = np.maximum((ch + 1) / float(ht), (cw + 1) / float(wd))
        scale = 2 ** np.random.uniform(self.min_scale, self.max_scale)
        scale = float(np.clip(scale, min_scale, None))
        p = AugmentParams(order, factors, order, factors, False, rects,
                          do_resize=bool(np.random.rand() < self.spatial_aug_prob), scale_x=scale, scale_y=scale)
        if self.do_flip:
            p.hflip = bool(np.random.rand() < 0.5)
        ht1, wd1 = resized_size(ht, wd, p)
        margin_y, margin_x = 20, 50
        y0 = np.random.randint(0, ht1 - ch + margin_y)
        x0 = np.random.randint(-margin_x, wd1 - cw + margin_x)
        p.y0 = int(np.clip(y0, 0, ht1 - ch))
        p.x0 = int(np.clip(x0, 0, wd1 - cw))
        return p

    def __call__(self, img1: np.ndarray, img2: np.ndarray, flow: np.ndarray, valid: np.ndarray):
        return self._call(img1, img2, flow, valid)
