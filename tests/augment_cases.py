"""A NumPy restatement of the augmentation arithmetic (include/oflow.h, oflow_augment_*) and the case table of the
augmentation tests. The restatement is written from the specification, independently of the product code
(data/augmentor.py, csrc/augment.hip), and follows the reference's own sequence literally: jitter the whole frames,
erase, resize the whole frame, flip, crop -- where the product computes only the crop's pixels by a gather. NumPy only;
every input comes from a seeded generator or is written out, so every process sees the same cases."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np

from data.augmentor import AugmentParams

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------- colour, as Pillow's C
def luma(rgb: np.ndarray) -> np.ndarray:
    """ImagingConvert RGB -> L of (..., 3) uint8: int32 levels."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.int32)


def blend(degenerate: np.ndarray, image: np.ndarray, factor: float) -> np.ndarray:
    """ImagingBlend(degenerate, image, factor) on integer levels: fp32, one product and one sum."""
    alpha = F32(factor)
    d = degenerate.astype(F32)
    x = image.astype(F32)
    diff = x - d  # exact
    prod = (alpha * diff).astype(F32)
    temp = (d + prod).astype(F32)
    if alpha >= 0 and alpha <= 1:
        return temp.astype(np.uint8)  # truncation; the value is inside [0, 255]
    out = np.trunc(temp)
    out[temp <= 0] = 0
    out[temp >= 255] = 255
    return out.astype(np.uint8)


def brightness(img: np.ndarray, f: float) -> np.ndarray:
    return blend(np.zeros_like(img), img, f)


def contrast(img: np.ndarray, f: float) -> np.ndarray:
    """ImageEnhance.Contrast: the degenerate image is the grey level int(mean(L) + 0.5) of THIS image."""
    grey = luma(img)
    mean = int(grey.sum(dtype=np.int64)) / grey.size
    return blend(np.full_like(img, int(mean + 0.5)), img, f)


def saturation(img: np.ndarray, f: float) -> np.ndarray:
    return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """Pillow's rgb2hsv on (N, 3) uint8."""
    c = rgb.astype(np.int32)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    out = np.zeros_like(c)
    out[:, 2] = maxc
    m = np.nonzero(maxc != minc)[0]
    r, g, b, mx, mn = r[m], g[m], b[m], maxc[m], minc[m]
    cr = (mx - mn).astype(F32)
    s = (cr / mx.astype(F32)).astype(F32)
    rc = ((mx - r).astype(F32) / cr).astype(F32)
    gc = ((mx - g).astype(F32) / cr).astype(F32)
    bc = ((mx - b).astype(F32) / cr).astype(F32)
    h = np.empty(len(m), F32)
    is_r = r == mx
    is_g = ~is_r & (g == mx)
    is_b = ~is_r & ~is_g
    h[is_r] = (bc - gc)[is_r]
    h[is_g] = ((2.0 + rc.astype(F64)) - bc.astype(F64)).astype(F32)[is_g]
    h[is_b] = ((4.0 + gc.astype(F64)) - rc.astype(F64)).astype(F32)[is_b]
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    out[m, 0] = np.clip(np.trunc(h.astype(F64) * 255.0), 0, 255).astype(np.int32)
    out[m, 1] = np.clip(np.trunc(s.astype(F64) * 255.0), 0, 255).astype(np.int32)
    return out.astype(np.uint8)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """Pillow's hsv2rgb on (N, 3) uint8."""
    h, s, v = (hsv[:, k].astype(np.int32) for k in range(3))
    hf = h.astype(F64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(F32).astype(F64)
    fs = (s.astype(F64) / 255.0).astype(F32).astype(F64)
    vd = v.astype(F64)

    def rnd(x):  # C round() for x >= 0, then CLIP8
        return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)

    p = rnd(vd * (1.0 - fs))
    q = rnd(vd * (1.0 - fs * f))
    t = rnd(vd * (1.0 - fs * (1.0 - f)))
    sextant = i.astype(np.int64) % 6
    out = np.empty((len(h), 3), np.int32)
    for k, (c0, c1, c2) in enumerate(((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))):
        m = sextant == k
        out[m, 0], out[m, 1], out[m, 2] = c0[m], c1[m], c2[m]
    grey = s == 0
    out[grey] = v[grey][:, None]
    return out.astype(np.uint8)


def hue(img: np.ndarray, f: float) -> np.ndarray:
    """torchvision's PIL adjust_hue: H += uint8(f * 255) with wrap-around, also for f == 0."""
    hsv = rgb_to_hsv(img.reshape(-1, 3)).astype(np.int32)
    hsv[:, 0] = (hsv[:, 0] + int(np.trunc(f * 255.0))) % 256
    return hsv_to_rgb(hsv.astype(np.uint8)).reshape(img.shape)


OPS = (brightness, contrast, saturation, hue)  # torchvision's fn_idx


def color_jitter(img: np.ndarray, order, factors) -> np.ndarray:
    for op in order:
        img = OPS[op](img, factors[op])
    return img


# ------------------------------------------------------------------------------------------- geometry
def resize_linear(src: np.ndarray, sx: float, sy: float) -> np.ndarray:
    """INTER_LINEAR of an (H, W, C) fp32 array to round_half_even(size * scale), unrounded fp32 result: horizontal pass
    into rows, then the vertical pass."""
    ht, wd = src.shape[:2]
    ht1, wd1 = int(round(ht * sy)), int(round(wd * sx))

    def taps(n_out, n_in, scale):
        i0 = np.empty(n_out, np.int64)
        al = np.empty(n_out, F32)
        inv = 1.0 / scale
        for d in range(n_out):
            f = F32((d + 0.5) * inv - 0.5)
            i = int(np.floor(f))
            a = F32(f - F32(i))
            if i < 0:
                i, a = 0, F32(0)
            if i >= n_in - 1:
                i, a = n_in - 1, F32(0)
            i0[d], al[d] = i, a
        return i0, np.minimum(i0 + 1, n_in - 1), al

    x0, x1, ax = taps(wd1, wd, sx)
    y0, y1, ay = taps(ht1, ht, sy)
    ax = ax[None, :, None]
    rows = (src[:, x0] * (F32(1) - ax)).astype(F32) + (src[:, x1] * ax).astype(F32)  # (H, W1, C)
    ay = ay[:, None, None]
    return ((rows[y0] * (F32(1) - ay)).astype(F32) + (rows[y1] * ay).astype(F32)).astype(F32)


def resize_sparse_flow_map(flow: np.ndarray, valid: np.ndarray, fx: float, fy: float):
    """(H, W, 2) fp32 flow and (H, W) valid -> the scattered maps; sources are written in row-major order, one by one,
    so the last one stays."""
    ht, wd = valid.shape
    ht1, wd1 = int(round(ht * fy)), int(round(wd * fx))
    flow_img = np.zeros((ht1, wd1, 2), F32)
    valid_img = np.zeros((ht1, wd1), F32)
    reached = np.zeros((ht1, wd1), np.int64)
    for y in range(ht):
        yy = int(np.rint(float(F32(y)) * fy))
        for x in np.nonzero(valid[y] >= 1)[0]:
            xx = int(np.rint(float(F32(x)) * fx))
            if 0 < xx < wd1 and 0 < yy < ht1:
                flow_img[yy, xx, 0] = F32(float(flow[y, x, 0]) * fx)
                flow_img[yy, xx, 1] = F32(float(flow[y, x, 1]) * fy)
                valid_img[yy, xx] = 1
                reached[yy, xx] += 1
    return flow_img, valid_img, reached


def augment_sample(sparse: bool, crop, img1, img2, flow, valid, p: AugmentParams):
    """One sample, in the reference's order. img*: (H, W, 3) uint8; flow: (2, H, W) fp32; valid: (H, W) fp32 or None.
    Returns CHW fp32 (img1, img2, flow, valid) and, for a resized sparse sample, the reach count map (else None)."""
    ht, wd = img1.shape[:2]
    # colour (augmentor.py:72-90): asymmetric = each frame its own draw; symmetric = the frames stacked as one image
    if p.asymmetric:
        img1 = color_jitter(img1, p.order1, p.factors1)
        img2 = color_jitter(img2, p.order2, p.factors2)
    else:
        stack = color_jitter(np.concatenate([img1, img2], axis=0), p.order1, p.factors1)
        img1, img2 = stack[:ht], stack[ht:]
    # eraser (92-107)
    if len(p.rects):
        img2 = img2.copy()
        sums = img2.reshape(-1, 3).astype(np.int64).sum(axis=0)
        mean_color = np.array([int(int(v) / float(ht * wd)) for v in sums], np.uint8)
        for x0, y0, dx, dy in p.rects:
            img2[y0 : y0 + dy, x0 : x0 + dx, :] = mean_color
    # spatial (109-159 / 264-310)
    a1, a2 = img1.astype(F32), img2.astype(F32)
    fl = np.ascontiguousarray(flow.transpose(1, 2, 0))
    va, reached = valid, None
    if p.do_resize:
        a1 = np.clip(np.rint(resize_linear(a1, p.scale_x, p.scale_y)), 0, 255).astype(F32)
        a2 = np.clip(np.rint(resize_linear(a2, p.scale_x, p.scale_y)), 0, 255).astype(F32)
        if sparse:
            fl, va, reached = resize_sparse_flow_map(fl, valid, p.scale_x, p.scale_y)
        else:
            fl = (resize_linear(fl, p.scale_x, p.scale_y).astype(F64) * np.array([p.scale_x, p.scale_y])).astype(F32)
    if p.hflip:
        a1, a2, fl = a1[:, ::-1], a2[:, ::-1], fl[:, ::-1] * np.array([-1.0, 1.0], F32)
        if sparse:
            va = va[:, ::-1]
    if p.vflip:
        a1, a2, fl = a1[::-1], a2[::-1], fl[::-1] * np.array([1.0, -1.0], F32)
    ch, cw = crop
    assert 0 <= p.y0 and p.y0 + ch <= a1.shape[0] and 0 <= p.x0 and p.x0 + cw <= a1.shape[1], "case leaves the frame"
    win = (slice(p.y0, p.y0 + ch), slice(p.x0, p.x0 + cw))
    a1, a2, fl = a1[win], a2[win], fl[win].astype(F32)
    if sparse:
        va = va[win].astype(F32)
    else:
        va = ((np.abs(fl[..., 0]) < 1000) & (np.abs(fl[..., 1]) < 1000)).astype(F32)
    chw = lambda a: np.ascontiguousarray(a.transpose(2, 0, 1))  # noqa: E731
    return chw(a1), chw(a2), chw(fl), np.ascontiguousarray(va), reached


# ------------------------------------------------------------------------------------------- inputs and cases
SIZE_A, CROP_A = (120, 160), (64, 96)
SIZE_B, CROP_B = (113, 171), (48, 80)


def flat_frame(ht: int, wd: int, seed: int) -> np.ndarray:
    """Blocks of constant colour, a third of them grey (max == min), with a few saturated primaries."""
    rng = np.random.default_rng(seed)
    img = np.zeros((ht, wd, 3), np.uint8)
    k = 0
    for y in range(0, ht, 16):
        for x in range(0, wd, 16):
            c = rng.integers(0, 256, 3)
            if k % 3 == 0:
                c[:] = c[0]
            elif k % 7 == 0:
                c = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)][k % 4])
            img[y : y + 16, x : x + 16] = c
            k += 1
    return img


@dataclass
class Case:
    name: str
    sparse: bool
    size: Tuple[int, int]
    crop: Tuple[int, int]
    params: List[AugmentParams]
    flat: bool = False  # frame 1 of sample 0 is the flat-block frame, frame 2 a shifted copy of it
    big_flow: bool = False  # flow holds values >= 1000
    seed: int = 0


def make_inputs(case: Case):
    """(img1, img2, flow, valid): uint8 (B, H, W, 3) x 2, fp32 (B, 2, H, W), fp32 (B, H, W) (~30 % ones)."""
    ht, wd = case.size
    b = len(case.params)
    rng = np.random.default_rng(1000 + case.seed)
    img1 = rng.integers(0, 256, (b, ht, wd, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (b, ht, wd, 3), dtype=np.uint8)
    if case.flat:
        img1[0] = flat_frame(ht, wd, case.seed)
        img2[0] = np.roll(img1[0], (5, 9), axis=(0, 1))
    flow = (rng.standard_normal((b, 2, ht, wd)) * 6).astype(F32)
    if case.big_flow:
        flow[:, 0, 10:40, 20:70] = 1000.0
        flow[:, 1, 50:90, 60:120] = -1234.5
        flow[:, 0, 70:75, 5:9] = 999.99
    valid = (rng.random((b, ht, wd)) < 0.3).astype(F32)
    return img1, img2, flow, valid


FAC = (1.3, 0.7, 1.2, 0.1)
FAC2 = (0.8, 1.25, 0.65, -0.07)
LO_D = (0.6, 0.6, 0.6, -0.5 / 3.14)
HI_D = (1.4, 1.4, 1.4, 0.5 / 3.14)
LO_S = (0.7, 0.7, 0.7, -0.3 / 3.14)
HI_S = (1.3, 1.3, 1.3, 0.3 / 3.14)


def P(order=(0, 1, 2, 3), fac=FAC, order2=None, fac2=None, asym=False, **kw) -> AugmentParams:
    return AugmentParams(order1=order, factors1=fac, order2=order2 if order2 is not None else order,
                         factors2=fac2 if fac2 is not None else fac, asymmetric=asym, **kw)


def _cases() -> List[Case]:
    A, CA, B, CB = SIZE_A, CROP_A, SIZE_B, CROP_B
    inside = (30, 20, 60, 55)  # inside frame and crop
    over_edge_a = (130, 90, 80, 70)  # crosses the right and the bottom edge of 120 x 160
    off_crop_a = (100, 70, 50, 50)  # inside the frame, outside a crop at (0, 0) of 64 x 96
    # the min_scale clip of FlowAugmentor at 120 x 160 / 64 x 96: max(72 / 120, 104 / 160)
    clip = float(np.maximum((64 + 8) / 120.0, (96 + 8) / 160.0))
    # 160 * 1.36 = 217.6 -> 218 columns, 120 * 1.23 = 147.6 -> 148 rows: the last output row / column map past
    # source index n - 1.5, so a crop that touches them hits the i >= n - 1 clamp; a crop at 0 hits i < 0
    up = dict(do_resize=True, scale_x=1.36, scale_y=1.23)
    cases = [
        # identity spatial, contrast first / second / third / last
        Case("contrast_first", False, A, CA, [P((1, 0, 2, 3), y0=10, x0=20)], seed=1),
        Case("contrast_second", False, A, CA, [P((0, 1, 2, 3), y0=0, x0=0)], seed=2),
        Case("contrast_third", False, B, CB, [P((3, 2, 1, 0), y0=65, x0=91)], flat=True, seed=3),
        Case("contrast_last", False, A, CA, [P((2, 3, 0, 1), y0=56, x0=64)], flat=True, seed=4),
        # the same factors drawn once for the stacked pair / once per frame: the contrast mean differs
        Case("symmetric", False, A, CA, [P((0, 1, 2, 3), y0=7, x0=3)], seed=5),
        Case("asymmetric", False, A, CA, [P((0, 1, 2, 3), asym=True, y0=7, x0=3)], seed=5),
        Case("asymmetric_two_draws", False, B, CB, [P((2, 0, 3, 1), FAC, (1, 3, 0, 2), FAC2, asym=True, y0=1, x0=2)],
             flat=True, seed=6),
        # every factor at both ends of its range (dense and sparse ranges), hue negative and zero
        Case("factors_low", False, A, CA, [P((0, 1, 2, 3), LO_D, y0=3, x0=5), P((3, 1, 0, 2), LO_S, y0=0, x0=0)],
             flat=True, seed=7),
        Case("factors_high", False, A, CA, [P((1, 2, 3, 0), HI_D, y0=3, x0=5), P((2, 0, 1, 3), HI_S, y0=50, x0=60)],
             flat=True, seed=8),
        Case("hue_zero_unit_factors", False, B, CB, [P((0, 1, 2, 3), (1.0, 1.0, 1.0, 0.0), y0=20, x0=30)], flat=True,
             seed=9),
        # eraser: 1 and 2 rectangles; one over the right / bottom edge; one that misses the crop
        Case("one_rect", False, A, CA, [P(rects=(inside,), y0=10, x0=10)], seed=10),
        Case("two_rects_edge", False, A, CA, [P(rects=(inside, over_edge_a), y0=56, x0=64)], seed=11),
        Case("rect_off_crop", False, A, CA, [P(rects=(off_crop_a,), y0=0, x0=0)], seed=12),
        Case("rect_resized", False, B, CB, [P(rects=((60, 40, 99, 50), (0, 100, 50, 99)), do_resize=True, scale_x=0.83,
                                              scale_y=0.91, y0=40, x0=55)], flat=True, seed=13),
        # scales: the min_scale clip, < 1, > 1, anisotropic
        Case("scale_min_clip", False, A, CA, [P(do_resize=True, scale_x=clip, scale_y=clip, y0=14, x0=8)], seed=14),
        Case("scale_down_aniso", False, A, CA, [P(do_resize=True, scale_x=0.8, scale_y=0.9, y0=20, x0=16)], seed=15),
        Case("scale_up_origin", False, A, CA, [P(**up, y0=0, x0=0)], seed=16),
        Case("scale_up_last_row_col", False, A, CA, [P(**up, y0=148 - 64, x0=218 - 96)], seed=17),
        Case("scale_odd_size", False, B, CB, [P(do_resize=True, scale_x=1.07, scale_y=0.77, y0=87 - 48, x0=183 - 80)],
             flat=True, seed=18),
        # flips
        Case("hflip", False, A, CA, [P(hflip=True, y0=5, x0=6)], seed=19),
        Case("vflip", False, A, CA, [P(vflip=True, y0=5, x0=6)], seed=20),
        Case("both_flips_resized", False, B, CB, [P(hflip=True, vflip=True, rects=((100, 60, 70, 70),), do_resize=True,
                                                    scale_x=0.9, scale_y=1.1, y0=124 - 48, x0=0)], seed=21),
        # a batch mixing all of it
        Case("batch3", False, A, CA, [
            P((1, 0, 2, 3), FAC, rects=(inside,), do_resize=True, scale_x=0.75, scale_y=0.7, hflip=True, y0=3, x0=9),
            P((3, 0, 1, 2), FAC, (0, 2, 1, 3), FAC2, asym=True, rects=(inside, over_edge_a), vflip=True, y0=56, x0=64),
            P((2, 1, 3, 0), HI_D, **up, hflip=True, vflip=True, y0=84, x0=122)], flat=True, seed=22),
        # flow values >= 1000: the dense valid mask has zeros
        Case("big_flow", False, A, CA, [P(do_resize=True, scale_x=0.95, scale_y=1.05, y0=10, x0=12), P(y0=30, x0=40)],
             big_flow=True, seed=23),
        # sparse: resize_sparse_flow_map at 0.87 (many shared pixels), no resize, the crop clipped at both margins
        Case("sparse_087", True, A, CA, [P(fac=HI_S, rects=(inside,), do_resize=True, scale_x=0.87, scale_y=0.87,
                                           y0=20, x0=30)], seed=24),
        Case("sparse_no_resize", True, A, CA, [P(fac=LO_S, y0=56, x0=0), P(fac=FAC2, hflip=True, y0=0, x0=64)],
             seed=25),
        Case("sparse_margins", True, B, CB, [
            P(do_resize=True, scale_x=1.1, scale_y=1.1, y0=0, x0=0),
            P(do_resize=True, scale_x=1.1, scale_y=1.1, hflip=True, rects=(over_edge_a,), y0=124 - 48, x0=188 - 80)],
            flat=True, seed=26),
        Case("sparse_down_flip", True, B, CB, [P(do_resize=True, scale_x=0.6, scale_y=0.6, hflip=True, y0=68 - 48,
                                                 x0=103 - 80)], seed=27),
    ]
    return cases


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@lru_cache(maxsize=None)
def expected(name: str):
    """(inputs, outputs, reach maps) of a case: the outputs as (B, ...) fp32 arrays. Computed once per process and
    shared by the tests: treat as read-only."""
    case = BY_NAME[name]
    inputs = make_inputs(case)
    outs, reach = [], []
    for i, p in enumerate(case.params):
        *o, r = augment_sample(case.sparse, case.crop, inputs[0][i], inputs[1][i], inputs[2][i],
                               inputs[3][i] if case.sparse else None, p)
        outs.append(o)
        reach.append(r)
    stacked = tuple(np.stack([o[k] for o in outs]) for k in range(4))
    for a in inputs + stacked:
        a.setflags(write=False)
    return inputs, stacked, reach
