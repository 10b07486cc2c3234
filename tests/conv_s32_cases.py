"""Case tables and float64 restatements for the update-block convolution tests (csrc/conv_s32.hip on every tile the
dispatcher picks, csrc/update_fused.hip): the plain convolution with its sum |x||w| bound, the SepConvGRU half-step
(update.py:91-97) in its full 384-channel form and in the hoisted form the split path runs ([h | motion | flow] plus
the loop-invariant context addend), and the three FusedUpdate elementwise operations. PyTorch on the CPU or the GPU
(float64 either way); inputs come from seeded ``torch.Generator``s. tests/test_conv_s32_cases_host.py pins these
restatements against the nn.Modules; tests/test_gpu_conv_s32_tiles.py and tests/test_gpu_update_fused.py compare the
kernels with them. Not a test module."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------- the dispatcher's leaves
# oflow_exp_last_conv_leaf() (csrc/conv_s32.hip record_leaf): 4 bits per template parameter from bit 0, BN 8 bits
_LEAF_FIELDS = (("kh", 0, 4), ("kw", 4, 4), ("bn", 8, 8), ("wm", 16, 4), ("wn", 20, 4), ("epi", 24, 4), ("ty", 28, 4),
                ("ain", 32, 4), ("breg", 36, 4), ("bd", 40, 4))


class Leaf(NamedTuple):
    """One instantiation conv_s32_kernel<KH, KW, BN, WM, WN, EPI, TY, AIN, BREG, BD>."""
    kh: int
    kw: int
    bn: int
    wm: int
    wn: int
    epi: int
    ty: int
    ain: int
    breg: int
    bd: int


def decode_leaf(v: int) -> Leaf:
    return Leaf(*(((int(v) >> shift) & ((1 << bits) - 1)) for _, shift, bits in _LEAF_FIELDS))


# leaf name -> (BN, WM, WN, TY, BREG, BD) as launch_bn() / dispatch_conv() instantiate it on S32 input
LEAVES = {
    "small": (64, 2, 2, 2, 0, 2),     # small-grid tiles: 2 rows x 32 columns, 64-channel blocks
    "lds128": (128, 2, 2, 4, 0, 2),   # LDS-staged weights, 4 x 32 tiles
    "lds96": (96, 4, 1, 4, 0, 2),
    "lds64": (64, 2, 2, 4, 0, 2),
    "lds32": (32, 4, 1, 4, 0, 2),
    "breg128": (128, 1, 4, 4, 1, 1),  # register-direct weights (d_wfrag)
    "breg64": (64, 2, 2, 4, 1, 1),    # 3x3 only
    "breg32": (32, 4, 1, 4, 1, 1),    # 3x3 only
}
# the block_n a call asks for to reach the leaf (the small-grid tiles: any block >= 64 whose n_pad is a multiple of 64)
LEAF_BLOCK_N = {"small": 64, "lds128": 128, "lds96": 96, "lds64": 64, "lds32": 32, "breg128": 128, "breg64": 64,
                "breg32": 32}
KERNELS = [(1, 1), (3, 3), (1, 5), (5, 1)]


def expected_leaf(kh: int, kw: int, epi: int, name: str) -> Leaf:
    bn, wm, wn, ty, breg, bd = LEAVES[name]
    return Leaf(kh, kw, bn, wm, wn, epi, ty, 0, breg, bd)


def epi0_leaves(kh: int, kw: int):
    """The leaves launch_bn<KH, KW, 0> can reach on S32 input without instance-norm partials."""
    names = ["small", "lds128", "lds96", "lds64", "lds32"]
    if kh * kw > 1:
        names.append("breg128")
    if (kh, kw) == (3, 3):
        names += ["breg64", "breg32"]
    return names


GRU_LEAVES = ["small", "lds128", "breg128"]

# output grids (B, H, W): the smallest at which a 4 x 32 / 2 x 32 tile kernel can still go wrong
SHAPE_RAGGED = (2, 9, 37)    # ragged rows and columns, two tile columns, a batch stride
SHAPE_SUBTILE = (1, 3, 31)   # smaller than one tile both ways
SHAPE_COLUMNS = (3, 5, 64)   # whole tile columns, ragged rows, three images
SHAPE_ROW = (2, 1, 33)       # a 5x1 halo wholly outside the image
SHAPE_NARROW = (1, 8, 2)     # a 1x5 halo mostly outside the image
# epilogue 0: (shape, input channels, output channels). Input groups: 12 (even), 11 (odd: the two-group body's
# one-group tail), 1; outputs N == n_pad for every block (384 = lcm of 128 and 96), 126 (N < n_pad) and 2 (the flow
# head's: 2 of 32)
EPI0_CASES = [
    (SHAPE_RAGGED, 352, 126),
    (SHAPE_SUBTILE, 32, 2),
    (SHAPE_COLUMNS, 384, 384),
    (SHAPE_ROW, 32, 126),
    (SHAPE_NARROW, 352, 2),
]
# GRU half-steps: (shape, gru_channels, motion + flow channels of the hoisted input)
# full-form input [h | inp | x] has ch + ch + xc channels: 384 (12 groups) / 352 (11) at ch 128, 160 (5) at ch 64;
# the hoisted input [h | x] 256 (8) / 224 (7) / 96 (3)
GRU_CASES = [
    (SHAPE_RAGGED, 128, 128),
    (SHAPE_SUBTILE, 64, 32),
    (SHAPE_COLUMNS, 128, 96),
    (SHAPE_ROW, 64, 32),
    (SHAPE_NARROW, 128, 128),
]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------ plain convolution
def conv_ref(x, w, b, kh: int, kw: int):
    """'same' convolution in float64 and its absolute-product sum (the kernels' error scale): (y, sum |x||w|)."""
    pad = (kh // 2, kw // 2)
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=pad)
    bound = F.conv2d(x.double().abs(), w.double().abs(), None, padding=pad)
    return y, bound


def conv_tol(bound, ref=None):
    """The project's convolution bound: 2e-6 * sum |x||w| + 1e-6, plus 2^-22 |ref| for a value read back from S32."""
    tol = 2e-6 * bound + 1e-6
    return tol if ref is None else tol + 2.0 ** -22 * ref.abs()


def epi0_operands(kh: int, kw: int, cin: int, n: int, shape, seed: int):
    """fp32 CPU operands of an epilogue-0 case: x ~ 1.5 N(0, 1), w ~ N(0, 1) / sqrt(fan-in), bias ~ N(0, 1)."""
    g = gen(seed)
    b, h, w = shape
    x = torch.randn(b, cin, h, w, generator=g) * 1.5
    wt = torch.randn(n, cin, kh, kw, generator=g) / math.sqrt(cin * kh * kw)
    bias = torch.randn(n, generator=g)
    return x, wt, bias


# ---------------------------------------------------------------------------------------- SepConvGRU half-step
class GruHalf(NamedTuple):
    z: torch.Tensor       # sigmoid(convz([h | x]))
    r: torch.Tensor       # sigmoid(convr([h | x]))
    rh: torch.Tensor      # r * h
    q: torch.Tensor       # tanh(convq([r*h | x]))
    h: torch.Tensor       # (1 - z) h + z q
    pre_z: torch.Tensor   # the three pre-activation values
    pre_r: torch.Tensor
    pre_q: torch.Tensor


def gru_half_full(h, x, wz, wr, wq, bz, br, bq, rh=None, z=None, h_conv=None) -> GruHalf:
    """update.py:91-97 in float64: hx = [h | x]; z = sigmoid(convz(hx)); r = sigmoid(convr(hx));
    q = tanh(convq([r*h | x])); h' = (1 - z) h + z q. Kernel (1, 5) or (5, 1) from the weights' shape.
    ``rh`` / ``z``: values to use in place of the computed r*h / z for the second half (what a kernel under test stored
    between its two launches), so that each launch is compared on the operands it actually read. ``h_conv``: the copy
    of h the z / r convolutions read where it differs from the h of r*h and of the blend (the split path keeps an fp32
    master h beside its 22-bit S32 copy)."""
    kh, kw = wz.shape[-2:]
    pad = (kh // 2, kw // 2)
    d = lambda t: None if t is None else t.double()
    h, x = h.double(), x.double()
    hx = torch.cat([h if h_conv is None else h_conv.double(), x], dim=1)
    pre_z = F.conv2d(hx, d(wz), d(bz), padding=pad)
    pre_r = F.conv2d(hx, d(wr), d(br), padding=pad)
    zc, r = torch.sigmoid(pre_z), torch.sigmoid(pre_r)
    rhc = r * h
    rh_in = rhc if rh is None else rh.double()
    z_in = zc if z is None else z.double()
    pre_q = F.conv2d(torch.cat([rh_in, x], dim=1), d(wq), d(bq), padding=pad)
    q = torch.tanh(pre_q)
    return GruHalf(zc, r, rhc, q, (1 - z_in) * h + z_in * q, pre_z, pre_r, pre_q)


def hoist_split(w, ch: int):
    """A gate's weight over [h | inp | x] -> (its [h | x] columns, its inp columns)."""
    return torch.cat([w[:, :ch], w[:, 2 * ch:]], dim=1), w[:, ch:2 * ch]


def gru_context_addend(inp, wz, wr, wq, bz, br, bq, ch: int):
    """The loop-invariant context term W_inp * inp + bias of the three gates, (B, 3 ch, H, W) = z | r | q, float64."""
    kh, kw = wz.shape[-2:]
    w_inp = torch.cat([hoist_split(w, ch)[1] for w in (wz, wr, wq)]).double()
    return F.conv2d(inp.double(), w_inp, torch.cat([bz, br, bq]).double(), padding=(kh // 2, kw // 2))


def gru_half_hoisted(h, x, addend, wz, wr, wq, rh=None, z=None, h_conv=None) -> GruHalf:
    """The same half-step as the split path runs it: convolutions without bias over [h | x] (x = motion | flow; the
    weights' [h | x] columns) plus ``addend`` = gru_context_addend(...) before the gate functions; ``addend`` None:
    no context term at all (the gates of the bare convolution). ``rh``, ``z``, ``h_conv``: as gru_half_full's."""
    kh, kw = wz.shape[-2:]
    pad = (kh // 2, kw // 2)
    h, x = h.double(), x.double()
    ch = h.shape[1]
    a = addend.double() if addend is not None else torch.zeros(1, 3 * ch, 1, 1, dtype=torch.float64, device=h.device)
    hx = torch.cat([h if h_conv is None else h_conv.double(), x], dim=1)
    pre_z = F.conv2d(hx, wz.double(), padding=pad) + a[:, :ch]
    pre_r = F.conv2d(hx, wr.double(), padding=pad) + a[:, ch:2 * ch]
    zc, r = torch.sigmoid(pre_z), torch.sigmoid(pre_r)
    rhc = r * h
    rh_in = rhc if rh is None else rh.double()
    z_in = zc if z is None else z.double()
    pre_q = F.conv2d(torch.cat([rh_in, x], dim=1), wq.double(), padding=pad) + a[:, 2 * ch:]
    q = torch.tanh(pre_q)
    return GruHalf(zc, r, rhc, q, (1 - z_in) * h + z_in * q, pre_z, pre_r, pre_q)


def gru_operands(kh: int, kw: int, ch: int, xc: int, shape, seed: int, wstd: float = 0.03):
    """fp32 CPU operands of a GRU half-step at the scales of test_gpu_conv_s32.py's GRU tests: h = tanh(N(0, 1)),
    inp = relu(N(0, 1)), x ~ N(0, 1), weights ~ wstd N(0, 1) over [h | inp | x], biases ~ N(0, 1).
    Returns (h, inp, x, (wz, wr, wq), (bz, br, bq))."""
    g = gen(seed)
    b, hh, ww = shape
    h = torch.tanh(torch.randn(b, ch, hh, ww, generator=g))
    inp = torch.relu(torch.randn(b, ch, hh, ww, generator=g))
    x = torch.randn(b, xc, hh, ww, generator=g)
    ws = tuple(torch.randn(ch, 2 * ch + xc, kh, kw, generator=g) * wstd for _ in range(3))
    bs = tuple(torch.randn(ch, generator=g) for _ in range(3))
    return h, inp, x, ws, bs


# ----------------------------------------------------------------------- FusedUpdate's elementwise operations
def act64(v, act: str):
    return {"none": v, "relu": torch.clamp(v, min=0), "sigmoid": torch.sigmoid(v), "tanh": torch.tanh(v)}[act]


def bias_act_ref(x, bias: Optional[torch.Tensor], act: str, scale: float, dtype=torch.float64):
    """oflow_bias_act_f32: act(x[b, c, p] + bias[c]) * scale, in ``dtype`` (float64: the reference; float32: the same
    formula op by op with PyTorch's CPU kernels, sigmoid as 1 / (1 + exp(-v)) like the device code)."""
    v = x.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype).view(1, -1, *([1] * (x.dim() - 2)))
    if act == "sigmoid" and dtype == torch.float32:
        v = 1.0 / (1.0 + torch.exp(-v))
    else:
        v = act64(v, act)
    return v * scale if scale != 1.0 else v


def _sig(v, dtype):
    return 1.0 / (1.0 + torch.exp(-v)) if dtype == torch.float32 else torch.sigmoid(v)


def gru_reset_ref(zr, br, h, dtype=torch.float64):
    """oflow_gru_reset_f32: sigmoid(zr[:, CH:] + br) * h  (zr = [z | r] pre-bias conv output, CH = h's channels)."""
    ch = h.shape[1]
    shape = (1, -1, *([1] * (h.dim() - 2)))
    return _sig(zr[:, ch:].to(dtype) + br.to(dtype).view(shape), dtype) * h.to(dtype)


def gru_blend_ref(zr, bz, q, bq, h, dtype=torch.float64):
    """oflow_gru_blend_f32: (1 - z) h + z tanh(q + bq), z = sigmoid(zr[:, :CH] + bz)."""
    ch = h.shape[1]
    shape = (1, -1, *([1] * (h.dim() - 2)))
    z = _sig(zr[:, :ch].to(dtype) + bz.to(dtype).view(shape), dtype)
    qq = torch.tanh(q.to(dtype) + bq.to(dtype).view(shape))
    return (1 - z) * h.to(dtype) + z * qq


# P = pixels per (batch, channel) row: 1028 > 4 x 256 (the float4 loop iterates), 1485 = 33 x 45 odd
FUSED_P = [1, 3, 4, 1028, 1485]
FUSED_BC = [(1, 1), (3, 5), (1, 128), (3, 128)]
# operand layouts: every base 16-B aligned and strides multiples of 4 ("vec": float4 when P % 4 == 0), a base off by
# one float ("offset"), a batch stride of the packed size + 1 ("stride")
FUSED_LAYOUTS = ["vec", "offset", "stride"]
