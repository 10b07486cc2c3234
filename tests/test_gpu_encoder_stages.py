"""The feature / context encoder's stages (model/extractor.py: SplitEncoder) one kernel at a time through the C ABI,
each against a float64 restatement of the same operation (tests/encoder_stage_cases.py, pinned against the nn.Modules
by tests/test_encoder_stages_host.py): oflow_norm_stats_finalize from synthetic partials, oflow_norm_apply_s32 in every
mode, the convolution epilogue's residual add and space-to-depth store, the stride-2 stage (2x2 convolution over the
space-to-depth input, sliced 1x1 shortcut), and the whole encoder against its float64 module at small ragged sizes.

Every convolution without instance-norm partials runs twice: with the default small-grid threshold (conv_s32.hip
small_grid(): under 16384 output pixels, S32 input, n_pad % 64 == 0 -> launch_conv<KH, KW, 64, 2, 2, 0, 2>, 2-row tiles
and 64-channel blocks) and with oflow_exp_set_small_grid_px(0) (the tiles the encoder runs on at benchmark sizes). The
two must agree bit for bit and each must meet the float64 bound. Convolution bound, as test_gpu_conv_s32.py's:
|d| <= 2e-6 * sum|x||w| + 1e-6, plus 2^-23 |res| for a residual add and 2^-22 |ref| for an S32 output.
"""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

import encoder_stage_cases as ec
from optical_flow import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 1234.0  # fp16 fill of every destination buffer: untouched bytes must keep its bit pattern
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -7  # include/oflow.h: OFLOW_E_NULL, OFLOW_E_SHAPE, OFLOW_E_ALIGN


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    lib = N.load()
    lib.oflow_exp_set_small_grid_px.argtypes = [ctypes.c_int]
    lib.oflow_exp_set_stats_8row.argtypes = [ctypes.c_int]


@contextlib.contextmanager
def _small_grid_px(px):
    lib = N.load()
    lib.oflow_exp_set_small_grid_px(px)
    try:
        yield
    finally:
        lib.oflow_exp_set_small_grid_px(16384)


@contextlib.contextmanager
def _stats_8row(on):
    lib = N.load()
    lib.oflow_exp_set_stats_8row(on)
    try:
        yield
    finally:
        lib.oflow_exp_set_stats_8row(1)


def _both_grids(run):
    """run() with the small-grid tiles and with the production tiles: outputs bit-identical; returns the first."""
    with _small_grid_px(16384):
        a = run()
    with _small_grid_px(0):
        c = run()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v), "small-grid tiles and production tiles differ"
    return a


def _sentinel_buf(b, h, w, groups):
    return torch.full((b, h, w, groups, 2, 32), SENTINEL, device=DEV, dtype=torch.float16)


def _check_slice(buf, g0, c, ref, tol, what=""):
    """Channels [0, c) of the slice starting at group g0 of the S32 buffer against ref (B, c, H, W) float64 within tol;
    every other half of the buffer still the sentinel, bit for bit."""
    got = N.s32_to_f32(buf)[:, g0 * 32:g0 * 32 + c].double().cpu()
    err = (got - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max err {float(err.max()):.3e}, worst err/tol {float((err / tol).max()):.2f}"
    mask = torch.zeros(buf.shape[3] * 32, dtype=torch.bool, device=DEV)
    mask[g0 * 32:g0 * 32 + c] = True
    mask = mask.view(buf.shape[3], 1, 32).expand(buf.shape[3], 2, 32)
    bits = buf.view(torch.int16)
    fill = torch.tensor(SENTINEL, dtype=torch.float16).view(torch.int16).item()
    assert bool((bits[:, :, :, ~mask] == fill).all()), f"{what}: wrote outside channels [0, {c}) of the slice"
    return got


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


def _nhwc(x):
    """(B, C, H, W) -> the kernels' fp32 [P, C] rows on the GPU."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous().to(DEV)


# ---------------------------------------------------------------------------------- 2. oflow_norm_stats_finalize
@pytest.mark.parametrize("b", ec.STATS_BATCH)
@pytest.mark.parametrize("c,n_pad", ec.STATS_CHANNELS)
@pytest.mark.parametrize("tiles", ec.STATS_TILES)
def test_norm_stats_from_synthetic_partials(tiles, c, n_pad, b):
    """norm_stats_kernel alone, from (count, mean, M2) partials of float64 samples cut into ragged runs of 1..128 and
    rounded to fp32, against the float64 merge of those same fp32 values (merge64): one partial per wave (<= 16 tiles),
    several (17, 48), the unrolled 4-in-flight loop (from 49 tiles) and its 64-tile period (63, 64, 65, 130, 257); one
    lane block, a full one, a ragged second one, n_pad > C with NaN in the padding columns; a constant channel (M2 = 0:
    alpha = 1/sqrt(eps)), one with mean 100 / std 1.01, one with mean ~0. alpha is one fp32 rounding of a float64
    value, beta = -fp32(mean) * alpha three:
        |alpha - a| <= 2^-23 a,   |beta - b| <= 2^-22 |b| + 1e-12 a max_t |mean_t|
    (the last term: the float64 sum's cancellation where the mean is ~0). Outputs finite, the buffers past B*C
    untouched, and a second call bit-identical (fixed merge order)."""
    part = ec.stats_partials_f32(b, c, n_pad, tiles, seed=1000 * tiles + c + b)
    a_ref, b_ref, mmax = ec.stats_reference(part, c)
    pg = part.to(DEV)
    lib = N.load()
    slack = 64
    outs = []
    for _ in range(2):
        alpha = torch.full((b * c + slack,), -7.5, device=DEV)
        beta = torch.full((b * c + slack,), -7.5, device=DEV)
        st = lib.oflow_norm_stats_finalize(pg.data_ptr(), b, tiles, n_pad, c, ec.EPS, alpha.data_ptr(), beta.data_ptr(),
                                           N._stream(DEV))
        assert st == 0, st
        torch.cuda.synchronize()
        outs.append((alpha.cpu(), beta.cpu()))
    (alpha, beta), (alpha2, beta2) = outs
    assert torch.equal(alpha, alpha2) and torch.equal(beta, beta2)
    assert bool((alpha[b * c:] == -7.5).all()) and bool((beta[b * c:] == -7.5).all())
    al, be = alpha[:b * c].view(b, c).double(), beta[:b * c].view(b, c).double()
    assert bool(torch.isfinite(al).all()) and bool(torch.isfinite(be).all())
    ea = (al - a_ref).abs()
    eb = (be - b_ref).abs()
    assert bool((ea <= 2.0 ** -23 * a_ref).all()), float((ea / a_ref).max())
    tol_b = 2.0 ** -22 * b_ref.abs() + 1e-12 * a_ref * mmax
    assert bool((eb <= tol_b).all()), float((eb / tol_b).max())
    assert torch.equal(al[:, 0].float(), a_ref[:, 0].float())  # the constant channel: var = 0 exactly, 1/sqrt(eps)


# --------------------------------------------------------------------------------------- 3. oflow_norm_apply_s32
def _apply_inputs(seed, b, c, h, w, integer=False):
    g = ec.gen(seed)
    if integer:
        x, res, x2 = (torch.randint(-8, 9, (b, c, h, w), generator=g).float() for _ in range(3))
        al, al2 = (torch.randint(1, 3, (b, c), generator=g).float() for _ in range(2))
        be, be2 = (torch.randint(-4, 5, (b, c), generator=g).float() for _ in range(2))
    else:
        x, x2 = (torch.randn(b, c, h, w, generator=g) * 3 + 0.5 for _ in range(2))
        res = torch.randn(b, c, h, w, generator=g) * 2
        al, al2 = (torch.rand(b, c, generator=g) + 0.5 for _ in range(2))
        be, be2 = (torch.randn(b, c, generator=g) for _ in range(2))
    return x, res, x2, al, be, al2, be2


def _run_norm_apply(shape, c, mode, act, res_act, s2d, integer=False):
    """One oflow_norm_apply_s32 call: destination = groups [1, 1 + ceil(Cd / 32)) of a sentinel buffer one group wider
    on each side (pixel stride > the slice), the mode-1 residual = groups [2, ...) of a buffer three groups wider
    (res_pixel_stride != C/32 * 128). Returns (buffer, g0, Cd, ref, mag): the float64 restatement on the fp32 inputs
    and the residual's hi + lo."""
    b, h, w = shape
    x, res, x2, al, be, al2, be2 = _apply_inputs(sum(shape) * 131 + c * 7 + mode, b, c, h, w, integer)
    rg = (c + 31) // 32
    res_wide = N.s32_from_f32(torch.cat([torch.full((b, 64, h, w), 5.0), res], dim=1).to(DEV), groups=rg + 3)
    res_slice = N.S32Slice(res_wide, 2, rg)
    res_seen = N.s32_to_f32(res_wide)[:, 64:64 + c].cpu()
    cd = 4 * c if s2d else c
    ho, wo = (h // 2, w // 2) if s2d else (h, w)
    dg = (cd + 31) // 32
    buf = _sentinel_buf(b, ho, wo, dg + 2)
    dev = lambda t: t.to(DEV)
    N.norm_apply(_nhwc(x), (b, c, h, w), dev(al), dev(be), act, N.S32Slice(buf, 1, dg),
                 res=res_slice if mode == 1 else None,
                 res_raw=(_nhwc(x2), dev(al2), dev(be2)) if mode >= 2 else None,
                 res_act=res_act, s2d=bool(s2d), res_raw_relu=mode == 3)
    torch.cuda.synchronize()
    ref, mag = ec.norm_apply64(x, al, be, act, mode, res=res_seen, x2=x2, alpha2=al2, beta2=be2, res_act=res_act, s2d=bool(s2d))
    return buf, 1, cd, ref, mag


@pytest.mark.parametrize("shape,c,mode,act,res_act,s2d", ec.APPLY_CASES, ids=_id)
def test_norm_apply_every_mode_matches_fp64(shape, c, mode, act, res_act, s2d):
    """norm_apply_kernel per element against norm_apply64: residual modes 0-3, both activations, the space-to-depth
    destination (channel (y&1)*2 + (x&1))*C + c of pixel (y/2, x/2), by ec.space_to_depth's index formula), sliced
    destination and residual, P*C/8 not a multiple of the 256-thread block (tail guard), C = 8 / 40 writing part of a
    32-channel group. The pairs SplitEncoder issues at every C, the rest of the cross product at C = 40. Bound: at most
    four fp32 roundings of the partial terms plus the 22-bit split,
        |d| <= 2^-22 (|x alpha| + |beta| + |residual terms| + |ref|) + 2^-24;
    the absolute floor follows from split_f16 (oflow_internal.h): lo = fp16(v - hi) is subnormal below 2^-14, where its
    rounding error is at most half the fp16 subnormal spacing, 2^-25 <= 2^-24; above, hi + lo keeps 22 bits. Every half
    outside the written channels keeps the sentinel's bits, the 24 untouched channels of the group at C = 8 too."""
    buf, g0, cd, ref, mag = _run_norm_apply(shape, c, mode, act, res_act, s2d)
    tol = 2.0 ** -22 * (mag + ref.abs()) + 2.0 ** -24
    _check_slice(buf, g0, cd, ref, tol, f"mode {mode} {act}/{res_act} s2d {s2d}")


@pytest.mark.parametrize("s2d", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("c", [8, 96])
def test_norm_apply_integer_exact(c, mode, s2d):
    """Small-integer x, residual and beta, alpha in {1, 2}: every intermediate is exact, so the S32 output equals the
    float64 restatement exactly -- the channel-octet and space-to-depth addressing on their own."""
    buf, g0, cd, ref, _ = _run_norm_apply((3, 4, 34), c, mode, "relu", "relu", s2d, integer=True)
    assert float(ref.abs().max()) >= 8
    _check_slice(buf, g0, cd, ref, torch.zeros_like(ref), f"integer mode {mode} s2d {s2d}")


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_norm_apply_libm_activations(act):
    """act 2 / 3 (expf, tanhf; no caller in the encoder) within the 2e-6 absolute bound test_conv_s32_gru_epilogues
    uses for the libm gates."""
    buf, g0, cd, ref, _ = _run_norm_apply((2, 6, 10), 40, 0, act, "none", 0)
    _check_slice(buf, g0, cd, ref, torch.full_like(ref, 2e-6), act)


def test_norm_apply_argument_errors():
    """The documented status codes: C % 8 != 0 and odd H with s2d -> OFLOW_E_SHAPE, residual mode 1 without a residual
    and mode 2 without x2 -> OFLOW_E_NULL, a misaligned y -> OFLOW_E_ALIGN; nothing is launched."""
    lib = N.load()
    b, c, h, w = 1, 16, 4, 6
    x = torch.zeros(b * h * w, c, device=DEV)
    al = torch.ones(b, c, device=DEV)
    be = torch.zeros(b, c, device=DEV)
    y = _sentinel_buf(b, h, w, 1)
    res = N.s32_empty(b, h, w, 1, DEV, zero=True)

    def call(c=c, h=h, mode=0, res_p=None, x2=None, s2d=0, yp=None):
        a2 = al.data_ptr() if x2 is not None else None
        b2 = be.data_ptr() if x2 is not None else None
        return lib.oflow_norm_apply_s32(x.data_ptr(), c, b, h, w, al.data_ptr(), be.data_ptr(), 1, mode, res_p, 128, x2,
                                        a2, b2, 1, s2d, y.data_ptr() if yp is None else yp, 128, N._stream(DEV))

    assert call(c=12) == E_SHAPE
    assert call(h=3, s2d=1) == E_SHAPE
    assert call(mode=1) == E_NULL
    assert call(mode=2) == E_NULL
    assert call(yp=y.data_ptr() + 8) == E_ALIGN
    assert call(mode=1, res_p=res.data_ptr()) == 0 and call(mode=2, x2=x.data_ptr()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------- 4. conv epilogue: residual add, space-to-depth store
def _conv_ref(xr, wt, bias, stride=1, pad=1):
    y = F.conv2d(xr.double(), wt.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    bound = F.conv2d(xr.double().abs(), wt.double().abs(), None, stride=stride, padding=pad)
    return y, bound


def _res_conv(n, shape, s2d, integer=False):
    """relu(relu(conv3x3(x) + bias) + res) into y0 and y1 (slices at group 1 / 2 of wider sentinel buffers), res a slice
    at group 1 of a wider buffer; returns per destination (buffer, g0), Cd and the float64 (ref, tol)."""
    b, h, w = shape
    if integer:
        g = ec.gen(9 + n)
        x = torch.randint(-8, 9, (b, n, h, w), generator=g).float()
        wt = torch.randint(-2, 3, (n, n, 3, 3), generator=g).float()
        bias = torch.randint(-4, 5, (n,), generator=g).float()
        res = torch.randint(-64, 65, (b, n, h, w), generator=g).float()
    else:
        x, wt, bias = ec.conv_inputs(n + h * w, b, n, n, h, w, 3)
        res = torch.randn(b, n, h, w, generator=ec.gen(n + 1)) * 2
    ng = n // 32
    xs = N.s32_from_f32(x.to(DEV))
    res_wide = N.s32_from_f32(torch.cat([torch.full((b, 32, h, w), 5.0), res], dim=1).to(DEV), groups=ng + 2)
    cw = N.ConvWeights(wt.to(DEV), bias.to(DEV), n)
    cd = 4 * n if s2d else n
    ho, wo = (h // 2, w // 2) if s2d else (h, w)
    dg = cd // 32

    def run():
        d0, d1 = _sentinel_buf(b, ho, wo, dg + 2), _sentinel_buf(b, ho, wo, dg + 3)
        N.conv_s32(N.S32Slice(xs), cw, n, act="relu", y0=N.S32Slice(d0, 1, dg), y1=N.S32Slice(d1, 2, dg),
                   res=N.S32Slice(res_wide, 1, ng), res_act="relu", s2d=s2d)
        return d0, d1

    d0, d1 = _both_grids(run)
    xr = N.s32_to_f32(xs, n).cpu()
    rr = N.s32_to_f32(res_wide)[:, 32:32 + n].cpu().double()
    y, bound = _conv_ref(xr, wt, bias)
    ref = torch.relu(torch.relu(y) + rr)
    tol = 2e-6 * bound + 1e-6 + 2.0 ** -23 * rr.abs()
    if s2d:
        ref, tol = ec.space_to_depth(ref), ec.space_to_depth(tol)
    return [(d0, 1), (d1, 2)], cd, ref, tol + 2.0 ** -22 * ref.abs()


@pytest.mark.parametrize("n,shape,s2d", ec.RES_CONV_CASES, ids=_id)
def test_conv_residual_epilogue_matches_fp64(n, shape, s2d):
    """The batch-norm encoder's block tail in the conv epilogue (a.res, a.s2d branches): 3x3 conv, ReLU, + S32 residual
    (a slice of a wider buffer), ReLU, to y0 and y1, plain and space-to-depth ((B, H/2, W/2, 4N) at a group offset of a
    wider sentinel buffer), against float64 on the operands' hi + lo. Kernel instances (launch_bn<3, 3, 0>): default
    threshold, 64 and 128 channels -> launch_conv<3, 3, 64, 2, 2, 0, 2>; threshold 0 -> 64: launch_conv<3, 3, 64, 2, 2, 0>
    (LDS-staged, 4-row tiles), 128: launch_conv<3, 3, 128, 1, 4, 0, kTY, true> (register-direct weights); 96 channels
    (n_pad % 64 != 0, never small-grid): launch_conv<3, 3, 96, 4, 1, 0> both times. Ragged tiles: W = 34 and 70,
    H = 6 and 10 against 4 x 32 (2 x 32) pixel tiles."""
    dests, cd, ref, tol = _res_conv(n, shape, s2d)
    assert float((ref > 0).double().mean()) > 0.3
    for buf, g0 in dests:
        _check_slice(buf, g0, cd, ref, tol, f"y at group {g0}")


@pytest.mark.parametrize("n", [64, 96, 128])
def test_conv_residual_s2d_integer_exact(n):
    """Small-integer operands, residual and bias: relu(relu(conv) + res) in space-to-depth order must be exact (integers
    below 2^22 are exact as hi + lo). Same kernel instances as test_conv_residual_epilogue_matches_fp64."""
    dests, cd, ref, _ = _res_conv(n, (2, 6, 34), True, integer=True)
    assert 64 <= float(ref.max()) < 2.0 ** 22
    for buf, g0 in dests:
        _check_slice(buf, g0, cd, ref, torch.zeros_like(ref), f"integer y at group {g0}")


# ------------------------------------------------------------------------------------------ 5. the stride-2 stage
def _s2_inputs(c, n, h, w, integer=False):
    b = ec.S2_BATCH
    if integer:
        g = ec.gen(3 + c)
        x = torch.randint(-8, 9, (b, c, 2 * h, 2 * w), generator=g).float()
        wt = torch.randint(-4, 5, (n, c, 3, 3), generator=g).float()
        bias = torch.randint(-4, 5, (n,), generator=g).float()
    else:
        x, wt, bias = ec.conv_inputs(c + 10 * h + w, b, c, n, 2 * h, 2 * w, 3)
    xs = N.s32_from_f32(ec.space_to_depth(x).to(DEV))  # (B, h, w, 4C/32, 2, 32)
    xr = N.s32_to_f32(xs, 4 * c).cpu()
    if integer:
        assert torch.equal(ec.space_to_depth(x), xr)
    # the image the kernel sees (hi + lo of every pixel), back in (B, C, 2h, 2w)
    seen = torch.empty_like(x)
    for a in range(2):
        for bb in range(2):
            seen[:, :, a::2, bb::2] = xr[:, (a * 2 + bb) * c:(a * 2 + bb + 1) * c]
    return b, x, seen, wt, bias, xs


def _s2d_cw(wt, bias, n):
    from model.extractor import _s2d_weight

    return N.ConvWeights(_s2d_weight(wt.to(DEV)), None if bias is None else bias.to(DEV), n)


def _run_s2_batch_form(xs, cw, n, b, h, w):
    def run():
        d0 = _sentinel_buf(b, h, w, n // 32 + 2)
        N.conv_s32(N.S32Slice(xs), cw, n, act="relu", y0=N.S32Slice(d0, 1, n // 32))
        return (d0,)

    return _both_grids(run)[0]


@pytest.mark.parametrize("h,w", ec.S2_SIZES)
@pytest.mark.parametrize("c,n", ec.S2_CHANNELS)
def test_stride2_conv_batch_form_matches_fp64(c, n, h, w):
    """A stride-2 block's first conv as the batch-norm encoder runs it: the 2x2 convolution with _s2d_weight(w) over the
    S32 space-to-depth input, bias, ReLU, S32 out -- against F.conv2d(x, w, b, stride=2, padding=1) in float64 on the
    pixels the kernel sees; sum|x||w| from the stride-2 conv of the absolute values. Output sizes 1x1 (every tap but
    the (0, 0) quadrant's on the zero border), 4x32 (one whole tile), 5x33 and 9x40 (ragged). Kernel instances
    (launch_bn<2, 2, 0>; the 2x2 kernels have no register-direct instance): default threshold, 64 and 128 channels ->
    launch_conv<2, 2, 64, 2, 2, 0, 2>; threshold 0 -> launch_conv<2, 2, 64, 2, 2, 0>, launch_conv<2, 2, 128, 2, 2, 0>;
    96 channels -> launch_conv<2, 2, 96, 4, 1, 0> both times."""
    b, x, seen, wt, bias, xs = _s2_inputs(c, n, h, w)
    d0 = _run_s2_batch_form(xs, _s2d_cw(wt, bias, n), n, b, h, w)
    y, bound = _conv_ref(seen, wt, bias, stride=2)
    ref = torch.relu(y)
    _check_slice(d0, 1, n, ref, 2e-6 * bound + 1e-6 + 2.0 ** -22 * ref.abs(), "2x2 s2d conv")


def _stats_variants(n):
    return (1, 0) if n == 64 else (1,)


@pytest.mark.parametrize("h,w", ec.S2_SIZES)
@pytest.mark.parametrize("c,n", ec.S2_CHANNELS)
def test_stride2_conv_instance_form_matches_fp64(c, n, h, w):
    """The same convolution as the instance-norm encoder runs it: raw fp32 NHWC output plus per-tile (count, mean, M2)
    partials (never small-grid). The output within 2e-6 sum|x||w| + 1e-6 of float64; norm_stats of the partials = the
    float64 statistics of the kernel's own output to 2e-6 (test_instance_norm_partials' measure). Kernel instances:
    launch_conv<2, 2, 128, 2, 2, 0>, launch_conv<2, 2, 96, 4, 1, 0>, and for 64 channels launch_conv<2, 2, 64, 4, 1, 0, 8>
    (8-row tiles, the default) and launch_conv<2, 2, 64, 2, 2, 0> (oflow_exp_set_stats_8row(0)), bit-identical."""
    b, x, seen, wt, bias, xs = _s2_inputs(c, n, h, w)
    cw = _s2d_cw(wt, bias, n)
    tiles = N.conv_tiles(h, w)
    y, bound = _conv_ref(seen, wt, bias, stride=2)
    raws = []
    for eight in _stats_variants(n):
        raw = torch.full((b * h * w, n), float("nan"), device=DEV)
        part = torch.full((b, tiles, cw.n_pad, 3), float("nan"), device=DEV)
        with _stats_8row(eight):
            N.conv_s32(N.S32Slice(xs), cw, n, nhwc=raw, stats=part)
            alpha, beta = N.norm_stats(part, b, tiles, cw.n_pad, n, ec.EPS)
            torch.cuda.synchronize()
        got = raw.view(b, h, w, n).permute(0, 3, 1, 2).double().cpu()
        err = (got - y).abs()
        tol = 2e-6 * bound + 1e-6
        assert bool((err <= tol).all()), f"8row {eight}: max err {float(err.max()):.3e}, worst {float((err / tol).max()):.2f}"
        assert bool(torch.isfinite(part[:, :, :n]).all())
        assert float(part[:, :, :n, 0].sum(dim=1).sub(h * w).abs().max()) == 0
        a_ref, b_ref = ec.instance_affine64(got)
        mean = got.mean(dim=(2, 3))
        ea = float(((alpha.double().cpu() - a_ref).abs() / a_ref).max())
        eb = float(((beta.double().cpu() - b_ref).abs() / (mean.abs() * a_ref + 1.0)).max())
        assert ea <= 2e-6 and eb <= 2e-6, (eight, ea, eb)
        raws.append(raw)
    for r in raws[1:]:
        assert torch.equal(raws[0], r)


@pytest.mark.parametrize("c,n", ec.S2_CHANNELS)
def test_stride2_conv_integer_exact_and_single_taps(c, n):
    """Small-integer image and weights: the 2x2 space-to-depth convolution equals the 3x3 / stride 2 / pad 1 one exactly
    (5x33 outputs, B = 2). Then output channel 0 with one tap at a time set to 1 on input channel 3, all nine taps: the
    output plane must be the image shifted by that tap, out[Y, X] = x[2Y + ky - 1, 2X + kx - 1] with zeros outside -- a
    mis-mapped quadrant or a wrong border shows as a shifted plane. Instances as
    test_stride2_conv_batch_form_matches_fp64 (batch form, act none)."""
    h, w = 5, 33
    b, x, seen, wt, bias, xs = _s2_inputs(c, n, h, w, integer=True)

    def conv(wt_):
        cw = _s2d_cw(wt_, bias, n)

        def run():
            d0 = _sentinel_buf(b, h, w, n // 32 + 2)
            N.conv_s32(N.S32Slice(xs), cw, n, y0=N.S32Slice(d0, 1, n // 32))
            return (d0,)

        return _both_grids(run)[0]

    ref = F.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=1)
    assert float(ref.abs().max()) < 2.0 ** 22
    _check_slice(conv(wt), 1, n, ref, torch.zeros_like(ref), "integer 2x2 s2d conv")
    for ky in range(3):
        for kx in range(3):
            w1 = wt.clone()
            w1[0] = 0
            w1[0, 3, ky, kx] = 1
            got = N.s32_to_f32(conv(w1))[:, 32].cpu()
            want = ec.shifted_tap(x[:, 3], ky, kx) + bias[0]
            assert torch.equal(got, want), f"tap ({ky}, {kx})"


@pytest.mark.parametrize("h,w", ec.S2_SIZES)
@pytest.mark.parametrize("c,n", ec.SHORTCUT_CHANNELS)
def test_stride2_shortcut_matches_fp64(c, n, h, w):
    """The 1x1 / stride 2 downsample shortcut: a 1x1 convolution over S32Slice(xs, 0, C/32), the first C of the
    space-to-depth tensor's 4C channels (input pixel stride 4x the slice's width), against
    F.conv2d(x, wd, bd, stride=2) in float64 -- as an S32 output (batch form, both grids) and as raw fp32 NHWC with
    partials (instance form). Kernel instances (launch_bn<1, 1, 0>): 96 channels -> launch_conv<1, 1, 96, 4, 1, 0>;
    128 -> launch_conv<1, 1, 64, 2, 2, 0, 2> (default threshold) and launch_conv<1, 1, 128, 2, 2, 0>."""
    b = ec.S2_BATCH
    x, wd, bd = ec.conv_inputs(77 + c + h, b, c, n, 2 * h, 2 * w, 1)
    xs = N.s32_from_f32(ec.space_to_depth(x).to(DEV))
    seen = N.s32_to_f32(xs, c).cpu()  # quadrant (0, 0): the pixels (2Y, 2X)
    cw = N.ConvWeights(wd.to(DEV), bd.to(DEV), n)
    xin = N.S32Slice(xs, 0, c // 32)
    assert xin.ps == 4 * c // 32 * 128

    def run():
        d0 = _sentinel_buf(b, h, w, n // 32 + 2)
        N.conv_s32(xin, cw, n, y0=N.S32Slice(d0, 1, n // 32))
        return (d0,)

    d0 = _both_grids(run)[0]
    ref, bound = _conv_ref(seen, wd, bd, pad=0)
    strided, _ = _conv_ref(N.s32_to_f32(N.s32_from_f32(x.to(DEV))).cpu(), wd, bd, stride=2, pad=0)
    assert torch.equal(ref, strided)
    tol = 2e-6 * bound + 1e-6
    _check_slice(d0, 1, n, ref, tol + 2.0 ** -22 * ref.abs(), "1x1 shortcut")
    raw = torch.full((b * h * w, n), float("nan"), device=DEV)
    part = torch.full((b, N.conv_tiles(h, w), n, 3), float("nan"), device=DEV)
    N.conv_s32(xin, cw, n, nhwc=raw, stats=part)
    torch.cuda.synchronize()
    err = (raw.view(b, h, w, n).permute(0, 3, 1, 2).double().cpu() - ref).abs()
    assert bool((err <= tol).all()), float((err / tol).max())


# ------------------------------------------------------------------------------------------- 6. the whole encoder
# max |split - enc64| / max |enc32 - enc64| allowed: split-fp16 keeps 22 significant bits against fp32's 24
ENCODER_FACTOR = 4.0
_split_encoders = {}


def _split_encoder(norm):
    from model.extractor import SplitEncoder
    import copy

    if norm not in _split_encoders:
        enc = copy.deepcopy(ec.encoder(norm)).to(DEV).eval()
        _split_encoders[norm] = SplitEncoder(enc)
    return _split_encoders[norm]


@pytest.mark.parametrize("variant", ec.ENCODER_VARIANTS)
@pytest.mark.parametrize("shape", ec.ENCODER_SHAPES, ids=_id)
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_split_encoder_matches_fp64_module(norm, shape, variant):
    """SplitEncoder against the float64 module on the CPU at small ragged sizes (stem outputs 12x20, 8x36, 20x12: every
    stage has partial 4 x 32 tiles, layer3 runs at 3x5 / 2x9 / 5x3), patch-matrix stem, split_out and
    stem_from_image. Yardstick: e32 = max |enc32 - enc64| of the fp32 module on the CPU (0 < e32 <= 1e-4 max |ref|:
    the inputs are well conditioned); the kernels' es = max |split - enc64| must stay within 4 * e32.
    Measured es / e32 on an MI355X (the three variants agree to the digits shown; e32 ~1e-5 instance, ~4e-6 batch):
        norm      2x3x24x40  1x3x16x72  3x3x40x24
        instance    0.98       1.05       1.16
        batch       2.15       0.99       1.52"""
    x, ref, e32 = ec.encoder_case(norm, shape)
    assert 0.0 < e32 <= 1e-4 * float(ref.abs().max())
    se = _split_encoder(norm)
    with torch.inference_mode():
        if variant == "split_out":
            got = N.s32_to_f32(se(x.to(DEV), split_out=True), 256)
        else:
            got = se(x.to(DEV), stem_from_image=variant == "stem_from_image")
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    es = float((got.double().cpu() - ref).abs().max())
    print(f"encoder {norm} {shape} {variant}: es {es:.3e} e32 {e32:.3e} ratio {es / e32:.2f} (max |ref| {float(ref.abs().max()):.2f})")
    assert es <= ENCODER_FACTOR * e32, (es, e32, es / e32)
