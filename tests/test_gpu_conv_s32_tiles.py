"""The update block's convolutions (csrc/conv_s32.hip through oflow_conv_s32) against float64 on every instantiation
dispatch_conv() / launch_bn() can pick for them, at the smallest shapes where a 4 x 32 / 2 x 32 tile kernel can go wrong.

The dispatcher decides by pixel count (small_grid(): B*H*W < 16384 -> launch_conv<KH, KW, 64, 2, 2, EPI, 2>), so tests at
small shapes otherwise only ever reach the small-grid tiles. Here oflow_exp_set_small_grid_px(0 | 16384) and the
register-direct switches (N.CONV_BREG / CONV_BREG64 / CONV_BREG32) select the leaf, and every call asserts through
oflow_exp_last_conv_leaf() (a host-side record of the template parameters launch_conv instantiated) that it ran the
leaf it meant to, so a later change of the dispatch rules cannot silently turn these back into small-grid tests.

Per case (tests/conv_s32_cases.py; float64 restatements pinned by tests/test_conv_s32_cases_host.py):
 1. float64 bounds, the project's existing ones: epilogue 0 |d| <= 2e-6 * sum|x||w| + 1e-6 (+ 2^-22 |ref| read back from
    S32); GRU z, r*h and h' 2e-6 at the operand scales of test_gpu_conv_s32.py (weights x 0.03, tanh'd h), 2^-21 between
    the fp32 master h and its S32 copy; the GRU cases under conv flags 0 (hardware exp2 / reciprocal gates) and 256
    (libm). Each launch is compared on the operands it read (hi + lo of the S32 input; the second GRU launch on the r*h
    and z the first one stored).
 2. bit identity across the leaves of a case, per output channel (the leaves differ in block width): every output of
    every leaf equals the LDS-staged 128-channel leaf's (fp32 NCHW, S32 bytes, NHWC, z, master h).
 3. nothing else is touched: every destination is a slice of a larger sentinel-filled buffer with one trailing guard
    image (or row block); all bytes outside the written channels keep their value, S32 padding channels above N included
    (zeros, as the S32 contract of include/oflow.h requires of the caller, on the first run; a sentinel on the second);
    each call runs twice on differently dirtied destinations and gives the same bits.
 4. one integer-exact case per GRU leaf: small-integer operands and one-hot weights make the pre-activation an exact
    small integer v, so z, r and q must be one single-valued function of v (the same bits wherever v recurs: a wrong
    accumulator lane map or addend row lands on another pixel's or channel's v) within 2e-6 of the float64 gate.

Leaves of dispatch_conv for {1x1, 3x3, 1x5, 5x1} x epilogue {0, 1, 2} on S32 input, and the test id asserting each
(KxK below = each of 1x1, 3x3, 1x5, 5x1; names as conv_s32_cases.LEAVES; <KH,KW,BN,WM,WN,EPI,TY,BREG>):
  epilogue 0  <K,K, 64,2,2,0,2>        small-grid   test_epi0_leaf[KxK-small]
              <K,K,128,2,2,0,4>        LDS 128      test_epi0_leaf[KxK-lds128]
              <K,K, 96,4,1,0,4>        LDS 96       test_epi0_leaf[KxK-lds96]
              <K,K, 64,2,2,0,4>        LDS 64       test_epi0_leaf[KxK-lds64]
              <K,K, 32,4,1,0,4>        LDS 32       test_epi0_leaf[KxK-lds32]
              <K,K,128,1,4,0,4,true>   BREG 128     test_epi0_leaf[3x3-breg128], [1x5-breg128], [5x1-breg128]
              <3,3, 64,2,2,0,4,true>   BREG 64      test_epi0_leaf[3x3-breg64]
              <3,3, 32,4,1,0,4,true>   BREG 32      test_epi0_leaf[3x3-breg32]
  epilogue 1  <1,5| 5,1, 64,2,2,1,2>       small-grid   test_gru_leaf[*-1x5-small-*], [*-5x1-small-*]
              <1,5| 5,1,128,2,2,1,4>       LDS 128      test_gru_leaf[*-1x5-lds128-*], [*-5x1-lds128-*]
              <1,5| 5,1,128,1,4,1,4,true>  BREG 128     test_gru_leaf[*-1x5-breg128-*], [*-5x1-breg128-*]
  epilogue 2  the same three rows with EPI 2: the same test ids (each runs the gates launch, then the candidate launch,
              and asserts the leaf after either); integer-exact: test_gru_leaf_integer_exact[KxK-leaf-*]
  (test_gru_leaf ids: [hw|libm-KxK-leaf-addend|bias]; test_gru_leaf_integer_exact ids: [KxK-leaf-gru_channels])
Left to other files: the 2x2 kernel, the normalise-on-load input (OFLOW_IN_F32_NORM), the residual / space-to-depth
epilogues and the 8-row instance-norm tiles -> tests/test_gpu_encoder_stages.py; the instance-norm partials (stats
kernels), OFLOW_IN_F32 and OFLOW_IN_FLOW7 inputs -> tests/test_gpu_conv_s32.py (test_instance_norm_partials,
test_conv_f32_input_equals_s32_input, test_convf1_from_flow_equals_patch_matrix); OFLOW_IN_IMG7S2 ->
tests/test_gpu_encoder_stages.py (stem_from_image); the flow-head epilogue (OFLOW_EPI_FLOW_HEAD) ->
tests/test_gpu_flow_head_fused.py; the fused lookup + convc1 -> tests/test_gpu_corr_convc1.py; the 8-row 64-channel
variant (oflow_exp_set_bn64_8row) is experiments-only.

Measured on an MI355X (worst error / tolerance over all cases of the family; every leaf of a family gives the same
figure, the leaves being bit-identical -- no leaf's claim turned out false):
  epilogue 0 (fp32 NCHW, NHWC and S32 destinations): 1x1 0.089, 3x3 0.111, 1x5 0.088, 5x1 0.095
  GRU z / r*h / h' against 2e-6: 1x5 0.544 with the addend, 0.787 with biases (libm gates 0.544 / 0.794);
                                 5x1 0.604 / 0.692 (libm 0.600 / 0.681)
  S32 copy of h' against 2^-21: 0.125
"""
import contextlib
import ctypes

import pytest
import torch

import conv_s32_cases as cc
from optical_flow import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FILLS = [(1234.0, 7.5e8), (-77.5, -3.25)]  # (fp16, fp32) sentinel of the two runs of every call
GUARD_ROWS = 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    lib = N.load()
    lib.oflow_exp_set_small_grid_px.argtypes = [ctypes.c_int]
    lib.oflow_exp_set_conv_flags.argtypes = [ctypes.c_int]
    lib.oflow_exp_last_conv_leaf.restype = ctypes.c_longlong
    lib.oflow_exp_last_conv_leaf.argtypes = []
    yield
    _CACHE.clear()


_CACHE = {}  # per case: operands, float64 references and the baseline leaf's outputs, computed once per module run


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@contextlib.contextmanager
def _leaf(monkeypatch, name):
    """Dispatcher state that selects leaf ``name``; the default state restored afterwards."""
    lib = N.load()
    breg = name.startswith("breg")
    with monkeypatch.context() as m:
        for attr in ("CONV_BREG", "CONV_BREG64", "CONV_BREG32"):
            m.setattr(N, attr, breg)
        lib.oflow_exp_set_small_grid_px(16384 if name == "small" else 0)
        try:
            yield
        finally:
            lib.oflow_exp_set_small_grid_px(16384)


@contextlib.contextmanager
def _small_grid_px(px):
    lib = N.load()
    lib.oflow_exp_set_small_grid_px(px)
    try:
        yield
    finally:
        lib.oflow_exp_set_small_grid_px(16384)


def _assert_leaf(kh, kw, epi, name):
    got = cc.decode_leaf(N.load().oflow_exp_last_conv_leaf())
    assert got == cc.expected_leaf(kh, kw, epi, name), f"meant leaf {name}, the dispatcher ran {got}"


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _s32_buf(b, h, w, groups, fill):
    """S32 buffer of b images plus a trailing guard image, every half the fp16 sentinel."""
    return torch.full((b + 1, h, w, groups, 2, 32), fill, device=DEV, dtype=torch.float16)


def _s32_mask(buf, b, g0, n):
    """True at the halves of channels [0, n) of the slice starting at group g0, first b images."""
    ch = torch.zeros(buf.shape[3] * 32, dtype=torch.bool, device=DEV)
    ch[g0 * 32:g0 * 32 + n] = True
    m = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    m[:b] = ch.view(buf.shape[3], 1, 32)
    return m


def _s32_written(buf, b, g0, n):
    """The hi | lo halves of channels [0, n) of the slice, (b, H, W, 2, n) fp16."""
    g = -(-n // 32)
    v = buf[:b, :, :, g0:g0 + g].permute(0, 1, 2, 4, 3, 5).reshape(b, buf.shape[1], buf.shape[2], 2, g * 32)
    return v[..., :n].contiguous()


def _s32_values(buf, b, g0, n):
    v = _s32_written(buf, b, g0, n).float()
    return (v[..., 0, :] + v[..., 1, :]).permute(0, 3, 1, 2).contiguous()  # (b, n, H, W)


def _untouched(buf, before, mask, what):
    assert torch.equal(_bits(buf)[~mask], _bits(before)[~mask]), f"{what}: wrote outside its destination"


def _same(outs, base, what):
    for key in base:
        assert torch.equal(_bits(outs[key]), _bits(base[key])), f"{what}: output {key!r} differs"


# ------------------------------------------------------------------------------------------------- epilogue 0
def _epi0_case(kh, kw, idx):
    def make():
        shape, cin, n = cc.EPI0_CASES[idx]
        x, wt, bias = (t.to(DEV) for t in cc.epi0_operands(kh, kw, cin, n, shape, seed=1000 * idx + 10 * kh + kw))
        xs = N.s32_from_f32(x)
        ref, bound = cc.conv_ref(N.s32_to_f32(xs, cin), wt, bias, kh, kw)
        return dict(shape=shape, cin=cin, n=n, wt=wt, bias=bias, xs=xs, ref=ref, bound=bound)
    return _cached(("epi0", kh, kw, idx), make)


def _run_epi0(case, kh, kw, name, fill, first):
    b, h, w = case["shape"]
    n = case["n"]
    bn = cc.LEAF_BLOCK_N[name]
    cw = N.ConvWeights(case["wt"], case["bias"], -(-n // bn) * bn)
    g = -(-n // 32)
    f16, f32fill = fill
    y0 = _s32_buf(b, h, w, g + 2, f16)
    y1 = _s32_buf(b, h, w, g + 1, f16)
    if first:  # the state the S32 contract asks of the caller: zeros in the padding channels of the last group
        y0[:b, :, :, g, :, n - (g - 1) * 32:] = 0
        y1[:b, :, :, g - 1, :, n - (g - 1) * 32:] = 0
    fbuf = torch.full((b + 1, n + 2, h, w), f32fill, device=DEV)
    nhwc = torch.full((b * h * w + GUARD_ROWS, n), f32fill, device=DEV) if n % 4 == 0 else None
    before = [t.clone() for t in (y0, y1, fbuf)] + ([nhwc.clone()] if nhwc is not None else [])
    N.conv_s32(N.S32Slice(case["xs"]), cw, bn, act="none", y0=N.S32Slice(y0[:b], 1, g), y1=N.S32Slice(y1[:b], 0, g),
               f32=fbuf[:b, 1:n + 1], nhwc=None if nhwc is None else nhwc[:b * h * w])
    torch.cuda.synchronize()
    _assert_leaf(kh, kw, 0, name)
    _untouched(y0, before[0], _s32_mask(y0, b, 1, n), "S32 y0")
    _untouched(y1, before[1], _s32_mask(y1, b, 0, n), "S32 y1")
    fm = torch.zeros(fbuf.shape, dtype=torch.bool, device=DEV)
    fm[:b, 1:n + 1] = True
    _untouched(fbuf, before[2], fm, "fp32 NCHW")
    outs = dict(f32=fbuf[:b, 1:n + 1].clone(), y0=_s32_written(y0, b, 1, n), y1=_s32_written(y1, b, 0, n))
    if first:
        pad = _s32_values(y0, b, 1, g * 32)[:, n:]
        assert bool((pad == 0).all()), "S32 padding channels above N no longer hold zeros"
    if nhwc is not None:
        nm = torch.zeros(nhwc.shape, dtype=torch.bool, device=DEV)
        nm[:b * h * w] = True
        _untouched(nhwc, before[3], nm, "fp32 NHWC")
        outs["nhwc"] = nhwc[:b * h * w].clone()
    return outs


def _epi0_outputs(monkeypatch, case, kh, kw, name, what):
    with _leaf(monkeypatch, name):
        a = _run_epi0(case, kh, kw, name, FILLS[0], True)
        c = _run_epi0(case, kh, kw, name, FILLS[1], False)
    _same(c, a, f"{what}: second run on differently dirtied destinations")
    return a


def _check_epi0(case, outs, what):
    b, h, w = case["shape"]
    ref, bound = case["ref"], case["bound"]
    tol = cc.conv_tol(bound)
    worst = 0.0
    for key, got in (("f32", outs["f32"].double()),
                     ("nhwc", outs["nhwc"].view(b, h, w, -1).permute(0, 3, 1, 2).double() if "nhwc" in outs else None)):
        if got is None:
            continue
        ratio = float(((got - ref).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what} {key}: worst err/tol {ratio:.3f}, max err {float((got - ref).abs().max()):.3e}"
    assert torch.equal(outs["y0"], outs["y1"]), f"{what}: the two S32 destinations differ"
    v = outs["y0"].float()
    got = (v[..., 0, :] + v[..., 1, :]).permute(0, 3, 1, 2).double()
    ratio = float(((got - ref).abs() / cc.conv_tol(bound, ref)).max())
    assert ratio <= 1.0, f"{what} S32: worst err/tol {ratio:.3f}"
    return max(worst, ratio)


@pytest.mark.parametrize("kh,kw,name", [pytest.param(kh, kw, name, id=f"{kh}x{kw}-{name}")
                                        for kh, kw in cc.KERNELS for name in cc.epi0_leaves(kh, kw)])
def test_epi0_leaf(monkeypatch, kh, kw, name):
    """Epilogue 0 (bias, S32 x 2 + fp32 NCHW + fp32 NHWC destinations) on one leaf over EPI0_CASES: float64 bound,
    bit identity with the LDS 128 leaf, untouched neighbours, two runs equal."""
    worst = 0.0
    for idx in range(len(cc.EPI0_CASES)):
        case = _epi0_case(kh, kw, idx)
        what = f"{kh}x{kw} {name} case {cc.EPI0_CASES[idx]}"
        base = _cached(("epi0-base", kh, kw, idx), lambda: _epi0_outputs(monkeypatch, case, kh, kw, "lds128", what))
        outs = _epi0_outputs(monkeypatch, case, kh, kw, name, what)
        worst = max(worst, _check_epi0(case, outs, what))
        _same(outs, base, f"{what} against the LDS 128 leaf")
    print(f"RATIO epi0 {kh}x{kw} {name}: {worst:.3f}")


# --------------------------------------------------------------------------------------------- GRU epilogues
def _gru_case(kh, kw, idx, addend):
    """Operands of one half-step on the GPU. Without the addend: the full form, input [h | inp | x] with biases; with
    it: the hoisted form, input [h | x], no bias, addend = fp32(W_inp * inp + bias) as NHWC column views."""
    def make():
        shape, ch, xc = cc.GRU_CASES[idx]
        b, hh, ww = shape
        h, inp, x, ws, bs = cc.gru_operands(kh, kw, ch, xc, shape, seed=77 * idx + kh)
        h, inp, x = h.to(DEV), inp.to(DEV), x.to(DEV)
        ws, bs = [t.to(DEV) for t in ws], [t.to(DEV) for t in bs]
        p = b * hh * ww
        if addend:
            wsel = [cc.hoist_split(t, ch)[0].contiguous() for t in ws]
            add = cc.gru_context_addend(inp, *ws, *bs, ch).float()  # fp32: the exact operand the kernel reads
            gx = torch.full((p, 3 * ch + 8), 5.5, device=DEV)
            gx[:, :3 * ch] = add.permute(0, 2, 3, 1).reshape(p, 3 * ch)
            xin = x
            czr = N.ConvWeights(torch.cat(wsel[:2]), None, -(-2 * ch // 128) * 128)
            cq = N.ConvWeights(wsel[2], None, 128)
            views = (gx[:, :2 * ch], gx[:, 2 * ch:3 * ch])
        else:
            wsel, add, views = ws, None, (None, None)
            xin = torch.cat([inp, x], dim=1)
            czr = N.ConvWeights(torch.cat(ws[:2]), torch.cat(bs[:2]), -(-2 * ch // 128) * 128)
            cq = N.ConvWeights(ws[2], bs[2], 128)
        in_s = N.s32_from_f32(torch.cat([h, xin], dim=1))
        seen = N.s32_to_f32(in_s)  # hi + lo: what the convolutions read
        ref = (lambda **kw_: cc.gru_half_hoisted(h, seen[:, ch:], add, *wsel, h_conv=seen[:, :ch], **kw_)) if addend else \
              (lambda **kw_: cc.gru_half_full(h, seen[:, ch:], *ws, *bs, h_conv=seen[:, :ch], **kw_))
        first = ref()
        return dict(shape=shape, ch=ch, kg=in_s.shape[3], h=h, in_s=in_s, czr=czr, cq=cq, views=views, ref=ref,
                    z_ref=first.z, rh_ref=first.rh)
    return _cached(("gru", kh, kw, idx, addend), make)


def _nhwc_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _nchw(rows, shape):
    b, hh, ww = shape
    return rows.view(b, hh, ww, -1).permute(0, 3, 1, 2)


def _run_gru(case, kh, kw, name, fill):
    """The gates launch (epilogue 1) then the candidate launch (epilogue 2) on sentinel-guarded buffers laid out as
    the model's: hx = [h | x...] and rhx = [r*h | x...] as groups 1.. of buffers with a guard group either side."""
    b, hh, ww = case["shape"]
    ch, kg = case["ch"], case["kg"]
    p = b * hh * ww
    f16, f32fill = fill
    hx = _s32_buf(b, hh, ww, kg + 2, f16)
    hx[:b, :, :, 1:1 + kg] = case["in_s"]
    rhx = hx.clone()
    rhx[:b, :, :, 1:1 + ch // 32] = f16  # r*h not yet written: dirt
    z = torch.full((p + GUARD_ROWS, ch), f32fill, device=DEV)
    hm = torch.full((p + GUARD_ROWS, ch), f32fill, device=DEV)
    hm[:p] = _nhwc_rows(case["h"])
    rows = torch.zeros(z.shape, dtype=torch.bool, device=DEV)
    rows[:p] = True
    before = [t.clone() for t in (hx, rhx, z, hm)]
    N.conv_s32(N.S32Slice(hx[:b], 1, kg), case["czr"], 128, epilogue=1, y0=N.S32Slice(rhx[:b], 1, ch // 32), gru_h=hm[:p],
               gru_z=z[:p], addend=case["views"][0])
    torch.cuda.synchronize()
    _assert_leaf(kh, kw, 1, name)
    assert torch.equal(_bits(hx), _bits(before[0])) and torch.equal(_bits(hm), _bits(before[3])), "gates launch wrote its inputs"
    _untouched(rhx, before[1], _s32_mask(rhx, b, 1, ch), "gates launch, S32 r*h")
    _untouched(z, before[2], rows, "gates launch, z")
    outs = dict(z=z[:p].clone(), rh=_s32_written(rhx, b, 1, ch))
    mid = [t.clone() for t in (hx, rhx, z, hm)]
    N.conv_s32(N.S32Slice(rhx[:b], 1, kg), case["cq"], 128, epilogue=2, y0=N.S32Slice(hx[:b], 1, ch // 32), gru_h=hm[:p],
               gru_z=z[:p], addend=case["views"][1])
    torch.cuda.synchronize()
    _assert_leaf(kh, kw, 2, name)
    assert torch.equal(_bits(rhx), _bits(mid[1])) and torch.equal(_bits(z), _bits(mid[2])), "candidate launch wrote its inputs"
    _untouched(hx, mid[0], _s32_mask(hx, b, 1, ch), "candidate launch, S32 h")
    _untouched(hm, mid[3], rows, "candidate launch, master h")
    outs.update(hm=hm[:p].clone(), hs=_s32_written(hx, b, 1, ch))
    return outs


def _gru_outputs(monkeypatch, case, kh, kw, name, what):
    with _leaf(monkeypatch, name):
        a = _run_gru(case, kh, kw, name, FILLS[0])
        c = _run_gru(case, kh, kw, name, FILLS[1])
    _same(c, a, f"{what}: second run on differently dirtied destinations")
    return a


def _s32_to_nchw(written):
    v = written.float()
    return (v[..., 0, :] + v[..., 1, :]).permute(0, 3, 1, 2).double()


def _check_gru(case, outs, what):
    shape = case["shape"]
    zg = _nchw(outs["z"], shape).double()
    rh = _s32_to_nchw(outs["rh"])
    e_z = float((zg - case["z_ref"]).abs().max())
    e_rh = float((rh - case["rh_ref"]).abs().max())
    second = case["ref"](rh=rh, z=zg)  # the candidate launch on what the gates launch stored
    hn = _nchw(outs["hm"], shape).double()
    e_h = float((hn - second.h).abs().max())
    e_s = float((_s32_to_nchw(outs["hs"]) - hn).abs().max())
    assert e_z <= 2e-6 and e_rh <= 2e-6 and e_h <= 2e-6, f"{what}: z {e_z:.3e}, r*h {e_rh:.3e}, h' {e_h:.3e} (bound 2e-6)"
    assert e_s <= 2.0 ** -21, f"{what}: S32 copy of h' off the fp32 master by {e_s:.3e}"
    return max(e_z, e_rh, e_h) / 2e-6, e_s / 2.0 ** -21


@pytest.mark.parametrize("addend", [True, False], ids=["addend", "bias"])
@pytest.mark.parametrize("name", cc.GRU_LEAVES)
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)], ids=["1x5", "5x1"])
@pytest.mark.parametrize("flags", [0, 256], ids=["hw", "libm"])
def test_gru_leaf(monkeypatch, flags, kh, kw, name, addend):
    """One SepConvGRU half-step (gates launch, candidate launch) on one leaf over GRU_CASES, with the hoisted context
    addend or in the full form with biases, with the hardware gates (flags 0) and libm's (256)."""
    lib = N.load()
    lib.oflow_exp_set_conv_flags(flags)
    worst = (0.0, 0.0)
    try:
        for idx in range(len(cc.GRU_CASES)):
            case = _gru_case(kh, kw, idx, addend)
            what = f"{kh}x{kw} {name} flags {flags} {'addend' if addend else 'bias'} case {cc.GRU_CASES[idx]}"
            base = _cached(("gru-base", flags, kh, kw, idx, addend),
                           lambda: _gru_outputs(monkeypatch, case, kh, kw, "lds128", what))
            outs = _gru_outputs(monkeypatch, case, kh, kw, name, what)
            r = _check_gru(case, outs, what)
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
            _same(outs, base, f"{what} against the LDS 128 leaf")
    finally:
        lib.oflow_exp_set_conv_flags(0)
    print(f"RATIO gru {kh}x{kw} {name} flags {flags} {'addend' if addend else 'bias'}: gates/blend {worst[0]:.3f}, "
          f"S32 copy {worst[1]:.3f}")


def _single_valued(values, keys, gate, what):
    """values (fp32) must be one function of the integer keys: the same bits wherever a key recurs, and that value
    within 2e-6 of the float64 gate of the key."""
    values, keys = values.reshape(-1), keys.reshape(-1)
    for k in torch.unique(keys).tolist():
        sel = values[keys == k]
        assert bool((_bits(sel) == _bits(sel[:1])).all()), f"{what}: pre-activation {k} gave {torch.unique(sel).tolist()}"
        err = abs(float(sel[0].double()) - float(gate(torch.tensor(float(k), dtype=torch.float64))))
        assert err <= 2e-6, f"{what}: gate({k}) off by {err:.3e}"


@pytest.mark.parametrize("ch", [128, 64])
@pytest.mark.parametrize("name", cc.GRU_LEAVES)
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)], ids=["1x5", "5x1"])
def test_gru_leaf_integer_exact(monkeypatch, kh, kw, name, ch):
    """Operands in {-1, 0, 1}, weights one-hot (the centre tap of channel (7n + 5) % cin, plus s(n) in {-1, 1, 2} times
    tap n % 5 of channel (5n + 3) % cin), integer biases and addend: every product and partial sum is exact, so the
    pre-activation is the integer v the float64 convolution gives. z and r (through r*h with h = +-1: r to the 22 bits
    of the S32 store) must then be single-valued in v, and with z = 1 the blend returns q = tanh(v) itself, with z = 0
    h itself, bit for bit. |v| <= 5, where neighbouring integers' gates differ by > 5e-4: a value taken from another
    lane's pixel or channel cannot pass."""
    g = cc.gen(31 + kh + ch)
    b, hh, ww = cc.SHAPE_RAGGED
    cin = ch + 96
    p = b * hh * ww
    xin = torch.randint(-1, 2, (b, cin, hh, ww), generator=g).float()
    hmaster = xin[:, :ch].clone()
    hmaster[hmaster == 0] = 1.0  # r*h reveals r only where h != 0; the master need not equal the S32 copy of h

    def onehot(n_out):
        wt = torch.zeros(n_out, cin, kh, kw)
        for n in range(n_out):
            wt.view(n_out, cin, -1)[n, (7 * n + 5) % cin, 2] += 1.0
            wt.view(n_out, cin, -1)[n, (5 * n + 3) % cin, n % 5] += (-1.0, 1.0, 2.0)[n % 3]
        return wt

    wzr, wq = onehot(2 * ch), onehot(ch)
    bzr = torch.randint(-1, 2, (2 * ch,), generator=g).float()
    bq = torch.randint(-1, 2, (ch,), generator=g).float()
    gx = torch.randint(-1, 2, (p, 3 * ch), generator=g).float().to(DEV)
    add = _nchw(gx, (b, hh, ww)).double().cpu()
    pad = (kh // 2, kw // 2)
    v_zr = torch.nn.functional.conv2d(xin.double(), wzr.double(), bzr.double(), padding=pad) + add[:, :2 * ch]
    v_q = torch.nn.functional.conv2d(xin.double(), wq.double(), bq.double(), padding=pad) + add[:, 2 * ch:]
    assert float(v_zr.abs().max()) <= 5 and float(v_q.abs().max()) <= 5
    in_s = N.s32_from_f32(xin.to(DEV))
    czr = N.ConvWeights(wzr.to(DEV), bzr.to(DEV), -(-2 * ch // 128) * 128)
    cq = N.ConvWeights(wq.to(DEV), bq.to(DEV), 128)
    kg = cin // 32
    what = f"{kh}x{kw} {name} ch {ch}"
    for flags in (0, 256):
        N.load().oflow_exp_set_conv_flags(flags)
        try:
            with _leaf(monkeypatch, name):
                rhx = _s32_buf(b, hh, ww, kg + 2, FILLS[0][0])
                z = torch.full((p, ch), FILLS[0][1], device=DEV)
                hm = _nhwc_rows(hmaster).to(DEV)
                N.conv_s32(N.S32Slice(in_s), czr, 128, epilogue=1, y0=N.S32Slice(rhx[:b], 1, ch // 32), gru_h=hm, gru_z=z,
                           addend=gx[:, :2 * ch])
                torch.cuda.synchronize()
                _assert_leaf(kh, kw, 1, name)
                zi = torch.zeros(p, ch)
                zi[::2, ::3] = 1.0
                zi[1::2, 1::2] = 1.0
                zi = zi.to(DEV)
                hx = _s32_buf(b, hh, ww, kg + 2, FILLS[0][0])
                hm2 = hm.clone()
                N.conv_s32(N.S32Slice(in_s), cq, 128, epilogue=2, y0=N.S32Slice(hx[:b], 1, ch // 32), gru_h=hm2, gru_z=zi,
                           addend=gx[:, 2 * ch:])
                torch.cuda.synchronize()
                _assert_leaf(kh, kw, 2, name)
        finally:
            N.load().oflow_exp_set_conv_flags(0)
        sig = torch.sigmoid
        _single_valued(_nchw(z, (b, hh, ww)).cpu(), v_zr[:, :ch].round().long(), sig, f"{what} flags {flags} z")
        rh = _s32_values(rhx, b, 1, ch).cpu()
        # r*h with h = +-1 is +-r, rounded to the S32 store's 22 bits; keyed by (v, sign of h)
        keys = v_zr[:, ch:].round().long()
        _single_valued(rh * hmaster, keys, sig, f"{what} flags {flags} r")
        hn = _nchw(hm2, (b, hh, ww)).cpu()
        zsel = _nchw(zi, (b, hh, ww)).cpu() == 1.0
        _single_valued(hn[zsel], v_q.round().long()[zsel], torch.tanh, f"{what} flags {flags} q")
        assert torch.equal(hn[~zsel], hmaster[~zsel]), f"{what}: z = 0 must return h itself"
        assert float((_s32_values(hx, b, 1, ch).cpu() - hn).abs().max()) <= 2.0 ** -21


# ----------------------------------------------------------------------------------------------- module level
class _FixedCorr:
    """Stands in for CorrBlock: hands the given lookup outputs to SplitUpdate (as NHWC rows) in order."""

    def __init__(self, corrs):
        self.corrs = list(corrs)

    def lookup_nhwc(self, coords, out):
        b, _, h, w = coords.shape
        out.view(b, h, w, -1).copy_(self.corrs.pop(0).permute(0, 2, 3, 1))
        return out


@contextlib.contextmanager
def _recorded_leaves(monkeypatch):
    """Every leaf N.conv_s32 launches inside the block, as a set."""
    seen = set()
    real = N.conv_s32

    def conv_s32(*args, **kwargs):
        real(*args, **kwargs)
        seen.add(cc.decode_leaf(N.load().oflow_exp_last_conv_leaf()))

    with monkeypatch.context() as m:
        m.setattr(N, "conv_s32", conv_s32)
        yield seen


def _assert_gru_leaves(seen, px):
    """The GRU launches ran on the small-grid tiles (threshold 16384) or on the register-direct production tiles (0),
    and no launch at all used the 2-row tiles under threshold 0."""
    name = "small" if px else "breg128"
    for kh, kw in ((1, 5), (5, 1)):
        for epi in (1, 2):
            assert cc.expected_leaf(kh, kw, epi, name) in seen, (px, kh, kw, epi, sorted(seen))
    if px == 0:
        assert all(leaf.ty != 2 for leaf in seen), sorted(seen)


def _raft():
    from model import RAFT, synthetic

    m = RAFT().eval()
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    return m.to(DEV)


def test_split_update_same_bits_on_small_grid_and_production_tiles(monkeypatch):
    """The body of test_gpu_raft.py::test_split_update_matches_module_update_block (two steps at 2 x 24 x 40, mask
    head on) under both small-grid thresholds: every output of the two runs bit-identical, each within that test's
    1e-4 * max(1, |ref|) of the nn.Module update block."""
    from model import synthetic
    from model.update import SplitUpdate
    from model.utils import coords_grid

    block = _raft().update_block
    b, h, w = 2, 24, 40
    g = lambda s, shape, std: torch.from_numpy(synthetic.hash_normal(s, shape, std)).to(DEV)
    cnet_out = g(1, (b, 256, h, w), 1.0)
    net, inp = torch.tanh(cnet_out[:, :128]), torch.relu(cnet_out[:, 128:])
    corr1, corr2 = g(3, (b, 324, h, w), 2.0), g(4, (b, 324, h, w), 2.0)
    coords0 = coords_grid(b, h, w, device=DEV)
    coords1 = coords0 + g(5, (b, 2, h, w), 3.0)
    runs = {}
    with torch.inference_mode():
        n1, m1, d1 = block(net, inp, corr1, coords1 - coords0)
        c1 = coords1 + d1
        n2, m2, d2 = block(n1, inp, corr2, c1 - coords0)
        c2 = c1 + d2
        for px in (16384, 0):
            with _small_grid_px(px), _recorded_leaves(monkeypatch) as seen:
                runner = SplitUpdate(block, cnet_out.contiguous(), 128)
                cc_ = coords1.clone()
                fake = _FixedCorr([corr1, corr2])
                s1 = runner.step(fake, cc_, need_mask=True).clone()
                cc1 = cc_.clone()
                h1 = runner.hm.view(b, h, w, 128).permute(0, 3, 1, 2).clone()
                s2 = runner.step(fake, cc_, need_mask=True).clone()
                h2 = runner.hm.view(b, h, w, 128).permute(0, 3, 1, 2).clone()
                torch.cuda.synchronize()
            _assert_gru_leaves(seen, px)
            runs[px] = dict(net1=h1, mask1=s1, coords1=cc1, net2=h2, mask2=s2, coords2=cc_)
    refs = dict(net1=n1, mask1=m1, coords1=c1, net2=n2, mask2=m2, coords2=c2)
    for px, outs in runs.items():
        for what, ref in refs.items():
            err = float((ref - outs[what]).abs().max())
            assert err <= 1e-4 * max(1.0, float(ref.abs().max())), (px, what, err)
    for what in refs:
        assert torch.equal(runs[0][what], runs[16384][what]), f"{what}: small-grid and production tiles differ"


def test_pair_lanes_forward_same_bits_on_small_grid_and_production_tiles(monkeypatch):
    """One two-lane forward of the model at a 24 x 40 grid under threshold 0 against threshold 16384: bit-identical."""
    from model import synthetic

    model = _raft()
    assert model.pair_lanes == 2
    img0, img1 = synthetic.synthetic_pair(2, 192, 320, seed=5)
    p0, p1 = img0.to(DEV), img1.to(DEV)
    outs = {}
    with torch.inference_mode():
        for px in (16384, 0):
            with _small_grid_px(px), _recorded_leaves(monkeypatch) as seen:
                low, up = model(p0, p1, iters=3, test_mode=True)
                outs[px] = (low.clone(), up.clone())
                torch.cuda.synchronize()
            _assert_gru_leaves(seen, px)
    assert bool(torch.isfinite(outs[0][1]).all())
    assert torch.equal(outs[0][0], outs[16384][0]) and torch.equal(outs[0][1], outs[16384][1])
