"""FusedUpdate's elementwise kernels (csrc/update_fused.hip: oflow_bias_act_f32, oflow_gru_reset_f32,
oflow_gru_blend_f32) through N.bias_act_, N.gru_reset, N.gru_blend_ against the float64 restatements of
tests/conv_s32_cases.py (pinned against the update block by tests/test_conv_s32_cases_host.py).

Each entry point picks a float4 kernel when P % 4 == 0, every base is 16-B aligned and every batch stride is a multiple
of 4 floats, else a scalar one. Both run here, chosen exactly as the entry points' ``v4`` expressions choose: layout
"vec" (aligned bases, packed strides), "offset" (every base one float further), "stride" (batch strides one float
longer), and P % 4 != 0; the test recomputes ``v4`` from the pointers it passes and asserts it takes the value the layout
was built for. On the same values all layouts must agree bit for bit. Every tensor is a channel slice of a larger
sentinel-filled buffer (the hx / rhx use in FusedUpdate) with a trailing guard batch; nothing outside the slice may
change.

Bounds. "none" and ReLU equal the fp32 CPU evaluation of (x + bias), max(., 0), * scale exactly (contraction is off in
update_fused.hip). The sigmoid / tanh paths call the device's expf / tanhf: the same formula is evaluated op by op with
PyTorch's fp32 CPU kernels, its maximum error against float64 on the same inputs is taken inside the test, and the GPU
may be off by 4x that, at least 2^-24 (a second libm may differ from the first by a couple of ulp).
Measured on an MI355X (worst GPU error / that allowance over all cases): bias_act sigmoid / tanh 0.668,
gru_reset 0.305, gru_blend 0.261 (most cases give 0.250: the GPU's worst error equal to the CPU evaluation's own).
"""
import ctypes

import pytest
import torch

import conv_s32_cases as cc
from optical_flow import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = -12345.5
E_NULL, E_SHAPE, E_MODE = -1, -2, -6  # include/oflow.h
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    N.load()


class _Slice:
    """Channels [c0, c0 + c) of a (b + 1, ctot, 1, p) fp32 buffer laid out by ``layout``, carved from a flat sentinel
    buffer; ``view`` is the (b, c, 1, p) tensor the wrappers take, ``mask`` marks its elements in the flat buffer."""

    def __init__(self, b, c, p, layout, c0=1, extra=2, values=None):
        ctot = c + c0 + extra
        bs = ctot * p + (1 if layout == "stride" else 0)
        off = c0 * p + (1 if layout == "offset" else 0)
        self.flat = torch.full(((b + 1) * bs + 8,), SENTINEL, device=DEV)
        size, stride = (b, c, 1, p), (bs, p, p, 1)
        self.view = self.flat.as_strided(size, stride, off)
        self.mask = torch.zeros(self.flat.shape, dtype=torch.bool, device=DEV)
        self.mask.as_strided(size, stride, off).fill_(True)
        if values is not None:
            self.view.copy_(values.view(size))
        self.before = self.flat.clone()

    def untouched(self, what):
        a, c = self.flat.view(torch.int32), self.before.view(torch.int32)
        assert torch.equal(a[~self.mask], c[~self.mask]), f"{what}: wrote outside its slice"

    def unchanged(self, what):
        assert torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32)), f"{what}: input was written"

    def vec_ok(self):
        return self.view.data_ptr() % 16 == 0 and self.view.stride(0) % 4 == 0


def _expect_branch(p, layout, *slices):
    """The entry points' ``v4`` for these operands; it must be what the layout was built to select."""
    v4 = p % 4 == 0 and all(s.vec_ok() for s in slices)
    assert v4 == (layout == "vec" and p % 4 == 0), (p, layout, [s.view.data_ptr() % 16 for s in slices])
    return v4


def _allow(f32, f64):
    """4x the fp32 CPU evaluation's own maximum error against float64, at least 2^-24."""
    return max(4.0 * float((f32.double() - f64).abs().max()), FLOOR)


BIAS_ACT_OPTIONS = [
    # act, scale, bias, out2, in place (y0 aliasing x)
    ("none", 1.0, True, False, True),
    ("relu", 1.0, True, True, False),    # the motion encoder's last ReLU into hx and rhx
    ("relu", 0.25, False, False, True),
    ("none", 0.25, True, True, False),   # the mask head's x0.25
    ("sigmoid", 1.0, True, False, False),
    ("sigmoid", 0.25, False, True, True),
    ("tanh", 1.0, True, True, True),
    ("tanh", 0.25, False, False, False),
]


@pytest.mark.parametrize("b,c", cc.FUSED_BC)
@pytest.mark.parametrize("p", cc.FUSED_P)
def test_bias_act(p, b, c):
    g = cc.gen(p * 1000 + b * 10 + c)
    x = torch.randn(b, c, p, generator=g) * 3
    x.view(-1)[:: max(1, x.numel() // 7)] = 0.0  # exact zeros: ReLU's boundary
    bias = torch.randn(c, generator=g)
    worst = 0.0
    saw = set()
    for act, scale, use_bias, use_out2, inplace in BIAS_ACT_OPTIONS:
        bb = bias if use_bias else None
        f64 = cc.bias_act_ref(x, bb, act, scale)
        f32 = cc.bias_act_ref(x, bb, act, scale, dtype=torch.float32)
        allow = 0.0 if act in ("none", "relu") else _allow(f32, f64)
        results = []
        for layout in cc.FUSED_LAYOUTS:
            what = f"bias_act {act} x{scale} bias={use_bias} out2={use_out2} inplace={inplace} {layout}"
            xs = _Slice(b, c, p, layout, values=x.to(DEV))
            ys = xs if inplace else _Slice(b, c, p, layout, c0=2, extra=1)
            y2 = _Slice(b, c, p, layout, c0=0, extra=3) if use_out2 else None
            saw.add(_expect_branch(p, layout, *(s for s in (xs, ys, y2) if s is not None)))
            out = N.bias_act_(xs.view, None if bb is None else bb.to(DEV), act, scale, out=None if inplace else ys.view,
                              out2=None if y2 is None else y2.view)
            torch.cuda.synchronize()
            assert out.data_ptr() == ys.view.data_ptr()
            if not inplace:
                xs.unchanged(what)
            ys.untouched(what)
            got = ys.view.reshape(b, c, p).cpu()
            if y2 is not None:
                y2.untouched(what)
                assert torch.equal(y2.view.reshape(b, c, p).cpu(), got), f"{what}: the two destinations differ"
            if allow == 0.0:
                assert torch.equal(got, f32), f"{what}: differs from the fp32 evaluation"
            else:
                err = float((got.double() - f64).abs().max())
                worst = max(worst, err / allow)
                assert err <= allow, f"{what}: max err {err:.3e}, allowed {allow:.3e}"
            results.append(got)
        for r in results[1:]:
            assert torch.equal(r, results[0]), f"bias_act {act}: the layouts (float4 / scalar branches) differ"
    assert saw == ({True, False} if p % 4 == 0 else {False})
    print(f"RATIO bias_act P={p} B={b} C={c}: {worst:.3f}")


@pytest.mark.parametrize("b,ch", cc.FUSED_BC)
@pytest.mark.parametrize("p", cc.FUSED_P)
def test_gru_reset_and_blend(p, b, ch):
    """gru_reset (r*h into the rhx slice) and gru_blend_ (h updated in place in the hx slice) on [z | r] and q
    pre-bias convolution outputs, h a channel slice of a wider buffer."""
    g = cc.gen(p * 1000 + b * 10 + ch + 1)
    zr = torch.randn(b, 2 * ch, p, generator=g) * 2
    q = torch.randn(b, ch, p, generator=g) * 2
    h = torch.tanh(torch.randn(b, ch, p, generator=g))
    bz, br, bq = (torch.randn(ch, generator=g) for _ in range(3))
    rh64, rh32 = cc.gru_reset_ref(zr, br, h), cc.gru_reset_ref(zr, br, h, dtype=torch.float32)
    hn64, hn32 = cc.gru_blend_ref(zr, bz, q, bq, h), cc.gru_blend_ref(zr, bz, q, bq, h, dtype=torch.float32)
    allow_r, allow_h = _allow(rh32, rh64), _allow(hn32, hn64)
    results = []
    saw = set()
    for layout in cc.FUSED_LAYOUTS:
        zs = _Slice(b, 2 * ch, p, layout, c0=0, extra=0, values=zr.to(DEV))
        hs = _Slice(b, ch, p, layout, c0=0, extra=5, values=h.to(DEV))    # hx = [h | x]
        rs = _Slice(b, ch, p, layout, c0=0, extra=5)                      # rhx = [r*h | x]
        qs = _Slice(b, ch, p, layout, c0=1, extra=0, values=q.to(DEV))
        saw.add(_expect_branch(p, layout, zs, hs, rs))
        N.gru_reset(zs.view, br.to(DEV), hs.view, rs.view)
        torch.cuda.synchronize()
        zs.unchanged(f"gru_reset {layout} zr")
        hs.unchanged(f"gru_reset {layout} h")
        rs.untouched(f"gru_reset {layout} rh")
        rh = rs.view.reshape(b, ch, p).cpu()
        err_r = float((rh.double() - rh64).abs().max())
        assert err_r <= allow_r, f"gru_reset {layout}: max err {err_r:.3e}, allowed {allow_r:.3e}"
        saw.add(_expect_branch(p, layout, zs, qs, hs))
        N.gru_blend_(zs.view, bz.to(DEV), qs.view, bq.to(DEV), hs.view)
        torch.cuda.synchronize()
        zs.unchanged(f"gru_blend {layout} zr")
        qs.unchanged(f"gru_blend {layout} q")
        hs.untouched(f"gru_blend {layout} h")
        hn = hs.view.reshape(b, ch, p).cpu()
        err_h = float((hn.double() - hn64).abs().max())
        assert err_h <= allow_h, f"gru_blend {layout}: max err {err_h:.3e}, allowed {allow_h:.3e}"
        results.append((rh, hn, err_r / allow_r, err_h / allow_h))
    for r in results[1:]:
        assert torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]), "the layouts (branches) differ"
    assert saw == ({True, False} if p % 4 == 0 else {False})
    print(f"RATIO gru_reset P={p} B={b} CH={ch}: {max(r[2] for r in results):.3f}; "
          f"gru_blend: {max(r[3] for r in results):.3f}")


def test_error_returns_write_nothing():
    """NULL x / y0 -> OFLOW_E_NULL, a non-positive size -> OFLOW_E_SHAPE, activation 4 -> OFLOW_E_MODE (raw entry
    points: the wrappers would refuse first); no destination byte changes."""
    lib = N.load()
    b, c, p = 2, 3, 8
    x = torch.randn(b, c, p).to(DEV)
    bias = torch.randn(c).to(DEV)
    y0 = torch.full((b, c, p), SENTINEL, device=DEV)
    y1 = torch.full((b, c, p), SENTINEL, device=DEV)
    s = c * p

    def bias_act(px, py, bb=b, cc_=c, pp=p, act=1):
        return lib.oflow_bias_act_f32(px, s, bias.data_ptr(), py, s, y1.data_ptr(), s, bb, cc_, pp, act, 1.0, None)

    assert bias_act(None, y0.data_ptr()) == E_NULL
    assert bias_act(x.data_ptr(), None) == E_NULL
    for kw in (dict(bb=0), dict(cc_=0), dict(pp=0), dict(bb=-1), dict(pp=-4)):
        assert bias_act(x.data_ptr(), y0.data_ptr(), **kw) == E_SHAPE, kw
    assert bias_act(x.data_ptr(), y0.data_ptr(), act=4) == E_MODE
    assert bias_act(x.data_ptr(), y0.data_ptr(), act=-1) == E_MODE
    zr = torch.randn(b, 2 * c, p).to(DEV)
    h = torch.full((b, c, p), SENTINEL, device=DEV)
    q = torch.randn(b, c, p).to(DEV)
    ptr = lambda t: t.data_ptr()
    reset = [ptr(zr), 2 * s, ptr(bias), ptr(h), s, ptr(y0), s, b, c, p, None]
    blend = [ptr(zr), 2 * s, ptr(bias), ptr(q), s, ptr(bias), ptr(h), s, b, c, p, None]
    for fn, args, ptrs, sizes in ((lib.oflow_gru_reset_f32, reset, (0, 2, 3, 5), (7, 8, 9)),
                                  (lib.oflow_gru_blend_f32, blend, (0, 2, 3, 5, 6), (8, 9, 10))):
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == E_NULL, (fn.__name__, i)
        for i in sizes:
            for v in (0, -3):
                bad = list(args)
                bad[i] = v
                assert fn(*bad) == E_SHAPE, (fn.__name__, i, v)
    torch.cuda.synchronize()
    for t in (y0, y1, h):
        assert bool((t == SENTINEL).all())
    # and the same arguments, valid, do run
    assert bias_act(x.data_ptr(), y0.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, torch.relu(x + bias.view(1, c, 1))) and torch.equal(y1, y0)
