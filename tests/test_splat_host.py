"""Forward warping without a GPU: identities of the float64 reference (tests/splat_cases.py), the fixed-point scheme's
NumPy emulation against the derived bound, the calibration of the backward tolerance, the CPU path of
optical_flow.splat and its autograd, interpolate_frame, the operators' registration / schemas / Meta kernels, and the C
ABI's argument errors (nothing is launched)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import splat_cases as sc
import optical_flow
from conftest import GOLDEN
from optical_flow import _native, _ops, interpolate_frame, splat

SMOOTH_SUM_IDS = [c.name for c in sc.CASES if c.name.endswith("-gauss2-sum")]
SMOOTH_SUM_2D_IDS = [c.name for c in sc.CASES if c.name.endswith("-gauss2-sum") and min(c.frame.shape[2:]) > 1]


# ------------------------------------------------------------------------------------------ the reference's identities
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_zero_flow_is_the_identity(shape):
    for mode in ("sum", "avg"):
        case = sc.BY_NAME["{}x{}x{}x{}-zero-{}".format(*shape, mode)]
        ref = sc.reference(case)
        assert np.array_equal(ref.weight, np.ones_like(ref.weight)) and not ref.hole.any()
        if mode == "sum":
            assert np.array_equal(ref.out, case.frame.astype(np.float64))
        else:
            np.testing.assert_allclose(ref.out, case.frame.astype(np.float64) / (1.0 + sc.EPS), rtol=1e-15, atol=0)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_integer_shift_moves_pixels_exactly(shape):
    case = sc.BY_NAME["{}x{}x{}x{}-shift-sum".format(*shape)]
    ref = sc.reference(case)
    dx, dy = sc.SHIFT
    b, c, h, w = shape
    want = np.zeros(shape)
    for i in range(h):
        for j in range(w):
            if 0 <= i + dy < h and 0 <= j + dx < w:
                want[:, :, i + dy, j + dx] = case.frame[:, :, i, j]
    assert np.array_equal(ref.out, want)


@pytest.mark.parametrize("name", SMOOTH_SUM_IDS)
def test_mass_is_conserved_for_sources_whose_taps_are_inside(name):
    """"sum" of a frame that is zero at every source with a tap outside: each source's four weights add up to 1."""
    case = sc.BY_NAME[name]
    geo = sc.geometry(case.flow)
    inside = np.logical_and.reduce([ok for ok, *_ in geo.taps]).reshape(case.flow.shape[0], 1, *case.flow.shape[2:])
    frame = np.where(inside, case.frame, np.float32(0))
    ref = sc.reference(case._replace(name=name + "-inside", frame=frame))
    total, mass = ref.out.sum(axis=(2, 3)), frame.astype(np.float64).sum(axis=(2, 3))
    scale = np.abs(frame).astype(np.float64).sum(axis=(2, 3))
    assert (np.abs(total - mass) <= 1e-13 * scale).all()


@pytest.mark.parametrize("name", SMOOTH_SUM_2D_IDS)
def test_transpose_identity(name):
    """<splat(x), g> = <x, bilinear-sample(g)>: the summation splat is the transpose of F.grid_sample (zeros padding,
    align_corners=True) at the landing positions."""
    case = sc.BY_NAME[name]  # (grid_sample's normalisation needs two pixels per axis: the 2-D shapes)
    b, c, h, w = case.frame.shape
    ref = sc.reference(case)
    g = torch.from_numpy(case.grad_out).double()
    px = (torch.arange(w, dtype=torch.float32).view(1, 1, w) + torch.from_numpy(case.flow[:, 0])).double()
    py = (torch.arange(h, dtype=torch.float32).view(1, h, 1) + torch.from_numpy(case.flow[:, 1])).double()
    grid = torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], dim=-1)
    sampled = F.grid_sample(g, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    lhs = float((torch.from_numpy(ref.out) * g).sum())
    rhs = float((torch.from_numpy(case.frame).double() * sampled).sum())
    scale = float((torch.from_numpy(ref.num_abs.reshape(ref.out.shape)) * g.abs()).sum())
    assert abs(lhs - rhs) <= 1e-9 * scale  # (float64 against float64: the grid normalisation's roundings)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_closed_form_gradients_equal_autograd(name):
    case = sc.BY_NAME[name]
    for ref, got in zip(sc.backward_reference(case), sc.closed_form(case)):
        if ref is None:
            assert got is None
            continue
        value, bound, _ = ref
        assert (np.abs(value - got) <= 1e-12 * bound).all()
    if "-nonfinite-" in name:  # skipped sources get zero gradients
        geo = sc.geometry(case.flow)
        skipped = ~geo.keep.reshape(case.flow.shape[0], 1, *case.flow.shape[2:])
        assert skipped.any()
        for ref in sc.backward_reference(case):
            if ref is not None:
                assert not ref[0][np.broadcast_to(skipped, ref[0].shape)].any()


def test_committed_cases_cover_what_they_claim():
    assert sc.frac_bits(1, 1) == 60 and sc.frac_bits(2048, 2048) == 38 and sc.frac_bits(436, 1024) == 41
    lib = _native.load()
    for h, w in ((1, 1), (1, 9), (33, 130), (55, 128), (436, 1024), (2048, 2048)):
        assert lib.oflow_splat_frac_bits(h, w) == sc.frac_bits(h, w)
    collapse = sc.reference(sc.BY_NAME["2x8x33x130-collapse-sum"])
    assert collapse.weight.max() == 33 * 130 and (collapse.weight > 0).sum() == 2  # every source on one pixel
    big = sc.reference(sc.BY_NAME["2x8x33x130-gaussbig-sum"])
    assert sc.geometry(sc.BY_NAME["2x8x33x130-gaussbig-sum"].flow).keep.mean() < 0.5 and big.hole.any()
    lin = sc.BY_NAME["3x3x7x65-gauss2-linear"]
    ref = sc.reference(lin)
    assert ((ref.weight == 0) & ~ref.hole).any()  # D = 0 where sources did land
    sat = sc.BY_NAME["2x8x33x130-gauss2-soft-s30"]
    m = sc.source_weight(sat, device_like=True)
    assert (m == 1).sum() == 2 and (m < sc.TINY32).mean() > 0.3  # saturated; small weights underflow
    border = sc.geometry(sc.BY_NAME["3x3x7x65-border-sum"].flow)
    assert border.keep.all()
    mixed = sc.BY_NAME["2x3x9x33-gauss2-sum-mixed"]
    e_n, _ = sc.exponents(mixed)
    assert e_n[0] - e_n[1] >= 26  # scales 1e8 apart


# ------------------------------------------------------------------------------------- the fixed-point scheme's emulation
@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_fixed_point_emulation_stays_within_the_bound(name):
    case = sc.BY_NAME[name]
    sc.assert_forward(case, *sc.emulate(case), "emulation")


def test_emulated_images_do_not_depend_on_their_batch():
    for case in sc.MIXED:
        out, weight = sc.emulate(case)
        for i in range(2):
            alone = case._replace(name=f"{case.name}-{i}", frame=case.frame[i:i + 1], flow=case.flow[i:i + 1],
                                  metric=None if case.metric is None else case.metric[i:i + 1],
                                  grad_out=case.grad_out[i:i + 1])
            o1, w1 = sc.emulate(alone)
            assert np.array_equal(o1.view(np.int32), out[i:i + 1].view(np.int32))
            assert np.array_equal(w1.view(np.int32), weight[i:i + 1].view(np.int32))


# ------------------------------------------------------------------------------------------ backward tolerance
def test_fp32_composition_calibrates_the_backward_tolerance():
    """The constants of splat_cases are four times what the operator's own fp32 composition needs."""
    worst = {n: (0.0, "") for n in sc.GRAD_NAMES}
    for case in sc.ALL_CASES:
        for n, r in zip(sc.GRAD_NAMES, sc.backward_ratios(case, sc.autograd_gradients(case, torch.float32))):
            if r is not None and r > worst[n][0]:
                worst[n] = (r, case.name)
    print("fp32 composition, worst err / (2^-24 bound):", worst)
    for n, k in zip(sc.GRAD_NAMES, (sc.K_FRAME, sc.K_FLOW, sc.K_METRIC)):
        assert worst[n][0] <= k / 4, (n, worst[n])
        assert worst[n][0] >= k / 16, (n, worst[n], "the constant is far from what was measured")


# ------------------------------------------------------------------------------------------ the operator's CPU path
@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_cpu_path_stays_within_the_bound_and_the_tolerance(name):
    case = sc.BY_NAME[name]
    frame, flow, metric = sc.tensors(case)
    out, weight = splat(frame, flow, metric, case.mode, return_weight=True)
    assert out.requires_grad and not weight.requires_grad
    sc.assert_forward(case, out.detach().numpy(), weight.numpy(), "cpu path")
    only = splat(frame, flow, metric, case.mode)
    assert isinstance(only, torch.Tensor) and torch.equal(only, out)
    leaves = [frame, flow] + ([metric] if metric is not None else [])
    grads = list(torch.autograd.grad((out * torch.from_numpy(case.grad_out)).sum(), leaves))
    sc.assert_backward(case, grads + [None] * (3 - len(grads)), "cpu path")


def test_cpu_path_converts_its_inputs():
    case = sc.BY_NAME["1x5x17x33-gauss2-soft-s2"]
    frame, flow, metric = sc.tensors(case, requires_grad=False)
    out, weight = splat(frame, flow, metric, "soft", return_weight=True)
    o64, w64 = splat(frame.double(), flow.double(), metric.double(), "soft", return_weight=True)
    assert o64.dtype == torch.float32 and torch.equal(o64, out) and torch.equal(w64, weight)
    wide = torch.zeros((1, 5, 17, 66))
    wide[..., ::2] = frame
    assert torch.equal(splat(wide[..., ::2], flow, metric, "soft"), out)
    empty, ew = splat(frame[:0], flow[:0], metric[:0], "soft", return_weight=True)
    assert tuple(empty.shape) == (0, 5, 17, 33) and tuple(ew.shape) == (0, 1, 17, 33)


def test_value_errors():
    f, fl, me = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError, match="unknown mode"):
        splat(f, fl, None, "max")
    for mode in ("sum", "avg"):
        with pytest.raises(ValueError, match="takes no metric"):
            splat(f, fl, me, mode)
    for mode in ("linear", "soft"):
        with pytest.raises(ValueError, match="needs a metric"):
            splat(f, fl, None, mode)
    with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
        splat(f, torch.zeros(1, 2, 4, 5))
    with pytest.raises(ValueError, match=r"\(B, 1, H, W\)"):
        splat(f, fl, torch.zeros(1, 2, 4, 4), "soft")
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        splat(torch.zeros(3, 4, 4), fl)
    with pytest.raises(TypeError, match="floating-point"):
        splat(f.long(), fl)
    with pytest.raises(ValueError, match="one device"):
        splat(f, fl.to("meta"))
    with pytest.raises(ValueError, match="unknown mode"):
        _native.splat(f, fl, None, "max")
    assert optical_flow.operator.splat is splat and optical_flow.operator.interpolate_frame is interpolate_frame
    assert "pixel units" in splat.__doc__ and "denormalize" in splat.__doc__


# ------------------------------------------------------------------------------------------ interpolate_frame
def test_interpolate_frame_of_a_translation():
    """A textured image translated by an even integer (dx, dy), exact flows, t = 0.5: the half-shifted image, exactly,
    on the pixels both frames reach."""
    g = torch.Generator().manual_seed(7)
    h, w, dx, dy = 12, 20, 4, -2
    canvas = torch.rand((2, 3, h + 8, w + 8), generator=g)

    def crop(ox, oy):  # the canvas seen through a window moved by (ox, oy): content moves by (-ox, -oy)
        return canvas[:, :, 4 + oy:4 + oy + h, 4 + ox:4 + ox + w].contiguous()

    frame0, mid, frame1 = crop(0, 0), crop(-dx // 2, -dy // 2), crop(-dx, -dy)
    flow_fw = torch.zeros(2, 2, h, w)
    flow_fw[:, 0], flow_fw[:, 1] = dx, dy
    got = interpolate_frame(frame0, frame1, flow_fw, -flow_fw, t=0.5)
    assert tuple(got.shape) == (2, 3, h, w) and got.dtype == torch.float32
    _, d0 = splat(frame0, 0.5 * flow_fw, None, "avg", return_weight=True)
    _, d1 = splat(frame1, -0.5 * flow_fw, None, "avg", return_weight=True)
    both = ((d0 > 0) & (d1 > 0)).expand_as(got)
    assert int(both.sum()) == 2 * 3 * (h - abs(dy)) * (w - abs(dx))
    # every reached pixel holds one source of weight 1: frame / (1 + EPS) in float64, rounded once
    want = (mid.double() / (1.0 + sc.EPS)).float()
    assert torch.equal(got[both], want[both])
    assert float((got[both] - mid[both]).abs().max()) <= 2.0**-22
    neither = ((d0 == 0) & (d1 == 0)).expand_as(got)
    assert not got[neither].any()
    # with metrics: softmax splatting; constant metrics change nothing here
    soft = interpolate_frame(frame0, frame1, flow_fw, -flow_fw, 0.5, torch.zeros(2, 1, h, w), torch.zeros(2, 1, h, w))
    assert torch.equal(soft, got)
    with pytest.raises(ValueError, match="both metrics"):
        interpolate_frame(frame0, frame1, flow_fw, -flow_fw, 0.5, torch.zeros(2, 1, h, w))
    doc = interpolate_frame.__doc__
    assert "-alpha * (frame0 - warp(frame1, normalize(flow_fw))).abs().mean(1, keepdim=True)" in doc


# ------------------------------------------------------------------------------------------ the registered operators
def test_ops_are_registered_with_the_recorded_schemas():
    _native.load()
    assert _ops.OPS_SPLAT == ("splat", "splat_backward") and not set(_ops.OPS_SPLAT) & set(_ops.OPS)
    with open(os.path.join(GOLDEN, "op_schemas_splat.txt")) as f:
        recorded = [line.rstrip("\n") for line in f if line.strip()]
    assert [str(getattr(torch.ops.oflow, name).default._schema) for name in _ops.OPS_SPLAT] == recorded
    for name in _ops.OPS_SPLAT:
        for key in ("CUDA", "CPU", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"oflow::{name}", key), (name, key)
    for sym in ("oflow_splat_frac_bits", "oflow_splat_workspace_bytes", "oflow_splat_f32", "oflow_splat_backward_f32"):
        assert sym in _native.SYMBOLS


def test_meta_kernels_and_gradients_on_meta_tensors():
    _native.load()
    meta = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    frame, flow, metric = meta(3, 5, 55, 128), meta(3, 2, 55, 128), meta(3, 1, 55, 128)
    for mode, me in ((0, None), (1, None), (2, metric), (3, metric)):
        out, weight = torch.ops.oflow.splat(frame, flow, me, mode)
        assert tuple(out.shape) == (3, 5, 55, 128) and tuple(weight.shape) == (3, 1, 55, 128)
        assert out.dtype == weight.dtype == torch.float32 and out.device.type == "meta"
        for mask in ([True, True, me is not None], [False, True, False], [True, False, False]):
            gs = torch.ops.oflow.splat_backward(out, frame, flow, me, out, weight, mode, mask)
            full = [(3, 5, 55, 128), (3, 2, 55, 128), (3, 1, 55, 128)]
            assert [tuple(g.shape) for g in gs] == [s if m else (0,) for s, m in zip(full, mask)]
    assert torch.ops.oflow.splat(frame.double(), flow, None, 0)[0].dtype == torch.float32
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        torch.ops.oflow.splat(frame, meta(3, 2, 55, 64), None, 0)
    with pytest.raises(RuntimeError, match="needs a metric"):
        torch.ops.oflow.splat(frame, flow, None, 3)
    with pytest.raises(RuntimeError, match="takes no metric"):
        torch.ops.oflow.splat(frame, flow, metric, 1)
    with pytest.raises(RuntimeError, match=r"outside \[0, 3\]"):
        torch.ops.oflow.splat(frame, flow, None, 4)
    with pytest.raises(RuntimeError, match="2\\^22"):
        torch.ops.oflow.splat(meta(1, 1, 2048, 2049), meta(1, 2, 2048, 2049), None, 0)
    # gradients flow on meta tensors: the autograd formula is wired, the weight is not differentiable
    fr, fl, me = (t.clone().requires_grad_() for t in (frame, flow, metric))
    out, weight = torch.ops.oflow.splat(fr, fl, me, 3)
    assert out.requires_grad and not weight.requires_grad
    grads = torch.autograd.grad(out.sum(), [fr, fl, me])
    assert [tuple(g.shape) for g in grads] == [tuple(t.shape) for t in (fr, fl, me)]
    out, _ = torch.ops.oflow.splat(frame, fl, None, 1)  # only the flow needs one
    (g,) = torch.autograd.grad(out.sum(), [fl])
    assert tuple(g.shape) == tuple(fl.shape)


def test_cpu_tensors_reaching_the_raw_ops_raise():
    _native.load()
    f, fl, me = torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.splat(f, fl, None, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.splat_backward(f, f, fl, me, f, me, 3, [True, True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.splat(f, fl, None, "sum")


# ------------------------------------------------------------------------------------------ the C ABI's argument errors
def test_c_abi_argument_errors_without_launch():
    lib = _native.load()
    NULL, SHAPE, MODE, ALIGN = -1, -2, -6, -7
    A = 1 << 20
    fr, fl, me, out, wt, ws, go, gfr, gfl, gme = (A * k for k in range(1, 11))
    fwd, bwd, size = lib.oflow_splat_f32, lib.oflow_splat_backward_f32, lib.oflow_splat_workspace_bytes
    assert size(2, 3, 5, 7) == 2 * 4 * 35 * 8 + 2 * 16 and size(8, 128, 55, 128) == 8 * 129 * 55 * 128 * 8 + 8 * 16
    for b, c, h, w in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0), (65536, 3, 4, 4), (1, 3, 2048, 2049)):
        assert size(b, c, h, w) == 0
        assert fwd(fr, fl, None, b, c, h, w, 0, out, wt, ws, None) == SHAPE
        assert bwd(go, fr, fl, None, out, wt, b, c, h, w, 0, gfr, gfl, None, ws, None) == SHAPE
    assert lib.oflow_splat_frac_bits(0, 4) == 0 and lib.oflow_splat_frac_bits(2048, 2049) == 0
    for miss in range(5):  # frame, flow, out, weight, workspace
        args = [fr, fl, None, 1, 3, 4, 4, 0, out, wt, ws, None]
        args[(0, 1, 8, 9, 10)[miss]] = None
        assert fwd(*args) == NULL
    assert fwd(fr, fl, None, 1, 3, 4, 4, 4, out, wt, ws, None) == MODE
    assert fwd(fr, fl, None, 1, 3, 4, 4, -1, out, wt, ws, None) == MODE
    assert fwd(fr, fl, me, 1, 3, 4, 4, 0, out, wt, ws, None) == MODE  # a metric where there must be none
    assert fwd(fr, fl, me, 1, 3, 4, 4, 1, out, wt, ws, None) == MODE
    assert fwd(fr, fl, None, 1, 3, 4, 4, 2, out, wt, ws, None) == NULL  # no metric where one is needed
    assert fwd(fr, fl, None, 1, 3, 4, 4, 3, out, wt, ws, None) == NULL
    assert fwd(fr + 2, fl, None, 1, 3, 4, 4, 0, out, wt, ws, None) == ALIGN
    assert fwd(fr, fl, None, 1, 3, 4, 4, 0, out, wt, ws + 4, None) == ALIGN
    # backward
    assert bwd(None, fr, fl, None, out, wt, 1, 3, 4, 4, 0, gfr, gfl, None, ws, None) == NULL
    assert bwd(go, fr, fl, None, out, wt, 1, 3, 4, 4, 0, None, None, None, ws, None) == NULL  # nothing asked for
    assert bwd(go, fr, fl, None, out, wt, 1, 3, 4, 4, 1, gfr, gfl, gme, ws, None) == MODE  # no metric gradient for "avg"
    assert bwd(go, fr, fl, None, out, wt, 1, 3, 4, 4, 3, gfr, gfl, gme, ws, None) == NULL
    assert bwd(go, fr, fl, me, None, wt, 1, 3, 4, 4, 3, gfr, gfl, gme, ws, None) == NULL  # normalised: out is read
    assert bwd(go, fr, fl, me, out, wt, 1, 3, 4, 4, 3, gfr, gfl, gme, None, None) == NULL
    assert bwd(go, fr, fl, me, out, wt, 1, 3, 4, 4, 5, gfr, gfl, gme, ws, None) == MODE
    assert bwd(go, fr, fl, me, out, wt, 1, 3, 4, 4, 3, gfr, gfl + 1, gme, ws, None) == ALIGN
