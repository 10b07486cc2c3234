"""The float64 closed forms, bounds and tolerance constants of the encoder backward tests
(tests/encoder_backward_cases.py) checked on the CPU against autograd of ``F.conv2d(stride=2)``, ``F.instance_norm`` and
eval ``F.batch_norm``, so the GPU tests compare the kernels with something that is itself pinned down; then the ABI and
operator layers as far as they go without a GPU (exported symbols, workspace queries, registration, Meta kernels, the
CPU refusal) and the model's routing attribute. No GPU needed."""
from __future__ import annotations

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import encoder_backward_cases as ec
from model import RAFT
from model import extractor as ext
from optical_flow import _native, _ops

META = torch.device("meta")
NEW_SYMBOLS = ("oflow_conv2d_strided_backward_input_f32", "oflow_conv2d_strided_backward_weight_workspace_floats",
               "oflow_conv2d_strided_backward_weight_f32", "oflow_conv2d_strided_backward_weight_generic_f32",
               "oflow_instance_norm_backward_f32", "oflow_frozen_batch_norm_backward_workspace_floats",
               "oflow_frozen_batch_norm_backward_f32")
NEW_OPS = ("conv2d_strided", "conv2d_strided_backward", "instance_norm_act", "instance_norm_act_backward",
           "frozen_batch_norm_act", "frozen_batch_norm_act_backward")


def _conv_autograd(case: ec.ConvCase, dtype):
    x, w = case.x.clone().to(dtype).requires_grad_(), case.weight.clone().to(dtype).requires_grad_()
    b = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    kh, kw = w.shape[-2:]
    F.conv2d(x, w, b, stride=case.stride, padding=(kh // 2, kw // 2)).backward(case.grad_out.to(dtype))
    return x.grad, w.grad, b.grad


def _norm_autograd(case: ec.NormCase, dtype):
    x = case.x.clone().to(dtype).requires_grad_()
    params = ()
    if case.kind == "instance":
        out = F.instance_norm(x, eps=ec.EPS)
    else:
        params = tuple(t.clone().to(dtype).requires_grad_() for t in (case.weight, case.bias))
        out = F.batch_norm(x, case.running_mean.to(dtype), case.running_var.to(dtype), params[0], params[1], False, 0.1,
                           ec.EPS)
    if case.relu:
        out = torch.relu(out)
    out.backward(case.grad_out.to(dtype))
    return (x.grad,) + tuple(p.grad for p in params)


def _plane(case: ec.NormCase) -> int:
    return case.x.shape[2] * case.x.shape[3]


# F.instance_norm refuses a plane of one element (the C ABI and the op do not: the gradient is 0)
AUTOGRAD_NORM_CASES = [c for c in ec.NORM_CASES if not (c.kind == "instance" and _plane(c) == 1)]
AUTOGRAD_NORM_IDS = [c.name for c in AUTOGRAD_NORM_CASES]


# ------------------------------------------------------------------------------------------------- convolution
def test_conv_cases_cover_the_kernels_edges():
    assert _native.load().oflow_conv2d_backward_weight_slab_pixels() == ec.SLAB
    assert len(set(ec.CONV_IDS)) == len(ec.CONV_CASES) and all(c.stride == 2 for c in ec.CONV_CASES)
    dims = [c.dims for c in ec.CONV_CASES]
    for k in (3, 7):  # images smaller than the kernel
        assert {(d[0], d[3], d[4]) for d in dims if d[5] == k} >= {(1, 1, 1), (1, 2, 2), (2, 5, 5)}
    assert {(d[0], d[3], d[4]) for d in dims if d[1:3] == (126, 33)} == {(2, 4, 8), (3, 5, 7), (2, 4, 7)}
    assert (2, 33, 33, 5, 7, 1, 1, 2) in dims
    in_pixels = {d[0] * d[3] * d[4] for d in dims if d[0] > 1}
    assert in_pixels >= {ec.PIXEL_TILE - 1, ec.PIXEL_TILE, ec.PIXEL_TILE + 1}
    out_pixels = {d[0] * ec.out_size(d[3], 2) * ec.out_size(d[4], 2) for d in dims}
    assert out_pixels >= {ec.PIXEL_TILE - 1, ec.PIXEL_TILE, ec.PIXEL_TILE + 1}  # the largest parity class of dx
    assert out_pixels >= {ec.K_CHUNK, ec.K_CHUNK + 1, ec.SLAB, ec.SLAB + 1, 3 * 41 * 37}
    assert 2 * ec.SLAB < 3 * 41 * 37 < 3 * ec.SLAB
    assert {d[1:3] + d[5:7] for d in dims} >= {(64, 3, 7, 7), (33, 4, 7, 7), (96, 64, 3, 3), (128, 96, 3, 3), (96, 64, 1, 1)}
    assert all(c.dims[2] > ec.FOLD_MAX_CIN for c in ec.STRIDE1_CASES) and all(c.stride == 1 for c in ec.STRIDE1_CASES)
    again = ec.make_conv_case(ec.CONV_SHAPES[7])
    assert all(torch.equal(a, b) for a, b in zip(again[1:4], ec.CONV_CASES[7][1:4])) and again.name == ec.CONV_CASES[7].name
    single = ec.CONV_CASES[-1]
    assert int((single.grad_out != 0).sum()) == single.dims[1]


@pytest.mark.parametrize("case", ec.CONV_CASES + ec.STRIDE1_CASES, ids=ec.CONV_IDS + ec.STRIDE1_IDS)
def test_conv_closed_form_equals_fp64_autograd(case):
    refs = _conv_autograd(case, torch.float64)
    got, bounds = ec.conv_backward64(case), ec.conv_bounds64(case)
    for r, g, bd in zip(refs, got, bounds):
        assert g.shape == r.shape and g.dtype == torch.float64
        assert bool(((g - r).abs() <= 1e-12 * bd).all())  # (a zero bound: exactly equal)
        assert bool((g.abs() <= bd * (1 + 1e-12)).all()) and bool((g[bd == 0] == 0).all())
    assert float(refs[1].abs().max()) > 0


def test_conv_1x1_stride_2_leaves_three_parity_classes_zero():
    case = ec.CONV_BY_NAME["1x1-c33-n33-2x5x7-s2"]
    dx, _, _ = ec.conv_backward64(case)
    bound = ec.conv_bounds64(case)[0]
    assert bool((dx[:, :, 1::2] == 0).all()) and bool((dx[:, :, :, 1::2] == 0).all())
    assert bool((bound[:, :, 1::2] == 0).all()) and bool((bound[:, :, :, 1::2] == 0).all())
    assert bool((dx[:, :, ::2, ::2] != 0).all())


def test_conv_single_pixel_gradient_touches_only_its_window():
    case = ec.CONV_BY_NAME["3x3-c33-n33-2x5x6-s2-single"]
    dx, _, _ = ec.conv_backward64(case)
    # output pixel (1, 1) of the last image reads input rows / columns 1..3
    live = torch.zeros_like(dx, dtype=torch.bool)
    live[1, :, 1:4, 1:4] = True
    assert bool((dx[~live] == 0).all()) and bool((dx[live] != 0).all())
    assert bool((ec.conv_bounds64(case)[0][~live] == 0).all())


def test_conv_reference_fp32_autograd_calibrates_the_tolerance():
    """K_CONV is four times what ATen's fp32 CPU autograd of F.conv2d(stride=2) needs on the committed cases."""
    worst = [0.0, 0.0, 0.0]
    for case in ec.CONV_CASES:
        ratios = ec.conv_error_ratios(*_conv_autograd(case, torch.float32), case)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    print(f"ATen fp32 CPU autograd, worst err / (U * bound): dx {worst[0]:.2f}, dw {worst[1]:.2f}, db {worst[2]:.2f}")
    assert max(worst) <= ec.K_CONV / 4


def test_conv_tolerance_catches_a_misplaced_term():
    """One product of one element's sum moved to its neighbour is far outside the tolerance, also for the longest sums."""
    for name in ("3x3-c8-n8-3x81x73-s2", "7x7-c3-n64-2x16x24-s2", "3x3-c96-n128-2x12x20-s2"):
        case = ec.CONV_BY_NAME[name]
        (dx, dw, db), (tx, tw, _), _ = ec.conv_reference(case)
        g, x, w = case.grad_out.double(), case.x.double(), case.weight.double()
        # dw[0, 0, 1, 1] loses the term of output pixel (0, 1, 1): input pixel (2 + 1 - py, 2 + 1 - px)
        py, px = w.shape[2] // 2, w.shape[3] // 2
        term = g[0, 0, 1, 1] * x[0, 0, 3 - py, 3 - px]
        assert abs(float(term)) > 4 * float(tw[0, 0, 1, 1])
        bad = dw.clone()
        bad[0, 0, 1, 1] -= term
        bad[0, 0, 1, 0] += term
        with pytest.raises(AssertionError):
            ec.assert_conv_close(None, bad.float(), None, case, "misplaced")
        # dx[0, 0, 2, 2] takes tap (py, px) of output pixel (1, 1) with the weight of the next input channel
        term = g[0, :, 1, 1] @ (w[:, 1, py, px] - w[:, 0, py, px])
        assert abs(float(term)) > 4 * float(tx[0, 0, 2, 2])
        bad = dx.clone()
        bad[0, 0, 2, 2] += term
        with pytest.raises(AssertionError):
            ec.assert_conv_close(bad.float(), None, None, case, "misplaced")
        ec.assert_conv_close(dx.float(), dw.float(), db.float(), case, "rounded reference")


def test_conv_zero_bound_elements_must_be_exact():
    case = ec.CONV_BY_NAME["1x1-c33-n33-2x5x7-s2"]
    dx = ec.conv_reference(case)[0][0].float()
    ec.assert_conv_close(dx, None, None, case, "exact zeros")
    dx[0, 0, 1, 1] = 1e-30
    with pytest.raises(AssertionError):
        ec.assert_conv_close(dx, None, None, case, "not exact")


def test_conv_padded_channels_leave_the_gradients_unchanged():
    case = ec.CONV_BY_NAME["7x7-c4-n33-2x9x10-s2"]
    wide = ec.pad_channels(case, 5)
    assert wide.dims[2] == 5 > ec.FOLD_MAX_CIN >= case.dims[2]
    (dx, dw, db), (dx5, dw5, db5) = ec.conv_backward64(case), ec.conv_backward64(wide)
    assert torch.equal(dw5[:, :4], dw) and not bool(dw5[:, 4].any()) and torch.equal(db5, db)
    assert torch.equal(dx5[:, :4], dx) and not bool(dx5[:, 4].any())


# ------------------------------------------------------------------------------------------------- norm layers
def test_norm_cases_cover_the_kernels_edges():
    assert len(set(ec.NORM_IDS)) == len(ec.NORM_CASES)
    for kind in ("instance", "frozen_bn"):
        for relu in (True, False):
            mine = [c for c in ec.NORM_CASES if c.kind == kind and c.relu == relu]
            assert {_plane(c) for c in mine} >= {1, 2, 63, 64, 65, 255, 256, 257, 35}
            assert {tuple(c.x.shape) for c in mine} >= {(2, 3, 5, 7), (2, 64, 12, 20)}
    assert {p % 4 for p in (63, 65, 35, 257)} == {1, 3}  # unaligned tails of the 16-byte loads
    for relu in ("-relu", ""):
        const = ec.NORM_BY_NAME["instance-1x2x8x8-constant" + relu]
        assert float(const.x[0, 0].var(unbiased=False)) == 0 and float(const.x[0, 1].var()) > 0
        off = ec.NORM_BY_NAME["instance-2x1x46x62-offset" + relu].x.double()
        assert abs(float(off.mean()) - 100) < 1e-2 and 0.05 < float(off.std()) < 0.2
    bn = ec.NORM_BY_NAME["frozen_bn-2x64x12x20-relu"]
    assert float(bn.running_var.min()) == pytest.approx(1e-6) and float(bn.weight[0]) < 0 < float(bn.weight[1:].min())


@pytest.mark.parametrize("case", [c for c in ec.NORM_CASES if c.relu], ids=[c.name for c in ec.NORM_CASES if c.relu])
def test_norm_relu_inputs_stay_clear_of_zero(case):
    """Every pre-ReLU output is at least RELU_GAP from 0 or exactly 0 (a constant or one-element plane)."""
    y = ec.norm_output64(case)
    live = y[y != 0]
    assert live.numel() == 0 or float(live.abs().min()) >= ec.RELU_GAP
    zero_planes = {(b, c) for b, c in (y == 0).flatten(2).all(dim=2).nonzero().tolist()}
    assert int((y == 0).sum()) == len(zero_planes) * _plane(case)  # zeros only as whole planes
    if case.kind == "frozen_bn" and _plane(case) > 8:  # the negative scale flips the mask against the sign of x - rm
        d = case.x.double()[:, 0] - float(case.running_mean[0])
        assert bool(((y[:, 0] > 0) != (d > 0)).any())


@pytest.mark.parametrize("case", AUTOGRAD_NORM_CASES, ids=AUTOGRAD_NORM_IDS)
def test_norm_closed_form_equals_fp64_autograd(case):
    refs = _norm_autograd(case, torch.float64)
    got, bounds = ec.norm_backward64(case), ec.norm_bounds64(case)
    assert len(got) == len(refs) == (1 if case.kind == "instance" else 3)
    for r, g, bd in zip(refs, got, bounds):
        assert g.shape == r.shape and g.dtype == torch.float64
        assert bool(((g - r).abs() <= 1e-10 * bd).all())
        assert bool((g.abs() <= bd * (1 + 1e-12)).all()) and bool((g[bd == 0] == 0).all())


def test_norm_one_element_and_constant_planes():
    for relu in (True, False):
        one = ec.make_norm_case("instance", (1, 2, 1, 1), relu)
        assert not bool(ec.norm_backward64(one)[0].any())  # g - mean(g) = 0, xh = 0
        const = ec.make_norm_case("instance", ec.CONSTANT_SHAPE, relu, "constant")
        dx = ec.norm_backward64(const)[0][0, 0]
        g = const.grad_out.double()[0, 0]
        want = torch.zeros_like(g) if relu else (g - g.mean()) / ec.EPS ** 0.5  # r = 1 / sqrt(eps), xh = 0
        assert torch.allclose(dx, want, rtol=1e-12, atol=0)


def test_norm_reference_fp32_autograd_calibrates_the_tolerance():
    """K_NORM is four times what ATen's fp32 CPU autograd needs on the committed cases."""
    worst = {}
    for case in AUTOGRAD_NORM_CASES:
        for i, r in enumerate(ec.norm_error_ratios(_norm_autograd(case, torch.float32), case)):
            key = (case.kind, ("dx", "dgamma", "dbeta")[i])
            worst[key] = max(worst.get(key, 0.0), r)
    print("ATen fp32 CPU autograd, worst err / (U * bound):", {k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= ec.K_NORM / 4


def test_norm_tolerance_catches_a_misplaced_term():
    """(Not on the offset plane: with |mu| r = 1000 the conditioning term of its bound is as large as one term of a
    2852-element mean.)"""
    for name in ("instance-2x64x12x20-relu", "instance-1x2x15x17", "frozen_bn-2x64x12x20-relu"):
        case = ec.NORM_BY_NAME[name]
        refs, tols, _ = ec.norm_reference(case)
        g = case.grad_out.double()
        if case.relu:
            g = g * (ec.norm_output64(case) > 0)
        # one element's g / HW left out of its plane's mean(g): every dx of the plane moves by r * g / HW
        b, c = case.x.shape[0] - 1, 0
        x = case.x.double()[b, c]
        r = 1.0 / float(torch.sqrt(x.var(unbiased=False) + ec.EPS))
        bad = [t.clone() for t in refs]
        if case.kind == "instance":
            k = int(g[b, c].abs().argmax())
            shift = r * float(g[b, c].flatten()[k]) / x.numel()
            assert abs(shift) > 4 * float(tols[0][b, c].min())
            bad[0][b, c] += shift
        else:  # one element's term added to the next channel's dgamma / dbeta
            k = int(g[b, c].abs().argmax())
            term = float(g[b, c].flatten()[k])
            assert abs(term) > 4 * float(tols[2][1])
            bad[2][0] -= term
            bad[2][1] += term
        with pytest.raises(AssertionError):
            ec.assert_norm_close([t.float() for t in bad], case, "misplaced")
        ec.assert_norm_close([t.float() for t in refs], case, "rounded reference")


def test_norm_zero_bound_elements_must_be_exact():
    case = ec.NORM_BY_NAME["instance-1x2x8x8-constant-relu"]
    refs, _, bounds = ec.norm_reference(case)
    assert not bool(bounds[0][0, 0].any()) and bool((bounds[0][0, 1] > 0).all())
    dx = refs[0].float()
    ec.assert_norm_close((dx,), case, "exact zeros")
    dx[0, 0, 3, 3] = 1e-30
    with pytest.raises(AssertionError):
        ec.assert_norm_close((dx,), case, "not exact")


def test_naive_fp32_variance_loses_the_offset_plane():
    """Why the backward recomputes its statistics in fp64: E[x^2] - E[x]^2 in fp32 on the offset plane is off by
    several percent, which the tolerance does not forgive."""
    x = ec.NORM_BY_NAME["instance-2x1x46x62-offset"].x[0, 0]
    true = float(x.double().var(unbiased=False))
    naive = float((x * x).mean() - x.mean() ** 2)
    print(f"offset plane: variance {true:.5f}, naive fp32 E[x^2] - E[x]^2 {naive:.5f}")
    assert abs(naive - true) > 1e-3 * true


# ------------------------------------------------------------------------------------------------- ABI and ops, no GPU
def test_symbols_and_workspace_queries():
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS and getattr(lib, name)
    q = lib.oflow_conv2d_strided_backward_weight_workspace_floats
    assert q(2, 64, 3, 9, 10, 7, 7, 2) == 1 * (64 * 3 * 49 + 64)
    assert q(3, 8, 8, 81, 73, 3, 3, 2) == 3 * (8 * 8 * 9 + 8)  # 4551 output pixels: three slabs
    assert q(3, 8, 8, 81, 73, 3, 3, 1) == lib.oflow_conv2d_backward_weight_workspace_floats(3, 8, 8, 81, 73, 3, 3)
    for bad in ((2, 64, 3, 9, 10, 7, 7, 0), (2, 64, 3, 9, 10, 7, 7, 3), (2, 64, 3, 9, 10, 4, 7, 2), (2, 64, 3, 9, 10, 9, 7, 2),
                (0, 64, 3, 9, 10, 7, 7, 2)):
        assert q(*bad) == 0
    n = lib.oflow_frozen_batch_norm_backward_workspace_floats
    assert n(2, 64, 240) == 2 * 2 * 64 and n(0, 64, 240) == 0 and n(2, 0, 240) == 0 and n(2, 64, 0) == 0


def test_ops_are_registered_with_meta_kernels():
    _ops.load()
    for name in NEW_OPS:
        assert name in _ops.OPS and getattr(torch.ops.oflow, name)
    O = torch.ops.oflow
    x, w = torch.empty(2, 3, 9, 10, device=META), torch.empty(64, 3, 7, 7, device=META)
    assert tuple(O.conv2d_strided(x, w, None, 2).shape) == (2, 64, 5, 5)
    assert tuple(O.conv2d_strided(x, w, torch.empty(64, device=META), 1).shape) == (2, 64, 9, 10)
    got = O.conv2d_strided_backward(torch.empty(2, 64, 5, 5, device=META), x, w, 2, [True, False, True])
    assert [tuple(t.shape) for t in got] == [(2, 3, 9, 10), (0,), (64,)]
    with pytest.raises(RuntimeError, match="stride"):
        O.conv2d_strided(x, w, None, 3)
    with pytest.raises(RuntimeError, match="grad_out"):
        O.conv2d_strided_backward(torch.empty(2, 64, 9, 10, device=META), x, w, 2, [True] * 3)
    assert tuple(O.instance_norm_act(x, 1e-5, True).shape) == tuple(x.shape)
    assert tuple(O.instance_norm_act_backward(x, x, 1e-5, True).shape) == tuple(x.shape)
    c = torch.empty(3, device=META)
    assert tuple(O.frozen_batch_norm_act(x, c, c, c, c, 1e-5, False).shape) == tuple(x.shape)
    got = O.frozen_batch_norm_act_backward(x, x, c, c, c, c, 1e-5, True, [False, True, True])
    assert [tuple(t.shape) for t in got] == [(0,), (3,), (3,)]
    with pytest.raises(RuntimeError, match="running_var"):
        O.frozen_batch_norm_act(x, c, c, c, torch.empty(4, device=META), 1e-5, False)


def test_cpu_tensors_are_refused():
    _ops.load()
    O = torch.ops.oflow
    x, w, c = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 3, 3), torch.zeros(3)
    for call in (lambda: O.conv2d_strided(x, w, None, 2),
                 lambda: O.conv2d_strided_backward(torch.zeros(1, 2, 2, 2), x, w, 2, [True] * 3),
                 lambda: O.instance_norm_act(x, 1e-5, True),
                 lambda: O.instance_norm_act_backward(x, x, 1e-5, True),
                 lambda: O.frozen_batch_norm_act(x, c, c, c, c, 1e-5, True),
                 lambda: O.frozen_batch_norm_act_backward(x, x, c, c, c, c, 1e-5, True, [True] * 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------------------------------------------- model routing
def test_encoder_backward_impl_attribute_and_cpu_routing():
    """The attribute defaults to "aten", is independent of conv_backward_impl, is validated in the forward, and on the
    CPU "native" calls the modules: the same output and gradients, the same state_dict keys."""
    model = RAFT(iters=1)
    assert model.encoder_backward_impl == "aten" and model.conv_backward_impl == "aten"
    assert "encoder_backward_impl" not in model.hparams
    keys = list(model.state_dict())
    enc = ext.BasicEncoder(output_dim=32, norm_fn="instance")
    assert enc.encoder_backward_impl == "aten"
    x = torch.randn(1, 3, 16, 24, generator=torch.Generator().manual_seed(1))
    outs, grads = [], []
    for impl in ("aten", "native"):
        enc.encoder_backward_impl = impl
        enc.zero_grad()
        y = enc(x)
        y.square().sum().backward()
        outs.append(y.detach())
        grads.append([p.grad.clone() for p in enc.parameters()])
        assert all(blk.encoder_backward_impl == impl for layer in (enc.layer1, enc.layer2, enc.layer3) for blk in layer)
    assert torch.equal(outs[0], outs[1]) and all(torch.equal(a, b) for a, b in zip(*grads))
    enc.encoder_backward_impl = "miopen"
    with pytest.raises(ValueError, match="encoder_backward_impl"):
        enc(x)
    model.encoder_backward_impl = "miopen"
    img = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="encoder_backward_impl"):
        model(img, img, iters=1)
    model.encoder_backward_impl, model.conv_backward_impl = "native", "miopen"
    with pytest.raises(ValueError, match="conv_backward_impl"):
        model(img, img, iters=1)
    assert list(model.state_dict()) == keys


def test_eligibility_of_convolutions_and_norms_on_the_cpu():
    """enc_conv / enc_norm_act call the module for everything the native ops do not cover; on the CPU that is
    everything, so the checks here are that nothing raises and the module's result comes back."""
    x = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(2), requires_grad=True)
    for conv in (nn.Conv2d(4, 4, 3, padding=1, stride=2), nn.Conv2d(4, 4, 3, padding=1, dilation=1, groups=2),
                 nn.Conv2d(4, 4, 3, padding=0), nn.Conv2d(4, 4, 2)):
        assert torch.equal(ext.enc_conv(conv, x, "native"), conv(x))
    for norm in (nn.InstanceNorm2d(4), nn.BatchNorm2d(4).eval(), nn.BatchNorm2d(4), nn.GroupNorm(2, 4), nn.Sequential()):
        for relu in (True, False):
            want = norm(x)
            want = torch.relu(want) if relu else want
            assert torch.equal(ext.enc_norm_act(norm, x, relu, "native"), want)
    with pytest.raises(ValueError, match="encoder_backward_impl"):
        ext.enc_conv(nn.Conv2d(4, 4, 3), x, "miopen")
    with pytest.raises(ValueError, match="encoder_backward_impl"):
        ext.enc_norm_act(nn.InstanceNorm2d(4), x, True, "miopen")
