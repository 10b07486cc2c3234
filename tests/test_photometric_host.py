"""The photometric losses without a GPU (optical_flow.losses.ssim_loss / charbonnier_loss): the float64 reference's
closed-form gradients against torch autograd over the plain textbook form, the package's CPU composition against the
reference within K / 4 on every case (tests/photometric_cases.py), gradcheck in float64, every argument error, the
registered operators and their Meta kernels, the C ABI's argument errors, and unsupervised_sequence_loss with the new
terms off (today's value) and on (the sum written out)."""
import os

import numpy as np
import pytest
import torch

import photometric_cases as pc
from conftest import GOLDEN
from optical_flow import _native, _ops, census_loss, charbonnier_loss, smoothness_loss, ssim_loss
from optical_flow.losses import ssim_window


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", [n for n in pc.SSIM_IDS if "-identical-" not in n])
def test_ssim_reference_gradient_is_autograd_of_the_plain_form(name):
    """The closed form of photometric_cases against torch autograd in float64 over the plain quotient: 1e-9 of the
    element's bound (float64 leaves 2^-53 times a few hundred operations). The identical-frames cases are left to the
    test below: there the true gradient is 0 and both sides are rounding noise."""
    case = pc.SSIM_BY_NAME[name]
    ref = pc.ssim_reference(case)
    if case.frame0.shape[2] < case.window or case.frame0.shape[3] < case.window:
        assert ref.loss == 0.0 and not ref.grads[0].any() and not ref.grads[1].any()
        return
    f0, f1, mask = pc.frame_tensors(case, requires_grad=True, dtype=torch.float64)
    loss = pc.ssim_plain_torch(f0, f1, mask, case)
    assert abs(float(loss.detach()) - ref.loss) <= 1e-12 * max(ref.bound_loss, 1e-30) + pc.REF_FLOOR
    grads = torch.autograd.grad(loss * pc.GRAD_LOSS, [f0, f1])
    for g, r, bound in zip(grads, ref.grads, ref.bounds):
        assert (np.abs(g.numpy() - r) <= 1e-9 * bound + 1e-300).all()


def test_ssim_reference_on_identical_frames_is_zero_to_float64_rounding():
    for name in [n for n in pc.SSIM_IDS if "-identical-" in n]:
        ref = pc.ssim_reference(pc.SSIM_BY_NAME[name])
        assert abs(ref.loss) <= pc.REF_FLOOR
        assert all((np.abs(g) <= 1e-12 * b + 1e-300).all() for g, b in zip(ref.grads, ref.bounds))


def test_window_weights_are_the_contracts():
    """Normalised in float64, rounded to fp32; the package's and the reference's are the same numbers."""
    for window, sigma in ((3, None), (5, None), (7, None), (9, None), (11, None), (11, 1.5), (5, 0.8), (7, 2.0)):
        w = ssim_window(window, sigma)
        assert len(w) == window and w == pc.window_weights(window, sigma).tolist()
        assert all(float(np.float32(v)) == v for v in w) and abs(sum(w) - 1.0) <= 1e-6 and w == w[::-1]
    assert ssim_window(3, None) == [float(np.float32(1 / 3))] * 3
    g = ssim_window(11, 1.5)
    assert abs(g[5] / g[4] - np.exp(0.5 / 1.5**2)) <= 1e-6


# ------------------------------------------------------------------------------------------ the CPU composition
def _cpu_ssim(case, need=(True, True)):
    f0, f1, mask = pc.frame_tensors(case)
    f0.requires_grad_(need[0]), f1.requires_grad_(need[1])
    loss, ssim_map = ssim_loss(f0, f1, mask, case.window, case.sigma, case.image_range, return_map=True)
    grads = torch.autograd.grad(loss * pc.GRAD_LOSS, [t for t, n in zip((f0, f1), need) if n], allow_unused=True)
    it = iter(grads)
    return loss.detach(), [next(it) if n else None for n in need], ssim_map


@pytest.mark.parametrize("name", pc.SSIM_IDS)
def test_ssim_composition_within_a_quarter_of_the_tolerances(name):
    case = pc.SSIM_BY_NAME[name]
    loss, grads, ssim_map = _cpu_ssim(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not ssim_map.requires_grad
    assert tuple(ssim_map.shape) == (case.frame0.shape[0], 1) + case.frame0.shape[2:] and ssim_map.dtype == torch.float32
    ref = pc.ssim_reference(case)
    if ref.sum_m == 0.0:  # H or W under the window, an all-zero mask: exactly 0, whether autograd reaches the frames or not
        assert float(loss) == 0.0 and all(g is None or not g.any() for g in grads)
        grads = [torch.zeros_like(torch.from_numpy(case.frame0)) if g is None else g for g in grads]
    pc.assert_ssim(case, "cpu", loss, grads, ssim_map, scale=0.25)
    if "-identical-" in name:
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
        inside = ref.bound_map > 0
        assert (ssim_map.numpy()[inside] == 1.0).all()


def test_ssim_measured_maxima_are_the_recorded_ones():
    """MEASURED is what this machine's CPU gave; the K's are four times it, rounded up, and none is above 400."""
    worst = {"loss": 0.0, "grad": 0.0, "map": 0.0}
    for case in pc.SSIM_CASES:
        loss, grads, ssim_map = _cpu_ssim(case)
        grads = [torch.zeros_like(torch.from_numpy(case.frame0)) if g is None else g for g in grads]
        for k, v in pc.ssim_ratios(case, loss, grads, ssim_map).items():
            worst[k] = max(worst[k], v)
    print("ssim composition maxima:", worst)
    for key, k in (("loss", pc.K_SSIM_LOSS), ("grad", pc.K_SSIM_GRAD), ("map", pc.K_SSIM_MAP)):
        assert worst[key] <= k / 4 and pc.MEASURED["ssim_" + key] <= k / 4 <= 100.0


@pytest.mark.parametrize("name", pc.CHARB_IDS)
def test_charbonnier_composition_within_a_quarter_of_the_tolerances(name):
    case = pc.CHARB_BY_NAME[name]
    f0, f1, mask = pc.frame_tensors(case, requires_grad=True)
    loss = charbonnier_loss(f0, f1, mask, case.eps, case.alpha, case.image_range)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    grads = torch.autograd.grad(loss * pc.GRAD_LOSS, [f0, f1])
    pc.assert_charb(case, "cpu", loss.detach(), grads, scale=0.25)
    ref = pc.charb_reference(case)
    if ref.sum_m == 0.0:
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
    if "-identical-" in name:
        assert not grads[0].any() and not grads[1].any()
    assert pc.MEASURED["charb_loss"] <= pc.K_CHARB_LOSS / 4 and pc.MEASURED["charb_grad"] <= pc.K_CHARB_GRAD / 4


def test_only_the_requested_gradient_is_formed_on_the_cpu():
    case = pc.SSIM_BY_NAME["1x3x9x65-w5-near-float"]
    _, both, _ = _cpu_ssim(case)
    for need in ((True, False), (False, True)):
        _, one, _ = _cpu_ssim(case, need)
        for asked, g, b in zip(need, one, both):
            assert (g is None) if not asked else torch.equal(g, b)
    f0, f1, mask = pc.frame_tensors(case, requires_grad=True)
    m = mask.clone().requires_grad_()
    (ssim_loss(f0, f1, m) + charbonnier_loss(f0, f1, m)).backward()
    assert m.grad is None and f0.grad is not None and f1.grad is not None  # the mask gets none


# ------------------------------------------------------------------------------------------ gradcheck in float64
@pytest.mark.parametrize("shape,window,sigma,masked", [((1, 2, 4, 5), 3, None, False), ((2, 1, 6, 6), 5, 0.8, True)])
def test_ssim_gradcheck_in_float64(shape, window, sigma, masked):
    g = torch.Generator().manual_seed(5)
    f0 = (255 * torch.rand(shape, generator=g, dtype=torch.float64)).requires_grad_()
    f1 = (f0.detach() + 20 * torch.randn(shape, generator=g, dtype=torch.float64)).requires_grad_()
    mask = (torch.rand((shape[0], 1) + shape[2:], generator=g) < 0.7) if masked else None
    assert ssim_loss(f0, f1, mask, window, sigma).dtype == torch.float64
    assert torch.autograd.gradcheck(lambda a, b: ssim_loss(a, b, mask, window, sigma), (f0, f1), eps=1e-4, atol=1e-9, rtol=1e-6)


@pytest.mark.parametrize("shape,alpha,masked", [((1, 2, 3, 4), 0.5, False), ((2, 3, 2, 3), 0.45, True)])
def test_charbonnier_gradcheck_in_float64(shape, alpha, masked):
    g = torch.Generator().manual_seed(6)
    f0 = (255 * torch.rand(shape, generator=g, dtype=torch.float64)).requires_grad_()
    f1 = (f0.detach() + 5 * torch.randn(shape, generator=g, dtype=torch.float64)).requires_grad_()
    mask = (torch.rand((shape[0], 1) + shape[2:], generator=g) < 0.7) if masked else None
    fn = lambda a, b: charbonnier_loss(a, b, mask, 1e-3, alpha)  # noqa: E731
    assert fn(f0, f1).dtype == torch.float64
    assert torch.autograd.gradcheck(fn, (f0, f1), eps=1e-6, atol=1e-10, rtol=1e-6)


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    import optical_flow
    from optical_flow import losses

    assert "ssim_loss" in optical_flow.__all__ and "charbonnier_loss" in optical_flow.__all__
    assert "ssim_loss" in losses.__all__ and "charbonnier_loss" in losses.__all__
    f, m = torch.zeros(2, 3, 9, 12), torch.ones(2, 1, 9, 12)
    for fn, what in ((ssim_loss, "ssim_loss"), (charbonnier_loss, "charbonnier_loss")):
        with pytest.raises(TypeError, match=f"{what}: frame0 must be a torch.Tensor"):
            fn(f.numpy(), f)
        with pytest.raises(TypeError, match=f"{what}: frame1 must be a torch.Tensor"):
            fn(f, None)
        with pytest.raises(TypeError, match=f"{what}: mask must be a torch.Tensor"):
            fn(f, f, m.numpy())
        with pytest.raises(TypeError, match=f"{what}: frame0 must be a floating-point tensor"):
            fn(f.long(), f)
        with pytest.raises(TypeError, match=f"{what}: mask must be a floating-point or bool tensor"):
            fn(f, f, m.long())
        with pytest.raises(ValueError, match=rf"{what}: frame0 .* must be equal \(B, C, H, W\)"):
            fn(f, f[..., :-1])
        with pytest.raises(ValueError, match=rf"{what}: frame0 .* must be equal \(B, C, H, W\)"):
            fn(f[0], f[0])
        with pytest.raises(ValueError, match=rf"{what}: mask must be \(B, 1, H, W\)"):
            fn(f, f, m[:, 0])
        with pytest.raises(ValueError, match=rf"{what}: mask must be \(B, 1, H, W\)"):
            fn(f, f, torch.ones(2, 3, 9, 12))
        with pytest.raises(ValueError, match=f"{what}: all tensors must be on one device"):
            fn(f, f.to("meta"))
        with pytest.raises(ValueError, match=f"{what}: all tensors must be on one device"):
            fn(f, f, m.to("meta"))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match=f"{what}: image_range"):
                fn(f, f, image_range=bad)
    for window in (1, 4, 13, 0, -3):
        with pytest.raises(ValueError, match="ssim_loss: window must be one of"):
            ssim_loss(f, f, window=window)
    for window in (3.0, True, "3"):
        with pytest.raises(TypeError, match="ssim_loss: window must be an int"):
            ssim_loss(f, f, window=window)
    for sigma in (0.0, -1.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ssim_loss: sigma"):
            ssim_loss(f, f, sigma=sigma)
    for bad in (0.0, -0.01, float("nan")):
        with pytest.raises(ValueError, match="ssim_loss: k1"):
            ssim_loss(f, f, k1=bad)
        with pytest.raises(ValueError, match="ssim_loss: k2"):
            ssim_loss(f, f, k2=bad)
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="charbonnier_loss: eps"):
            charbonnier_loss(f, f, eps=eps)
    for alpha in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="charbonnier_loss: alpha"):
            charbonnier_loss(f, f, alpha=alpha)
    assert float(charbonnier_loss(f, f, alpha=1.0)) == pytest.approx(1e-6, rel=1e-5)  # alpha = 1 is allowed: eps^2


# ------------------------------------------------------------------------------------------ the registered operators
def test_ops_are_registered_with_the_recorded_schemas():
    _native.load()
    assert _ops.OPS_PHOTOMETRIC == ("ssim_loss", "ssim_loss_backward", "charbonnier_loss", "charbonnier_loss_backward")
    assert not set(_ops.OPS_PHOTOMETRIC) & (set(_ops.OPS) | set(_ops.OPS_SPLAT) | set(_ops.OPS_LOSSES))
    with open(os.path.join(GOLDEN, "op_schemas_photometric.txt")) as f:
        recorded = [line.rstrip("\n") for line in f if line.strip()]
    assert [str(getattr(torch.ops.oflow, name).default._schema) for name in _ops.OPS_PHOTOMETRIC] == recorded
    for name in _ops.OPS_PHOTOMETRIC:
        for key in ("CUDA", "CPU", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"oflow::{name}", key), (name, key)
    for sym in ("oflow_ssim_loss_workspace_bytes", "oflow_ssim_loss_f32", "oflow_ssim_loss_backward_f32",
                "oflow_charbonnier_loss_f32", "oflow_charbonnier_loss_backward_f32"):
        assert sym in _native.SYMBOLS and hasattr(_native.load(), sym)


def test_meta_kernels_and_gradients_on_meta_tensors():
    _native.load()
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)  # noqa: E731
    f0, f1, mask = meta(3, 3, 55, 128), meta(3, 3, 55, 128, dtype=torch.float64), meta(3, 1, 55, 128, dtype=torch.bool)
    win = ssim_window(7, None)
    for m in (None, mask, meta(3, 1, 55, 128)):
        for with_map in (True, False):
            loss, sum_m, ssim_map = torch.ops.oflow.ssim_loss(f0, f1, m, win, 6.5, 58.5, with_map)
            assert tuple(loss.shape) == () and loss.dtype == torch.float32 and loss.device.type == "meta"
            assert tuple(sum_m.shape) == () and sum_m.dtype == torch.float64
            assert tuple(ssim_map.shape) == ((3, 1, 55, 128) if with_map else (0,)) and ssim_map.dtype == torch.float32
        closs, csum = torch.ops.oflow.charbonnier_loss(f0, f1, m, 1e-3, 0.5, 255.0)
        assert tuple(closs.shape) == () and closs.dtype == torch.float32 and csum.dtype == torch.float64
        for om in ([True, True], [True, False], [False, True]):
            for gs in (torch.ops.oflow.ssim_loss_backward(loss, f0, f1, m, sum_m, win, 6.5, 58.5, om),
                       torch.ops.oflow.charbonnier_loss_backward(closs, f0, f1, m, csum, 1e-3, 0.5, 255.0, om)):
                assert [tuple(g.shape) for g in gs] == [(3, 3, 55, 128) if o else (0,) for o in om]
                assert all(g.dtype == torch.float32 for g in gs)
    with pytest.raises(RuntimeError, match=r"must be equal \(B, C, H, W\)"):
        torch.ops.oflow.ssim_loss(f0, meta(3, 3, 55, 64), None, win, 6.5, 58.5, False)
    with pytest.raises(RuntimeError, match=r"mask must be \(B, 1, H, W\)"):
        torch.ops.oflow.charbonnier_loss(f0, f1, meta(3, 2, 55, 128), 1e-3, 0.5, 255.0)
    with pytest.raises(RuntimeError, match="not one of 3, 5, 7, 9, 11"):
        torch.ops.oflow.ssim_loss(f0, f1, None, [0.25] * 4, 6.5, 58.5, False)
    with pytest.raises(RuntimeError, match="c1"):
        torch.ops.oflow.ssim_loss(f0, f1, None, win, 0.0, 58.5, False)
    with pytest.raises(RuntimeError, match="eps"):
        torch.ops.oflow.charbonnier_loss(f0, f1, None, 0.0, 0.5, 255.0)
    with pytest.raises(RuntimeError, match="alpha"):
        torch.ops.oflow.charbonnier_loss(f0, f1, None, 1e-3, 1.5, 255.0)
    with pytest.raises(RuntimeError, match="image_range"):
        torch.ops.oflow.charbonnier_loss(f0, f1, None, 1e-3, 0.5, 0.0)
    # gradients flow on meta tensors: the autograd formulas are wired, sum M and the map are not differentiable
    a, b = f0.clone().requires_grad_(), f0.clone().requires_grad_()
    loss, sum_m, ssim_map = torch.ops.oflow.ssim_loss(a, b, mask, win, 6.5, 58.5, True)
    assert loss.requires_grad and not sum_m.requires_grad and not ssim_map.requires_grad
    ga, gb = torch.autograd.grad(loss, [a, b])
    assert tuple(ga.shape) == tuple(gb.shape) == (3, 3, 55, 128)
    loss, sum_m = torch.ops.oflow.charbonnier_loss(f0, b, None, 1e-3, 0.45, 255.0)  # only frame1 needs one
    assert loss.requires_grad and not sum_m.requires_grad
    (gb,) = torch.autograd.grad(loss, [b])
    assert tuple(gb.shape) == (3, 3, 55, 128)


def test_cpu_tensors_reaching_the_raw_ops_raise():
    _native.load()
    f, m = torch.zeros(1, 3, 9, 9), torch.ones(1, 1, 9, 9)
    one, one64 = torch.ones(()), torch.ones((), dtype=torch.float64)
    win = ssim_window(3, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.ssim_loss(f, f, None, win, 6.5, 58.5, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.ssim_loss_backward(one, f, f, m, one64, win, 6.5, 58.5, [True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.charbonnier_loss(f, f, m, 1e-3, 0.5, 255.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.charbonnier_loss_backward(one, f, f, None, one64, 1e-3, 0.5, 255.0, [True, False])


# ------------------------------------------------------------------------------------------ the C ABI's argument errors
def test_c_abi_argument_errors_without_launch():
    import ctypes

    lib = _native.load()
    NULL, SHAPE, MODE, ALIGN = -1, -2, -6, -7
    A = 1 << 20
    f0, f1, mk, mp, ws, lo, su, gl, g0, g1 = (A * k for k in range(1, 11))
    wt = (ctypes.c_float * 11)(*([1.0 / 11] * 11))
    size = lib.oflow_ssim_loss_workspace_bytes
    assert size(1, 3, 3) == 16 and size(2, 23, 133) == 16 * 2 * 3 * 3 and size(8, 436, 1024) == 16 * 8 * 55 * 16
    sf, sb = lib.oflow_ssim_loss_f32, lib.oflow_ssim_loss_backward_f32
    cf, cb = lib.oflow_charbonnier_loss_f32, lib.oflow_charbonnier_loss_backward_f32
    ssim_f = lambda **k: [k.get("f0", f0), k.get("f1", f1), k.get("mask"), k.get("kind", 0), k.get("b", 1), k.get("c", 3),  # noqa: E731
                          k.get("h", 9), k.get("w", 9), k.get("window", 7), k.get("wt", wt), k.get("c1", 6.5),
                          k.get("c2", 58.5), k.get("map", mp), k.get("ws", ws), k.get("loss", lo), k.get("sum", su), None]
    ssim_b = lambda **k: [k.get("gl", gl), k.get("f0", f0), k.get("f1", f1), k.get("mask"), k.get("kind", 0),  # noqa: E731
                          k.get("sum", su), k.get("b", 1), k.get("c", 3), k.get("h", 9), k.get("w", 9), k.get("window", 7),
                          k.get("wt", wt), k.get("c1", 6.5), k.get("c2", 58.5), k.get("g0", g0), k.get("g1", g1), None]
    charb_f = lambda **k: [k.get("f0", f0), k.get("f1", f1), k.get("mask"), k.get("kind", 0), k.get("b", 1), k.get("c", 3),  # noqa: E731
                           k.get("h", 9), k.get("w", 9), k.get("eps", 1e-3), k.get("alpha", 0.5), k.get("range", 255.0),
                           k.get("ws", ws), k.get("loss", lo), k.get("sum", su), None]
    charb_b = lambda **k: [k.get("gl", gl), k.get("f0", f0), k.get("f1", f1), k.get("mask"), k.get("kind", 0),  # noqa: E731
                           k.get("sum", su), k.get("b", 1), k.get("c", 3), k.get("h", 9), k.get("w", 9), k.get("eps", 1e-3),
                           k.get("alpha", 0.5), k.get("range", 255.0), k.get("g0", g0), k.get("g1", g1), None]
    for b, h, w in ((0, 9, 9), (1, 0, 9), (1, 9, 0), (65536, 9, 9), (1, 16384, 16385)):
        assert size(b, h, w) == 0
        for fn, args in ((sf, ssim_f), (sb, ssim_b), (cf, charb_f), (cb, charb_b)):
            assert fn(*args(b=b, h=h, w=w)) == SHAPE
    for fn, args in ((sf, ssim_f), (sb, ssim_b), (cf, charb_f), (cb, charb_b)):
        assert fn(*args(c=0)) == SHAPE
        assert fn(*args(f0=None)) == NULL and fn(*args(f1=None)) == NULL and fn(*args(sum=None)) == NULL
        assert fn(*args(kind=1)) == NULL  # a mask kind without a mask
        assert fn(*args(mask=mk, kind=3)) == MODE and fn(*args(mask=mk, kind=-1)) == MODE
        assert fn(*args(f0=f0 + 2)) == ALIGN and fn(*args(mask=mk + 1, kind=1)) == ALIGN
        assert fn(*args(sum=su + 4)) == ALIGN
    for fn, args in ((sf, ssim_f), (cf, charb_f)):
        assert fn(*args(ws=None)) == NULL and fn(*args(loss=None)) == NULL
        assert fn(*args(ws=ws + 4)) == ALIGN and fn(*args(loss=lo + 2)) == ALIGN
    for fn, args in ((sb, ssim_b), (cb, charb_b)):
        assert fn(*args(gl=None)) == NULL and fn(*args(g0=None, g1=None)) == NULL  # nothing asked for
        assert fn(*args(g1=g1 + 1)) == ALIGN and fn(*args(gl=gl + 2)) == ALIGN
    for fn, args in ((sf, ssim_f), (sb, ssim_b)):
        for window in (1, 4, 13, 0, -3):
            assert fn(*args(window=window)) == MODE
        assert fn(*args(wt=None)) == NULL
        assert fn(*args(c1=0.0)) == SHAPE and fn(*args(c2=-1.0)) == SHAPE and fn(*args(c1=float("inf"))) == SHAPE
        bad = (ctypes.c_float * 11)(*([1.0 / 11] * 10 + [float("nan")]))
        assert fn(*args(wt=bad, window=11)) == SHAPE
    assert sf(*ssim_f(map=mp + 2)) == ALIGN
    for fn, args in ((cf, charb_f), (cb, charb_b)):
        for eps in (0.0, -1e-3, float("inf"), float("nan")):
            assert fn(*args(eps=eps)) == SHAPE
        for alpha in (0.0, -0.5, 1.5, float("nan")):
            assert fn(*args(alpha=alpha)) == SHAPE
        for rng in (0.0, -255.0, float("inf"), float("nan")):
            assert fn(*args(range=rng)) == SHAPE


# ------------------------------------------------------------------------------------------ the training entry point
def test_unsupervised_sequence_loss_with_the_new_terms_off_and_on():
    import inspect

    import torch.nn.functional as F

    import model
    from model.raft import unsupervised_sequence_loss
    from optical_flow import normalize, warp_grid

    g = torch.Generator().manual_seed(11)
    img0 = torch.randint(0, 256, (2, 3, 23, 40), generator=g).float()
    img1 = (img0 + 6 * torch.randn((2, 3, 23, 40), generator=g)).clamp(0, 255)
    preds = [torch.randn((2, 2, 23, 40), generator=g).requires_grad_() for _ in range(3)]
    mask = torch.rand((2, 1, 23, 40), generator=g) < 0.8
    gamma, wc, ws, order = 0.7, 0.5, 2.0, 2
    kw = dict(gamma=gamma, w_census=wc, w_smooth=ws, smooth_order=order)

    def terms(flow):
        grid = warp_grid(normalize(flow).permute(0, 2, 3, 1))
        warped = F.grid_sample(img1, grid, mode="bilinear", padding_mode="border", align_corners=True)
        return warped, wc * census_loss(img0, warped, mask) + ws * smoothness_loss(flow, img0, order=order)

    # off (the defaults, and written out as 0): exactly the existing terms' value, and no node of the new ops
    today = 0.0
    for i, flow in enumerate(preds):
        today = today + gamma ** (2 - i) * terms(flow)[1]
    for extra in ({}, dict(w_ssim=0.0, w_charbonnier=0.0), dict(w_ssim=0, ssim_window=11, ssim_sigma=1.5)):
        got = unsupervised_sequence_loss(preds, img0, img1, mask, **kw, **extra)
        assert got.dim() == 0 and float(got) == float(today)
    names = set()
    stack = [got.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is not None and fn not in names:
            names.add(fn)
            stack += [nf for nf, _ in fn.next_functions]
    assert not any("Ssim" in type(fn).__name__ for fn in names)
    # on: the sum written out, on the same warped image and mask as the census term
    wss, wch = 0.85, 0.15
    on = unsupervised_sequence_loss(preds, img0, img1, mask, **kw, w_ssim=wss, w_charbonnier=wch, ssim_window=5,
                                    ssim_sigma=0.8)
    want = 0.0
    for i, flow in enumerate(preds):
        warped, term = terms(flow)
        term = term + wss * ssim_loss(img0, warped, mask, window=5, sigma=0.8)
        term = term + wch * charbonnier_loss(img0, warped, mask)
        want = want + gamma ** (2 - i) * term
    assert float(on) == float(want) and float(on) != float(today)
    on.backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in preds)
    only = unsupervised_sequence_loss(preds, img0, img1, mask, **kw, w_ssim=wss)
    assert float(today) < float(only) < float(on)
    for fn in (unsupervised_sequence_loss, model.RAFT.unsupervised_step):
        params = inspect.signature(fn).parameters
        assert [params[k].default for k in ("w_ssim", "w_charbonnier", "ssim_window", "ssim_sigma")] == [0.0, 0.0, 3, None]
    assert "w_ssim" in unsupervised_sequence_loss.__doc__ and "w_ssim" in model.RAFT.unsupervised_step.__doc__
