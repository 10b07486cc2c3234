"""The photometric losses on the GPU (csrc/photometric_loss.hip): the operators and the C ABI on a side stream against the
float64 reference on every case (tests/photometric_cases.py, the calibrated tolerances), and the bit-level properties:
a second run gives the same bits in both directions, the gradients asked for do not change the others' bits, an image
computed alone has the map bits it has inside its batch; then unsupervised_sequence_loss with the new terms on against
the CPU in float64 and RAFT.unsupervised_step with w_ssim > 0 end to end."""
import ctypes

import pytest
import torch

import losses_cases as lc
import photometric_cases as pc
from optical_flow import _native, census_loss, charbonnier_loss, ssim_loss
from optical_flow.losses import ssim_window

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ABI_SSIM = ["2x3x23x133-w7-near-float", "2x3x23x133-w7-near-bool", "2x3x23x133-w11g1.5-noise-none", "1x3x2x20-w3-near-float",
            "1x3x9x65-w3-near-float", "1x3x9x65-w5g0.8-near-float", "2x3x11x75-w11-near-float", "2x3x23x133-w9-near-float"]
ABI_CHARB = ["2x3x33x130-a0.5-near-float", "2x3x33x130-a0.45-near-bool", "2x3x24x132-a0.45-near-bool", "2x3x5x64-a0.5-noise-none",
             "1x1x1x1-a0.45-near-float"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _grads(loss, frames, need):
    grads = torch.autograd.grad(loss * pc.GRAD_LOSS, [t for t, n in zip(frames, need) if n])
    it = iter(grads)
    return [next(it) if n else None for n in need]


def _ssim(case, need=(True, True)):
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    f0.requires_grad_(need[0]), f1.requires_grad_(need[1])
    loss, ssim_map = ssim_loss(f0, f1, mask, case.window, case.sigma, case.image_range, return_map=True)
    return loss.detach(), _grads(loss, (f0, f1), need), ssim_map


def _charb(case, need=(True, True)):
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    f0.requires_grad_(need[0]), f1.requires_grad_(need[1])
    loss = charbonnier_loss(f0, f1, mask, case.eps, case.alpha, case.image_range)
    return loss.detach(), _grads(loss, (f0, f1), need)


def _kind(mask):
    return 0 if mask is None else (2 if mask.dtype == torch.bool else 1)


# ------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("name", pc.SSIM_IDS)
def test_ssim_operator_matches_reference(name):
    case = pc.SSIM_BY_NAME[name]
    loss, grads, ssim_map = _ssim(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == DEV and not ssim_map.requires_grad
    pc.assert_ssim(case, "gpu", loss, grads, ssim_map)
    ref = pc.ssim_reference(case)
    if ref.sum_m == 0.0:  # H or W under the window, an all-zero mask: exactly 0
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
    if "-identical-" in name:
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
        inside = torch.from_numpy(ref.bound_map > 0).to(DEV)
        assert bool((ssim_map[inside] == 1.0).all())
    # a second run gives the same bits in both directions; the single-output form gives the same loss
    loss2, grads2, map2 = _ssim(case)
    assert _same(loss2, loss) and _same(map2, ssim_map) and all(_same(a, b) for a, b in zip(grads2, grads))
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    assert _same(ssim_loss(f0, f1, mask, case.window, case.sigma, case.image_range), loss)
    # only the requested gradients are formed, and asking for one does not change the other's bits
    for need in ((True, False), (False, True)):
        _, one, _ = _ssim(case, need)
        for asked, g, both in zip(need, one, grads):
            assert (g is None) if not asked else _same(g, both)
    win, (c1, c2) = ssim_window(case.window, case.sigma), pc.ssim_constants(case)
    raw = torch.ops.oflow.ssim_loss(f0, f1, mask, win, c1, c2, False)
    assert raw[2].numel() == 0 and _same(raw[0], loss)
    gl = torch.full((), pc.GRAD_LOSS, device=DEV)
    for om in ([True, False], [False, True]):
        got = torch.ops.oflow.ssim_loss_backward(gl, f0, f1, mask, raw[1], win, c1, c2, om)
        assert [g.numel() > 0 for g in got] == om
        assert all(_same(g, both) for o, g, both in zip(om, got, grads) if o)


@pytest.mark.parametrize("name", ABI_SSIM)
def test_ssim_c_abi_on_a_side_stream_with_dirty_memory(name):
    """The workspace and every output are filled with NaN beforehand: every element must be written."""
    case = pc.SSIM_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    lib = _native.load()
    words = lib.oflow_ssim_loss_workspace_bytes(b, h, w) // 8
    assert words == 2 * b * ((h + 7) // 8) * ((w + 63) // 64)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)  # noqa: E731
    runs = [(nan(b, 1, h, w), nan(words, dtype=torch.float64), nan(1), nan(1, dtype=torch.float64)) for _ in range(2)]
    grads = [(nan(b, c, h, w), nan(b, c, h, w)) for _ in range(2)]
    gl = torch.full((1,), pc.GRAD_LOSS, device=DEV)
    wt = (ctypes.c_float * case.window)(*ssim_window(case.window, case.sigma))
    c1, c2 = (ctypes.c_float(v) for v in pc.ssim_constants(case))
    torch.cuda.synchronize(DEV)  # the inputs and fills are in place before the side stream touches them
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(DEV):
        for ssim_map, ws, loss, sum_m in runs:
            assert lib.oflow_ssim_loss_f32(p(f0), p(f1), p(mask), _kind(mask), b, c, h, w, case.window, wt, c1, c2,
                                           p(ssim_map), p(ws), p(loss), p(sum_m), st) == 0
        ssim_map, _, loss, sum_m = runs[0]
        for g0, g1 in grads:
            assert lib.oflow_ssim_loss_backward_f32(p(gl), p(f0), p(f1), p(mask), _kind(mask), p(sum_m), b, c, h, w,
                                                    case.window, wt, c1, c2, p(g0), p(g1), st) == 0
    stream.synchronize()
    # no NaN of the fills survives: every element of every output was written (and none of them is inf)
    for map_, _, loss_, sum_m_ in runs:
        assert all(bool(torch.isfinite(t).all()) for t in (map_, loss_, sum_m_))
    assert all(bool(torch.isfinite(g).all()) for pair in grads for g in pair)
    assert abs(float(sum_m) - pc.ssim_reference(case).sum_m) == 0.0
    pc.assert_ssim(case, "c abi", loss[0], grads[0], ssim_map)
    assert _same(runs[1][0], ssim_map) and _same(runs[1][2], loss)
    assert _same(grads[1][0], grads[0][0]) and _same(grads[1][1], grads[0][1])
    # the operator on the default stream gives the same bits as the C ABI
    oloss, ograds, omap = _ssim(case)
    assert _same(oloss.reshape(1), loss) and _same(omap, ssim_map) and all(_same(a, b_) for a, b_ in zip(ograds, grads[0]))
    # the forward without a map gives the same loss
    with torch.cuda.device(DEV):
        _, ws, loss3, sum3 = runs[1]
        loss3.fill_(float("nan"))
        torch.cuda.synchronize(DEV)
        assert lib.oflow_ssim_loss_f32(p(f0), p(f1), p(mask), _kind(mask), b, c, h, w, case.window, wt, c1, c2, None, p(ws),
                                       p(loss3), p(sum3), st) == 0
    stream.synchronize()
    assert bool(torch.isfinite(loss3).all()) and _same(loss3, loss)


def test_abi_error_codes_on_device_pointers():
    case = pc.SSIM_BY_NAME["1x3x9x65-w5-noise-none"]
    b, c, h, w = case.frame0.shape
    f0, f1, _ = pc.frame_tensors(case, device=DEV)
    lib = _native.load()
    ws = torch.zeros(lib.oflow_ssim_loss_workspace_bytes(b, h, w) // 8, device=DEV, dtype=torch.float64)
    loss, sum_m = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV, dtype=torch.float64)
    g0 = torch.zeros(b, c, h, w, device=DEV)
    p, F = (lambda t: t.data_ptr()), ctypes.c_float
    wt = (ctypes.c_float * 5)(*ssim_window(5, None))
    NULL, SHAPE, MODE = -1, -2, -6
    fwd, bwd = lib.oflow_ssim_loss_f32, lib.oflow_ssim_loss_backward_f32
    assert fwd(None, p(f1), None, 0, b, c, h, w, 5, wt, F(6.5), F(58.5), None, p(ws), p(loss), p(sum_m), None) == NULL
    assert fwd(p(f0), p(f1), None, 0, b, c, 0, w, 5, wt, F(6.5), F(58.5), None, p(ws), p(loss), p(sum_m), None) == SHAPE
    assert fwd(p(f0), p(f1), None, 0, b, c, h, w, 6, wt, F(6.5), F(58.5), None, p(ws), p(loss), p(sum_m), None) == MODE
    assert fwd(p(f0), p(f1), None, 0, b, c, h, w, 5, None, F(6.5), F(58.5), None, p(ws), p(loss), p(sum_m), None) == NULL
    assert bwd(p(loss), p(f0), p(f1), None, 0, p(sum_m), b, c, h, w, 5, wt, F(6.5), F(58.5), None, None, None) == NULL
    assert bwd(p(loss), p(f0), p(f1), None, 0, p(sum_m), b, c, h, w, 13, wt, F(6.5), F(58.5), p(g0), None, None) == MODE
    cf, cb = lib.oflow_charbonnier_loss_f32, lib.oflow_charbonnier_loss_backward_f32
    assert cf(p(f0), None, None, 0, b, c, h, w, F(1e-3), F(0.5), F(255.0), p(ws), p(loss), p(sum_m), None) == NULL
    assert cf(p(f0), p(f1), None, 0, b, c, h, w, F(0.0), F(0.5), F(255.0), p(ws), p(loss), p(sum_m), None) == SHAPE
    assert cf(p(f0), p(f1), None, 0, b, c, h, w, F(1e-3), F(1.5), F(255.0), p(ws), p(loss), p(sum_m), None) == SHAPE
    assert cf(p(f0), p(f1), None, 3, b, c, h, w, F(1e-3), F(0.5), F(255.0), p(ws), p(loss), p(sum_m), None) == MODE
    assert cb(p(loss), p(f0), p(f1), None, 0, p(sum_m), b, c, h, w, F(1e-3), F(0.5), F(255.0), None, None, None) == NULL
    torch.cuda.synchronize(DEV)
    assert not loss.any() and not sum_m.any() and not g0.any()  # nothing was launched


def test_an_image_alone_has_the_map_and_gradient_bits_it_has_in_its_batch():
    """An image's SSIM map does not depend on its batch at all. Its gradient shares only the scalar grad_loss / (sum M +
    1e-6): with every other image fully masked that scalar is the one of the image run alone, so the bits agree, and
    the masked images get exact zeros."""
    case = pc.SSIM_BY_NAME["2x3x23x133-w11g1.5-near-float"]
    f0, f1, mask = pc.frame_tensors(case, device=DEV, requires_grad=True)
    args = (case.window, case.sigma, case.image_range)
    _, whole = ssim_loss(f0, f1, mask, *args, return_map=True)
    b = f0.shape[0]
    for i in range(b):
        only = torch.zeros_like(mask)
        only[i] = mask[i]
        loss, ssim_map = ssim_loss(f0, f1, only, *args, return_map=True)
        g0, g1 = torch.autograd.grad(loss * pc.GRAD_LOSS, [f0, f1])
        a0, a1 = f0[i:i + 1].detach().requires_grad_(), f1[i:i + 1].detach().requires_grad_()
        alone, map_alone = ssim_loss(a0, a1, mask[i:i + 1], *args, return_map=True)
        h0, h1 = torch.autograd.grad(alone * pc.GRAD_LOSS, [a0, a1])
        assert _same(map_alone, whole[i:i + 1]) and _same(map_alone, ssim_map[i:i + 1])
        assert _same(alone.detach(), loss.detach())
        assert _same(h0, g0[i:i + 1]) and _same(h1, g1[i:i + 1]), i
        others = [j for j in range(b) if j != i]
        assert g0[i].any() and not g0[others].any() and not g1[others].any()


# ------------------------------------------------------------------------------------------ Charbonnier
@pytest.mark.parametrize("name", pc.CHARB_IDS)
def test_charbonnier_operator_matches_reference(name):
    case = pc.CHARB_BY_NAME[name]
    loss, grads = _charb(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == DEV
    pc.assert_charb(case, "gpu", loss, grads)
    if pc.charb_reference(case).sum_m == 0.0:
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
    if "-identical-" in name:
        assert not grads[0].any() and not grads[1].any()
    loss2, grads2 = _charb(case)
    assert _same(loss2, loss) and all(_same(a, b) for a, b in zip(grads2, grads))
    for need in ((True, False), (False, True)):
        _, one = _charb(case, need)
        for asked, g, both in zip(need, one, grads):
            assert (g is None) if not asked else _same(g, both)


@pytest.mark.parametrize("name", ABI_CHARB)
def test_charbonnier_c_abi_on_a_side_stream_with_dirty_memory(name):
    case = pc.CHARB_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    lib = _native.load()
    words = lib.oflow_ssim_loss_workspace_bytes(b, h, w) // 8
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)  # noqa: E731
    runs = [(nan(words, dtype=torch.float64), nan(1), nan(1, dtype=torch.float64), nan(b, c, h, w), nan(b, c, h, w))
            for _ in range(2)]
    gl = torch.full((1,), pc.GRAD_LOSS, device=DEV)
    torch.cuda.synchronize(DEV)
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    eps, alpha, rng = (ctypes.c_float(v) for v in (case.eps, case.alpha, case.image_range))
    with torch.cuda.device(DEV):
        for ws, loss, sum_m, g0, g1 in runs:
            assert lib.oflow_charbonnier_loss_f32(p(f0), p(f1), p(mask), _kind(mask), b, c, h, w, eps, alpha, rng, p(ws),
                                                  p(loss), p(sum_m), st) == 0
            assert lib.oflow_charbonnier_loss_backward_f32(p(gl), p(f0), p(f1), p(mask), _kind(mask), p(sum_m), b, c, h, w,
                                                           eps, alpha, rng, p(g0), p(g1), st) == 0
    stream.synchronize()
    _, loss, sum_m, g0, g1 = runs[0]
    assert all(bool(torch.isfinite(t).all()) for run in runs for t in run[1:])
    assert abs(float(sum_m) - pc.charb_reference(case).sum_m) == 0.0
    pc.assert_charb(case, "c abi", loss[0], (g0, g1))
    assert all(_same(a, b_) for a, b_ in zip(runs[1][1:2] + runs[1][3:], (loss, g0, g1)))
    oloss, ograds = _charb(case)
    assert _same(oloss.reshape(1), loss) and _same(ograds[0], g0) and _same(ograds[1], g1)


def test_inputs_of_other_dtypes_and_strides():
    case = pc.SSIM_BY_NAME["1x3x9x65-w5-near-float"]
    f0, f1, mask = pc.frame_tensors(case, device=DEV)
    for fn in (lambda a, b, m: ssim_loss(a, b, m, 5), lambda a, b, m: charbonnier_loss(a, b, m, alpha=0.45)):
        loss = fn(f0, f1, mask)
        wide = torch.zeros((1, 3, 9, 130), device=DEV)
        wide[..., ::2] = f0
        f64 = f1.double().requires_grad_()
        got = fn(wide[..., ::2], f64, mask.double())
        assert got.dtype == torch.float32 and _same(got.detach(), loss)
        (g,) = torch.autograd.grad(got, [f64])
        assert g.dtype == torch.float64 and tuple(g.shape) == tuple(f1.shape) and bool(g.any())
        half = fn(f0.half(), f1.half(), mask.half())  # integer levels below 2048 are exact in fp16
        assert half.dtype == torch.float32 and _same(half, fn(f0.half().float(), f1.half().float(), mask))
        with pytest.raises(ValueError, match="one device"):
            fn(f0, f1.cpu(), None)
        with pytest.raises(ValueError, match="one device"):
            fn(f0, f1, mask.cpu())


# ------------------------------------------------------------------------------------------ the training entry points
def test_unsupervised_sequence_loss_with_the_new_terms_against_the_cpu_in_float64():
    """The setting of tests/test_gpu_losses.py's test (3 synthetic predictions at 2x3x23x133) with w_ssim = 0.85 (window
    5, sigma 0.8) and w_charbonnier = 0.15 added. The tolerance is built the same way: every term within its K of its
    value, plus the fp32 warp in front of the photometric terms: a warped level carries a few 2^-24 of 255 (the chosen
    factor 8 of that test) and d loss / d level is bounded by the l1 norm of the float64 gradient of the census, SSIM and
    Charbonnier terms together with respect to their second frame, which the test measures and prints. The flow
    gradients are compared with 1e-3 of the largest float64 gradient element of the prediction, as there. Measured on an
    MI355X (the figures this test prints): |loss - float64| = 6.9e-8 against a tolerance of 7.6e-5; the sensitivity
    through the warp 0.598, of which the two new terms contribute 0.0575; the largest gradient errors of the three
    predictions 6.6e-7, 9.5e-7 and 1.5e-6 against largest float64 gradient elements of 2.12e-3, 2.45e-3 and 4.64e-3."""
    from model.raft import unsupervised_sequence_loss
    from optical_flow import normalize, smoothness_loss, warp_grid

    g = torch.Generator().manual_seed(23)
    b, h, w = 2, 23, 133
    img0 = torch.randint(0, 256, (b, 3, h, w), generator=g).float()
    img0 = torch.nn.functional.avg_pool2d(img0, 5, stride=1, padding=2)  # (some structure for the warp to follow)
    img1 = (img0.roll(1, dims=-1) + 2 * torch.randn((b, 3, h, w), generator=g)).clamp(0, 255)
    flows = [(1.0 + 0.5 * torch.randn((b, 2, h, w), generator=g)) for _ in range(3)]
    mask = torch.rand((b, 1, h, w), generator=g) < 0.8
    wss, wch = 0.85, 0.15
    kw = dict(gamma=0.8, w_census=1.0, w_smooth=1.0, smooth_order=1, w_ssim=wss, w_charbonnier=wch, ssim_window=5,
              ssim_sigma=0.8)

    def run(dev, dtype):
        preds = [f.to(device=dev, dtype=dtype).requires_grad_() for f in flows]
        loss = unsupervised_sequence_loss(preds, img0.to(dev, dtype), img1.to(dev, dtype), mask.to(dev), **kw)
        return loss, torch.autograd.grad(loss, preds)

    ref, ref_grads = run("cpu", torch.float64)
    got, grads = run(DEV, torch.float32)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.device == DEV
    sens, sens_new, tol_terms = 0.0, 0.0, 0.0
    i0 = img0.double()
    for i, f in enumerate(flows):
        grid = warp_grid(normalize(f.double()).permute(0, 2, 3, 1))
        warped = torch.nn.functional.grid_sample(img1.double(), grid, mode="bilinear", padding_mode="border",
                                                 align_corners=True).requires_grad_()
        t_census, t_ssim = census_loss(i0, warped, mask), ssim_loss(i0, warped, mask, window=5, sigma=0.8)
        t_charb = charbonnier_loss(i0, warped, mask)
        (gw,) = torch.autograd.grad(t_census + wss * t_ssim + wch * t_charb, [warped], retain_graph=True)
        (gn,) = torch.autograd.grad(wss * t_ssim + wch * t_charb, [warped])
        weight = 0.8 ** (2 - i)
        sens += weight * float(gw.abs().sum())
        sens_new += weight * float(gn.abs().sum())
        t_smooth = smoothness_loss(f.double(), i0, order=1)
        values = [float(t.detach()) for t in (t_census, t_smooth, t_ssim, t_charb)]
        tol_terms += weight * lc.U * (lc.K_CENSUS_LOSS * values[0] + lc.K_SMOOTH_LOSS * values[1]
                                      + pc.K_SSIM_LOSS * wss * values[2] + pc.K_CHARB_LOSS * wch * values[3])
    tol = tol_terms + sens * 8 * lc.U * 255.0
    got_, ref_ = float(got.detach()), float(ref.detach())
    print(f"sequence loss with ssim + charbonnier: gpu {got_:.9g} cpu64 {ref_:.9g} "
          f"|d| {abs(got_ - ref_):.3g} tol {tol:.3g}; sensitivity through the warp (l1 of d loss / d warped "
          f"level) {sens:.4g}, of which the new terms {sens_new:.4g}")
    assert abs(got_ - ref_) <= tol
    for i, (a, r) in enumerate(zip(grads, ref_grads)):
        err = float((a.cpu().double() - r).abs().max())
        print(f"prediction {i}: max |d grad| {err:.3g} of max |grad| {float(r.abs().max()):.3g}")
        assert float(a.abs().sum()) > 0  # the gradient reaches every prediction
        assert err <= 1e-3 * float(r.abs().max())


def test_raft_unsupervised_step_with_ssim():
    """A hash-weighted model, 2 pairs of 128x128 (the smallest padded pair), iters=2, w_ssim and w_charbonnier on: a
    finite 0-dim loss that differs from the default one; after backward() every parameter that training_step gives a
    gradient has a finite one; nothing synchronises with the host before backward() returns."""
    from model import RAFT, synthetic

    torch.manual_seed(0)
    model = RAFT(iters=2).train()
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(DEV)
    model.freeze_bn()
    img0, img1 = (t.to(DEV) for t in synthetic.synthetic_pair(2, 128, 128, seed=3))
    flow_gt, valid = torch.zeros(2, 2, 128, 128, device=DEV), torch.ones(2, 128, 128, device=DEV)
    model.training_step((img0, img1, flow_gt, valid)).backward()
    supervised = {n for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        plain = model.unsupervised_step((img0, img1))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = model.unsupervised_step((img0, img1), w_ssim=0.85, w_charbonnier=0.15, ssim_window=7)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    assert float(loss.detach()) > float(plain)  # both added terms are positive
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert supervised <= set(grads)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for top in {n.split(".")[0] for n in supervised}:
        assert any(bool(g.any()) for n, g in grads.items() if n.split(".")[0] == top), top
