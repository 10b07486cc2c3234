"""The unsupervised losses on the GPU (csrc/census_loss.hip, csrc/smoothness_loss.hip): the operators and the C ABI on a
side stream against the float64 reference on every case (tests/losses_cases.py, the calibrated tolerances), and the
bit-level properties: a second run gives the same bits in both directions, the gradients asked for do not change the
others' bits, an image computed alone has the gradient bits it has inside its batch; then unsupervised_sequence_loss
against the CPU in float64 and RAFT.unsupervised_step end to end."""
import ctypes

import numpy as np
import pytest
import torch

import losses_cases as lc
from optical_flow import _native, census_loss, smoothness_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ABI_CENSUS = ["2x3x23x133-p7-near-float", "2x3x23x133-p7-near-bool", "2x3x23x133-p7-noise-none", "1x3x6x20-p7-near-float",
              "1x3x9x70-p3-near-float", "1x3x9x70-p5-near-float", "1x3x15x71-p7-near-float"]
ABI_SMOOTH = ["2x3x33x130-o1-gauss-smooth", "2x3x33x130-o2-gauss-smooth", "2x3x2x2-o2-gauss-smooth", "1x3x1x9-o1-gauss-smooth"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _census(case, need=(True, True)):
    f0, f1, mask = lc.census_tensors(case, device=DEV)
    f0.requires_grad_(need[0]), f1.requires_grad_(need[1])
    loss, s_map = census_loss(f0, f1, mask, case.patch, case.image_range, return_map=True)
    grads = torch.autograd.grad(loss * lc.GRAD_LOSS, [t for t, n in zip((f0, f1), need) if n])
    it = iter(grads)
    return loss.detach(), [next(it) if n else None for n in need], s_map


# ------------------------------------------------------------------------------------------ census
@pytest.mark.parametrize("name", lc.CENSUS_IDS)
def test_census_operator_matches_reference(name):
    case = lc.CENSUS_BY_NAME[name]
    loss, grads, s_map = _census(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == DEV and not s_map.requires_grad
    lc.assert_census(case, "gpu", loss, grads, s_map)
    ref = lc.census_reference(case)
    if ref.loss == 0.0:  # H or W under the patch, an all-zero mask: exactly 0
        assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
    if "-identical-" in name or "-constant-" in name:
        assert abs(float(loss) - 0.01**0.4) <= lc.K_CENSUS_LOSS * lc.U * 0.01**0.4
        assert not grads[0].any() and not grads[1].any() and not s_map.any()
    # a second run gives the same bits in both directions; the single-output form gives the same loss
    loss2, grads2, s_map2 = _census(case)
    assert _same(loss2, loss) and _same(s_map2, s_map) and all(_same(a, b) for a, b in zip(grads2, grads))
    f0, f1, mask = lc.census_tensors(case, device=DEV)
    assert _same(census_loss(f0, f1, mask, case.patch, case.image_range), loss)
    # only the requested gradients are formed, and asking for one does not change the other's bits
    for need in ((True, False), (False, True)):
        _, one, _ = _census(case, need)
        for asked, g, both in zip(need, one, grads):
            assert (g is None) if not asked else _same(g, both)
    raw = torch.ops.oflow.census_loss(f0, f1, mask, case.patch, case.image_range)
    gl = torch.full((), lc.GRAD_LOSS, device=DEV)
    for om in ([True, False], [False, True]):
        got = torch.ops.oflow.census_loss_backward(gl, f0, f1, mask, raw[1], raw[2], case.patch, case.image_range, om)
        assert [g.numel() > 0 for g in got] == om
        assert all(_same(g, both) for o, g, both in zip(om, got, grads) if o)


@pytest.mark.parametrize("name", ABI_CENSUS)
def test_census_c_abi_on_a_side_stream_with_dirty_memory(name):
    """The workspace and every output are filled with NaN / garbage beforehand: every element must be written. The
    backward runs once from the saved map and once recomputing s (d_s_map = NULL)."""
    case = lc.CENSUS_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    f0, f1, mask = lc.census_tensors(case, device=DEV)
    kind = 0 if mask is None else (2 if mask.dtype == torch.bool else 1)
    lib = _native.load()
    words = lib.oflow_census_loss_workspace_bytes(b, h, w) // 8
    assert words == 2 * b * ((h + 7) // 8) * ((w + 63) // 64)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)  # noqa: E731
    runs = [(nan(b, 1, h, w), nan(words, dtype=torch.float64), nan(1), nan(1, dtype=torch.float64)) for _ in range(2)]
    grads = [(nan(b, c, h, w), nan(b, c, h, w)) for _ in range(3)]
    gl = torch.full((1,), lc.GRAD_LOSS, device=DEV)
    torch.cuda.synchronize(DEV)  # the inputs and fills are in place before the side stream touches them
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    F = ctypes.c_float
    with torch.cuda.device(DEV):
        for s_map, ws, loss, sum_m in runs:
            assert lib.oflow_census_loss_f32(p(f0), p(f1), p(mask), kind, b, c, h, w, case.patch, F(case.image_range),
                                             p(s_map), p(ws), p(loss), p(sum_m), st) == 0
        s_map, _, loss, sum_m = runs[0]
        for (g0, g1), saved in zip(grads, (s_map, s_map, None)):
            assert lib.oflow_census_loss_backward_f32(p(gl), p(f0), p(f1), p(mask), kind, p(saved), p(sum_m), b, c, h, w,
                                                      case.patch, F(case.image_range), p(g0), p(g1), st) == 0
    stream.synchronize()
    # no NaN of the fills survives: every element of every output was written (and none of them is inf)
    for s_map_, _, loss_, sum_m_ in runs:
        assert all(bool(torch.isfinite(t).all()) for t in (s_map_, loss_, sum_m_))
    assert all(bool(torch.isfinite(g).all()) for pair in grads for g in pair)
    assert abs(float(sum_m) - lc.census_reference(case).sum_m) == 0.0
    lc.assert_census(case, "c abi", loss[0], grads[0], s_map)
    assert _same(runs[1][0], s_map) and _same(runs[1][2], loss)
    assert _same(grads[1][0], grads[0][0]) and _same(grads[1][1], grads[0][1])
    lc.assert_census(case, "c abi, s recomputed", grads=grads[2])
    # the operator on the default stream gives the same bits as the C ABI
    oloss, ograds, omap = _census(case)
    assert _same(oloss.reshape(1), loss) and _same(omap, s_map) and all(_same(a, b_) for a, b_ in zip(ograds, grads[0]))
    # the forward without a map gives the same loss
    with torch.cuda.device(DEV):
        _, ws, loss3, sum3 = runs[1]
        loss3.fill_(float("nan"))
        torch.cuda.synchronize(DEV)
        assert lib.oflow_census_loss_f32(p(f0), p(f1), p(mask), kind, b, c, h, w, case.patch, F(case.image_range), None,
                                         p(ws), p(loss3), p(sum3), st) == 0
    stream.synchronize()
    assert bool(torch.isfinite(loss3).all()) and _same(loss3, loss)


def test_census_abi_error_codes_on_device_pointers():
    case = lc.CENSUS_BY_NAME["1x3x9x65-p7-noise-none"]
    b, c, h, w = case.frame0.shape
    f0, f1, _ = lc.census_tensors(case, device=DEV)
    lib = _native.load()
    ws = torch.zeros(lib.oflow_census_loss_workspace_bytes(b, h, w) // 8, device=DEV, dtype=torch.float64)
    loss, sum_m = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV, dtype=torch.float64)
    p, F = (lambda t: t.data_ptr()), ctypes.c_float
    NULL, SHAPE, MODE = -1, -2, -6
    assert lib.oflow_census_loss_f32(None, p(f1), None, 0, b, c, h, w, 7, F(255.0), None, p(ws), p(loss), p(sum_m), None) == NULL
    assert lib.oflow_census_loss_f32(p(f0), p(f1), None, 0, b, c, 0, w, 7, F(255.0), None, p(ws), p(loss), p(sum_m), None) == SHAPE
    assert lib.oflow_census_loss_f32(p(f0), p(f1), None, 0, b, c, h, w, 6, F(255.0), None, p(ws), p(loss), p(sum_m), None) == MODE
    fl, im = torch.zeros(1, 2, 5, 6, device=DEV), torch.zeros(1, 3, 5, 6, device=DEV)
    assert lib.oflow_smoothness_loss_f32(p(fl), None, 1, 3, 5, 6, 1, F(150.0), F(255.0), p(ws), p(loss), None) == NULL
    assert lib.oflow_smoothness_loss_f32(p(fl), p(im), 1, 3, 5, 0, 1, F(150.0), F(255.0), p(ws), p(loss), None) == SHAPE
    assert lib.oflow_smoothness_loss_f32(p(fl), p(im), 1, 3, 5, 6, 3, F(150.0), F(255.0), p(ws), p(loss), None) == MODE


def test_an_image_alone_has_the_gradient_bits_it_has_in_its_batch():
    """The one thing an image's gradient shares with its batch is the scalar grad_loss / (sum M + 1e-6). With every
    other image of the batch fully masked, sum M is the image's own, so the scalar is the one of the image run alone:
    the image's gradient bits (and its map's) must then be the same, and the masked images get exact zeros."""
    case = lc.CENSUS_BY_NAME["2x3x23x133-p7-near-float"]
    f0, f1, mask = lc.census_tensors(case, device=DEV, requires_grad=True)
    b = f0.shape[0]
    for i in range(b):
        only = torch.zeros_like(mask)
        only[i] = mask[i]
        loss, s_map = census_loss(f0, f1, only, return_map=True)
        g0, g1 = torch.autograd.grad(loss * lc.GRAD_LOSS, [f0, f1])
        a0, a1 = f0[i:i + 1].detach().requires_grad_(), f1[i:i + 1].detach().requires_grad_()
        alone, s_alone = census_loss(a0, a1, mask[i:i + 1], return_map=True)
        h0, h1 = torch.autograd.grad(alone * lc.GRAD_LOSS, [a0, a1])
        assert _same(alone.detach(), loss.detach()) and _same(s_alone, s_map[i:i + 1])
        assert _same(h0, g0[i:i + 1]) and _same(h1, g1[i:i + 1]), i
        others = [j for j in range(b) if j != i]
        assert g0[i].any() and not g0[others].any() and not g1[others].any()


# ------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("name", lc.SMOOTH_IDS)
def test_smoothness_operator_matches_reference(name):
    case = lc.SMOOTH_BY_NAME[name]

    def run():
        flow, image = lc.smooth_tensors(case, device=DEV, requires_grad=True)
        loss = smoothness_loss(flow, image, case.order, case.edge_weight, case.image_range)
        (grad,) = torch.autograd.grad(loss * lc.GRAD_LOSS, [flow])
        return loss.detach(), grad

    loss, grad = run()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == DEV
    lc.assert_smooth(case, "gpu", loss, grad)
    if lc.smooth_reference(case).loss == 0.0:
        assert float(loss) == 0.0 and not grad.any()
    if "-const-" in name:
        assert not grad.any()
    loss2, grad2 = run()
    assert _same(loss2, loss) and _same(grad2, grad)


@pytest.mark.parametrize("name", ABI_SMOOTH)
def test_smoothness_c_abi_on_a_side_stream_with_dirty_memory(name):
    case = lc.SMOOTH_BY_NAME[name]
    b, c, h, w = case.image.shape
    flow, image = lc.smooth_tensors(case, device=DEV)
    lib = _native.load()
    words = lib.oflow_smoothness_loss_workspace_bytes(b, h, w) // 8
    assert words == 2 * ((b * h * w + 255) // 256)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device=DEV, dtype=dtype)  # noqa: E731
    runs = [(nan(words, dtype=torch.float64), nan(1), nan(b, 2, h, w)) for _ in range(2)]
    gl = torch.full((1,), lc.GRAD_LOSS, device=DEV)
    torch.cuda.synchronize(DEV)
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    p, F = (lambda t: t.data_ptr()), ctypes.c_float
    with torch.cuda.device(DEV):
        for ws, loss, grad in runs:
            assert lib.oflow_smoothness_loss_f32(p(flow), p(image), b, c, h, w, case.order, F(case.edge_weight),
                                                 F(case.image_range), p(ws), p(loss), st) == 0
            assert lib.oflow_smoothness_loss_backward_f32(p(gl), p(flow), p(image), b, c, h, w, case.order,
                                                          F(case.edge_weight), F(case.image_range), p(grad), st) == 0
    stream.synchronize()
    _, loss, grad = runs[0]
    # no NaN of the fills survives: every element of every output was written (and none of them is inf)
    assert all(bool(torch.isfinite(t).all()) for _, loss_, grad_ in runs for t in (loss_, grad_))
    lc.assert_smooth(case, "c abi", loss[0], grad)
    assert _same(runs[1][1], loss) and _same(runs[1][2], grad)
    fl = flow.clone().requires_grad_()
    oloss = smoothness_loss(fl, image, case.order, case.edge_weight, case.image_range)
    (ograd,) = torch.autograd.grad(oloss * lc.GRAD_LOSS, [fl])
    assert _same(oloss.detach().reshape(1), loss) and _same(ograd, grad)


def test_inputs_of_other_dtypes_and_strides():
    case = lc.CENSUS_BY_NAME["1x3x15x71-p7-near-float"]
    f0, f1, mask = lc.census_tensors(case, device=DEV)
    loss = census_loss(f0, f1, mask)
    wide = torch.zeros((1, 3, 15, 142), device=DEV)
    wide[..., ::2] = f0
    f64 = f1.double().requires_grad_()
    got = census_loss(wide[..., ::2], f64, mask.double())
    assert got.dtype == torch.float32 and _same(got.detach(), loss)
    (g,) = torch.autograd.grad(got, [f64])
    assert g.dtype == torch.float64 and tuple(g.shape) == tuple(f1.shape)
    with pytest.raises(ValueError, match="one device"):
        census_loss(f0, f1.cpu())
    with pytest.raises(ValueError, match="one device"):
        smoothness_loss(torch.zeros(1, 2, 15, 71, device=DEV), f0.cpu())


# ------------------------------------------------------------------------------------------ the training entry points
def test_unsupervised_sequence_loss_against_the_cpu_in_float64():
    """3 synthetic predictions at 2x3x23x133. The loss and the gradients of the predictions against the same
    composition on the CPU in float64. Tolerances, summed over the terms: each census term within K_CENSUS_LOSS and each
    smoothness term within K_SMOOTH_LOSS of its value, plus the fp32 warp in front of the census term: a warped level
    carries a few 2^-24 of 255 and d loss / d level is bounded by the float64 gradient's l1 norm, which the test
    measures. The flow gradients are compared with 1e-3 of the largest float64 gradient element of the prediction: they
    pass through the fp32 warp backward (atomics), whose error the loss tolerances do not describe. Both of these are
    chosen, not calibrated: the factor 8 x 2^-24 x 255 per warped level and the 1e-3. Measured on an MI355X (the figures
    this test prints): |loss - float64| = 2.1e-7 against a tolerance of 7.9e-5; the largest gradient error of the three
    predictions 6.6e-7, 9.5e-7 and 1.5e-6 against largest float64 gradient elements of 2.09e-3, 2.37e-3 and 4.58e-3, i.e.
    3.2e-4, 4.0e-4 and 3.3e-4 of them, where 1e-3 is allowed. Both leave room to be tightened once the warp backward has
    a calibrated bound of its own."""
    from model.raft import unsupervised_sequence_loss

    g = torch.Generator().manual_seed(23)
    b, h, w = 2, 23, 133
    img0 = torch.randint(0, 256, (b, 3, h, w), generator=g).float()
    img0 = torch.nn.functional.avg_pool2d(img0, 5, stride=1, padding=2)  # (some structure for the warp to follow)
    img1 = (img0.roll(1, dims=-1) + 2 * torch.randn((b, 3, h, w), generator=g)).clamp(0, 255)
    flows = [(1.0 + 0.5 * torch.randn((b, 2, h, w), generator=g)) for _ in range(3)]
    mask = torch.rand((b, 1, h, w), generator=g) < 0.8
    kw = dict(gamma=0.8, w_census=1.0, w_smooth=1.0, smooth_order=1)

    def run(dev, dtype):
        preds = [f.to(device=dev, dtype=dtype).requires_grad_() for f in flows]
        loss = unsupervised_sequence_loss(preds, img0.to(dev, dtype), img1.to(dev, dtype), mask.to(dev), **kw)
        return loss, torch.autograd.grad(loss, preds)

    ref, ref_grads = run("cpu", torch.float64)
    got, grads = run(DEV, torch.float32)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.device == DEV
    # d loss / d warped level, l1: the census gradient of each term with respect to its second frame
    from optical_flow import normalize, warp_grid
    sens = 0.0
    for i, f in enumerate(flows):
        grid = warp_grid(normalize(f.double()).permute(0, 2, 3, 1))
        warped = torch.nn.functional.grid_sample(img1.double(), grid, mode="bilinear", padding_mode="border",
                                                 align_corners=True).requires_grad_()
        (gw,) = torch.autograd.grad(census_loss(img0.double(), warped, mask), [warped])
        sens += 0.8 ** (2 - i) * float(gw.abs().sum())
    tol = (lc.K_CENSUS_LOSS + lc.K_SMOOTH_LOSS) * lc.U * float(ref) + sens * 8 * lc.U * 255.0
    print(f"sequence loss: gpu {float(got):.9g} cpu64 {float(ref):.9g} |d| {abs(float(got) - float(ref)):.3g} tol {tol:.3g}")
    assert abs(float(got) - float(ref)) <= tol
    for i, (a, r) in enumerate(zip(grads, ref_grads)):
        err = float((a.cpu().double() - r).abs().max())
        print(f"prediction {i}: max |d grad| {err:.3g} of max |grad| {float(r.abs().max()):.3g}")
        assert float(a.abs().sum()) > 0  # the gradient reaches every prediction
        assert err <= 1e-3 * float(r.abs().max())


def test_raft_unsupervised_step():
    """A hash-weighted model, 2 pairs of 128x128, iters=2: a finite 0-dim loss; after backward() every parameter that
    training_step gives a gradient has a finite one, and each top-level submodule has a non-zero one; nothing
    synchronises with the host before backward() returns (torch's sync debug mode raises on any)."""
    from model import RAFT, synthetic

    torch.manual_seed(0)
    model = RAFT(iters=2).train()  # (hparams.iters = 2)
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(DEV)
    model.freeze_bn()
    img0, img1 = (t.to(DEV) for t in synthetic.synthetic_pair(2, 128, 128, seed=3))
    flow_gt, valid = torch.zeros(2, 2, 128, 128, device=DEV), torch.ones(2, 128, 128, device=DEV)
    model.training_step((img0, img1, flow_gt, valid)).backward()
    supervised = {n for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = model.unsupervised_step((img0, img1))
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert supervised <= set(grads)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for top in {n.split(".")[0] for n in supervised}:
        assert any(bool(g.any()) for n, g in grads.items() if n.split(".")[0] == top), top
