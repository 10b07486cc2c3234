"""Forward warping on the GPU (csrc/splat.hip, csrc/splat_backward.hip): the operator and the C ABI on a side stream
against the float64 reference on every case (tests/splat_cases.py: the derived per-pixel bound, holes exactly 0), the
gradients against float64 autograd within the calibrated tolerance, and the bit-level properties: a second run gives the
same bits in both directions, an image computed alone has the bits it has inside a batch, and the gradients asked for do
not change the others' bits."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import splat_cases as sc
from optical_flow import _native, splat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ABI_IDS = [c.name for c in sc.ALL_CASES if any(k in c.name for k in ("-gauss2-", "-gaussbig-", "-collapse-", "-nonfinite-"))]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _gpu(case, requires_grad=False):
    return sc.tensors(case, device=DEV, requires_grad=requires_grad)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_operator_matches_reference(name):
    case = sc.BY_NAME[name]
    frame, flow, metric = _gpu(case)
    out, weight = splat(frame, flow, metric, case.mode, return_weight=True)
    assert out.device == frame.device and not out.requires_grad
    sc.assert_forward(case, out.cpu().numpy(), weight.cpu().numpy(), "gpu")
    # a second run, the raw op and the single-output form: the same bits
    out2, weight2 = splat(frame, flow, metric, case.mode, return_weight=True)
    assert _same(out2, out) and _same(weight2, weight)
    raw = torch.ops.oflow.splat(frame, flow, metric, sc.MODES[case.mode])
    assert _same(raw[0], out) and _same(raw[1], weight)
    assert _same(splat(frame, flow, metric, case.mode), out)


@pytest.mark.parametrize("name", [c.name for c in sc.MIXED])
def test_an_image_alone_has_the_bits_it_has_in_its_batch(name):
    case = sc.BY_NAME[name]
    frame, flow, metric = _gpu(case)
    out, weight = splat(frame, flow, metric, case.mode, return_weight=True)
    for i in range(frame.shape[0]):
        o1, w1 = splat(frame[i:i + 1], flow[i:i + 1], None if metric is None else metric[i:i + 1], case.mode,
                       return_weight=True)
        assert _same(o1, out[i:i + 1]) and _same(w1, weight[i:i + 1]), (name, i)


@pytest.mark.parametrize("name", ABI_IDS)
def test_c_abi_on_a_side_stream_with_dirty_memory(name):
    """The workspace and every output are filled with garbage beforehand: the library's own zeroing is what is tested,
    and every output element must be written (no NaN survives)."""
    case = sc.BY_NAME[name]
    b, c, h, w = case.frame.shape
    frame, flow, metric = _gpu(case)
    grad_out = torch.from_numpy(case.grad_out).to(DEV)
    lib = _native.load()
    words = lib.oflow_splat_workspace_bytes(b, c, h, w) // 8
    assert words * 8 == 8 * b * (c + 1) * h * w + 16 * b
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    dirty = lambda: torch.full((words,), 0x5A5A5A5A5A5A5A5A, device=DEV, dtype=torch.int64)  # noqa: E731
    runs = [(nan(b, c, h, w), nan(b, 1, h, w), dirty()) for _ in range(2)]
    grads = [(nan(b, c, h, w), nan(b, 2, h, w), nan(b, 1, h, w), dirty()) for _ in range(2)]
    torch.cuda.synchronize(DEV)  # the inputs and fills are in place before the side stream touches them
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    mode = sc.MODES[case.mode]
    with torch.cuda.device(DEV):
        for out, weight, ws in runs:
            assert lib.oflow_splat_f32(p(frame), p(flow), p(metric), b, c, h, w, mode, p(out), p(weight), p(ws), st) == 0
        for gfr, gfl, gme, ws in grads:
            assert lib.oflow_splat_backward_f32(p(grad_out), p(frame), p(flow), p(metric), p(runs[0][0]), p(runs[0][1]), b, c,
                                                h, w, mode, p(gfr), p(gfl), p(gme) if metric is not None else None, p(ws),
                                                st) == 0
    stream.synchronize()
    out, weight, _ = runs[0]
    sc.assert_forward(case, out.cpu().numpy(), weight.cpu().numpy(), "c abi")
    assert _same(runs[1][0], out) and _same(runs[1][1], weight)
    gfr, gfl, gme, _ = grads[0]
    sc.assert_backward(case, [gfr, gfl, gme if metric is not None else None], "c abi")
    assert _same(grads[1][0], gfr) and _same(grads[1][1], gfl)
    if metric is not None:
        assert _same(grads[1][2], gme)
    # the operator on the default stream gives the same bits as the C ABI
    o2, w2 = splat(frame, flow, metric, case.mode, return_weight=True)
    assert _same(o2, out) and _same(w2, weight)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_backward_matches_float64_autograd(name):
    case = sc.BY_NAME[name]
    frame, flow, metric = _gpu(case, requires_grad=True)
    leaves = [frame, flow] + ([metric] if metric is not None else [])
    grad_out = torch.from_numpy(case.grad_out).to(DEV)
    out, weight = splat(frame, flow, metric, case.mode, return_weight=True)
    assert out.requires_grad and not weight.requires_grad
    grads = list(torch.autograd.grad((out * grad_out).sum(), leaves, retain_graph=True))
    sc.assert_backward(case, grads + [None] * (3 - len(grads)), "gpu")
    again = torch.autograd.grad((out * grad_out).sum(), leaves)
    assert all(_same(a, g) for a, g in zip(again, grads))
    # skipped sources get zero gradients
    skipped = torch.from_numpy(~sc.geometry(case.flow).keep.reshape(case.flow.shape[0], 1, *case.flow.shape[2:])).to(DEV)
    for g in grads:
        assert not g[skipped.expand_as(g)].any()
    # every output_mask subset leaves the other gradients' bits unchanged
    mode = sc.MODES[case.mode]
    o, wt = out.detach(), weight
    for mask in itertools.product((False, True), repeat=3):
        if mask[2] and metric is None:
            continue
        got = torch.ops.oflow.splat_backward(grad_out, frame.detach(), flow.detach(),
                                             None if metric is None else metric.detach(), o, wt, mode, list(mask))
        for asked, g, ref in zip(mask, got, list(grads) + [None]):
            if asked:
                assert _same(g, ref), (name, mask)
            else:
                assert g.numel() == 0


def test_inputs_are_handled_as_fb_consistency_handles_them():
    case = sc.BY_NAME["1x5x17x33-gauss2-soft-s2"]
    frame, flow, metric = _gpu(case)
    out, weight = splat(frame, flow, metric, "soft", return_weight=True)
    # a non-contiguous view of the same values, and float64 inputs (exactly representable: the same fp32 values)
    wide = torch.zeros((1, 5, 17, 66), device=DEV)
    wide[..., ::2] = frame
    view = wide[..., ::2]
    assert not view.is_contiguous()
    o2, w2 = splat(view, flow.double(), metric.double(), "soft", return_weight=True)
    assert o2.dtype == torch.float32 and _same(o2, out) and _same(w2, weight)
    # requires_grad inputs: the same forward bits, gradients in the inputs' dtypes
    fl64 = flow.double().requires_grad_()
    o3 = splat(view, fl64, metric, "soft")
    assert o3.requires_grad and _same(o3.detach(), out)
    (g,) = torch.autograd.grad(o3.sum(), [fl64])
    assert g.dtype == torch.float64 and tuple(g.shape) == tuple(flow.shape)
    # B = 0: empty tensors of the right shape
    e, ew = splat(frame[:0], flow[:0], metric[:0], "soft", return_weight=True)
    assert tuple(e.shape) == (0, 5, 17, 33) and tuple(ew.shape) == (0, 1, 17, 33) and e.device == frame.device
    raw = torch.ops.oflow.splat(frame[:0], flow[:0], None, 0)
    assert tuple(raw[0].shape) == (0, 5, 17, 33) and tuple(raw[1].shape) == (0, 1, 17, 33)
    # shape mismatches raise
    with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
        splat(frame, flow[..., :-1], metric, "soft")
    with pytest.raises(ValueError, match=r"\(B, 1, H, W\)"):
        splat(frame, flow, metric[..., :-1], "soft")
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        torch.ops.oflow.splat(frame, flow[:, :, :-1], None, 0)
    with pytest.raises(RuntimeError, match="shape"):
        torch.ops.oflow.splat_backward(out[..., :-1], frame, flow, metric, out, weight, 3, [True, True, True])
    with pytest.raises(ValueError, match="one device"):
        splat(frame, flow.cpu(), metric, "soft")


def test_interpolate_frame_runs_on_the_gpu():
    from optical_flow import interpolate_frame

    g = torch.Generator().manual_seed(3)
    f0, f1 = torch.rand((1, 3, 16, 24), generator=g), torch.rand((1, 3, 16, 24), generator=g)
    fw = torch.randn((1, 2, 16, 24), generator=g)
    want = interpolate_frame(f0, f1, fw, -fw, 0.25)
    got = interpolate_frame(f0.to(DEV), f1.to(DEV), fw.to(DEV), -fw.to(DEV), 0.25)
    assert got.device.type == "cuda" and float((got.cpu() - want).abs().max()) <= 2.0**-20  # (values in [0, 1])
