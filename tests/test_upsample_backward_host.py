"""The float64 closed form, bounds and tolerance constants of the convex-upsampling backward tests
(tests/upsample_backward_cases.py) checked on the CPU against autograd of the reference composition
(oracle/raft.py:upsample_flow), so the GPU tests compare the kernel with something that is itself pinned down; then the
operator layer as far as it goes without a GPU (registration, Meta kernels, autograd wiring, the CPU refusal) and
RAFT.training_step around a stand-in forward. No GPU needed."""
from __future__ import annotations

import pytest
import torch
import torch.nn as nn

import upsample_backward_cases as uc
from model import RAFT
from model.raft import sequence_loss_torch
from optical_flow import _native, _ops
from oracle import raft as oraft

META = torch.device("meta")


def _reference_grads(case: uc.Case, dtype):
    flow, mask = case.flow.clone().to(dtype).requires_grad_(), case.mask.clone().to(dtype).requires_grad_()  # (copies)
    oraft.upsample_flow(flow, mask).backward(case.grad_out.to(dtype))
    return flow.grad, mask.grad


# ------------------------------------------------------------------------------------------------- the references
def test_cases_cover_the_issue_list():
    assert uc.SHAPES == [(1, 1, 1), (2, 1, 9), (1, 9, 1), (2, 5, 32), (3, 7, 33), (1, 2, 65), (2, 9, 31)]
    assert uc.MASK_SIGMAS == [0.0, 3.0, 30.0] and uc.FLOW_SIGMA == 6.0
    assert len(uc.CASES) == len(uc.SHAPES) * len(uc.MASK_SIGMAS) + 1 and len(set(uc.CASE_IDS)) == len(uc.CASES)
    single = uc.CASES[-1]
    assert int((single.grad_out != 0).sum()) == 2  # both channels of one sub-pixel
    sat = uc.make_case((2, 5, 32), 30.0)
    assert float(torch.softmax(sat.mask.view(2, 9, 64, 5, 32), dim=1).amax(dim=1).median()) > 0.99  # saturated
    assert bool((uc.make_case((2, 5, 32), 0.0).mask == 0).all())  # uniform weights
    again = uc.make_case((3, 7, 33), 3.0)
    assert all(torch.equal(a, b) for a, b in zip(again[1:], uc.CASES[13][1:])) and uc.CASES[13].name == again.name


@pytest.mark.parametrize("case", uc.CASES, ids=uc.CASE_IDS)
def test_closed_form_equals_fp64_autograd_of_the_reference(case):
    ref_flow, ref_mask = _reference_grads(case, torch.float64)
    got_flow, got_mask = uc.backward64(case.grad_out, case.flow, case.mask)
    assert got_flow.shape == case.flow.shape and got_mask.shape == case.mask.shape
    assert float((got_flow - ref_flow).abs().max()) <= 1e-12
    assert float((got_mask - ref_mask).abs().max()) <= 1e-12
    assert float(ref_flow.abs().max()) > 0 and float(ref_mask.abs().max()) > 0


@pytest.mark.parametrize("case", uc.CASES, ids=uc.CASE_IDS)
def test_bounds_dominate_the_gradients(case):
    got_flow, got_mask = uc.backward64(case.grad_out, case.flow, case.mask)
    bound_flow, bound_mask = uc.bounds64(case.grad_out, case.flow, case.mask)
    assert bool((got_flow.abs() <= bound_flow * (1 + 1e-12)).all())
    assert bool((got_mask.abs() <= bound_mask * (1 + 1e-12)).all())
    assert bool((got_flow[bound_flow == 0] == 0).all()) and bool((got_mask[bound_mask == 0] == 0).all())
    assert bool((uc.logit_gap(case.mask) >= 0).all())


def test_only_the_centre_tap_reaches_a_1x1_grid():
    """(1, 1, 1): every neighbour is padding, so grad_flow = 8 * sum_ij w_4 g and a_k = 0 for k != 4."""
    case = uc.CASES[1]
    assert case.flow.shape == (1, 2, 1, 1)
    got_flow, _ = uc.backward64(case.grad_out, case.flow, case.mask)
    w4 = torch.softmax(case.mask.double().view(9, 8, 8), dim=0)[4]
    assert torch.allclose(got_flow.view(2), 8 * (w4 * case.grad_out.double().view(2, 8, 8)).sum(dim=(1, 2)), rtol=1e-13, atol=0)


def test_reference_fp32_autograd_calibrates_the_tolerance():
    """The calibration of K_F and K_M: the reference's own fp32 ATen composition, differentiated on the CPU, needs at
    most K / 4 of the tolerance formula on every committed case (K = 4 x that maximum: the device's expf and summation
    order differ from the CPU's)."""
    worst_f = worst_m = 0.0
    for case in uc.CASES:
        g_flow, g_mask = _reference_grads(case, torch.float32)
        k_f, k_m = uc.error_ratios(g_flow, g_mask, case)
        print(f"{case.name}: fp32 reference needs {k_f:.3f} U bound_flow, {k_m:.3f} U bound_mask (1 + d)")
        worst_f, worst_m = max(worst_f, k_f), max(worst_m, k_m)
    print(f"maxima: flow {worst_f:.3f} (K_F / 4 = {uc.K_F / 4}), mask {worst_m:.3f} (K_M / 4 = {uc.K_M / 4})")
    assert worst_f <= uc.K_F / 4 and worst_m <= uc.K_M / 4
    assert worst_f >= uc.K_F / 8 and worst_m >= uc.K_M / 8  # and the constants are not looser than measured
    for case in uc.CASES:  # the same statement through the assertion the GPU tests use
        uc.assert_close(*_reference_grads(case, torch.float32), case, "fp32 reference")


# ------------------------------------------------------------------------------------------------- operator layer
def test_ops_are_registered():
    _native.load()
    assert "convex_upsample" in _ops.OPS and "convex_upsample_backward" in _ops.OPS
    assert "oflow_convex_upsample_backward_f32" in _native.SYMBOLS
    for name in ("convex_upsample", "convex_upsample_backward"):
        assert getattr(torch.ops.oflow, name).default._schema.name == f"oflow::{name}"


def test_meta_shapes_and_argument_errors():
    _native.load()
    ops = torch.ops.oflow
    flow, mask = torch.empty(3, 2, 7, 33, device=META), torch.empty(3, 576, 7, 33, device=META)
    out = ops.convex_upsample(flow, mask)
    assert tuple(out.shape) == (3, 2, 56, 264) and out.dtype == torch.float32
    assert ops.convex_upsample(flow.half(), mask.half()).dtype == torch.float32
    g = torch.empty(3, 2, 56, 264, device=META)
    for need in ([True, True], [True, False], [False, True], [False, False]):
        g_flow, g_mask = ops.convex_upsample_backward(g, flow, mask, need)
        assert tuple(g_flow.shape) == (tuple(flow.shape) if need[0] else (0,))
        assert tuple(g_mask.shape) == (tuple(mask.shape) if need[1] else (0,))
        assert g_flow.dtype == g_mask.dtype == torch.float32
    bad = [
        (torch.empty(3, 3, 7, 33, device=META), mask),  # flow channels
        (flow, torch.empty(3, 575, 7, 33, device=META)),  # mask channels
        (flow, torch.empty(2, 576, 7, 33, device=META)),  # batch
        (flow, torch.empty(3, 576, 7, 32, device=META)),  # width
        (flow[0], mask[0]),  # rank
    ]
    for f, m in bad:
        with pytest.raises(RuntimeError, match=r"must be \(B, 2, H, W\) and mask"):
            ops.convex_upsample(f, m)
        with pytest.raises(RuntimeError, match=r"must be \(B, 2, H, W\) and mask"):
            ops.convex_upsample_backward(g, f, m, [True, True])
    with pytest.raises(RuntimeError, match="65535"):
        ops.convex_upsample(torch.empty(1, 2, 65536, 1, device=META), torch.empty(1, 576, 65536, 1, device=META))
    for bad_g in (g[:, :1], g[..., :-1], g[:, :, :-8], g[:2]):
        with pytest.raises(RuntimeError, match="grad_out"):
            ops.convex_upsample_backward(bad_g, flow, mask, [True, True])


def test_gradients_flow_on_meta_tensors():
    _native.load()
    flow = torch.empty(2, 2, 5, 9, device=META, requires_grad=True)
    mask = torch.empty(2, 576, 5, 9, device=META, requires_grad=True)
    out = torch.ops.oflow.convex_upsample(flow, mask)
    assert out.requires_grad
    out[..., 3:-2].sum().backward()  # a cropped, non-contiguous gradient
    assert flow.grad.shape == flow.shape and mask.grad.shape == mask.shape
    # one input only; and the Python entry point takes the op under autograd
    flow2 = torch.empty(2, 2, 5, 9, device=META, requires_grad=True)
    _native.convex_upsample(flow2, mask.detach()).sum().backward()
    assert flow2.grad.shape == flow2.shape
    mask2 = torch.empty(2, 576, 5, 9, device=META, dtype=torch.float16, requires_grad=True)
    _native.convex_upsample(flow2.detach(), mask2).sum().backward()
    assert mask2.grad.shape == mask2.shape and mask2.grad.dtype == torch.float16


def test_cpu_tensors_raise():
    _native.load()
    flow, mask, g = torch.zeros(1, 2, 2, 3), torch.zeros(1, 576, 2, 3), torch.zeros(1, 2, 16, 24)
    for call in (
        lambda: torch.ops.oflow.convex_upsample(flow, mask),
        lambda: torch.ops.oflow.convex_upsample_backward(g, flow, mask, [True, True]),
        lambda: _native.convex_upsample(flow, mask),
        lambda: _native.convex_upsample(flow.clone().requires_grad_(), mask),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_upsample_impl_attribute():
    model = RAFT()
    assert model.upsample_impl == "native" and model.update_impl == "split" and model.encoder_impl == "split"
    case = uc.CASES[4]
    flow, mask = case.flow.clone().requires_grad_(), case.mask.clone().requires_grad_()
    for impl in ("native", "aten"):  # CPU tensors: the reference composition either way
        assert torch.equal(RAFT.upsample_flow(flow, mask, impl), oraft.upsample_flow(flow, mask))
    with pytest.raises(ValueError, match="upsample_impl"):
        RAFT.upsample_flow(flow, mask, "triton")


# ------------------------------------------------------------------------------------------------- training_step
class _ScaledRAFT(RAFT):
    """RAFT with the forward replaced by a differentiable per-pixel function of the frames and one parameter (the
    product's forward needs the GPU): what training_step does around the forward runs as is."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.gain = nn.Parameter(torch.tensor(0.05))

    def forward(self, image0, image1, iters=12, flow_init=None, upsample=True, test_mode=False):
        assert not test_mode
        self.seen = iters
        base = image1[:, :2] - image0[:, 1:3]
        return [base * self.gain * (i + 1) / iters for i in range(iters)]


def test_training_step_equals_the_reference_formula_on_cpu():
    from model import synthetic

    iters, gamma = 5, 0.85
    model = _ScaledRAFT(iters=iters, gamma=gamma)
    img0, img1 = synthetic.synthetic_pair(2, 24, 40, seed=3)
    flow = uc.gaussian(11, (2, 2, 24, 40), 3.0)
    flow[0, :, 2, 3] = 500.0  # past max_flow: excluded from the loss
    valid = (uc.gaussian(12, (2, 24, 40)) > -0.5).float()
    loss = model.training_step((img0, img1, flow, valid), 0)
    assert model.seen == iters and loss.requires_grad and loss.dim() == 0
    loss.backward()

    ref_model = _ScaledRAFT(iters=iters, gamma=gamma)
    preds = ref_model(img0, img1, iters=iters)
    weights = [gamma ** (iters - i - 1) for i in range(iters)]
    ref_loss, ref_px = sequence_loss_torch(preds, flow, valid, weights, 400.0)
    ref_loss.backward()
    assert torch.equal(loss.detach(), ref_loss.detach()) and torch.equal(model.gain.grad, ref_model.gain.grad)
    assert float(model.gain.grad.abs()) > 0
    assert model.last_train_metrics == ref_px and set(ref_px) == {"1px", "3px", "5px"}
    keep = valid.reshape(-1) >= 0.5
    epe = torch.norm(preds[-1].detach() - flow, p=2, dim=1).reshape(-1)[keep]
    assert torch.allclose(model.epe_train.compute(), epe.double().mean().float(), rtol=1e-6)
    assert model.epe_val.compute().isnan()  # the validation metrics are untouched
    model.training_step((img0, img1, flow, valid))  # batch_idx defaults to 0; the metric accumulates
    assert float(model.epe_train._state[1]) == 2 * int(keep.sum())
