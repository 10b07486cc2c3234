"""The convex-upsampling backward (csrc/upsample_backward.hip) against float64: the C ABI called directly, its null-output
and shape contracts, then ``torch.ops.oflow.convex_upsample`` under autograd (eager and torch.compile), RAFT.upsample_flow
and one training step. Closed form, inputs and tolerances: tests/upsample_backward_cases.py (checked and calibrated on
the CPU by tests/test_upsample_backward_host.py).

Tolerance per element: grad_flow K_F * 2^-24 * bound_flow; grad_mask K_M * 2^-24 * bound_mask * (1 + d) + 1e-30 * 8
max|flow| max|grad_out|, with the bounds the closed form on absolute values, d = max_k' m_k' - m_k, and K_F, K_M four
times what the reference's own fp32 autograd needs on the CPU.
"""
from __future__ import annotations

import ctypes

import pytest
import torch

import upsample_backward_cases as uc
from model import RAFT, synthetic
from model.raft import sequence_loss
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
E_NULL, E_SHAPE = -1, -2
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _abi(g, flow, mask, want_flow=True, want_mask=True, with_scratch=True, dims=None):
    """oflow_convex_upsample_backward_f32 on NaN-filled outputs and scratch -> (status, grad_flow, grad_mask, scratch)."""
    b, _, h, w = flow.shape
    gf, gm = torch.full(flow.shape, NAN, device=DEV), torch.full(mask.shape, NAN, device=DEV)
    sc = torch.full((b, 18, h, w), NAN, device=DEV)
    st = _native.load().oflow_convex_upsample_backward_f32(
        g.data_ptr(), flow.data_ptr(), mask.data_ptr(), *(dims or (b, h, w)), gf.data_ptr() if want_flow else None,
        gm.data_ptr() if want_mask else None, sc.data_ptr() if with_scratch else None, _stream())
    torch.cuda.synchronize()
    return st, gf.cpu(), gm.cpu(), sc.cpu()


def _dev(case):
    return case.grad_out.to(DEV), case.flow.to(DEV), case.mask.to(DEV)


# ----------------------------------------------------------------------------------------------------------
# C ABI (include/oflow.h), called directly
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.CASES, ids=uc.CASE_IDS)
def test_abi_backward_matches_fp64(case):
    """Every element of both outputs is written (the buffers start as NaN) and is within tolerance of float64."""
    st, gf, gm, _ = _abi(*_dev(case))
    assert st == 0
    uc.assert_close(gf, gm, case, "C ABI")


def test_abi_forms_only_the_requested_outputs():
    """A NULL output is not formed and the other is bit-identical to the both-outputs call; the mask-only call needs no
    scratch and leaves it alone; no output at all, a missing input or a flow gradient without scratch is OFLOW_E_NULL
    and writes nothing."""
    case = uc.CASES[13]  # 3x7x33, sigma 3
    g, flow, mask = _dev(case)
    st, both_f, both_m, sc = _abi(g, flow, mask)
    assert st == 0 and bool(torch.isfinite(sc).all())
    st, only_f, no_m, _ = _abi(g, flow, mask, want_mask=False)
    assert st == 0 and torch.equal(only_f, both_f) and bool(torch.isnan(no_m).all())
    for with_scratch in (True, False):
        st, no_f, only_m, sc = _abi(g, flow, mask, want_flow=False, with_scratch=with_scratch)
        assert st == 0 and torch.equal(only_m, both_m) and bool(torch.isnan(no_f).all()) and bool(torch.isnan(sc).all())
    untouched = lambda r: all(bool(torch.isnan(t).all()) for t in r[1:])  # noqa: E731
    r = _abi(g, flow, mask, want_flow=False, want_mask=False)
    assert r[0] == E_NULL and untouched(r)
    r = _abi(g, flow, mask, with_scratch=False)
    assert r[0] == E_NULL and untouched(r)
    lib, b, h, w = _native.load(), *case.flow.shape[:1], *case.flow.shape[2:]
    out = torch.full(mask.shape, NAN, device=DEV)
    for args in ((None, flow.data_ptr(), mask.data_ptr()), (g.data_ptr(), None, mask.data_ptr()), (g.data_ptr(), flow.data_ptr(), None)):
        assert lib.oflow_convex_upsample_backward_f32(*args, b, h, w, None, out.data_ptr(), None, _stream()) == E_NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("dims", [(0, 7, 33), (3, 0, 33), (3, 7, 0), (-1, 7, 33), (65536, 7, 33), (3, 65536, 33)])
def test_abi_bad_shapes_return_e_shape(dims):
    st, gf, gm, sc = _abi(*_dev(uc.CASES[13]), dims=dims)
    assert st == E_SHAPE
    assert bool(torch.isnan(gf).all()) and bool(torch.isnan(gm).all()) and bool(torch.isnan(sc).all())


# ----------------------------------------------------------------------------------------------------------
# torch.ops.oflow.convex_upsample / convex_upsample_backward
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [uc.CASES[i] for i in (1, 13, 17, 20)], ids=[uc.CASE_IDS[i] for i in (1, 13, 17, 20)])
def test_forward_op_equals_the_ctypes_path(case):
    _, flow, mask = _dev(case)
    with torch.no_grad():
        want = _native.convex_upsample(flow, mask)
        assert torch.equal(OPS.convex_upsample(flow, mask), want)
    got = _native.convex_upsample(flow.clone().requires_grad_(), mask)  # under autograd: the op
    assert got.requires_grad and torch.equal(got.detach(), want)


@pytest.mark.parametrize("case", uc.CASES, ids=uc.CASE_IDS)
def test_autograd_matches_fp64(case):
    g, flow, mask = _dev(case)
    flow, mask = flow.requires_grad_(), mask.requires_grad_()
    OPS.convex_upsample(flow, mask).backward(g)
    uc.assert_close(flow.grad, mask.grad, case, "autograd")


def test_autograd_with_a_noncontiguous_grad_out():
    """grad_out as a cropped view of a larger tensor (what InputPadder.unpad's backward hands over): the same bits as
    with its contiguous copy, and within tolerance."""
    case = uc.CASES[13]
    g, flow, mask = _dev(case)
    wide = torch.full((g.shape[0], 2, g.shape[2] + 5, g.shape[3] + 3), NAN, device=DEV)
    view = wide[:, :, 2 : 2 + g.shape[2], 1 : 1 + g.shape[3]]
    view.copy_(g)
    assert not view.is_contiguous()
    grads = []
    for gout in (g, view):
        f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
        OPS.convex_upsample(f, m).backward(gout)
        grads.append((f.grad, m.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    uc.assert_close(*grads[1], case, "non-contiguous grad_out")
    # and through an actual crop of the output, whose gradient is zero outside the crop
    f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
    keep = (slice(None), slice(None), slice(3, -2), slice(1, -4))
    OPS.convex_upsample(f, m)[keep].backward(g[keep])
    zeroed = torch.zeros_like(case.grad_out)
    zeroed[keep] = case.grad_out[keep]
    uc.assert_close(f.grad, m.grad, uc.Case(case.name + "-cropped", zeroed, case.flow, case.mask), "cropped output")


def test_autograd_forms_only_the_wanted_gradients():
    case = uc.CASES[13]
    g, flow, mask = _dev(case)
    f = flow.clone().requires_grad_()
    OPS.convex_upsample(f, mask).backward(g)
    uc.assert_close(f.grad, None, case, "flow only")
    m = mask.clone().requires_grad_()
    OPS.convex_upsample(flow, m).backward(g)
    uc.assert_close(None, m.grad, case, "mask only")
    for need in ([True, False], [False, True], [False, False]):
        gf, gm = OPS.convex_upsample_backward(g, flow, mask, need)
        assert gf.numel() == (flow.numel() if need[0] else 0) and gm.numel() == (mask.numel() if need[1] else 0)
    h16 = mask.half().requires_grad_()  # a low-precision input gets a gradient of its own dtype
    OPS.convex_upsample(flow, h16).sum().backward()
    assert h16.grad.dtype == torch.float16 and h16.grad.shape == mask.shape
    with pytest.raises(RuntimeError, match="grad_out"):
        OPS.convex_upsample_backward(g[..., :-1], flow, mask, [True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.convex_upsample_backward(g.cpu(), flow, mask, [True, True])
    empty = OPS.convex_upsample_backward(torch.zeros(0, 2, 16, 24, device=DEV), torch.zeros(0, 2, 2, 3, device=DEV),
                                         torch.zeros(0, 576, 2, 3, device=DEV), [True, True])
    assert tuple(empty[0].shape) == (0, 2, 2, 3) and tuple(empty[1].shape) == (0, 576, 2, 3)


def test_backward_is_deterministic_on_dirty_memory():
    """No atomics and nothing left to the caller to zero: with the allocator's free blocks filled with NaN beforehand
    (the outputs and the scratch land in them), two runs give finite, bit-identical gradients."""
    g, flow, mask = _dev(uc.CASES[17])  # 1x2x65, sigma 30
    runs = []
    for _ in range(2):
        junk = [torch.full((1 << s,), NAN, device=DEV) for s in range(8, 21)]
        del junk
        gf, gm = OPS.convex_upsample_backward(g, flow, mask, [True, True])
        runs.append((gf.clone(), gm.clone()))
        torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_compile_fullgraph_forward_and_backward():
    torch._dynamo.reset()
    g, flow, mask = _dev(uc.CASES[13])

    def loss(f, m):
        return (torch.ops.oflow.convex_upsample(f, m) * g).sum()

    grads = []
    for fn in (loss, torch.compile(loss, fullgraph=True, dynamic=False)):
        f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
        value = fn(f, m)
        value.backward()
        grads.append((value.detach(), f.grad, m.grad))
    torch.testing.assert_close(grads[1][0], grads[0][0], rtol=1e-5, atol=1e-5)
    assert torch.equal(grads[1][1], grads[0][1]) and torch.equal(grads[1][2], grads[0][2])


# ----------------------------------------------------------------------------------------------------------
# RAFT
# ----------------------------------------------------------------------------------------------------------
def test_raft_upsample_flow_under_grad_equals_inference():
    _, flow, mask = _dev(uc.CASES[13])
    with torch.inference_mode():
        want = RAFT.upsample_flow(flow, mask)
    f, m = flow.clone().requires_grad_(), mask.clone().requires_grad_()
    got = RAFT.upsample_flow(f, m)
    assert got.requires_grad and torch.equal(got.detach(), want)
    assert "ConvexUpsample" in type(got.grad_fn).__name__ or "convex_upsample" in str(got.grad_fn).lower()
    aten = RAFT.upsample_flow(f, m, "aten")
    assert "convex_upsample" not in str(aten.grad_fn).lower()
    torch.testing.assert_close(aten, got, rtol=1e-5, atol=1e-5)


def _train_model():
    m = RAFT(iters=3)
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    m = m.to(DEV).train()
    for mod in m.modules():  # eval-mode batch norm, as test_raft_training_gradients_match_oracle
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    return m


def _biases_under_instance_norm(model):
    """Names of the convolution biases whose output goes straight into an InstanceNorm2d without affine parameters
    (extractor.py: conv1 -> norm1, conv2 -> norm2 and the downsample pair of fnet's blocks, and fnet's stem): the norm
    subtracts the per-channel mean, which removes a per-channel constant, so dL/dbias is exactly 0 and what autograd
    returns is rounding noise. Found from the module structure, not from any gradient."""
    plain = lambda n: isinstance(n, torch.nn.InstanceNorm2d) and not n.affine  # noqa: E731
    names = set()
    for prefix, mod in model.named_modules():
        for conv, norm in (("conv1", "norm1"), ("conv2", "norm2")):
            c = getattr(mod, conv, None)
            if isinstance(c, torch.nn.Conv2d) and c.bias is not None and plain(getattr(mod, norm, None)):
                names.add(f"{prefix}.{conv}.bias")
        ds = getattr(mod, "downsample", None)
        if isinstance(ds, torch.nn.Sequential) and len(ds) == 2 and isinstance(ds[0], torch.nn.Conv2d) and plain(ds[1]):
            names.add(f"{prefix}.downsample.0.bias")
    return names


def test_training_step_native_and_aten_upsampling_agree():
    """One 128 x 128, 3-iteration training step: every parameter gradient with the native upsampling backward vs the
    ATen composition's to a relative norm of 1e-3 (the bar of test_raft_training_gradients_match_oracle), the mask
    head's last convolution -- whose gradient exists only through this kernel -- by name; and training_step returns
    the loss of the hand-written composition.

    The relative norm |native - aten| / |aten| is 0 / 0 for the biases in front of fnet's instance norms (exact
    gradient 0, see _biases_under_instance_norm: measured 1.18 on fnet.conv1.bias, noise against noise, and it would
    be O(1) between two runs of either path alone). For those the test asserts what exact arithmetic says instead: each
    path's bias gradient norm is <= 1e-3 of the same convolution's weight-gradient norm, i.e. below what the bar
    already tolerates on that layer. Every other parameter is held to the relative norm as stated."""
    img0, img1 = (x.to(DEV) for x in synthetic.synthetic_pair(1, 128, 128, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (1, 2, 128, 128), 2.0)).to(DEV)
    valid = (torch.from_numpy(synthetic.hash_normal(32, (1, 128, 128), 1.0)) > -1.0).float().to(DEV)
    grads, losses = {}, {}
    for impl in ("native", "aten"):
        model = _train_model()
        model.upsample_impl = impl
        loss = model.training_step((img0, img1, target, valid), 0)
        loss.backward()
        losses[impl] = loss.detach()
        grads[impl] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        if impl == "native":
            assert set(model.last_train_metrics) == {"1px", "3px", "5px"}
            assert float(model.epe_train.compute()) > 0
            preds = model(img0, img1, iters=3)  # the hand-written composition, same model and path
            assert len(preds) == 3 and "convex_upsample" in str(preds[-1].grad_fn).lower()
            hand, px = sequence_loss(preds, target, valid, gamma=model.hparams.gamma)
            assert torch.equal(hand.detach(), losses[impl]) and px == model.last_train_metrics
    assert set(grads["native"]) == set(grads["aten"])
    assert "update_block.mask.2.weight" in grads["native"] and "update_block.mask.0.weight" in grads["native"]
    torch.testing.assert_close(losses["native"], losses["aten"], rtol=1e-5, atol=0)
    null = _biases_under_instance_norm(model)
    assert null and null <= set(grads["aten"]) and all(k.startswith("fnet.") and k.endswith(".bias") for k in null)
    rels = {}
    for k, want in grads["aten"].items():
        got = grads["native"][k]
        if k in null:
            # exact gradient 0: both sides are rounding noise, far below what the bar tolerates on the same
            # convolution's weight gradient
            w = grads["aten"][k[: -len("bias")] + "weight"].norm()
            rels[k] = max(float(got.norm() / w), float(want.norm() / w))
        else:
            assert float(want.norm()) > 0, k
            rels[k] = float((got - want).norm() / want.norm())
    for k, rel in sorted(rels.items(), key=lambda t: -t[1])[:8]:
        print(f"training step: {k}: {rel:.2e}" + (" (zero gradient: norm / weight-gradient norm)" if k in null else ""))
    print(f"training step: update_block.mask.2.weight: {rels['update_block.mask.2.weight']:.2e}; "
          f"{len(rels) - len(null)} parameters compared, {len(null)} with an exactly zero gradient")
    assert "update_block.mask.2.weight" not in null and rels["update_block.mask.2.weight"] <= 1e-3
    bad = {k: r for k, r in rels.items() if not r <= 1e-3}
    assert not bad, bad
