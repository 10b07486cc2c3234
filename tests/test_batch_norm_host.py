"""The float64 closed forms, bounds and tolerance constants of the batch-statistics batch norm tests
(tests/batch_norm_cases.py) checked on the CPU against ``relu(F.batch_norm(..., training=True))`` and its autograd, the
buffer-update formula against ``nn.BatchNorm2d``, then the ABI and operator layers as far as they go without a GPU
(exported symbols, the workspace query, registration, Meta kernels, the CPU refusal) and the model's switch. No GPU
needed."""
from __future__ import annotations

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import batch_norm_cases as bc
from model import RAFT
from model import extractor as ext
from optical_flow import _native, _ops

META = torch.device("meta")
NEW_SYMBOLS = ("oflow_batch_norm_chunk_elements", "oflow_batch_norm_workspace_floats", "oflow_batch_norm_forward_f32",
               "oflow_batch_norm_backward_f32")
NEW_OPS = ("batch_norm_act", "batch_norm_act_backward")


def _aten(case: bc.BNCase, dtype):
    """(y, mean, var, dx, dgamma, dbeta) by ATen on the CPU in ``dtype``. The statistics are what the call leaves in
    zero-initialised running buffers at momentum 1: the mean, and the unbiased variance, taken back to the biased one in
    float64."""
    x, w, b = (t.clone().to(dtype).requires_grad_() for t in (case.x, case.weight, case.bias))
    c = x.shape[1]
    n = x.numel() // c
    rm, rv = torch.zeros(c, dtype=dtype), torch.zeros(c, dtype=dtype)
    y = F.batch_norm(x, rm, rv, w, b, True, 1.0, bc.EPS)
    y = torch.relu(y) if case.relu else y
    y.backward(case.grad_out.to(dtype))
    return y.detach(), rm, rv.double() * (n - 1) / n, x.grad, w.grad, b.grad


@pytest.mark.parametrize("case", bc.BN_CASES, ids=bc.BN_IDS)
def test_closed_forms_equal_float64_autograd(case):
    refs, _, _ = bc.reference(case)
    for name, got, ref in zip(bc.NAMES, _aten(case, torch.float64), refs):
        scale = float(ref.abs().max()) + 1e-30
        assert tuple(got.shape) == tuple(ref.shape), name
        assert float((got - ref).abs().max()) <= 1e-10 * max(scale, 1e-3), (case.name, name)


def test_cases_cover_the_kernels_edges_and_keep_the_relu_gap():
    """Every float64 pre-ReLU output is at least RELU_GAP from 0; the constant channel has var = 0 and an empty mask; a
    negative scale is present everywhere; the chunked case has two chunks with a ragged second one."""
    for case in bc.BN_CASES:
        pre = bc.output64(case)
        assert float(pre.abs().min()) >= bc.RELU_GAP, (case.name, float(pre.abs().min()))
        assert float(case.weight[0]) < 0 and bool((case.weight[1:] > 0).all())
        assert bool((pre > 0).any()) and bool((pre < 0).any())
    const = bc.BN_BY_NAME["2x2x4x8-constant-relu"]
    refs, _, bounds = bc.reference(const)
    assert float(refs[2][1]) == 0.0 and float(bounds[2][1]) == 0.0 and float(refs[2][0]) > 0.5
    assert not bool((bc.output64(const)[:, 1] > 0).any()) and not bool(refs[3][:, 1].any())
    plain = bc.BN_BY_NAME["2x2x4x8-constant"]  # without the ReLU the constant channel sees r = 1 / sqrt(eps)
    dx = bc.reference(plain)[0][3][:, 1]
    g = plain.grad_out.double()[:, 1]
    want = float(plain.weight[1]) / bc.EPS ** 0.5 * (g - g.mean())
    assert float((dx - want).abs().max()) <= 1e-12
    off = bc.BN_BY_NAME["2x1x46x62-offset"]
    assert abs(float(bc.reference(off)[0][1]) - 100.0) < 1e-3 and abs(float(bc.reference(off)[0][2]) - 0.01) < 1e-3
    b, c, hw = bc.BN_BY_NAME[bc.TWO_CHUNKS].dims
    assert (hw + bc.CHUNK - 1) // bc.CHUNK == 2 and hw % bc.CHUNK == 5
    assert {(c.x.shape[2] * c.x.shape[3]) for c in bc.BN_CASES} >= {2, 63, 35, 255, 256, 257, 240}


def test_reference_fp32_calibrates_the_tolerances():
    """K_OUT, K_STAT and K_GRAD are four times what ATen's fp32 CPU computation needs on the committed cases."""
    worst = {}
    for case in bc.BN_CASES:
        for name, r in zip(bc.NAMES, bc.error_ratios(_aten(case, torch.float32), case)):
            worst[name] = max(worst.get(name, 0.0), r)
    print("ATen fp32 CPU, worst err / (U * bound):", {k: round(v, 2) for k, v in worst.items()})
    for name, k in zip(bc.NAMES, bc.KS):
        assert worst[name] <= k / 4, (name, worst[name])


def test_tolerance_catches_a_misplaced_term_and_a_biased_variance():
    case = bc.BN_BY_NAME["2x64x12x20-relu"]
    refs, tols, _ = bc.reference(case)
    bc.assert_close([t.float() for t in refs], case, "rounded reference")
    n = case.x.numel() // case.x.shape[1]
    bad = [t.clone() for t in refs]
    bad[2] = bad[2] * n / (n - 1)  # the unbiased variance in the biased one's place
    with pytest.raises(AssertionError):
        bc.assert_close([t.float() for t in bad], case, "unbiased variance")
    bad = [t.clone() for t in refs]
    bad[3] = bad[3] + (case.weight.double().view(1, -1, 1, 1) * refs[5].view(1, -1, 1, 1) / n)  # dbeta / n left out, r = 1
    assert float((bad[3] - refs[3]).abs().max()) > 4 * float(tols[3].min())
    with pytest.raises(AssertionError):
        bc.assert_close([t.float() for t in bad], case, "misplaced")


def test_buffer_update_formula_reproduces_the_module():
    """running_mean, running_var (the unbiased estimate) and num_batches_tracked after one train-mode call, float64."""
    case = bc.BN_BY_NAME["3x3x5x7"]
    c = case.x.shape[1]
    n = case.x.numel() // c
    for momentum in (0.1, 0.37):
        m = nn.BatchNorm2d(c, eps=bc.EPS, momentum=momentum).double().train()
        with torch.no_grad():
            m.running_mean.copy_(torch.tensor([0.3, -0.2, 0.1]))
            m.running_var.copy_(torch.tensor([0.5, 1.5, 2.5]))
            m.num_batches_tracked.fill_(7)
        before = (m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone())
        m(case.x.double())
        refs, _, _ = bc.reference(case)
        rm, rv, tracked = bc.updated_buffers(*before, refs[1], refs[2], n, momentum)
        assert float((m.running_mean - rm).abs().max()) <= 1e-14 and float((m.running_var - rv).abs().max()) <= 1e-14
        assert int(m.num_batches_tracked) == int(tracked) == 8


def test_symbols_workspace_query_and_chunk_constant():
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS and getattr(lib, name)
    assert lib.oflow_batch_norm_chunk_elements() == bc.CHUNK
    for b, c, hw in ((1, 1, 1), (2, 3, bc.CHUNK), (2, 3, bc.CHUNK + 1), (8, 64, 184 * 248), (3, 5, 3 * bc.CHUNK - 1)):
        assert lib.oflow_batch_norm_workspace_floats(b, c, hw) == bc.workspace_floats(b, c, hw)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 2, 2), (65536, 65536, 1)):
        assert lib.oflow_batch_norm_workspace_floats(*bad) == 0


def test_ops_are_registered_with_meta_kernels():
    _ops.load()
    for name in NEW_OPS:
        assert name in _ops.OPS and getattr(torch.ops.oflow, name)
    O = torch.ops.oflow
    x, p = torch.zeros(2, 3, 5, 7, device=META), torch.zeros(3, device=META)
    assert [tuple(t.shape) for t in O.batch_norm_act(x, p, p, 1e-5, True)] == [(2, 3, 5, 7), (3,), (3,)]
    got = O.batch_norm_act_backward(x, x, p, p, p, p, 1e-5, True, [True, False, True])
    assert [tuple(t.shape) for t in got] == [(2, 3, 5, 7), (0,), (3,)]
    with pytest.raises(RuntimeError, match="weight"):
        O.batch_norm_act(x, p[:2], p, 1e-5, True)
    with pytest.raises(RuntimeError, match="var"):
        O.batch_norm_act_backward(x, x, p, p, p, p[:2], 1e-5, True, [True] * 3)
    with pytest.raises(RuntimeError, match="grad_out"):
        O.batch_norm_act_backward(x[..., :-1], x, p, p, p, p, 1e-5, True, [True] * 3)


def test_cpu_tensors_are_refused():
    _ops.load()
    O = torch.ops.oflow
    x, p = torch.zeros(2, 3, 4, 4), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.batch_norm_act(x, p, p, 1e-5, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.batch_norm_act_backward(x, x, p, p, p, p, 1e-5, True, [True] * 3)


def test_batch_norm_impl_attribute_and_cpu_routing():
    """The attribute defaults to "aten", is not a hyper-parameter, is validated in the forward, and on the CPU "native"
    takes the module path: output, gradients and buffers equal the default's bit for bit."""
    model = RAFT(iters=1)
    assert model.batch_norm_impl == "aten" and model.encoder_backward_impl == "aten"
    assert "batch_norm_impl" not in model.hparams
    keys = list(model.state_dict())
    x = torch.randn(2, 3, 16, 24, generator=torch.Generator().manual_seed(1))
    runs = []
    for impl in ("aten", "native"):
        torch.manual_seed(3)
        enc = ext.BasicEncoder(output_dim=32, norm_fn="batch").train()
        assert enc.batch_norm_impl == "aten"
        enc.batch_norm_impl = impl
        y = enc(x)
        y.square().sum().backward()
        assert all(blk.batch_norm_impl == impl for layer in (enc.layer1, enc.layer2, enc.layer3) for blk in layer)
        runs.append([y.detach()] + [p.grad for p in enc.parameters()] + [b.clone() for b in enc.buffers()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))
    enc.batch_norm_impl = "miopen"
    with pytest.raises(ValueError, match="batch_norm_impl"):
        enc(x)
    with pytest.raises(ValueError, match="batch_norm_impl"):
        ext.enc_norm_act(nn.BatchNorm2d(3), x, True, "aten", "miopen")
    model.batch_norm_impl = "miopen"
    img = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="batch_norm_impl"):
        model(img, img, iters=1)
    assert list(model.state_dict()) == keys


def test_ineligible_layers_call_the_module_on_the_cpu():
    """Everything is ineligible on the CPU: the module's result, buffer updates and errors come back unchanged."""
    x = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(2), requires_grad=True)
    for norm in (nn.BatchNorm2d(4), nn.BatchNorm2d(4, momentum=None), nn.BatchNorm2d(4, track_running_stats=False),
                 nn.BatchNorm2d(4, affine=False), nn.BatchNorm2d(4).eval(), nn.InstanceNorm2d(4)):
        twin = type(norm)(4, **{k: getattr(norm, k) for k in ("momentum", "affine", "track_running_stats")})
        twin.train(norm.training)
        got, want = ext.enc_norm_act(norm, x, True, "aten", "native"), torch.relu(twin(x))
        assert torch.equal(got, want)
        assert all(torch.equal(a, b) for a, b in zip(norm.buffers(), twin.buffers()))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ext.enc_norm_act(nn.BatchNorm2d(4), x[:1, :, :1, :1], True, "aten", "native")
