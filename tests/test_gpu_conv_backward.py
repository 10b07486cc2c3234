"""The convolution backward (csrc/conv_backward.hip) against float64: the C ABI called directly, its null-output and
shape contracts, then ``torch.ops.oflow.conv2d_same`` under autograd (eager and torch.compile) and one training step with
``RAFT.conv_backward_impl = "native"`` against ``"aten"``. Closed form, inputs and tolerances:
tests/conv_backward_cases.py (checked and calibrated on the CPU by tests/test_conv_backward_host.py).

Tolerance per element: min(K, n + 2) * 2^-24 * bound, with bound the closed form on absolute values, n the number of
terms of the element's sum and K four times what ATen's own fp32 autograd needs on the CPU.
"""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_backward_cases as cc
from model import RAFT, synthetic
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
E_NULL, E_SHAPE = -1, -2
NAN = float("nan")
PICK = ("3x3-c33-n126-2x4x8", "1x5-c126-n33-5x1x13", "7x7-c2-n33-2x5x9", "3x3-c8-n8-3x41x37")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(case):
    return case.grad_out.to(DEV), case.x.to(DEV), case.weight.to(DEV)


def _nan_buffers(case):
    lib = _native.load()
    n_ws = lib.oflow_conv2d_backward_weight_workspace_floats(*case.dims)
    assert n_ws > 0
    return (torch.full(case.x.shape, NAN, device=DEV), torch.full(case.weight.shape, NAN, device=DEV),
            torch.full((case.dims[1],), NAN, device=DEV), torch.full((n_ws,), NAN, device=DEV))


def _ptr(t, keep=True):
    return t.data_ptr() if keep else None


def _abi_weight(case, g, x, want_w=True, want_b=True, dims=None, with_g=True, with_x=True, with_ws=True):
    """oflow_conv2d_backward_weight_f32 on NaN-filled outputs and workspace -> (status, grad_weight, grad_bias,
    workspace)."""
    _, gw, gb, ws = _nan_buffers(case)
    st = _native.load().oflow_conv2d_backward_weight_f32(_ptr(g, with_g), _ptr(x, with_x), *(dims or case.dims),
                                                         _ptr(gw, want_w), _ptr(gb, want_b), _ptr(ws, with_ws), _stream())
    torch.cuda.synchronize()
    return st, gw.cpu(), gb.cpu(), ws.cpu()


def _abi_input(case, g, w, dims=None, with_g=True, with_w=True, with_out=True):
    """oflow_conv2d_backward_input_f32 on a NaN-filled output -> (status, grad_input)."""
    gx = _nan_buffers(case)[0]
    st = _native.load().oflow_conv2d_backward_input_f32(_ptr(g, with_g), _ptr(w, with_w), *(dims or case.dims),
                                                        _ptr(gx, with_out), _stream())
    torch.cuda.synchronize()
    return st, gx.cpu()


# ----------------------------------------------------------------------------------------------------------
# C ABI (include/oflow.h), called directly
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CASES, ids=cc.CASE_IDS)
def test_abi_backward_matches_fp64(case):
    """Every element of the three outputs is written (the buffers and the workspace start as NaN) and is within
    tolerance of float64."""
    g, x, w = _dev(case)
    st, gx = _abi_input(case, g, w)
    assert st == 0
    st, gw, gb, _ = _abi_weight(case, g, x)
    assert st == 0
    cc.assert_close(gx, gw, gb, case, "C ABI")


@pytest.mark.parametrize("name", ["3x3-c8-n8-3x41x37", "1x5-c126-n33-5x1x13"])
def test_abi_forms_only_the_requested_outputs(name):
    """A NULL gradient is not formed and the other is bit-identical to the both-outputs call (the bias gradient alone
    needs no x); no output at all, a missing input or a missing workspace is OFLOW_E_NULL and writes nothing."""
    case = cc.BY_NAME[name]
    g, x, w = _dev(case)
    st, both_w, both_b, ws = _abi_weight(case, g, x)
    assert st == 0 and bool(torch.isfinite(ws).all())  # the whole workspace the query asks for is used
    st, only_w, no_b, _ = _abi_weight(case, g, x, want_b=False)
    assert st == 0 and torch.equal(only_w, both_w) and bool(torch.isnan(no_b).all())
    for with_x in (True, False):
        st, no_w, only_b, _ = _abi_weight(case, g, x, want_w=False, with_x=with_x)
        assert st == 0 and torch.equal(only_b, both_b) and bool(torch.isnan(no_w).all())
    untouched = lambda r: all(bool(torch.isnan(t).all()) for t in r[1:])  # noqa: E731
    for kw in (dict(want_w=False, want_b=False), dict(with_g=False), dict(with_x=False), dict(with_ws=False)):
        r = _abi_weight(case, g, x, **kw)
        assert r[0] == E_NULL and untouched(r), kw
    for kw in (dict(with_g=False), dict(with_w=False)):
        r = _abi_input(case, g, w, **kw)
        assert r[0] == E_NULL and untouched(r), kw
    assert _abi_input(case, g, w, with_out=False)[0] == E_NULL


@pytest.mark.parametrize("dims", [(0, 126, 33, 4, 8, 3, 3), (2, 0, 33, 4, 8, 3, 3), (2, 126, 0, 4, 8, 3, 3),
                                  (2, 126, 33, 0, 8, 3, 3), (2, 126, 33, 4, -8, 3, 3), (2, 126, 33, 4, 8, 2, 3),
                                  (2, 126, 33, 4, 8, 3, 4), (2, 126, 33, 4, 8, 9, 3), (2, 126, 33, 4, 8, 3, 0),
                                  (2, 65536, 33, 4, 8, 3, 3), (65536, 126, 33, 2048, 1, 3, 3)])
def test_abi_bad_shapes_return_e_shape(dims):
    case = cc.BY_NAME["3x3-c33-n126-2x4x8"]
    g, x, w = _dev(case)
    st, gx = _abi_input(case, g, w, dims=dims)
    assert st == E_SHAPE and bool(torch.isnan(gx).all())
    st, gw, gb, ws = _abi_weight(case, g, x, dims=dims)
    assert st == E_SHAPE
    assert bool(torch.isnan(gw).all()) and bool(torch.isnan(gb).all()) and bool(torch.isnan(ws).all())


# ----------------------------------------------------------------------------------------------------------
# torch.ops.oflow.conv2d_same / conv2d_same_backward
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PICK + ("5x1-c33-n33-2x7x6", "1x1-c33-n576-1x4x9"))
def test_forward_is_bit_identical_to_conv2d(name):
    case = cc.BY_NAME[name]
    _, x, w = _dev(case)
    kh, kw = w.shape[-2:]
    bias = cc.gaussian(7, (w.shape[0],)).to(DEV)
    for b in (bias, None):
        want = F.conv2d(x, w, b, padding=(kh // 2, kw // 2))
        with torch.no_grad():
            assert torch.equal(OPS.conv2d_same(x, w, b), want)
        got = OPS.conv2d_same(x.clone().requires_grad_(), w, b)  # under autograd
        assert got.requires_grad and torch.equal(got.detach(), want)


def _op_grads(case, gout=None, bias=True):
    g, x, w = _dev(case)
    x, w = x.requires_grad_(), w.requires_grad_()
    b = torch.zeros(w.shape[0], device=DEV, requires_grad=True) if bias else None
    OPS.conv2d_same(x, w, b).backward(g if gout is None else gout)
    return x.grad, w.grad, (b.grad if bias else None)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.CASE_IDS)
def test_autograd_matches_fp64(case):
    cc.assert_close(*_op_grads(case), case, "autograd")


def test_autograd_with_a_noncontiguous_and_an_expanded_grad_out():
    """grad_out as a cropped view of a larger tensor: the same bits as with its contiguous copy; and the stride-0
    expanded gradient ``.sum()`` hands over: within tolerance of float64 for an all-ones gradient."""
    case = cc.BY_NAME["1x5-c126-n33-5x1x13"]
    g = case.grad_out.to(DEV)
    wide = torch.full((g.shape[0], g.shape[1], g.shape[2] + 5, g.shape[3] + 3), NAN, device=DEV)
    view = wide[:, :, 2 : 2 + g.shape[2], 1 : 1 + g.shape[3]]
    view.copy_(g)
    assert not view.is_contiguous()
    plain, cropped = _op_grads(case), _op_grads(case, gout=view)
    assert all(torch.equal(a, b) for a, b in zip(plain, cropped))
    cc.assert_close(*cropped, case, "non-contiguous grad_out")
    _, x, w = _dev(case)
    x, w, b = x.requires_grad_(), w.requires_grad_(), torch.zeros(w.shape[0], device=DEV, requires_grad=True)
    OPS.conv2d_same(x, w, b).sum().backward()
    ones = cc.Case(case.name + "-ones", torch.ones_like(case.grad_out), case.x, case.weight)
    cc.assert_close(x.grad, w.grad, b.grad, ones, "expanded grad_out")


def test_autograd_forms_only_the_wanted_gradients():
    case = cc.BY_NAME["3x3-c33-n126-2x4x8"]
    g, x, w = _dev(case)
    xr = x.clone().requires_grad_()
    OPS.conv2d_same(xr, w, None).backward(g)
    cc.assert_close(xr.grad, None, None, case, "input only")
    wr = w.clone().requires_grad_()
    OPS.conv2d_same(x, wr, None).backward(g)  # convf1's situation: the input needs no gradient
    cc.assert_close(None, wr.grad, None, case, "weight only")
    br = torch.zeros(w.shape[0], device=DEV, requires_grad=True)
    OPS.conv2d_same(x, w, br).backward(g)
    cc.assert_close(None, None, br.grad, case, "bias only")
    full = OPS.conv2d_same_backward(g, x, w, [True, True, True])
    for need in ([True, False, False], [False, True, False], [False, False, True], [True, False, True], [False] * 3):
        got = OPS.conv2d_same_backward(g, x, w, need)
        for n, t, f in zip(need, got, full):
            assert t.numel() == (f.numel() if n else 0) and (not n or torch.equal(t, f))
    with pytest.raises(RuntimeError, match="grad_out"):
        OPS.conv2d_same_backward(g[..., :-1], x, w, [True, True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.conv2d_same_backward(g.cpu(), x, w, [True, True, True])
    with pytest.raises(RuntimeError, match="not supported"):
        OPS.conv2d_same(x, torch.zeros(4, 33, 2, 2, device=DEV), None)
    with pytest.raises(RuntimeError, match="not supported"):
        OPS.conv2d_same_backward(g, x, torch.zeros(126, 33, 9, 9, device=DEV), [True, True, True])
    empty = OPS.conv2d_same_backward(torch.zeros(0, 126, 4, 8, device=DEV), torch.zeros(0, 33, 4, 8, device=DEV), w, [True] * 3)
    assert tuple(empty[0].shape) == (0, 33, 4, 8) and not bool(empty[1].any()) and not bool(empty[2].any())


def test_backward_is_deterministic_on_dirty_memory():
    """No atomics and nothing left to the caller to zero: with the allocator's free blocks filled with NaN beforehand
    (the outputs and the slab workspace land in them), two runs give finite, bit-identical gradients."""
    g, x, w = _dev(cc.BY_NAME["3x3-c8-n8-3x41x37"])  # three slabs
    runs = []
    for _ in range(2):
        junk = [torch.full((1 << s,), NAN, device=DEV) for s in range(8, 22)]
        del junk
        runs.append([t.clone() for t in OPS.conv2d_same_backward(g, x, w, [True, True, True])])
        torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_compile_fullgraph_forward_and_backward():
    torch._dynamo.reset()
    g, x, w = _dev(cc.BY_NAME["3x3-c33-n126-2x4x8"])
    b = cc.gaussian(9, (w.shape[0],)).to(DEV)

    def loss(xx, ww, bb):
        return (torch.ops.oflow.conv2d_same(xx, ww, bb) * g).sum()

    grads = []
    for fn in (loss, torch.compile(loss, fullgraph=True, dynamic=False)):
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        value = fn(xr, wr, br)
        value.backward()
        grads.append((value.detach(), xr.grad, wr.grad, br.grad))
    torch.testing.assert_close(grads[1][0], grads[0][0], rtol=1e-5, atol=1e-9)
    assert all(torch.equal(a, b) for a, b in zip(grads[1][1:], grads[0][1:]))


# ----------------------------------------------------------------------------------------------------------
# RAFT
# ----------------------------------------------------------------------------------------------------------
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


def _graph_nodes(root, needle: str) -> int:
    """The number of autograd nodes reachable from ``root`` whose class name contains ``needle``."""
    seen, stack, count = set(), [root], 0
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        count += needle in type(node).__name__.lower()
        stack.extend(fn for fn, _ in node.next_functions)
    return count


def test_training_step_native_and_aten_convolution_backward_agree():
    """One 128 x 128, 3-iteration training step with ``conv_backward_impl`` "native" and "aten": the same loss bit for
    bit (the forward is the same kernel either way), every parameter gradient to a relative norm of 1e-3 (the bar of
    test_raft_training_gradients_match_oracle), the native graph holds one conv2d_same node per update-block
    convolution and iteration (15 x 3: motion encoder 5, SepConvGRU 6, flow head 2, mask head 2) and the ATen graph
    none.

    The biases in front of fnet's affine-free instance norms have an exactly zero gradient (see
    _biases_under_instance_norm): for those each path's bias-gradient norm is held to 1e-3 of the same convolution's
    weight-gradient norm instead of the 0 / 0 relative norm."""
    img0, img1 = (x.to(DEV) for x in synthetic.synthetic_pair(1, 128, 128, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (1, 2, 128, 128), 2.0)).to(DEV)
    valid = (torch.from_numpy(synthetic.hash_normal(32, (1, 128, 128), 1.0)) > -1.0).float().to(DEV)
    grads, losses, nodes = {}, {}, {}
    for impl in ("native", "aten"):
        model = _train_model()
        assert model.conv_backward_impl == "aten"  # the default
        model.conv_backward_impl = impl
        loss = model.training_step((img0, img1, target, valid), 0)
        nodes[impl] = _graph_nodes(loss.grad_fn, "conv2d_same")
        loss.backward()
        losses[impl] = loss.detach()
        grads[impl] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    n_convs = sum(isinstance(m, torch.nn.Conv2d) for m in model.update_block.modules())
    assert n_convs == 15 and nodes["native"] == n_convs * 3 and nodes["aten"] == 0, nodes
    assert torch.equal(losses["native"], losses["aten"])
    assert set(grads["native"]) == set(grads["aten"])
    block = {k for k in grads["aten"] if k.startswith("update_block.")}
    assert len(block) == 2 * n_convs
    null = _biases_under_instance_norm(model)
    assert null and null <= set(grads["aten"]) and all(k.startswith("fnet.") and k.endswith(".bias") for k in null)
    rels = {}
    for k, want in grads["aten"].items():
        got = grads["native"][k]
        if k in null:
            w = grads["aten"][k[: -len("bias")] + "weight"].norm()
            rels[k] = max(float(got.norm() / w), float(want.norm() / w))
        else:
            assert float(want.norm()) > 0, k
            rels[k] = float((got - want).norm() / want.norm())
    for k, rel in sorted(rels.items(), key=lambda t: -t[1])[:8]:
        print(f"training step: {k}: {rel:.2e}" + (" (zero gradient: norm / weight-gradient norm)" if k in null else ""))
    print(f"training step: worst update-block parameter: {max(rels[k] for k in block):.2e}; "
          f"{len(rels) - len(null)} parameters compared, {len(null)} with an exactly zero gradient")
    bad = {k: r for k, r in rels.items() if not r <= 1e-3}
    assert not bad, bad
    model.conv_backward_impl = "miopen"
    with pytest.raises(ValueError, match="conv_backward_impl"):
        model.training_step((img0, img1, target, valid), 0)
