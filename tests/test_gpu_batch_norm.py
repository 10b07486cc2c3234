"""Batch norm on batch statistics (csrc/batch_norm.hip), forward and backward, against float64: the C ABI with its
null-output, shape and workspace contracts, the operators under autograd (eager and torch.compile), the module parity of
``enc_norm_act`` (output, running statistics), then ``BasicEncoder("batch")`` in train mode and one RAFT training step
without ``freeze_bn()`` with ``batch_norm_impl = "native"``. Closed forms, inputs and tolerances:
tests/batch_norm_cases.py (checked and calibrated on the CPU by tests/test_batch_norm_host.py).

Tolerances: K * 2^-24 * bound per element, bound the closed form on absolute values plus the |mean| * r conditioning
term, K four times what ATen's own fp32 CPU computation needs (K_OUT for y, K_STAT for mean / var, K_GRAD for the
gradients).
"""
from __future__ import annotations

import copy
import ctypes

import pytest
import torch

import batch_norm_cases as bc
from model import RAFT, synthetic
from model import extractor as ext
from model.extractor import BasicEncoder
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -7
NAN = float("nan")
U = bc.U


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t, keep=True):
    return t.data_ptr() if keep and t is not None else None


def _dirty_allocator():
    """Fill the allocator's free blocks with NaN: later outputs and workspaces land in them."""
    junk = [torch.full((1 << s,), NAN, device=DEV) for s in range(8, 22)]
    del junk


def _nan(shape, offset=0):
    """A NaN-filled tensor of ``shape`` whose base pointer is ``offset`` floats past an aligned allocation."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n + offset,), NAN, device=DEV)[offset:].view(shape)


def _put(t, offset=0):
    out = _nan(tuple(t.shape), offset)
    out.copy_(t)
    return out


def _dev(case, offset=0):
    """(grad_out, x, weight, bias) on the device."""
    return _put(case.grad_out, offset), _put(case.x, offset), case.weight.to(DEV), case.bias.to(DEV)


def _ws(case):
    """The queried workspace, NaN-filled as what it holds: fp64 values (two floats each; a pair of fp32 NaNs read as
    one fp64 is a finite number, so the fill and the finiteness checks are made in float64)."""
    n = _native.load().oflow_batch_norm_workspace_floats(*case.dims)
    assert n == bc.workspace_floats(*case.dims) and n > 0 and n % 2 == 0
    return torch.full((n // 2,), NAN, device=DEV, dtype=torch.float64)


def _abi_forward(case, x, w, b, dims=None, eps=bc.EPS, want_y=True, with_x=True, with_w=True, with_b=True, with_mean=True,
                 with_var=True, with_ws=True, ws_shift=0, offset=0):
    """oflow_batch_norm_forward_f32 on NaN-filled outputs and workspace -> (status, y, mean, var, workspace)."""
    c = case.x.shape[1]
    y, mean, var, ws = _nan(tuple(case.x.shape), offset), _nan((c,)), _nan((c,)), _ws(case)
    ws_ptr = ws.data_ptr() + ws_shift if with_ws else None
    st = _native.load().oflow_batch_norm_forward_f32(_ptr(x, with_x), _ptr(w, with_w), _ptr(b, with_b), *(dims or case.dims),
                                                     eps, int(case.relu), _ptr(y, want_y), _ptr(mean, with_mean),
                                                     _ptr(var, with_var), ws_ptr, _stream())
    torch.cuda.synchronize()
    return st, y, mean, var, ws


def _abi_backward(case, g, x, w, b, mean, var, want=(True, True, True), dims=None, eps=bc.EPS, with_g=True, with_x=True,
                  with_w=True, with_b=True, with_mean=True, with_var=True, with_ws=True, ws_shift=0, offset=0):
    """oflow_batch_norm_backward_f32 on NaN-filled outputs and workspace -> (status, dx, dgamma, dbeta, workspace)."""
    c = case.x.shape[1]
    dx, dw, db, ws = _nan(tuple(case.x.shape), offset), _nan((c,)), _nan((c,)), _ws(case)
    ws_ptr = ws.data_ptr() + ws_shift if with_ws else None
    st = _native.load().oflow_batch_norm_backward_f32(
        _ptr(g, with_g), _ptr(x, with_x), _ptr(w, with_w), _ptr(b, with_b), _ptr(mean, with_mean), _ptr(var, with_var),
        *(dims or case.dims), eps, int(case.relu), _ptr(dx, want[0]), _ptr(dw, want[1]), _ptr(db, want[2]), ws_ptr, _stream())
    torch.cuda.synchronize()
    return st, dx, dw, db, ws


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


# ----------------------------------------------------------------------------------------------------------
# C ABI
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.BN_CASES, ids=bc.BN_IDS)
def test_abi_matches_fp64(case):
    """Every element of the six outputs is written (buffers and workspace start as NaN) and is within tolerance of
    float64; the whole queried workspace is written by the forward and again by the backward; the constant channel's
    variance is exactly 0 (its bound is)."""
    g, x, w, b = _dev(case)
    st, y, mean, var, ws = _abi_forward(case, x, w, b)
    assert st == 0 and bool(torch.isfinite(ws).all())
    st, dx, dw, db, ws = _abi_backward(case, g, x, w, b, mean, var)
    assert st == 0 and bool(torch.isfinite(ws).all())
    bc.assert_close((y, mean, var, dx, dw, db), case, "C ABI")


def test_workspace_query_equals_the_formula():
    lib = _native.load()
    assert lib.oflow_batch_norm_chunk_elements() == bc.CHUNK
    for dims in [c.dims for c in bc.BN_CASES] + [(8, 64, 184 * 248), (8, 96, 92 * 124), (8, 128, 46 * 62), (1, 1, bc.CHUNK),
                                                  (1, 1, bc.CHUNK + 1)]:
        assert lib.oflow_batch_norm_workspace_floats(*dims) == bc.workspace_floats(*dims)


@pytest.mark.parametrize("name", ["2x2x7x9-relu", "3x3x5x7", bc.TWO_CHUNKS])
def test_abi_unaligned_base_pointers(name):
    """x, grad_out, y and dx four bytes past a 16-byte boundary: everything moves as scalars, within tolerance."""
    case = bc.BN_BY_NAME[name]
    g, x, w, b = _dev(case, offset=1)
    assert x.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4
    st, y, mean, var, _ = _abi_forward(case, x, w, b, offset=1)
    assert st == 0 and y.data_ptr() % 16 == 4
    st, dx, dw, db, _ = _abi_backward(case, g, x, w, b, mean, var, offset=1)
    assert st == 0
    bc.assert_close((y, mean, var, dx, dw, db), case, "unaligned")


def test_abi_requested_outputs_equal_the_full_run():
    """Each combination of requested backward outputs equals the full run bit for bit and leaves the others NaN; the
    forward without y (statistics only, no parameters needed) gives the full run's statistics."""
    for name in ("3x3x5x7-relu", bc.TWO_CHUNKS):
        case = bc.BN_BY_NAME[name]
        g, x, w, b = _dev(case)
        st, y, mean, var, _ = _abi_forward(case, x, w, b)
        assert st == 0
        st, y2, mean2, var2, ws = _abi_forward(case, x, None, None, want_y=False)
        assert st == 0 and _all_nan(y2) and torch.equal(mean2, mean) and torch.equal(var2, var)
        assert bool(torch.isfinite(ws).all())
        st, *full = _abi_backward(case, g, x, w, b, mean, var)
        assert st == 0
        for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            st, *got = _abi_backward(case, g, x, w, b, mean, var, want=want)
            assert st == 0 and bool(torch.isfinite(got[3]).all())
            for n, t, f in zip(want, got[:3], full[:3]):
                assert torch.equal(t, f) if n else _all_nan(t), (name, want)


def test_abi_null_pointer_shape_and_alignment_contracts():
    case = bc.BN_BY_NAME["3x3x5x7-relu"]
    g, x, w, b = _dev(case)
    st, _, mean, var, _ = _abi_forward(case, x, w, b)
    assert st == 0
    B, C, HW = case.dims
    for kw in ({"with_x": False}, {"with_w": False}, {"with_b": False}, {"with_mean": False}, {"with_var": False},
               {"with_ws": False}):
        st, *outs = _abi_forward(case, x, w, b, **kw)
        assert st == E_NULL and _all_nan(*outs), kw
    for kw in ({"with_g": False}, {"with_x": False}, {"with_w": False}, {"with_b": False}, {"with_mean": False},
               {"with_var": False}, {"with_ws": False}, {"want": (0, 0, 0)}):
        st, *outs = _abi_backward(case, g, x, w, b, mean, var, **kw)
        assert st == E_NULL and _all_nan(*outs), kw
    bad = [{"dims": (0, C, HW)}, {"dims": (B, 0, HW)}, {"dims": (B, C, 0)}, {"dims": (-1, C, HW)}, {"eps": -1e-5},
           {"eps": NAN}, {"dims": (65536, 65536, 1)}]  # (the last: 2^32 planes, past the grid range)
    for kw in bad:
        st, *outs = _abi_forward(case, x, w, b, **kw)
        assert st == E_SHAPE and _all_nan(*outs), kw
        st, *outs = _abi_backward(case, g, x, w, b, mean, var, **kw)
        assert st == E_SHAPE and _all_nan(*outs), kw
    st, *outs = _abi_forward(case, x, w, b, ws_shift=4)  # the fp64 partials need an 8-byte aligned workspace
    assert st == E_ALIGN and _all_nan(*outs)
    st, *outs = _abi_backward(case, g, x, w, b, mean, var, ws_shift=4)
    assert st == E_ALIGN and _all_nan(*outs)
    assert _native.load().oflow_batch_norm_workspace_floats(65536, 65536, 1) == 0


# ----------------------------------------------------------------------------------------------------------
# operators
# ----------------------------------------------------------------------------------------------------------
def _op_run(case, gout=None):
    g, x, w, b = _dev(case)
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
    y, mean, var = OPS.batch_norm_act(xr, wr, br, bc.EPS, case.relu)
    assert y.requires_grad and not mean.requires_grad and not var.requires_grad
    y.backward(g if gout is None else gout)
    return y.detach(), mean, var, xr.grad, wr.grad, br.grad


@pytest.mark.parametrize("case", bc.BN_CASES, ids=bc.BN_IDS)
def test_op_forward_and_autograd_match_fp64(case):
    got = _op_run(case)
    bc.assert_close(got, case, "autograd")
    with torch.no_grad():
        g, x, w, b = _dev(case)
        plain = OPS.batch_norm_act(x, w, b, bc.EPS, case.relu)
    assert all(torch.equal(a, p) for a, p in zip(got[:3], plain))  # the same forward with and without autograd


def test_op_mask_of_a_negative_scale_channel():
    """Channel 0 has gamma < 0: the kept elements are those with x below the mean. The mask the forward applied (y > 0)
    is float64's, and dbeta, the sum of grad_out over it, follows."""
    case = bc.BN_BY_NAME["2x64x12x20-relu"]
    y, _, _, _, _, db = _op_run(case)
    pre = bc.output64(case)
    assert torch.equal(y.cpu() > 0, pre > 0)
    x64 = case.x.double()
    assert torch.equal(pre[:, 0] > 0, (x64[:, 0] - x64[:, 0].mean()) * float(case.weight[0]) > -float(case.bias[0])
                       * torch.sqrt(x64[:, 0].var(unbiased=False) + bc.EPS))
    want = (case.grad_out.double()[:, 0] * (pre[:, 0] > 0)).sum()
    assert abs(float(db[0]) - float(want)) <= float(bc.reference(case)[1][5][0])


def test_op_grad_out_views_masks_empty_batches_refusals_and_meta():
    case = bc.BN_BY_NAME["3x3x5x7-relu"]
    g, x, w, b = _dev(case)
    plain = _op_run(case)
    wide = torch.full((3, 3, 9, 10), NAN, device=DEV)
    view = wide[:, :, 2:7, 1:8]
    view.copy_(g)
    assert not view.is_contiguous()
    assert all(torch.equal(a, p) for a, p in zip(_op_run(case, gout=view), plain))
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
    OPS.batch_norm_act(xr, wr, br, bc.EPS, True)[0].sum().backward()  # a stride-0 expanded gradient
    ones = case._replace(name=case.name + "-ones", grad_out=torch.ones_like(case.grad_out))
    bc.assert_close((None, None, None, xr.grad, wr.grad, br.grad), ones, "expanded grad_out")
    _, mean, var = plain[:3]
    full = OPS.batch_norm_act_backward(g, x, w, b, mean, var, bc.EPS, True, [True] * 3)
    assert all(torch.equal(a, p) for a, p in zip(full, plain[3:]))
    for need in ([True, False, False], [False, True, False], [False, False, True], [False, True, True], [False] * 3):
        got = OPS.batch_norm_act_backward(g, x, w, b, mean, var, bc.EPS, True, need)
        for n, t, f in zip(need, got, full):
            assert t.numel() == (f.numel() if n else 0) and (not n or torch.equal(t, f))
    wr = w.clone().requires_grad_()  # only the scale needs a gradient
    OPS.batch_norm_act(x, wr, b, bc.EPS, True)[0].backward(g)
    assert torch.equal(wr.grad, full[1])
    e = torch.zeros(0, 3, 5, 7, device=DEV)
    ey, em, ev = OPS.batch_norm_act(e, w, b, bc.EPS, True)
    assert tuple(ey.shape) == (0, 3, 5, 7) and tuple(em.shape) == (3,) and not bool(em.any()) and not bool(ev.any())
    got = OPS.batch_norm_act_backward(e, e, w, b, em, ev, bc.EPS, True, [True] * 3)
    assert tuple(got[0].shape) == (0, 3, 5, 7) and not bool(got[1].any()) and not bool(got[2].any())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.batch_norm_act(x.cpu(), w, b, bc.EPS, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.batch_norm_act_backward(g.cpu(), x, w, b, mean, var, bc.EPS, True, [True] * 3)
    with pytest.raises(RuntimeError, match="grad_out"):
        OPS.batch_norm_act_backward(g[..., :-1], x, w, b, mean, var, bc.EPS, True, [True] * 3)
    with pytest.raises(RuntimeError, match="bias"):
        OPS.batch_norm_act(x, w, b[:-1], bc.EPS, True)
    with pytest.raises(RuntimeError, match="var"):
        OPS.batch_norm_act_backward(g, x, w, b, mean, var[:-1], bc.EPS, True, [True] * 3)
    with pytest.raises(RuntimeError, match="float32"):
        OPS.batch_norm_act(x.double(), w, b, bc.EPS, True)
    xm, pm = x.to("meta"), w.to("meta")
    assert [tuple(t.shape) for t in OPS.batch_norm_act(xm, pm, pm, bc.EPS, True)] == [tuple(x.shape), (3,), (3,)]
    assert [tuple(t.shape) for t in OPS.batch_norm_act_backward(xm, xm, pm, pm, pm, pm, bc.EPS, True, [True, False, True])] == [
        tuple(x.shape), (0,), (3,)]


def test_forward_and_backward_are_deterministic_on_dirty_memory():
    """No atomics and nothing left to the caller to zero: with the allocator's free blocks filled with NaN beforehand
    (outputs and workspaces land in them), two runs give finite, bit-identical results."""
    for name in ("2x64x12x20-relu", bc.TWO_CHUNKS):
        case = bc.BN_BY_NAME[name]
        g, x, w, b = _dev(case)
        runs = []
        for _ in range(2):
            _dirty_allocator()
            y, mean, var = (t.clone() for t in OPS.batch_norm_act(x, w, b, bc.EPS, True))
            _dirty_allocator()
            grads = [t.clone() for t in OPS.batch_norm_act_backward(g, x, w, b, mean, var, bc.EPS, True, [True] * 3)]
            torch.cuda.synchronize()
            runs.append([y, mean, var] + grads)
        assert all(bool(torch.isfinite(t).all()) for t in runs[0])
        assert all(torch.equal(a, b_) for a, b_ in zip(*runs))


def test_compile_fullgraph_forward_and_backward():
    import encoder_backward_cases as ec

    torch._dynamo.reset()
    conv = ec.CONV_BY_NAME["3x3-c33-n126-3x5x7-s2"]
    x, w = conv.x.to(DEV), conv.weight.to(DEV)
    b = ec.gaussian(9, (w.shape[0],)).to(DEV)
    gamma = (1 + 0.2 * ec.gaussian(10, (w.shape[0],))).to(DEV)
    beta = (0.1 * ec.gaussian(11, (w.shape[0],))).to(DEV)
    gi = ec.gaussian(12, tuple(conv.grad_out.shape), ec.GRAD_SIGMA).to(DEV)

    def loss(xx, ww, bb, ga, be):
        y, mean, var = torch.ops.oflow.batch_norm_act(torch.ops.oflow.conv2d_strided(xx, ww, bb, 2), ga, be, bc.EPS, True)
        return (y * gi).sum()

    grads = []
    for fn in (loss, torch.compile(loss, fullgraph=True, dynamic=False)):
        leaves = [t.clone().requires_grad_() for t in (x, w, b, gamma, beta)]
        value = fn(*leaves)
        value.backward()
        grads.append((value.detach(),) + tuple(t.grad for t in leaves))
    torch.testing.assert_close(grads[1][0], grads[0][0], rtol=1e-5, atol=1e-9)
    assert all(torch.equal(a, b_) for a, b_ in zip(grads[1][1:], grads[0][1:]))


# ----------------------------------------------------------------------------------------------------------
# module parity
# ----------------------------------------------------------------------------------------------------------
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


def _module(case, momentum=0.1):
    c = case.x.shape[1]
    m = torch.nn.BatchNorm2d(c, eps=bc.EPS, momentum=momentum).to(DEV).train()
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        m.weight.copy_(case.weight)
        m.bias.copy_(case.bias)
        m.running_mean.copy_(0.3 * torch.randn(c, generator=gen))
        m.running_var.copy_(0.5 + torch.rand(c, generator=gen))
        m.num_batches_tracked.fill_(5)
    return m


@pytest.mark.parametrize("name", ["3x3x5x7-relu", "2x64x12x20", "2x1x46x62-offset-relu"])
def test_enc_norm_act_matches_the_module_and_updates_its_buffers(name):
    """nn.BatchNorm2d in train mode beside enc_norm_act with the switch native: output and gradients against float64,
    running_mean / running_var within the statistics tolerance of the float64 update (the batch statistic's tolerance
    scaled by the momentum, plus three fp32 roundings of the update itself), num_batches_tracked equal."""
    case = bc.BN_BY_NAME[name]
    g, x, _, _ = _dev(case)
    mod, ref_mod = _module(case, 0.25), _module(case, 0.25)
    old = (mod.running_mean.double().cpu(), mod.running_var.double().cpu(), 5)
    xr = x.clone().requires_grad_()
    y = ext.enc_norm_act(mod, xr, case.relu, "aten", "native")
    assert _graph_nodes(y.grad_fn, "norm_act") == 1 and _graph_nodes(y.grad_fn, "batchnorm") == 0
    y.backward(g)
    bc.assert_close((y.detach(), None, None, xr.grad, mod.weight.grad, mod.bias.grad), case, "enc_norm_act")
    want = ref_mod(x)
    want = torch.relu(want) if case.relu else want
    # (the module's own output is printed, not asserted: on the offset case MIOpen's is 82 tolerances from float64)
    print(f"{name}: the module's y, worst err / (U * bound) = {bc.error_ratios((want.detach(),) + (None,) * 5, case)[0]:.2f}"
          f" (K_OUT = {bc.K_OUT})")
    refs, tols, _ = bc.reference(case)
    n, m = case.x.numel() // case.x.shape[1], 0.25
    rm, rv, tracked = bc.updated_buffers(*old, refs[1], refs[2], n, m)
    tol_m = m * tols[1] + 3 * U * ((1 - m) * old[0].abs() + m * refs[1].abs())
    tol_v = m * n / (n - 1) * tols[2] + 3 * U * rv.abs()
    for what, got, ref, tol in (("running_mean", mod.running_mean, rm, tol_m), ("running_var", mod.running_var, rv, tol_v)):
        err = (got.double().cpu() - ref).abs()
        print(f"{name} {what}: worst err / tol = {float((err / tol).max()):.3f}; the module's: "
              f"{float(((getattr(ref_mod, what).double().cpu() - ref).abs() / tol).max()):.3f}")
        assert bool((err <= tol).all()), what
    assert int(mod.num_batches_tracked) == int(ref_mod.num_batches_tracked) == tracked == 6


def test_enc_norm_act_leaves_ineligible_layers_to_the_module():
    """momentum=None (a cumulative average), eval mode, no-grad, buffers that are not fp32 and a single value per channel
    call the module; the last raises the module's own error."""
    case = bc.BN_BY_NAME["3x3x5x7-relu"]
    _, x, _, _ = _dev(case)
    xr = x.clone().requires_grad_()
    cum = _module(case, None)
    twin = copy.deepcopy(cum)
    y = ext.enc_norm_act(cum, xr, True, "aten", "native")
    assert _graph_nodes(y.grad_fn, "norm_act") == 0 and _graph_nodes(y.grad_fn, "batchnorm") == 1
    assert torch.equal(y, torch.relu(twin(x)))
    assert all(torch.equal(a, b) for a, b in zip(cum.buffers(), twin.buffers()))
    ev = _module(case).eval()
    y = ext.enc_norm_act(ev, xr, True, "aten", "native")
    assert _graph_nodes(y.grad_fn, "norm_act") == 0 and int(ev.num_batches_tracked) == 5
    y = ext.enc_norm_act(ev, xr, True, "native", "native")  # eval mode stays the frozen op's
    assert _graph_nodes(y.grad_fn, "norm_act") == 1 and "frozen" in type(y.grad_fn).__name__.lower()
    tr = _module(case)
    with torch.no_grad():
        y = ext.enc_norm_act(tr, x, True, "aten", "native")
    assert y.grad_fn is None and int(tr.num_batches_tracked) == 6
    odd = _module(case)  # fp32 parameters, float64 buffers: not this op's to update
    odd.running_mean, odd.running_var = odd.running_mean.double(), odd.running_var.double()
    twin = copy.deepcopy(odd)
    try:
        want, err = torch.relu(twin(x)), None
    except Exception as e:  # (whatever the module makes of it is what comes back)
        want, err = None, type(e)
    if err is None:
        y = ext.enc_norm_act(odd, xr, True, "aten", "native")
        assert _graph_nodes(y.grad_fn, "norm_act") == 0 and torch.equal(y, want)
        assert all(torch.equal(a, b) for a, b in zip(odd.buffers(), twin.buffers()))
    else:
        with pytest.raises(err):
            ext.enc_norm_act(odd, xr, True, "aten", "native")
    twin = copy.deepcopy(tr)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ext.enc_norm_act(tr, xr[:1, :, :1, :1], True, "aten", "native")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        twin(xr[:1, :, :1, :1])
    assert all(torch.equal(a, b) for a, b in zip(tr.buffers(), twin.buffers()))  # (the module counts the call it refuses)


# ----------------------------------------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------------------------------------
def _zero_grad_biases(model):
    """Names of the convolution biases whose output goes straight into a norm layer that subtracts a per-channel mean
    of its own input (an InstanceNorm2d without affine parameters, a BatchNorm2d in train mode): dL/dbias is exactly 0
    and what autograd returns is rounding noise (tests/test_gpu_encoder_backward.py::_biases_under_instance_norm)."""
    plain = lambda n: ((isinstance(n, torch.nn.InstanceNorm2d) and not n.affine)  # noqa: E731
                       or (isinstance(n, torch.nn.BatchNorm2d) and n.training))
    names = set()
    for prefix, mod in model.named_modules():
        dot = prefix + "." if prefix else ""
        for conv, norm in (("conv1", "norm1"), ("conv2", "norm2")):
            c = getattr(mod, conv, None)
            if isinstance(c, torch.nn.Conv2d) and c.bias is not None and plain(getattr(mod, norm, None)):
                names.add(f"{dot}{conv}.bias")
        ds = getattr(mod, "downsample", None)
        if isinstance(ds, torch.nn.Sequential) and len(ds) == 2 and isinstance(ds[0], torch.nn.Conv2d) and plain(ds[1]):
            names.add(f"{dot}downsample.0.bias")
    return names


def _compare_grads(got, want, null, what):
    """Every gradient of ``got`` within a relative norm of 1e-3 of ``want``'s; for the exactly-zero ones (``null``) each
    side's norm within 1e-3 of the same convolution's weight-gradient norm (the existing encoder test's rule)."""
    assert set(got) == set(want)
    rels = {}
    for k, w in want.items():
        if k in null:
            wn = want[k[: -len("bias")] + "weight"].norm()
            rels[k] = max(float(got[k].norm() / wn), float(w.norm() / wn))
        else:
            assert float(w.norm()) > 0, k
            rels[k] = float((got[k] - w).norm() / w.norm())
    for k, rel in sorted(rels.items(), key=lambda t: -t[1])[:6]:
        print(f"{what}: {k}: {rel:.2e}" + (" (zero gradient: norm / weight-gradient norm)" if k in null else ""))
    bad = {k: r for k, r in rels.items() if not r <= 1e-3}
    assert not bad, (what, bad)


def _encoder():
    torch.manual_seed(11)
    enc = BasicEncoder(output_dim=64, norm_fn="batch")
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for m in enc.modules():  # non-trivial statistics and affine parameters
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
                m.weight.copy_(1 + 0.2 * torch.randn(n, generator=gen))
                m.bias.copy_(0.1 * torch.randn(n, generator=gen))
    return enc.train()


def _bn_layers(enc):
    """The 15 BatchNorm2d layers in forward order (a stride-2 block's projection norm after its norm2)."""
    out = [("norm1", enc.norm1)]
    for li, layer in enumerate((enc.layer1, enc.layer2, enc.layer3), 1):
        for bi, blk in enumerate(layer):
            out += [(f"layer{li}.{bi}.norm1", blk.norm1), (f"layer{li}.{bi}.norm2", blk.norm2)]
            if blk.downsample is not None:
                out.append((f"layer{li}.{bi}.norm3", blk.norm3))
    return out


def _encoder_run(enc, enc_impl, bn_impl, x, gout):
    enc.encoder_backward_impl, enc.batch_norm_impl = enc_impl, bn_impl
    enc.zero_grad(set_to_none=True)
    before = {k: v.clone() for k, v in enc.named_buffers()}
    out = enc(x)
    nodes = {n: _graph_nodes(out.grad_fn, n) for n in ("conv2d_strided", "norm_act", "convolution", "batchnorm")}
    out.backward(gout)
    after = {k: v.clone() for k, v in enc.named_buffers()}
    with torch.no_grad():  # (the running statistics moved: put them back for the next run)
        for k, v in enc.named_buffers():
            v.copy_(before[k])
    return out.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}, nodes, after


def _buffer_bounds(mod, t):
    """The statistics bounds (tests/batch_norm_cases.py: mean, var) of a batch norm's float64 input ``t``, carried through
    the buffer update: (1 - m) |old| + m * bound, with n / (n - 1) on the variance's -> (running_mean, running_var)."""
    t = t.double()
    n = t.numel() // t.shape[1]
    mean = t.mean(dim=(0, 2, 3))
    dev = (t - mean.view(1, -1, 1, 1)).abs().mean(dim=(0, 2, 3))
    var = t.var(dim=(0, 2, 3), unbiased=False)
    m = mod.momentum
    return ((1 - m) * mod.running_mean.double().abs() + m * t.abs().mean(dim=(0, 2, 3)),
            (1 - m) * mod.running_var.double().abs() + m * n / (n - 1) * (var + 2 * mean.abs() * dev))


def test_encoder_in_train_mode_native_against_default():
    """``BasicEncoder("batch")`` in train mode on 2 x 3 x 40 x 56 with a fixed output gradient, both switches native
    against all-default, under ``cudnn.flags(deterministic=True)`` (the reason:
    tests/test_gpu_encoder_backward.py::test_encoder_native_backward_matches_aten).

    The native forward is not ATen's bit for bit, so the outputs are judged against a float64 CPU run of the same
    module: the native run's relative error norm is at most four times the default GPU run's.

    Buffers, the statistics tolerance being K_STAT * 2^-24 * bound with the bound of the layer's input carried through
    the update formula (momentum; n / (n - 1) for the variance; plus the old value, whose update is rounded too):
    (1) Every one of the 15 layers is given the input it had in the default run through both paths (the module, and
    ``enc_norm_act`` with the switch native, on copies of the layer): the two sets of buffers agree within that
    tolerance, ratio <= 1 (measured 0.15 to 0.42 on running_mean, 0.24 to 0.33 on running_var).
    (2) After one whole run of each encoder the buffers are compared as well. There layer k (k = 1 .. 15 in forward
    order) sees an input that already carries the rounding of the k - 1 conv + norm stages before it, which differs
    between the two runs, so this comparison does not meet ratio <= 1 everywhere: measured, running_mean of layer 11
    (layer3.0.norm1) is at 1.53, every other buffer at 0.15 to 0.98 (running_var at most 0.67). Each run's distance from the
    float64 run's buffers is printed beside it (layer 11: native 1.15, default 0.96; layer 12: native 0.73, default 1.17). The whole-run comparison is asserted at k times the tolerance (each stage
    adds an error of the order of its own tolerance); that is the looser bound, (1) is the one the layer is held to."""
    enc = _encoder()
    x = bc.gaussian(21, (2, 3, 40, 56))
    gout = bc.gaussian(22, (2, 64, 5, 7), bc.GRAD_SIGMA)
    # float64 on the CPU, with each batch norm's input statistics bounds recorded
    ref = copy.deepcopy(enc).double()
    bounds = {}
    for name, mod in _bn_layers(ref):
        mod.register_forward_pre_hook(lambda m, args, name=name: bounds.__setitem__(name, _buffer_bounds(m, args[0])))
    with torch.no_grad():
        out64 = ref(x.double())
    assert len(bounds) == 15
    ref64 = {k: v.clone() for k, v in ref.named_buffers()}  # the float64 run's buffers after its one call
    enc = enc.to(DEV)
    x, gout = x.to(DEV), gout.to(DEV)
    inputs = {}  # each batch norm's input in the default run (the modules are called there)
    hooks = [mod.register_forward_pre_hook(lambda m, args, name=name: inputs.__setitem__(name, args[0].detach().clone()))
             for name, mod in _bn_layers(enc)]
    with torch.backends.cudnn.flags(deterministic=True):
        out_a, grads_a, nodes_a, buf_a = _encoder_run(enc, "aten", "aten", x, gout)
        for h in hooks:
            h.remove()
        assert len(inputs) == 15
        # the same recorded input through both paths of every layer: the buffers agree within the statistics tolerance
        for depth, (name, mod) in enumerate(_bn_layers(enc), 1):
            relu = not name.endswith("norm3")
            by_module, by_op = copy.deepcopy(mod), copy.deepcopy(mod)
            want = by_module(inputs[name])
            got = ext.enc_norm_act(by_op, inputs[name].clone().requires_grad_(), relu, "aten", "native")
            assert _graph_nodes(got.grad_fn, "norm_act") == 1
            same = float((got - (torch.relu(want) if relu else want)).norm() / want.norm())
            for key, bd in zip(("running_mean", "running_var"), _buffer_bounds(mod, inputs[name])):
                ratio = float(((getattr(by_module, key).double() - getattr(by_op, key).double()).abs()
                               / (bc.K_STAT * U * bd)).max())
                print(f"same input: {name}.{key} (layer {depth}): |native - default| / (K_STAT U bound) = {ratio:.3f}")
                assert ratio <= 1, (name, key, ratio)
            assert torch.equal(by_module.num_batches_tracked, by_op.num_batches_tracked)
            assert same <= 1e-5, (name, same)
        out_n, grads_n, nodes_n, buf_n = _encoder_run(enc, "native", "native", x, gout)
        _dirty_allocator()
        out_n2, grads_n2, _, buf_n2 = _encoder_run(enc, "native", "native", x, gout)
        out_b, grads_b, nodes_b, buf_b = _encoder_run(enc, "aten", "native", x, gout)
    print("graph nodes:", nodes_a, nodes_n, nodes_b)
    assert nodes_a == {"conv2d_strided": 0, "norm_act": 0, "convolution": 16, "batchnorm": 15}, nodes_a
    assert nodes_n == {"conv2d_strided": 16, "norm_act": 15, "convolution": 0, "batchnorm": 0}, nodes_n
    assert nodes_b == {"conv2d_strided": 0, "norm_act": 15, "convolution": 16, "batchnorm": 0}, nodes_b
    rel = lambda t: float((t.double().cpu() - out64).norm() / out64.norm())  # noqa: E731
    print(f"forward relative error norm against float64: native {rel(out_n):.3e}, default {rel(out_a):.3e}, "
          f"batch_norm_impl alone {rel(out_b):.3e}")
    assert rel(out_n) <= 4 * rel(out_a) and rel(out_b) <= 4 * rel(out_a)
    null = _zero_grad_biases(enc)
    assert len(null) == 15
    _compare_grads(grads_n, grads_a, null, "encoder, both switches native")
    _compare_grads(grads_b, grads_a, null, "encoder, batch_norm_impl alone")
    assert torch.equal(out_n2, out_n) and all(torch.equal(grads_n[k], grads_n2[k]) for k in grads_n)
    assert all(torch.equal(buf_n[k], buf_n2[k]) for k in buf_n)
    assert all(bool(torch.isfinite(v).all()) for v in grads_n.values())
    worst = 0.0
    for depth, (name, _) in enumerate(_bn_layers(enc), 1):
        for key, bd in zip(("running_mean", "running_var"), bounds[name]):
            a, n_ = buf_a[f"{name}.{key}"].double().cpu(), buf_n[f"{name}.{key}"].double().cpu()
            ratio = float(((a - n_).abs() / (bc.K_STAT * U * bd)).max())
            worst = max(worst, ratio / depth)
            r64 = ref64[f"{name}.{key}"]
            print(f"buffers: {name}.{key} (layer {depth}): |native - default| / (K_STAT U bound) = {ratio:.3f}; against the "
                  f"float64 run: native {float(((n_ - r64).abs() / (bc.K_STAT * U * bd)).max()):.3f}, default "
                  f"{float(((a - r64).abs() / (bc.K_STAT * U * bd)).max()):.3f}")
            assert ratio <= depth, (name, key, ratio)
        assert torch.equal(buf_a[f"{name}.num_batches_tracked"], buf_n[f"{name}.num_batches_tracked"])
        assert int(buf_n[f"{name}.num_batches_tracked"]) == 1
    print(f"buffers: worst ratio / depth = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------
# RAFT
# ----------------------------------------------------------------------------------------------------------
def _train_model():
    m = RAFT(iters=3)
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    return m.to(DEV).train()  # no freeze_bn(): cnet normalises with batch statistics (the Chairs stage)


def test_training_step_without_freeze_bn_all_native():
    """One 128 x 128, 3-iteration training step with synthetic weights and cnet's batch norm in train mode: (a) defaults,
    (c) all three switches native, (c2) the same again on dirty memory. (c) holds no ATen convolution or batch-norm node
    and 30 native norm nodes (fnet's 15 instance norms, cnet's 15 batch norms); its gradients match (a)'s to 1e-3, the 30
    biases in front of a mean-subtracting norm by the zero-gradient rule; (c) and (c2) agree bit for bit. The native
    forward is not ATen's bit for bit, so the losses are not required to be equal: their relative difference is printed
    (the forward is judged against float64 at the encoder level, test_encoder_in_train_mode_native_against_default).
    Under ``cudnn.flags(deterministic=True)`` for the forward's convolutions, as the existing step test."""
    img0, img1 = (x.to(DEV) for x in synthetic.synthetic_pair(1, 128, 128, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (1, 2, 128, 128), 2.0)).to(DEV)
    valid = (torch.from_numpy(synthetic.hash_normal(32, (1, 128, 128), 1.0)) > -1.0).float().to(DEV)
    settings = {"a": "aten", "c": "native", "c2": "native"}
    grads, losses, nodes, buffers = {}, {}, {}, {}
    for tag, impl in settings.items():
        model = _train_model()
        assert model.batch_norm_impl == "aten"  # the default
        model.encoder_backward_impl = model.conv_backward_impl = model.batch_norm_impl = impl
        if tag == "c2":
            _dirty_allocator()
        with torch.backends.cudnn.flags(deterministic=True):
            loss = model.training_step((img0, img1, target, valid), 0)
            nodes[tag] = {n: _graph_nodes(loss.grad_fn, n)
                          for n in ("conv2d_strided", "norm_act", "conv2d_same", "convolution", "batchnorm")}
            loss.backward()
        losses[tag] = loss.detach()
        grads[tag] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        buffers[tag] = {k: v.clone() for k, v in model.named_buffers()}
    print("graph nodes:", nodes)
    assert nodes["a"]["norm_act"] == 0 and nodes["a"]["batchnorm"] >= 15 and nodes["a"]["convolution"] > 0
    assert nodes["c"]["convolution"] == 0 and nodes["c"]["batchnorm"] == 0, nodes["c"]
    assert nodes["c"]["norm_act"] == 30 and nodes["c"]["conv2d_strided"] == 32 and nodes["c"]["conv2d_same"] == 45
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    print(f"loss: default {float(losses['a']):.9g}, native {float(losses['c']):.9g}, relative difference "
          f"{abs(float(losses['c']) - float(losses['a'])) / abs(float(losses['a'])):.3e}")
    null = _zero_grad_biases(model)
    assert len(null) == 30 and sum(k.startswith("cnet.") for k in null) == 15
    _compare_grads(grads["c"], grads["a"], null, "training step, all native")
    differ = [k for k in grads["c"] if not torch.equal(grads["c"][k], grads["c2"][k])]
    assert not differ and torch.equal(losses["c"], losses["c2"]), differ
    assert all(torch.equal(buffers["c"][k], buffers["c2"][k]) for k in buffers["c"])
    tracked = [k for k in buffers["c"] if k.startswith("cnet.") and k.endswith("num_batches_tracked")]
    assert len(tracked) == 15 and all(torch.equal(buffers["c"][k], buffers["a"][k]) for k in tracked)
    model.batch_norm_impl = "miopen"
    with pytest.raises(ValueError, match="batch_norm_impl"):
        model.training_step((img0, img1, target, valid), 0)
