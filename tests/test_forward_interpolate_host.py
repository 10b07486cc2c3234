"""forward_interpolate without a GPU: the CPU path of model.utils.forward_interpolate against the float64 brute-force
reference (tests/forward_interpolate_cases.py), exactly; the reference against scipy's griddata(method="nearest"), what
upstream RAFT's forward_interpolate calls, where scipy is installed; the operator's Meta kernel and argument checks."""
import numpy as np
import pytest
import torch

import forward_interpolate_cases as fic
from model import forward_interpolate
from optical_flow import _native

RANDOM_IDS = [c.name for c in fic.CASES if c.random and c.flow.shape[0] == 1 and c.name.startswith("rand-")]


def test_case_table_is_what_it_claims():
    # the properties the cases were chosen for (counted, not assumed)
    assert fic.landed_count(fic.BY_NAME["rand-17x33-s40-5"].flow[0]) == 23
    assert fic.tie_count(fic.BY_NAME["tie-9x13"].flow[0]) == 13
    assert fic.landed_count(fic.BY_NAME["none-landed"].flow[0]) == 0
    assert fic.landed_count(fic.BY_NAME["one-landed"].flow[0]) == 1
    assert fic.landed_count(fic.BY_NAME["row-1x37"].flow[0]) >= 10 and fic.landed_count(fic.BY_NAME["col-29x1"].flow[0]) >= 10
    for c in fic.CASES:
        assert c.flow.dtype == np.float32 and c.flow.ndim == 4 and c.flow.shape[1] == 2, c.name


@pytest.mark.parametrize("name", fic.CASE_IDS)
def test_cpu_path_equals_reference_exactly(name):
    case = fic.BY_NAME[name]
    ref = fic.expected(case)  # (asserts the gap bound of a random case)
    flow = torch.from_numpy(case.flow)
    out = forward_interpolate(flow)
    assert out.shape == flow.shape and out.dtype == torch.float32 and out.device == flow.device
    assert np.array_equal(out.numpy(), ref, equal_nan=False), name
    # upstream's (2, H, W) signature, image by image
    for i in range(min(flow.shape[0], 2)):
        one = forward_interpolate(flow[i])
        assert one.shape == flow.shape[1:] and np.array_equal(one.numpy(), ref[i]), (name, i)


def test_edge_case_outputs():
    exp = {n: fic.expected(fic.BY_NAME[n]) for n in ("none-landed", "one-landed", "constant", "zero-flow")}
    assert not exp["none-landed"].any()
    assert (exp["one-landed"][0, 0] == 0.25).all() and (exp["one-landed"][0, 1] == -0.5).all()
    assert (exp["constant"][0, 0] == 0.5).all() and (exp["constant"][0, 1] == 0.25).all()
    assert not exp["zero-flow"].any()  # row 0 and column 0 do not land (strict > 0); the rest carry zero flow anyway


def test_nonfinite_sources_are_never_selected():
    case = fic.BY_NAME["nonfinite-12x19"]
    ref = fic.expected(case)
    assert not np.isfinite(case.flow).all() and np.isfinite(ref).all()
    removed = case.flow.copy()
    for y, x in fic.NONFINITE_SOURCES:
        removed[0, :, y, x] = 1000.0  # the same field with those sources thrown out of the frame
    assert np.isfinite(removed).all()
    assert np.array_equal(fic.interpolate64(removed[0])[0], ref[0])
    assert np.array_equal(forward_interpolate(torch.from_numpy(case.flow)).numpy(), ref)


@pytest.mark.parametrize("name", RANDOM_IDS)
def test_reference_equals_scipy_griddata(name):
    """Upstream RAFT: griddata((x1, y1), dx / dy, (x0, y0), method="nearest") over the sources kept by the strict frame
    test, on float64 coordinates. Without near-ties (asserted per case) the nearest source is unique and scipy's KD-tree
    must pick the same one."""
    interpolate = pytest.importorskip("scipy.interpolate")
    case = fic.BY_NAME[name]
    flow = case.flow[0]
    _, h, w = flow.shape
    dx, dy = flow[0].astype(np.float64), flow[1].astype(np.float64)
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    got = np.stack([interpolate.griddata((x1[valid], y1[valid]), v.reshape(-1)[valid], (x0, y0), method="nearest",
                                         fill_value=0) for v in (dx, dy)]).astype(np.float32)
    assert np.array_equal(got, fic.expected(case)[0]), name


def test_meta_kernel_shape_and_dtype():
    _native.load()
    out = torch.ops.oflow.forward_interpolate(torch.empty(3, 2, 55, 128, device="meta"))
    assert out.device.type == "meta" and tuple(out.shape) == (3, 2, 55, 128) and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        torch.ops.oflow.forward_interpolate(torch.empty(3, 3, 8, 8, device="meta"))
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.oflow.forward_interpolate(torch.empty(1, 2, 8, 8, device="meta", dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.forward_interpolate(torch.zeros(1, 2, 8, 8))


def test_c_abi_argument_errors_without_launch():
    lib = _native.load()
    assert lib.oflow_forward_interpolate_f32(None, 1, 4, 4, 4096, None) == -1
    assert lib.oflow_forward_interpolate_f32(4096, 1, 4, 4, None, None) == -1
    for b, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (65536, 4, 4), (1, 65536, 65536)):
        assert lib.oflow_forward_interpolate_f32(4096, b, h, w, 8192, None) == -2, (b, h, w)


def test_wrong_rank_channels_and_dtype_raise():
    with pytest.raises(ValueError, match="forward_interpolate"):
        forward_interpolate(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="forward_interpolate"):
        forward_interpolate(torch.zeros(1, 1, 2, 8, 8))
    with pytest.raises(ValueError, match="forward_interpolate"):
        forward_interpolate(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="forward_interpolate"):
        forward_interpolate(torch.zeros(2, 3, 8, 8))
    with pytest.raises(TypeError, match="float32"):
        forward_interpolate(torch.zeros(2, 8, 8, dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        forward_interpolate(torch.zeros(1, 2, 8, 8, dtype=torch.float16))
    with pytest.raises(TypeError, match="torch.Tensor"):
        forward_interpolate(np.zeros((2, 8, 8), np.float32))


def test_requires_grad_input_is_detached():
    case = fic.BY_NAME["rand-9x13-s3-1"]
    flow = torch.from_numpy(case.flow.copy()).requires_grad_()
    out = forward_interpolate(flow)
    assert not out.requires_grad and out.grad_fn is None
    assert np.array_equal(out.numpy(), fic.expected(case))
    assert flow.requires_grad  # the caller's tensor is untouched
