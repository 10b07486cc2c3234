"""``torch.ops.oflow`` (csrc/torch_ops.cpp): the operator library loads on the CPU, registers every op with a Meta
kernel (what torch.compile's fake tensors run), carries the autograd formulas of optical_flow/_ops.py, and refuses
CPU tensors. No kernel is launched here; the GPU half (values, torch.compile fullgraph) is in test_gpu_ops.py."""
import os

import pytest
import torch

from conftest import REPO
from optical_flow import _native, _ops

META = torch.device("meta")


def test_every_op_is_registered():
    _native.load()
    for name in _ops.OPS:
        op = getattr(torch.ops.oflow, name)
        assert op.default._schema.name == f"oflow::{name}"


def test_meta_shapes():
    _native.load()
    f = torch.empty(2, 64, 55, 128, device=META)
    pyr = torch.ops.oflow.corr_pyramid(f, f, 4)
    assert [tuple(p.shape) for p in pyr] == [(14080, 1, 55, 128), (14080, 1, 27, 64), (14080, 1, 13, 32), (14080, 1, 6, 16)]
    tp = torch.ops.oflow.corr_pyramid_tiled(f, f, 4)
    per = [int(_native.load().oflow_corr_tiled_level_floats(h, w)) for h, w in _native.pyramid_dims(55, 128, 4)]
    assert [tuple(t.shape) for t in tp] == [(14080, n) for n in per]
    co = torch.empty(2, 2, 55, 128, device=META)
    assert tuple(torch.ops.oflow.corr_lookup(pyr, co, 4).shape) == (2, 324, 55, 128)
    assert tuple(torch.ops.oflow.corr_lookup_tiled(tp, co, 3).shape) == (2, 196, 55, 128)
    f1h, f2h = torch.ops.oflow.corr_otf_prepare(f, f, 3)
    assert f1h.dtype == torch.float16 and tuple(f1h.shape) == (2, 55, 128, 64)
    assert [tuple(t.shape) for t in f2h] == [(2, 55, 128, 64), (2, 27, 64, 64), (2, 13, 32, 64)]
    assert tuple(torch.ops.oflow.corr_lookup_otf(f1h, f2h, co, 4).shape) == (2, 243, 55, 128)
    fr = torch.empty(3, 5, 20, 30, device=META)
    assert tuple(torch.ops.oflow.grid_warp(fr, torch.empty(3, 2, 20, 30, device=META), 0, 1, False).shape) == (3, 5, 20, 30)
    assert tuple(torch.ops.oflow.grid_sample(fr, torch.empty(3, 7, 9, 2, device=META), 2, 0, True).shape) == (3, 5, 7, 9)


def test_meta_argument_checks():
    _native.load()
    f = torch.empty(1, 64, 16, 16, device=META)
    co = torch.empty(1, 2, 16, 16, device=META)
    pyr = torch.ops.oflow.corr_pyramid(f, f, 2)
    with pytest.raises(RuntimeError, match="radius 8 outside"):
        torch.ops.oflow.corr_lookup(pyr, co, 8)
    with pytest.raises(RuntimeError, match="must be equal"):
        torch.ops.oflow.corr_pyramid(f, torch.empty(1, 64, 16, 8, device=META), 2)
    with pytest.raises(RuntimeError, match="C % 32"):
        torch.ops.oflow.corr_otf_prepare(torch.empty(1, 40, 16, 16, device=META), torch.empty(1, 40, 16, 16, device=META), 2)
    with pytest.raises(ValueError, match="interpolation mode"):
        torch.ops.oflow.grid_warp(torch.empty(1, 3, 4, 4, device=META), torch.empty(1, 2, 4, 4, device=META), 5, 0, False)


def test_autograd_formulas_are_wired():
    """Gradients flow (as shapes, on meta tensors) through pyramid -> lookup and through warp / grid_sample."""
    _native.load()
    f1 = torch.empty(2, 32, 16, 16, device=META, requires_grad=True)
    f2 = torch.empty(2, 32, 16, 16, device=META, requires_grad=True)
    pyr = _native.corr_pyramid(f1, f2, 3)
    out = _native.corr_lookup(pyr, torch.empty(2, 2, 16, 16, device=META), 2)
    assert out.requires_grad
    out.sum().backward()
    assert f1.grad.shape == f1.shape and f2.grad.shape == f2.shape
    fr = torch.empty(1, 3, 8, 8, device=META, requires_grad=True)
    fl = torch.empty(1, 2, 8, 8, device=META, requires_grad=True)
    _native.grid_warp(fr, fl, "bicubic", "zeros", True).sum().backward()
    assert fr.grad.shape == fr.shape and fl.grad.shape == fl.shape
    g = torch.empty(1, 5, 6, 2, device=META, requires_grad=True)
    _native.grid_sample(fr.detach().requires_grad_(), g, "bilinear", "zeros", True).sum().backward()
    assert g.grad.shape == g.shape


@pytest.mark.parametrize("key", ["CUDA", "CPU", "Meta"])
def test_every_op_has_a_kernel_for_every_key(key):
    """The HIP kernel, the CPU kernel (which refuses) and the Meta kernel (torch.compile's) of every op: an op left
    out of one of them fails only for that op and only on that path."""
    _native.load()
    for name in _ops.OPS:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"oflow::{name}", key), (name, key)


def test_schemas_are_unchanged():
    """tests/golden/op_schemas.txt: str(op.default._schema) of every op, recorded before the ops were bound from one
    function each (names and signatures only)."""
    _native.load()
    with open(os.path.join(REPO, "tests", "golden", "op_schemas.txt")) as f:
        recorded = f.read().splitlines()
    assert [str(getattr(torch.ops.oflow, name).default._schema) for name in _ops.OPS] == recorded


def _cpu_args():
    """One tiny valid-shaped argument set per op, all on the CPU."""
    z = torch.zeros
    f8, f32 = z(1, 8, 16, 16), z(1, 32, 8, 8)
    co16, co8 = z(1, 2, 16, 16), z(1, 2, 8, 8)
    tiled = [z(256, int(_native.load().oflow_corr_tiled_level_floats(16, 16)))]
    f1h, f2h = z(1, 8, 8, 32, dtype=torch.float16), [z(1, 8, 8, 32, dtype=torch.float16)]
    frame, flow, grid = z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 2, 2, 2)
    valid, mask = z(1, 4, 4), z(1, 576, 4, 4)
    x, w, c4 = z(1, 4, 6, 6), z(8, 4, 3, 3), z(4)
    img = z(1, 8, 8, 3, dtype=torch.uint8)
    two, three = [True, True], [True, True, True]
    return {
        "corr_pyramid": (f8, f8, 2),
        "corr_pyramid_tiled": (f8, f8, 2),
        "corr_lookup": ([z(256, 1, 16, 16)], co16, 2),
        "corr_lookup_tiled": (tiled, co16, 2),
        "corr_lookup_tiled_nhwc": (tiled, co16, 2, z(256, 25)),
        "corr_otf_prepare": (f32, f32, 1),
        "corr_lookup_otf": (f1h, f2h, co8, 2),
        "grid_warp": (frame, flow, 0, 0, False),
        "grid_sample": (frame, grid, 0, 0, False),
        "corr_lookup_backward": (z(1, 25, 8, 8), co8, 2, 8, 8, 1),
        "corr_pyramid_backward": ([z(64, 1, 8, 8)], f32, f32),
        "grid_warp_backward": (z(1, 3, 4, 4), frame, flow, 0, 0, False, two),
        "grid_sample_backward": (z(1, 3, 2, 2), frame, grid, 0, 0, False, two),
        "flow_error_stats": (flow, flow, None, 3.0, 0.05, 400.0, z(8, dtype=torch.float64), False),
        "sequence_loss": ([flow], flow, valid, [1.0], 400.0),
        "sequence_loss_backward": (torch.ones(()), [flow], flow, valid, [1.0], 400.0, [1]),
        "convex_upsample": (flow, mask),
        "convex_upsample_backward": (z(1, 2, 32, 32), flow, mask, two),
        "corr_lookup_alt": (f32, f32, f1h, f2h, co8, 2),
        "corr_lookup_alt_backward": (z(1, 25, 8, 8), f1h, f2h, co8, 2, two),
        "forward_interpolate": (flow,),
        "augment_batch": (img, img, z(1, 2, 8, 8), None, z(1, _native.AUG_PARAM_DOUBLES, dtype=torch.float64), 4, 4),
        "conv2d_same": (x, w, None),
        "conv2d_same_backward": (z(1, 8, 6, 6), x, w, three),
        "conv2d_strided": (x, w, None, 2),
        "conv2d_strided_backward": (z(1, 8, 3, 3), x, w, 2, three),
        "instance_norm_act": (x, 1e-5, True),
        "instance_norm_act_backward": (x, x, 1e-5, True),
        "frozen_batch_norm_act": (x, c4, c4, c4, c4, 1e-5, True),
        "frozen_batch_norm_act_backward": (x, x, c4, c4, c4, c4, 1e-5, True, three),
        "batch_norm_act": (x, c4, c4, 1e-5, True),
        "batch_norm_act_backward": (x, x, c4, c4, c4, c4, 1e-5, True, three),
        "fb_consistency": (flow, flow, 0.01, 0.5, True, False),
    }


def test_cpu_tensors_raise():
    """Every op refuses CPU tensors with the one "no CPU fallback" message (what each op raised for these arguments
    before the ops were bound from one function each: all 33 this message, none PyTorch's generic "could not run")."""
    args = _cpu_args()
    assert sorted(args) == sorted(_ops.OPS)
    for name in _ops.OPS:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(torch.ops.oflow, name)(*args[name])
