"""CPU checks of the on-the-fly correlation backward's references (tests/corr_otf_backward_cases.py) and of its
interface: the float64 reference equals float64 autograd of the reference project's dense composition where the fp16
path is exact, the calibrated K of the GPU tolerance is re-measured on the fp32 CPU composition, and the new symbol / ops
are declared, listed and give the right shapes on meta tensors. No kernel is launched here."""
from __future__ import annotations

import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import corr_backward_cases as cc
import corr_otf_backward_cases as oc
from optical_flow import _native, _ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = torch.device("meta")


def test_reference_equals_dense_autograd_on_dyadic_inputs():
    """Integer features and C = 64: fmap1 / sqrt(C) and every pooled level are exact in fp16 (.half() changes nothing),
    so the fp16 path is the dense composition matmul / sqrt(C), avg_pool2d, window lookup, and the reference must equal
    float64 autograd of that composition."""
    r, (h, w), levels, c = oc.DYADIC
    f1, f2, coords, g = oc.dyadic_inputs()
    f1h, f2h = oc.prepare_emulated(f1, f2, levels)
    assert f1h.dtype == torch.float16 and all(t.dtype == torch.float16 for t in f2h)
    assert torch.equal(f1h.double(), (f1.double() / 8.0).permute(0, 2, 3, 1))
    cur = f2.double()
    for l in range(levels):
        if l:
            cur = F.avg_pool2d(cur, 2, stride=2)
        assert tuple(f2h[l].shape[1:3]) == cc.level_dims(h, w, levels)[l]
        assert torch.equal(f2h[l].double(), cur.permute(0, 2, 3, 1)), l  # the fp16 rounding is the identity here
    for got, want, name in zip(oc.reference64(f1h, f2h, coords, g, r), oc.dense_composition64(f1, f2, coords, g, levels, r),
                               ("grad_fmap1", "grad_fmap2")):
        assert got.shape == want.shape == f1.shape
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"dyadic {name}: max |closed form - dense autograd| / max |dense| = {rel:.3e}")
        assert float(want.abs().max()) > 0 and rel <= 1e-12, (name, rel)


def test_dyadic_inputs_keep_every_partial_sum_exact_in_fp32():
    """The condition the GPU's bit-for-bit test relies on, from the float64 bound: every partial sum is a multiple of
    2^-m and stays below 2^(24-m)."""
    r, _, levels, _ = oc.DYADIC
    f1, f2, coords, g = oc.dyadic_inputs()
    f1h, f2h = oc.prepare_emulated(f1, f2, levels)
    m = oc.DYADIC_QUANTUM_BITS
    for ref, bound in zip(oc.reference64(f1h, f2h, coords, g, r), oc.bound64(f1h, f2h, coords, g, r)):
        assert float(bound.max()) < 2.0 ** (24 - m), float(bound.max())
        assert torch.equal(ref * 2.0**m, torch.round(ref * 2.0**m))
        assert torch.equal(ref.float().double(), ref)


@functools.lru_cache(maxsize=None)
def _calibration():
    worst = [0.0, 0.0]
    live = [0, 0]
    dead = [0, 0]
    for case in oc.GAUSS_CASES:
        r, _, levels, _, _ = case
        f1, f2, coords, g = oc.case_inputs(case)
        f1h, f2h = oc.prepare_emulated(f1, f2, levels)
        ref = oc.reference64(f1h, f2h, coords, g, r)
        bound = oc.bound64(f1h, f2h, coords, g, r)
        got = oc.composition32(f1h, f2h, coords, g, r)
        for i in range(2):
            lv = bound[i] > 0
            live[i] += int(lv.sum())
            dead[i] += int((~lv).sum())
            assert bool((got[i][~lv] == 0).all()) and bool((ref[i][~lv] == 0).all())
            ratio = float(((got[i].double() - ref[i]).abs()[lv] / (oc.EPS24 * bound[i][lv])).max())
            worst[i] = max(worst[i], ratio)
    return worst, live, dead


def test_calibrated_k_is_the_fp32_compositions_worst_ratio():
    """K = 4 x the worst |err| / (2^-24 * bound) of the fp32 CPU composition against float64 over the Gaussian cases. The
    recorded ratios must cover a re-measurement (another BLAS may sum in another order: they may be up to 2 x larger
    than what this machine measures, never smaller)."""
    worst, live, dead = _calibration()
    print(f"calibration: worst ratio grad_fmap1 {worst[0]:.3f}, grad_fmap2 {worst[1]:.3f}; live {live}, dead {dead}")
    assert min(live) > 0 and min(dead) > 0
    for measured, recorded, k in ((worst[0], oc.CALIBRATED_RATIO_G1, oc.K_G1), (worst[1], oc.CALIBRATED_RATIO_G2, oc.K_G2)):
        assert k == 4.0 * recorded
        assert measured <= recorded <= 2.0 * measured, (measured, recorded)


def test_symbol_and_ops_are_declared_and_listed():
    text = open(os.path.join(REPO, "include", "oflow.h")).read()
    assert re.search(r"\bint\s+oflow_corr_lookup_otf_backward_f32\s*\(", text)
    assert "oflow_corr_lookup_otf_backward_f32" in _native.SYMBOLS
    assert "corr_lookup_alt" in _ops.OPS and "corr_lookup_alt_backward" in _ops.OPS
    lib = _native.load()
    assert lib.oflow_corr_lookup_otf_backward_f32 is not None and lib.oflow_abi_version() == _native.ABI_VERSION
    for name in ("corr_lookup_alt", "corr_lookup_alt_backward"):
        assert getattr(torch.ops.oflow, name).default._schema.name == f"oflow::{name}"


def _meta_inputs(requires_grad=False):
    b, c, h, w, levels = 2, 64, 17, 37, 4
    f1 = torch.empty(b, c, h, w, device=META, requires_grad=requires_grad)
    f2 = torch.empty(b, c, h, w, device=META, requires_grad=requires_grad)
    f1h, f2h = torch.ops.oflow.corr_otf_prepare(f1.detach(), f2.detach(), levels)
    return f1, f2, f1h, list(f2h), torch.empty(b, 2, h, w, device=META)


def test_meta_shapes_and_dtypes():
    _native.load()
    f1, f2, f1h, f2h, co = _meta_inputs()
    assert [tuple(t.shape) for t in f2h] == [(2, 17, 37, 64), (2, 8, 18, 64), (2, 4, 9, 64), (2, 2, 4, 64)]
    out = torch.ops.oflow.corr_lookup_alt(f1, f2, f1h, f2h, co, 4)
    assert tuple(out.shape) == (2, 4 * 81, 17, 37) and out.dtype == torch.float32 and out.device.type == "meta"
    for mask in ([True, True], [True, False], [False, True], [False, False]):
        g1, g2 = torch.ops.oflow.corr_lookup_alt_backward(out, f1h, f2h, co, 4, mask)
        assert tuple(g1.shape) == ((2, 64, 17, 37) if mask[0] else (0,)), mask
        assert tuple(g2.shape) == ((2, 64, 17, 37) if mask[1] else (0,)), mask
        assert g1.dtype == torch.float32 and g2.dtype == torch.float32
    with pytest.raises(RuntimeError, match="radius"):
        torch.ops.oflow.corr_lookup_alt(f1, f2, f1h, f2h, co, 5)
    with pytest.raises(RuntimeError, match="grad_out"):
        torch.ops.oflow.corr_lookup_alt_backward(out[:, :-1], f1h, f2h, co, 4, [True, True])
    with pytest.raises(RuntimeError, match="prepared from"):
        torch.ops.oflow.corr_lookup_alt(f1[:, :32], f2[:, :32], f1h, f2h, co, 4)


def test_autograd_formula_is_wired_on_meta_tensors():
    _native.load()
    for need in ((True, True), (True, False), (False, True)):
        f1, f2, f1h, f2h, co = _meta_inputs()
        f1.requires_grad_(need[0])
        f2.requires_grad_(need[1])
        out = torch.ops.oflow.corr_lookup_alt(f1, f2, f1h, f2h, co, 4)
        assert out.requires_grad
        out.sum().backward()
        for t, n in ((f1, need[0]), (f2, need[1])):
            assert (t.grad is not None) == n
            if n:
                assert t.grad.shape == t.shape and t.grad.dtype == torch.float32


def test_cpu_tensors_are_refused():
    _native.load()
    f = torch.zeros(1, 32, 4, 4)
    f1h, f2h, co = torch.zeros(1, 4, 4, 32, dtype=torch.float16), [torch.zeros(1, 4, 4, 32, dtype=torch.float16)], torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.corr_lookup_alt(f, f, f1h, f2h, co, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.corr_lookup_alt_backward(torch.zeros(1, 9, 4, 4), f1h, f2h, co, 1, [True, True])
