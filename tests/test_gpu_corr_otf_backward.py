"""The native backward of the on-the-fly (fp16, volume-free) correlation lookup (csrc/corr_otf_backward.hip) against
float64: the kernels through ``torch.ops.oflow.corr_lookup_alt_backward`` and through the C ABI, the autograd wiring of
``AlternateCorrBlock``, its memory, and one ``RAFT(alternate_corr=True)`` training step. References and inputs:
tests/corr_otf_backward_cases.py (checked on the CPU by tests/test_corr_otf_backward_host.py).

Tolerance: per element |got - ref| <= K * 2^-24 * bound + 1e-30 with bound = the reference pipeline on
|g|, |a|, |F_l| and K = 4 x the worst ratio of the same composition run in fp32 on the CPU (K = 12.52 for grad_fmap1,
12.60 for grad_fmap2; calibrated on that composition, never on the kernel); exactly 0 where the bound is 0. On dyadic
inputs both gradients equal float64 bit for bit, whatever order the atomics arrive in.
"""
from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import corr_backward_cases as cc
import corr_otf_backward_cases as oc
import model.raft as raft_module
from model import RAFT, AlternateCorrBlock, synthetic
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
NAN = float("nan")
E_NULL, E_SHAPE, E_LEVELS, E_TINY, E_RADIUS = -1, -2, -3, -4, -5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _prepared(f1, f2, levels):
    f1h, f2h = OPS.corr_otf_prepare(f1.to(DEV), f2.to(DEV), levels)
    return f1h, list(f2h)


@functools.lru_cache(maxsize=None)
def _gauss(index):
    """Inputs on the device, the fp16 tensors the prepare op returned, and the float64 reference / bound from them."""
    case = oc.GAUSS_CASES[index]
    r, _, levels, _, _ = case
    f1, f2, coords, g = oc.case_inputs(case)
    f1h, f2h = _prepared(f1, f2, levels)
    host = (f1h.cpu(), [t.cpu() for t in f2h])
    ref = oc.reference64(*host, coords, g, r)
    bound = oc.bound64(*host, coords, g, r)
    return r, f1h, f2h, coords.to(DEV), g.to(DEV), ref, bound


def _assert_close(got, ref, bound, k, what, need_dead=True):
    assert got.shape == ref.shape and got.dtype == torch.float32, (what, got.shape)
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), what
    live = bound > 0
    err = (got - ref).abs()
    worst = float((err[live] / (oc.EPS24 * bound[live])).max())
    print(f"{what}: {int(live.sum())} live / {int((~live).sum())} dead elements, worst |err| / (2^-24 bound) = {worst:.3f}"
          f" (K = {k:.2f})")
    assert int(live.sum()) > 0 and (not need_dead or int((~live).sum()) > 0), what
    assert bool((got[~live] == 0).all()), (what, "an element nothing reaches is not exactly 0")
    assert bool((err <= k * oc.EPS24 * bound + 1e-30).all()), (what, worst)


# ----------------------------------------------------------------------------------------------------------
# parity with float64
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(oc.GAUSS_CASES)), ids=oc.CASE_IDS)
def test_backward_matches_fp64(index):
    r, f1h, f2h, coords, g, ref, bound = _gauss(index)
    g1, g2 = OPS.corr_lookup_alt_backward(g, f1h, f2h, coords, r, [True, True])
    _assert_close(g1, ref[0], bound[0], oc.K_G1, f"{oc.CASE_IDS[index]} grad_fmap1")
    _assert_close(g2, ref[1], bound[1], oc.K_G2, f"{oc.CASE_IDS[index]} grad_fmap2")


def test_backward_exact_on_dyadic_inputs():
    """Half-pixel coordinates, gradients in {-1, 0, 1}, integer features, C = 64: every partial sum is a multiple of
    2^-17 below 2^7 (asserted from the float64 bound), so both gradients equal float64 bit for bit in any summation
    order: the index mapping with no tolerance to hide in."""
    r, _, levels, _ = oc.DYADIC
    f1, f2, coords, g = oc.dyadic_inputs()
    f1h, f2h = _prepared(f1, f2, levels)
    e1h, e2h = oc.prepare_emulated(f1, f2, levels)
    assert torch.equal(f1h.cpu(), e1h) and all(torch.equal(a.cpu(), b) for a, b in zip(f2h, e2h))
    ref = oc.reference64(e1h, e2h, coords, g, r)
    bound = oc.bound64(e1h, e2h, coords, g, r)
    m = oc.DYADIC_QUANTUM_BITS
    for rf, bd in zip(ref, bound):
        assert float(bd.max()) < 2.0 ** (24 - m) and torch.equal(rf * 2.0**m, torch.round(rf * 2.0**m))
    got = OPS.corr_lookup_alt_backward(g.to(DEV), f1h, f2h, coords.to(DEV), r, [True, True])
    for name, a, rf in zip(("grad_fmap1", "grad_fmap2"), got, ref):
        assert int((rf != 0).sum()) > rf.numel() // 2, name
        assert torch.equal(a.cpu().double(), rf), (name, float((a.cpu().double() - rf).abs().max()))


# ----------------------------------------------------------------------------------------------------------
# C ABI contracts (include/oflow.h), called directly
# ----------------------------------------------------------------------------------------------------------
def _abi(g, f1h, f2h, coords, radius, want1=True, want2=True, with_scratch=True, c=None, levels=None, dims=None,
         null_grad_out=False):
    b, _, h, w = coords.shape
    ch = int(f1h.shape[3])
    dims = [tuple(int(v) for v in t.shape[1:3]) for t in f2h] if dims is None else dims
    nl = len(f2h) if levels is None else levels
    o1, o2 = torch.full((b, ch, h, w), NAN, device=DEV), torch.full((b, ch, h, w), NAN, device=DEV)
    scratch = torch.full((b * ch * sum(hl * wl for hl, wl in dims),), NAN, device=DEV)
    ptrs = (ctypes.c_void_p * _native.MAX_LEVELS)(*[t.data_ptr() for t in f2h])
    hs = (ctypes.c_int * _native.MAX_LEVELS)(*[d[0] for d in dims])
    ws = (ctypes.c_int * _native.MAX_LEVELS)(*[d[1] for d in dims])
    st = _native.load().oflow_corr_lookup_otf_backward_f32(
        None if null_grad_out else g.data_ptr(), f1h.data_ptr(), ptrs, hs, ws, nl, coords.data_ptr(), b,
        ch if c is None else c, h, w, radius, o1.data_ptr() if want1 else None, o2.data_ptr() if want2 else None,
        scratch.data_ptr() if with_scratch else None, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return st, o1, o2


def test_abi_overwrites_every_element_and_forms_only_the_requested_outputs():
    """NaN-filled outputs and scratch: every element is overwritten (the call zeroes the scratch itself). Either output
    may be NULL: grad_fmap1 is bit-identical to the both-outputs call (fixed order), grad_fmap2 within tolerance
    (atomics); the scratch may be NULL only without grad_fmap2."""
    index = oc.CASE_IDS.index("r4-17x37-L4-C64-mixed")
    r, f1h, f2h, coords, g, ref, bound = _gauss(index)
    st, b1, b2 = _abi(g, f1h, f2h, coords, r)
    assert st == 0
    _assert_close(b1, ref[0], bound[0], oc.K_G1, "C ABI grad_fmap1")
    _assert_close(b2, ref[1], bound[1], oc.K_G2, "C ABI grad_fmap2")
    st, o1, n2 = _abi(g, f1h, f2h, coords, r, want2=False, with_scratch=False)
    assert st == 0 and torch.equal(o1, b1) and bool(torch.isnan(n2).all())
    st, n1, o2 = _abi(g, f1h, f2h, coords, r, want1=False)
    assert st == 0 and bool(torch.isnan(n1).all())
    _assert_close(o2, ref[1], bound[1], oc.K_G2, "C ABI grad_fmap2 alone")
    st, n1, n2 = _abi(g, f1h, f2h, coords, r, with_scratch=False)
    assert st == E_NULL and bool(torch.isnan(n1).all()) and bool(torch.isnan(n2).all())
    st, n1, n2 = _abi(g, f1h, f2h, coords, r, want1=False, want2=False, with_scratch=False)
    assert st == 0 and bool(torch.isnan(n1).all()) and bool(torch.isnan(n2).all())


def test_abi_argument_errors_return_the_documented_codes():
    r, f1h, f2h, coords, g, _, _ = _gauss(oc.CASE_IDS.index("r4-17x37-L4-C64-mixed"))
    dims = [tuple(int(v) for v in t.shape[1:3]) for t in f2h]
    for kwargs, radius, code in (
        ({}, 5, E_RADIUS), ({}, -1, E_RADIUS), ({"c": 48}, r, E_SHAPE), ({"c": 0}, r, E_SHAPE),
        ({"levels": 0}, r, E_LEVELS), ({"levels": _native.MAX_LEVELS + 1}, r, E_LEVELS),
        ({"dims": dims[:3] + [(1, 4)]}, r, E_TINY), ({"dims": dims[:3] + [(2, 1)]}, r, E_TINY),
        ({"null_grad_out": True}, r, E_NULL),
    ):
        st, n1, n2 = _abi(g, f1h, f2h, coords, radius, **kwargs)
        assert st == code, (kwargs, radius, st)
        assert bool(torch.isnan(n1).all()) and bool(torch.isnan(n2).all()), (kwargs, "nothing may be enqueued")


# ----------------------------------------------------------------------------------------------------------
# stray coordinates
# ----------------------------------------------------------------------------------------------------------
def test_stray_coordinates_contribute_nothing():
    """NaN, +-inf, 1e9 and the per-level 2^22 edges among ordinary coordinates: those queries' grad_fmap1 rows are
    exactly 0 (a zero window at the affected levels, far outside at the others), everything is finite, every other
    grad_fmap1 row is bit-identical to a run with the specials replaced by a far-away finite value, and both gradients
    match float64."""
    r, (h, w), levels, c = oc.SPECIALS
    base = cc.mixed_coords(55, (oc.BATCH, 2, h, w), r, h, w)
    coords, rows = cc.with_specials(base, levels)
    far, _ = cc.with_specials(base, levels, replace_by=cc.FAR)
    f1, f2 = cc.gaussian(56, (oc.BATCH, c, h, w)), cc.gaussian(57, (oc.BATCH, c, h, w))
    g = cc.gaussian(58, (oc.BATCH, levels * (2 * r + 1) ** 2, h, w))
    f1h, f2h = _prepared(f1, f2, levels)
    g1, g2 = OPS.corr_lookup_alt_backward(g.to(DEV), f1h, f2h, coords.to(DEV), r, [True, True])
    p1, p2 = OPS.corr_lookup_alt_backward(g.to(DEV), f1h, f2h, far.to(DEV), r, [True, True])
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())
    rows1 = g1.permute(0, 2, 3, 1).reshape(-1, c)
    assert bool((rows1[rows] == 0).all()) and bool((rows1 != 0).any())
    assert torch.equal(g1, p1)
    host = (f1h.cpu(), [t.cpu() for t in f2h])
    ref, bound = oc.reference64(*host, coords, g, r), oc.bound64(*host, coords, g, r)
    _assert_close(g1, ref[0], bound[0], oc.K_G1, "specials grad_fmap1")
    _assert_close(g2, ref[1], bound[1], oc.K_G2, "specials grad_fmap2", need_dead=False)
    _assert_close(p2, ref[1], bound[1], oc.K_G2, "specials replaced grad_fmap2", need_dead=False)


# ----------------------------------------------------------------------------------------------------------
# autograd wiring
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["both", "fmap1", "fmap2", "same"])
def test_alternate_corr_block_gradients_match_fp64(mode):
    case = oc.GAUSS_CASES[oc.CASE_IDS.index("r4-17x37-L4-C64-smooth")]
    r, _, levels, _, _ = case
    f1, f2, coords, g = oc.case_inputs(case)
    d1 = f1.to(DEV).requires_grad_(mode != "fmap2")
    d2 = d1 if mode == "same" else f2.to(DEV).requires_grad_(mode != "fmap1")
    blk = AlternateCorrBlock(d1, d2, num_levels=levels, radius=r)
    out = blk(coords.to(DEV))
    assert out.requires_grad and "corr_lookup_alt" in str(out.grad_fn).lower()
    with torch.no_grad():
        plain = AlternateCorrBlock(d1, d2, num_levels=levels, radius=r)
        want = plain(coords.to(DEV))
    assert not want.requires_grad and torch.equal(out.detach(), want)  # the forward is the inference path, bit for bit
    assert torch.equal(blk.fmap1_f16, plain.fmap1_f16)
    out.backward(g.to(DEV))
    host = (blk.fmap1_f16.cpu(), [t.cpu() for t in blk.fmap2_pyramid_f16])
    ref, bound = oc.reference64(*host, coords, g, r), oc.bound64(*host, coords, g, r)
    if mode == "same":
        tol = oc.K_G1 * oc.EPS24 * bound[0] + oc.K_G2 * oc.EPS24 * bound[1] + oc.EPS24 * (bound[0] + bound[1]) + 1e-30
        err = (d1.grad.cpu().double() - (ref[0] + ref[1])).abs()  # (one more rounding: the sum of the two gradients)
        assert d1.grad.dtype == torch.float32 and bool((err <= tol).all()), float((err / tol).max())
        return
    if mode != "fmap2":
        _assert_close(d1.grad, ref[0], bound[0], oc.K_G1, f"wiring {mode} grad_fmap1")
    else:
        assert d1.grad is None
    if mode != "fmap1":
        _assert_close(d2.grad, ref[1], bound[1], oc.K_G2, f"wiring {mode} grad_fmap2")
    else:
        assert d2.grad is None


def test_inference_entry_points_still_refuse_autograd_inputs():
    f = torch.zeros(1, 32, 8, 8, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="requires grad"):
        _native.otf_prepare(f, f, 2)


# ----------------------------------------------------------------------------------------------------------
# memory
# ----------------------------------------------------------------------------------------------------------
def test_forward_and_backward_allocate_no_volume():
    """(1, 256, 96, 128): the peak over the inputs stays below a quarter of the dense level-0 volume
    ((96 * 128)^2 * 4 B = 604 MB): the purpose of the block, not a tuned number."""
    b, c, h, w = 1, 256, 96, 128
    f1 = torch.randn(b, c, h, w, device=DEV, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_()
    f2 = torch.randn(b, c, h, w, device=DEV, generator=torch.Generator(DEV).manual_seed(2)).requires_grad_()
    coords = oc.grid_coords(b, h, w).to(DEV) + 1.5 * torch.randn(b, 2, h, w, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    AlternateCorrBlock(f1, f2)(coords).sum().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(DEV) - base
    volume = (h * w) ** 2 * 4
    print(f"memory: peak over the inputs {extra / 1e6:.1f} MB, dense level-0 volume {volume / 1e6:.1f} MB")
    assert f1.grad is not None and f2.grad is not None and bool(torch.isfinite(f1.grad).all())
    assert bool((f1.grad != 0).any()) and bool((f2.grad != 0).any())
    assert extra < volume / 4, (extra, volume)


# ----------------------------------------------------------------------------------------------------------
# RAFT(alternate_corr=True).training_step
# ----------------------------------------------------------------------------------------------------------
class _ReferenceBlock:
    """AlternateCorrBlock restated with torch ops: each level is the matmul of the straight-through fp16-rounded
    features (fmap2 pooled by avg_pool2d first), looked up with the differentiable ``_native.corr_lookup``.

    The lookup returns the native forward's values with this restatement's gradient (``native + (ref - ref.detach())``,
    after checking that the two agree): both training steps then run the same forward bit for bit and the comparison
    isolates the backward."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        def st(x):
            return x + (x.half().float() - x).detach()

        b, c, h, w = fmap1.shape
        a = st(fmap1 * (1.0 / math.sqrt(c))).reshape(b, c, h * w).transpose(1, 2)
        self.radius, self.levels, cur = radius, [], fmap2
        for l in range(num_levels):
            if l:
                cur = F.avg_pool2d(cur, 2, stride=2)
            self.levels.append(torch.matmul(a, st(cur).reshape(b, c, -1)).reshape(b * h * w, 1, *cur.shape[-2:]))
        with torch.no_grad():
            self.native = AlternateCorrBlock(fmap1, fmap2, num_levels=num_levels, radius=radius)

    def __call__(self, coords):
        ref = _native.corr_lookup(self.levels, coords, self.radius)
        with torch.no_grad():
            native = self.native(coords.detach())
        torch.testing.assert_close(ref.detach(), native, rtol=1e-4, atol=1e-4)
        return native + (ref - ref.detach())


def _train_model():
    m = RAFT(iters=3, alternate_corr=True)
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    m = m.to(DEV).train()
    for mod in m.modules():  # eval-mode batch norm, as test_raft_training_gradients_match_oracle
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    return m


def _biases_under_instance_norm(model):
    """Names of the convolution biases whose output goes straight into an InstanceNorm2d without affine parameters
    (tests/test_gpu_upsample_backward.py's helper): the norm removes a per-channel constant, so dL/dbias is exactly 0
    and what autograd returns is rounding noise. Found from the module structure, not from any gradient."""
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


def test_training_step_with_alternate_corr_matches_the_reference_block(monkeypatch):
    """One 128 x 128, batch 2, 3-iteration training step of RAFT(alternate_corr=True): every parameter gradient with the
    native backward vs the same step with AlternateCorrBlock replaced by the torch restatement, to a relative norm of
    1e-3 (the project's training-step bar); the biases in front of fnet's instance norms (exact gradient 0) are held to
    1e-3 of their convolution's weight-gradient norm."""
    img0, img1 = (x.to(DEV) for x in synthetic.synthetic_pair(2, 128, 128, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (2, 2, 128, 128), 2.0)).to(DEV)
    valid = (torch.from_numpy(synthetic.hash_normal(32, (2, 128, 128), 1.0)) > -1.0).float().to(DEV)
    grads, losses = {}, {}
    # fp32 convolutions in both steps: the bar compares fp32 gradients, and a reduced-precision (TF32-class) solver picked
    # for one step's convolution backward but not the other's shows up as ~1e-3 on the mask head
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    for impl in ("native", "reference"):
        if impl == "reference":
            monkeypatch.setattr(raft_module, "AlternateCorrBlock", _ReferenceBlock)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # both steps start from an empty allocator cache (see the note at the end of the file)
        model = _train_model()
        loss = model.training_step((img0, img1, target, valid), 0)
        loss.backward()
        losses[impl] = loss.detach()
        grads[impl] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads["native"]) == set(grads["reference"])
    assert "fnet.conv1.weight" in grads["native"] and bool((grads["native"]["fnet.conv1.weight"] != 0).any())
    torch.testing.assert_close(losses["native"], losses["reference"], rtol=1e-3, atol=0)  # (the gradients' bar)
    null = _biases_under_instance_norm(model)
    assert null and null <= set(grads["reference"])
    rels = {}
    for k, want in grads["reference"].items():
        got = grads["native"][k]
        if k in null:
            wn = grads["reference"][k[: -len("bias")] + "weight"].norm()
            rels[k] = max(float(got.norm() / wn), float(want.norm() / wn))
        else:
            assert float(want.norm()) > 0, k
            rels[k] = float((got - want).norm() / want.norm())
    for k, rel in sorted(rels.items(), key=lambda t: -t[1])[:8]:
        print(f"training step: {k}: {rel:.2e}" + (" (zero gradient: norm / weight-gradient norm)" if k in null else ""))
    print(f"training step: fnet.conv1.weight: {rels['fnet.conv1.weight']:.2e}; {len(rels) - len(null)} parameters "
          f"compared, {len(null)} with an exactly zero gradient")
    bad = {k: r for k, r in rels.items() if not r <= 1e-3}
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------
# torch.compile (kept last in this file). Note on the training-step comparison above: when other tests of this file had
# run in the process before it, the mask head's first convolution -- which the new kernel does not reach -- differed
# between the two steps by 1.19e-3 (bias) / 9.57e-4 (weight), three runs out of three, although both steps run the same
# forward bit for bit; alone in a process, or with the allocator cache emptied before each step, it agrees to 3e-6 (as do
# two native steps, or two reference steps). So that gradient depends on what the caching allocator hands out, i.e. on
# stale memory somewhere in the convolution backward; where is not found. The comparison empties the cache before each step.
# ----------------------------------------------------------------------------------------------------------
def test_compile_fullgraph_lookup_and_backward():
    torch._dynamo.reset()
    r, f1h, f2h, coords, g, ref, bound = _gauss(oc.CASE_IDS.index("r2-5x13-L2-C32-smooth"))
    b, _, h, w = coords.shape
    c = int(f1h.shape[3])

    def loss(a1, a2):
        return (torch.ops.oflow.corr_lookup_alt(a1, a2, f1h, f2h, coords, r) * g).sum()

    grads = []
    for fn in (loss, torch.compile(loss, fullgraph=True, dynamic=False)):
        a1 = torch.zeros(b, c, h, w, device=DEV, requires_grad=True)  # (values are not read: f1h / f2h carry them)
        a2 = torch.zeros(b, c, h, w, device=DEV, requires_grad=True)
        value = fn(a1, a2)
        value.backward()
        grads.append((value.detach(), a1.grad, a2.grad))
    torch.testing.assert_close(grads[1][0], grads[0][0], rtol=1e-5, atol=1e-5)
    assert torch.equal(grads[1][1], grads[0][1])
    for run in grads:
        _assert_close(run[1], ref[0], bound[0], oc.K_G1, "compile grad_fmap1")
        _assert_close(run[2], ref[1], bound[1], oc.K_G2, "compile grad_fmap2")
