"""fb_consistency without a GPU: the CPU path of optical_flow.fb_consistency against the float64 reference
(tests/fb_consistency_cases.py); the reference against an independent F.grid_sample composition and against the
written-out values of the hand-checkable cases; the operator's Meta kernel and argument checks; the C ABI's argument
errors (nothing is launched)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fb_consistency_cases as fc
import optical_flow
from optical_flow import _native, fb_consistency

RANDOM_IDS = [c.name for c in fc.CASES if c.random]


def _t(x):
    return torch.from_numpy(x)


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_cpu_path_matches_reference(name):
    case = fc.BY_NAME[name]
    fc.expected(case)  # (asserts the exemption cap and, for a random case, the class balance)
    fw, bw = _t(case.fw), _t(case.bw)
    (m_fw, e_fw), (m_bw, e_bw) = fb_consistency(fw, bw, case.alpha, case.beta, both=True, return_error=True)
    for t in (m_fw, m_bw):
        assert t.dtype == torch.bool and tuple(t.shape) == (fw.shape[0], 1, *fw.shape[2:])
    fc.compare(case, 0, m_fw.numpy(), e_fw.numpy())
    fc.compare(case, 1, m_bw.numpy(), e_bw.numpy())
    # the other return forms are the same tensors
    one = fb_consistency(fw, bw, case.alpha, case.beta)
    assert isinstance(one, torch.Tensor) and torch.equal(one, m_fw)
    a, b = fb_consistency(fw, bw, case.alpha, case.beta, both=True)
    assert torch.equal(a, m_fw) and torch.equal(b, m_bw)
    m, e = fb_consistency(bw, fw, case.alpha, case.beta, return_error=True)  # swapped arguments = the other direction
    assert torch.equal(m, m_bw) and torch.equal(e.view(torch.int32), e_bw.view(torch.int32))


def test_defaults_are_unflows():
    case = fc.BY_NAME["rand-33x65"]
    assert (case.alpha, case.beta) == (0.01, 0.5)
    assert torch.equal(fb_consistency(_t(case.fw), _t(case.bw)), fb_consistency(_t(case.fw), _t(case.bw), 0.01, 0.5))


def test_written_out_cases():
    zero = fc.expected(fc.BY_NAME["zero-flow-7x10"])
    for r in zero:
        assert not r.mask.any() and not r.err.any() and r.inside.all()
    half = fc.expected(fc.BY_NAME["half-pixel-4x8"])[0]
    for i in range(4):
        assert half.err[0, 0, i].tolist() == fc.HALF_PIXEL_ERR  # dyadic: exact
        assert half.mask[0, 0, i].tolist() == fc.HALF_PIXEL_MASK
    got_m, got_e = fb_consistency(_t(fc.BY_NAME["half-pixel-4x8"].fw), _t(fc.BY_NAME["half-pixel-4x8"].bw), return_error=True)
    assert got_e[0, 0, 2].tolist() == fc.HALF_PIXEL_ERR and got_m[0, 0, 2].tolist() == fc.HALF_PIXEL_MASK
    edge = fc.expected(fc.BY_NAME["frame-edge-5x9"])[0]
    for i, j, u, v, inside in fc.EDGE_PIXELS:
        assert bool(edge.inside[0, 0, i, j]) == inside, (i, j)
        if inside:
            assert edge.err[0, 0, i, j] == u * u + v * v  # (bw = 0: nothing cancels the flow)
        else:
            assert edge.err[0, 0, i, j] == np.inf and edge.mask[0, 0, i, j]
    one = fc.expected(fc.BY_NAME["one-pixel-1x1-b2"])[0]
    assert one.inside[:, 0, 0, 0].tolist() == [True, False] and one.mask[:, 0, 0, 0].tolist() == [False, True]


def test_nonfinite_entries_are_occluded():
    case = fc.BY_NAME["nonfinite-13x17"]
    r_fw, r_bw = fc.expected(case)
    for _, i, j, _ in fc.NONFINITE_FW:  # a non-finite own flow: outside
        assert r_fw.mask[0, 0, i, j] and not r_fw.inside[0, 0, i, j] and r_fw.err[0, 0, i, j] == np.inf
    for _, i, j, _ in fc.NONFINITE_BW:
        assert r_bw.mask[0, 0, i, j] and not r_bw.inside[0, 0, i, j]
    # a non-finite tap: a NaN residual, occluded; each planted tap is read by some inside pixel of the other direction
    assert np.isnan(r_fw.err).sum() >= len(fc.NONFINITE_BW) and np.isnan(r_bw.err).sum() >= len(fc.NONFINITE_FW)
    for r in (r_fw, r_bw):
        assert r.mask[np.isnan(r.err)].all() and r.inside[np.isnan(r.err)].all()
    # throwing the planted pixels out changes nothing away from them
    clean = fc.check64(*(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0) for x in (case.fw, case.bw)), case.alpha, case.beta)
    same = np.isfinite(r_fw.err)
    assert np.array_equal(clean.mask[same], r_fw.mask[same])


@pytest.mark.parametrize("name", RANDOM_IDS)
def test_reference_equals_grid_sample_composition(name):
    """An independent statement of the check on the interior pixels (target at least one pixel inside the frame, so
    that neither the border clamp nor zero padding plays a part): F.grid_sample of the other flow at the normalised
    target, in float64."""
    case = fc.BY_NAME[name]
    for d, (a, o) in enumerate(((case.fw, case.bw), (case.bw, case.fw))):
        ref = fc.expected(case)[d]
        a64, o64 = _t(a).double(), _t(o).double()
        b, _, h, w = a64.shape
        # the target at the fp32-rounded position, as the contract states
        px = (torch.arange(w, dtype=torch.float32).view(1, 1, w) + _t(a)[:, 0]).double()
        py = (torch.arange(h, dtype=torch.float32).view(1, h, 1) + _t(a)[:, 1]).double()
        grid = torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], dim=-1)
        s = F.grid_sample(o64, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        err = ((a64 + s) ** 2).sum(1, keepdim=True)
        thr = case.alpha * ((a64**2).sum(1, keepdim=True) + (s**2).sum(1, keepdim=True)) + case.beta
        interior = ((px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)).unsqueeze(1).numpy()
        assert interior.sum() >= 0.3 * interior.size
        # float64 against float64: the normalisation's roundings only
        np.testing.assert_allclose(err.numpy()[interior], ref.err[interior], rtol=1e-9, atol=1e-12)
        clear = interior & (np.abs(ref.err - ref.thr) > 1e-9)
        assert np.array_equal((err > thr).numpy()[clear], ref.mask[clear])


def test_inputs_are_detached_and_converted():
    case = fc.BY_NAME["rand-13x17-b3"]
    fw, bw = _t(case.fw.copy()).requires_grad_(), _t(case.bw.copy()).requires_grad_()
    m, e = fb_consistency(fw, bw, return_error=True)
    assert not m.requires_grad and not e.requires_grad and e.grad_fn is None and fw.requires_grad
    # float64 and non-contiguous inputs are converted, as warp converts its inputs
    m64 = fb_consistency(_t(case.fw).double(), _t(case.bw).double())
    assert torch.equal(m64, m)
    wide = torch.zeros((3, 2, 13, 34))
    wide[..., ::2] = _t(case.fw)
    assert torch.equal(fb_consistency(wide[..., ::2], _t(case.bw)), m)


def test_operator_argument_errors():
    z = torch.zeros(1, 2, 8, 8)
    with pytest.raises(TypeError, match="torch.Tensor"):
        fb_consistency(np.zeros((1, 2, 8, 8), np.float32), z)
    with pytest.raises(TypeError, match="floating-point"):
        fb_consistency(z.long(), z)
    with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
        fb_consistency(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
        fb_consistency(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match=r"\(B, 2, H, W\)"):
        fb_consistency(z, torch.zeros(1, 2, 8, 9))
    with pytest.raises(ValueError, match="different devices"):
        fb_consistency(z, z.to("meta"))
    assert optical_flow.operator.fb_consistency is fb_consistency
    empty = fb_consistency(torch.zeros(0, 2, 4, 4), torch.zeros(0, 2, 4, 4))
    assert tuple(empty.shape) == (0, 1, 4, 4) and empty.dtype == torch.bool


def test_meta_kernel_shapes_and_dtypes():
    _native.load()
    op = torch.ops.oflow.fb_consistency
    fw, bw = torch.empty(3, 2, 55, 128, device="meta"), torch.empty(3, 2, 55, 128, device="meta")
    for both in (False, True):
        for with_error in (False, True):
            m_fw, m_bw, e_fw, e_bw = op(fw, bw, 0.01, 0.5, both, with_error)
            full, none = (3, 1, 55, 128), (0,)
            assert [tuple(t.shape) for t in (m_fw, m_bw, e_fw, e_bw)] == [
                full, full if both else none, full if with_error else none, full if both and with_error else none]
            assert m_fw.dtype == m_bw.dtype == torch.bool and e_fw.dtype == e_bw.dtype == torch.float32
            assert all(t.device.type == "meta" for t in (m_fw, m_bw, e_fw, e_bw))
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        op(torch.empty(3, 3, 8, 8, device="meta"), torch.empty(3, 3, 8, 8, device="meta"), 0.01, 0.5, False, False)
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        op(fw, torch.empty(3, 2, 55, 64, device="meta"), 0.01, 0.5, False, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), 0.01, 0.5, False, False)
    assert "fb_consistency" in _native._ops.OPS and "oflow_fb_consistency_f32" in _native.SYMBOLS


def test_c_abi_argument_errors_without_launch():
    fn = _native.load().oflow_fb_consistency_f32
    A, n = 1 << 20, 4 * 4  # fake device addresses 1 MiB apart; a 1 x 4 x 4 call's flows are 128 bytes
    fw, bw, m0, m1, e0, e1 = (A * k for k in range(1, 7))
    NULL, SHAPE, ALIGN = -1, -2, -7
    assert fn(None, bw, 1, 4, 4, 0.01, 0.5, m0, None, None, None, None) == NULL
    assert fn(fw, None, 1, 4, 4, 0.01, 0.5, m0, None, None, None, None) == NULL
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, None, m1, e0, e1, None) == NULL  # the first mask is required
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, None, e0, e1, None) == NULL  # a reverse residual without its mask
    for b, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (65536, 4, 4), (1, 65536, 65536)):
        assert fn(fw, bw, b, h, w, 0.01, 0.5, m0, m1, e0, e1, None) == SHAPE, (b, h, w)
    # an output that overlaps an input, or another output, is refused
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, fw, None, None, None, None) == SHAPE
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, bw + 8 * n - 1, None, None, None, None) == SHAPE  # the flow's last byte
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, None, bw, None, None) == SHAPE
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, m1, e0, fw + 64, None) == SHAPE
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, m0, None, None, None) == SHAPE
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, m1, e0, e0 + 4, None) == SHAPE
    assert fn(fw + 2, bw, 1, 4, 4, 0.01, 0.5, m0, None, None, None, None) == ALIGN
    assert fn(fw, bw, 1, 4, 4, 0.01, 0.5, m0, None, e0 + 1, None, None) == ALIGN
