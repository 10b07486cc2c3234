"""fb_consistency on the GPU (csrc/fb_consistency.hip): the operator and the C ABI on a side stream against the float64
reference on every case (tests/fb_consistency_cases.py: masks exactly outside the derived exemption band, residuals
within the derived E), and the bit-level properties: both directions in one launch equal the two single-direction
launches, optional outputs do not change the others, a second run gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import fb_consistency_cases as fc
from optical_flow import _native, fb_consistency

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))  # (NaN == NaN by bits)


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_operator_matches_reference(name):
    case = fc.BY_NAME[name]
    refs = fc.expected(case)
    fw, bw = torch.from_numpy(case.fw).to(DEV), torch.from_numpy(case.bw).to(DEV)
    (m_fw, e_fw), (m_bw, e_bw) = fb_consistency(fw, bw, case.alpha, case.beta, both=True, return_error=True)
    for d, (m, e) in enumerate(((m_fw, e_fw), (m_bw, e_bw))):
        assert m.device == fw.device and m.dtype == torch.bool and e.dtype == torch.float32
        fin = np.isfinite(refs[d].err)
        diff = np.abs(e.cpu().numpy()[fin].astype(np.float64) - refs[d].err[fin])
        rel = float((diff / np.maximum(refs[d].tol[fin], 1e-300)).max()) if fin.any() and diff.max() > 0 else 0.0
        wrong = int(((m.cpu().numpy() != refs[d].mask) & ~refs[d].exempt).sum())
        print(f"{name} dir {d}: max |err - err64| / E = {rel:.3f}, {wrong} wrong mask pixels, "
              f"{int(refs[d].exempt.sum())} exempt of {refs[d].mask.size}")
        fc.compare(case, d, m.cpu().numpy(), e.cpu().numpy())
    # the raw op: bool masks, empty tensors for what was not asked
    o = torch.ops.oflow.fb_consistency(fw, bw, case.alpha, case.beta, False, False)
    assert _same(o[0], m_fw) and all(t.numel() == 0 for t in o[1:])
    assert o[1].dtype == torch.bool and o[2].dtype == o[3].dtype == torch.float32

    # both directions in one launch = the two single-direction launches, bit for bit
    s_fw, se_fw = fb_consistency(fw, bw, case.alpha, case.beta, return_error=True)
    s_bw, se_bw = fb_consistency(bw, fw, case.alpha, case.beta, return_error=True)
    assert _same(s_fw, m_fw) and _same(se_fw, e_fw) and _same(s_bw, m_bw) and _same(se_bw, e_bw)
    # leaving the residuals out does not change the masks
    n_fw, n_bw = fb_consistency(fw, bw, case.alpha, case.beta, both=True)
    assert _same(n_fw, m_fw) and _same(n_bw, m_bw) and _same(fb_consistency(fw, bw, case.alpha, case.beta), m_fw)
    # a second run: the same bits
    (m2_fw, e2_fw), (m2_bw, e2_bw) = fb_consistency(fw, bw, case.alpha, case.beta, both=True, return_error=True)
    assert _same(m2_fw, m_fw) and _same(e2_fw, e_fw) and _same(m2_bw, m_bw) and _same(e2_bw, e_bw)


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_c_abi_on_a_side_stream_matches_reference(name):
    case = fc.BY_NAME[name]
    fc.expected(case)
    b, _, h, w = case.fw.shape
    fw, bw = torch.from_numpy(case.fw).to(DEV), torch.from_numpy(case.bw).to(DEV)
    fill_m = lambda: torch.full((b, 1, h, w), 7, device=DEV, dtype=torch.uint8)  # noqa: E731
    fill_e = lambda: torch.full((b, 1, h, w), -3.0, device=DEV)  # noqa: E731
    full = [fill_m(), fill_m(), fill_e(), fill_e()]
    again = [fill_m(), fill_m(), fill_e(), fill_e()]
    masks_only = [fill_m(), fill_m()]
    fw_only = [fill_m(), fill_e()]
    torch.cuda.synchronize(DEV)  # the inputs and fills are in place before the side stream touches them
    stream = torch.cuda.Stream(DEV)
    st = ctypes.c_void_p(stream.cuda_stream)
    lib = _native.load()
    p = lambda t: t.data_ptr()  # noqa: E731
    args = (fw.data_ptr(), bw.data_ptr(), b, h, w, case.alpha, case.beta)
    with torch.cuda.device(DEV):
        for o in (full, again):
            assert lib.oflow_fb_consistency_f32(*args, p(o[0]), p(o[1]), p(o[2]), p(o[3]), st) == 0
        assert lib.oflow_fb_consistency_f32(*args, p(masks_only[0]), p(masks_only[1]), None, None, st) == 0
        assert lib.oflow_fb_consistency_f32(*args, p(fw_only[0]), None, p(fw_only[1]), None, st) == 0
    stream.synchronize()
    for d in (0, 1):
        m = full[d].cpu().numpy()
        assert set(np.unique(m).tolist()) <= {0, 1}, name  # every byte written, 0 or 1
        fc.compare(case, d, m.astype(np.bool_), full[2 + d].cpu().numpy())
    for a, c in zip(full, again):
        assert _same(a, c)
    # NULL optional outputs: the others are the same bits
    assert _same(masks_only[0], full[0]) and _same(masks_only[1], full[1])
    assert _same(fw_only[0], full[0]) and _same(fw_only[1], full[2])


def test_inputs_are_converted_as_warp_converts_them():
    case = fc.BY_NAME["rand-33x65"]
    fw, bw = torch.from_numpy(case.fw).to(DEV), torch.from_numpy(case.bw).to(DEV)
    m, e = fb_consistency(fw, bw, return_error=True)
    # a non-contiguous view of the same values, and float64 inputs (exactly representable: the same fp32 values)
    wide = torch.zeros((1, 2, 33, 130), device=DEV)
    wide[..., ::2] = fw
    view = wide[..., ::2]
    assert not view.is_contiguous()
    m2, e2 = fb_consistency(view, bw.double(), return_error=True)
    assert _same(m2, m) and _same(e2, e)
    g = fw.clone().requires_grad_()
    m3, e3 = fb_consistency(g, bw, return_error=True)
    assert not e3.requires_grad and _same(e3, e) and _same(m3, m)
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        torch.ops.oflow.fb_consistency(fw, bw[:, :, :-1], 0.01, 0.5, False, False)
    out = torch.ops.oflow.fb_consistency(fw[:0], bw[:0], 0.01, 0.5, True, True)
    assert [tuple(t.shape) for t in out] == [(0, 1, 33, 65)] * 4
