"""The flow head with its 256 -> 2 output conv folded into conv1's epilogue (oflow_conv_s32 with
OFLOW_EPI_FLOW_HEAD, csrc/conv_s32.hip; oflow_flow_head_finish_f32, csrc/s32_io.hip; FLOW_HEAD_MODE "fused").

Reference: ``coords + F.conv2d(relu(conv1(x)), w2, b2, padding=1)`` in float64 on the exact fp32 relu(conv1) values
(the unfused conv1 with an fp32 destination: the same MFMAs in the same order). Tolerance: the one
tests/test_gpu_conv_s32.py::test_flow_head2_matches_fp64 uses for an fp32 FMA chain of this length,
2e-6 * sum|x||w| + 1e-6 + 2^-23 |ref|.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from model import RAFT, InputPadder, synthetic
from optical_flow import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
V = N.S32Slice

# a one-pixel image, a tile edge at column 32, ragged rows and columns, KITTI's grid
SHAPES = [(1, 1, 1), (2, 5, 33), (1, 13, 70), (1, 47, 156)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    N.load()


_CASES = {}


def _case(b, h, w):
    """Inputs of one shape, built once: S32 net (128 channels), conv1 / conv2 weights, random coords, and the exact
    relu(conv1) values from the unfused conv."""
    key = (b, h, w)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * b + 7 * h + w)
        x = (torch.randn(b, 128, h, w, generator=g) * 1.5).to(DEV)
        w1 = (torch.randn(256, 128, 3, 3, generator=g) / math.sqrt(128 * 9)).to(DEV)
        b1 = (torch.randn(256, generator=g) * 0.2).to(DEV)
        w2 = (torch.randn(2, 256, 3, 3, generator=g) / 48.0).to(DEV)
        b2 = torch.randn(2, generator=g).to(DEV)
        coords = (torch.randn(b, 2, h, w, generator=g) * 3.0).to(DEV)
        xs = N.s32_from_f32(x)
        cw = N.ConvWeights(w1, b1, 256)
        relu1 = torch.empty(b, 256, h, w, device=DEV)
        N.conv_s32(V(xs), cw, 64, "relu", f32=relu1)
        torch.cuda.synchronize()
        _CASES[key] = dict(xs=xs, cw=cw, w2=w2, b2=b2, w2r=N.flow_head_fused_weights(w2), coords=coords, relu1=relu1)
    return _CASES[key]


def _fused(c, bn, coords, partial=None, flow0=None, flow1=None):
    b, h, w = c["xs"].shape[:3]
    if partial is None:
        partial = N.flow_head_partial_empty(b, h, w, DEV)
    N.conv_s32_flow_head(V(c["xs"]), c["cw"], bn, c["w2r"], partial)
    N.flow_head_finish(partial, c["b2"], coords, flow0, flow1)
    torch.cuda.synchronize()
    return coords


@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_fused_flow_head_matches_fp64(b, h, w, bn):
    c = _case(b, h, w)
    r = c["relu1"].double()
    ref = c["coords"].double() + F.conv2d(r, c["w2"].double(), c["b2"].double(), padding=1)
    bound = F.conv2d(r.abs(), c["w2"].double().abs(), None, padding=1)
    got = _fused(c, bn, c["coords"].clone())
    err = (got.double() - ref).abs()
    tol = 2e-6 * bound + 1e-6 + 2.0 ** -23 * ref.abs()
    print(f"fused flow head {b}x{h}x{w} bn {bn}: max |d| {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), float(err.max())


@pytest.mark.parametrize("b,h,w", SHAPES + [(3, 55, 128)])
def test_block_size_and_weight_staging_are_bit_identical(b, h, w):
    """64-channel blocks (LDS-staged weights) and 128-channel blocks (register-direct weights) give the same coords1
    and the same partial sums, bit for bit; (3, 55, 128) is a grid over the 16384-pixel small-grid threshold."""
    c = _case(b, h, w)
    p64, p128 = (N.flow_head_partial_empty(b, h, w, DEV) for _ in range(2))
    c64 = _fused(c, 64, c["coords"].clone(), p64)
    c128 = _fused(c, 128, c["coords"].clone(), p128)
    assert torch.equal(p64, p128)
    assert torch.equal(c64, c128)


@pytest.mark.parametrize("b,h,w", SHAPES)
def test_finish_writes_flow_prep_bytes(b, h, w):
    """The flow channels of hx / rhx after the finish kernel = what flow_prep writes for the updated coords1."""
    c = _case(b, h, w)
    hx, rhx, hx_ref, rhx_ref = (N.s32_empty(b, h, w, 8, DEV, zero=True) for _ in range(4))
    coords = _fused(c, 64, c["coords"].clone(), None, (V(hx), 254), (V(rhx), 254))
    N.flow_prep(coords, None, (V(hx_ref), 254), (V(rhx_ref), 254))
    torch.cuda.synchronize()
    for got, ref in ((hx, hx_ref), (rhx, rhx_ref)):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert bool((hx[..., 7, :, 30:].float().abs().sum() > 0))  # (the flow channels were written at all)


@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_dirty_buffers(b, h, w, bn):
    """NaN-filled partial sums and NaN around coords: two calls give finite, identical results (every value read was
    written on that call), and nothing outside the image's elements is written."""
    c = _case(b, h, w)
    outs = []
    for _ in range(2):
        pbig = torch.full((N.FLOW_HEAD_SLABS * b * 18 * h * w + 64,), float("nan"), device=DEV)
        partial = pbig[32:-32].view(N.FLOW_HEAD_SLABS, b, 18, h, w)
        cbig = torch.full((b + 2, 2, h, w), float("nan"), device=DEV)
        coords = cbig[1 : b + 1]
        coords.copy_(c["coords"])
        assert coords.is_contiguous()
        _fused(c, bn, coords, partial)
        assert bool(torch.isfinite(coords).all()) and bool(torch.isfinite(partial).all())
        assert bool(torch.isnan(pbig[:32]).all()) and bool(torch.isnan(pbig[-32:]).all())
        assert bool(torch.isnan(cbig[0]).all()) and bool(torch.isnan(cbig[-1]).all())
        outs.append((coords.clone(), partial.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_argument_errors():
    b, h, w = 2, 5, 33
    c = _case(b, h, w)
    partial = N.flow_head_partial_empty(b, h, w, DEV)
    x = V(c["xs"])
    with pytest.raises(RuntimeError):  # null partial buffer
        N.conv_s32_flow_head(x, c["cw"], 64, c["w2r"], None)
    with pytest.raises(RuntimeError):  # wrong slab count
        N.conv_s32_flow_head(x, c["cw"], 64, c["w2r"], torch.empty(3, b, 18, h, w, device=DEV))
    g = torch.Generator().manual_seed(3)
    cw128 = N.ConvWeights((torch.randn(128, 128, 3, 3, generator=g) * 0.05).to(DEV), None, 128)
    with pytest.raises(RuntimeError):  # N != 256
        N.conv_s32_flow_head(x, cw128, 64, c["w2r"], partial)
    with pytest.raises(RuntimeError):  # a channel block the epilogue is not built for
        N.conv_s32_flow_head(x, c["cw"], 32, c["w2r"], partial)
    wide = torch.zeros(b, 2, h, 2 * w, device=DEV)
    with pytest.raises(RuntimeError):  # non-contiguous coords1
        N.flow_head_finish(partial, c["b2"], wide[..., :w])
    with pytest.raises(RuntimeError):  # wrong slab count
        N.flow_head_finish(torch.empty(3, b, 18, h, w, device=DEV), c["b2"], torch.zeros(b, 2, h, w, device=DEV))
    # the raw entry reports a null partial buffer without a launch
    lib = N.load()
    st = lib.oflow_flow_head_finish_f32(None, 4, c["b2"].data_ptr(), b, h, w, partial.data_ptr(), None, 0, None, 0, None)
    assert st == -1
    torch.cuda.synchronize()


def _model():
    m = RAFT().eval()
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    return m.to(DEV)


@pytest.fixture(scope="module")
def raft_runs():
    """3 pairs at 440 x 1024 (55 x 128 grid, 21120 px: over the flow-head threshold, lanes of 7040 / 14080 px), 3
    iterations: 'tiled' and 'fused' on two lanes, 'fused' on one lane and through GraphedRAFT."""
    from model.graph import GraphedRAFT

    img0, img1 = synthetic.synthetic_pair(3, 440, 1024, seed=9)
    p0, p1 = img0.to(DEV), img1.to(DEV)
    assert 3 * 55 * 128 >= N.FLOW_HEAD2_MAX_PIXELS
    model = _model()
    out = {}
    with torch.inference_mode():
        for mode, lanes in (("tiled", 2), ("fused", 2), ("fused", 1)):
            model.update_block.flow_head_mode = mode
            model.pair_lanes = lanes
            out[(mode, lanes)] = model(p0, p1, iters=3, test_mode=True)
        model.pair_lanes = 2
        g = GraphedRAFT(model, p0, p1, iters=3)
        out["graph"] = tuple(t.clone() for t in g(p0, p1))
    torch.cuda.synchronize()
    return out


def test_raft_fused_matches_tiled(raft_runs):
    """Equivalent arithmetic in another summation order: mean EPE <= 1e-5 px on the low-res and the upsampled flow."""
    for k in (0, 1):
        e = torch.norm(raft_runs[("fused", 2)][k] - raft_runs[("tiled", 2)][k], dim=1)
        print(f"fused vs tiled [{'low' if k == 0 else 'up'}]: EPE mean {float(e.mean()):.2e} max {float(e.max()):.2e}")
        assert float(e.mean()) <= 1e-5


def test_raft_fused_lanes_bit_identical(raft_runs):
    a, c = raft_runs[("fused", 2)], raft_runs[("fused", 1)]
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_raft_fused_graph_equals_eager(raft_runs):
    a, c = raft_runs[("fused", 2)], raft_runs["graph"]
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
