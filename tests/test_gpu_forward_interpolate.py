"""forward_interpolate on the GPU (csrc/forward_interpolate.hip): the operator and the C ABI against the float64
brute-force reference (tests/forward_interpolate_cases.py), exactly, on every case; then ``flow_init`` through the
product forward against the oracle model on the GPU (SURVEY §8(c)'s bar, as test_product_matches_oracle_on_gpu holds
the cold path to), and predict.py's ``warm_start`` against the manual chain, byte for byte."""
import ctypes

import numpy as np
import pytest
import torch

import forward_interpolate_cases as fic
from model import RAFT, InputPadder, forward_interpolate, synthetic
from optical_flow import _native
from optical_flow.io.middlebury import MAGIC_NUMBER
from oracle import raft as oraft

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _model(cls):
    m = cls().eval()
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    return m.to(DEV)


@pytest.mark.parametrize("name", fic.CASE_IDS)
def test_op_equals_reference_exactly(name):
    case = fic.BY_NAME[name]
    ref = fic.expected(case)
    flow = torch.from_numpy(case.flow).to(DEV)
    out = torch.ops.oflow.forward_interpolate(flow)
    assert out.shape == flow.shape and out.dtype == torch.float32 and out.device == flow.device
    got = out.cpu().numpy()
    bad = int((got != ref).sum()) if got.shape == ref.shape else -1
    print(f"{name}: {bad} of {ref.size} elements differ from the float64 reference")
    assert np.array_equal(got, ref), (name, bad)
    assert torch.equal(torch.ops.oflow.forward_interpolate(flow), out)  # a second run: the same bits
    # the public function: (B, 2, H, W) and upstream's (2, H, W)
    assert torch.equal(forward_interpolate(flow), out)
    one = forward_interpolate(flow[0])
    assert one.shape == flow.shape[1:] and np.array_equal(one.cpu().numpy(), ref[0])
    # a non-contiguous view of the same values
    view = flow.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert view.shape == flow.shape and (not view.is_contiguous() or min(flow.shape[2:]) == 1)
    assert torch.equal(torch.ops.oflow.forward_interpolate(view), out)


@pytest.mark.parametrize("name", fic.CASE_IDS)
def test_c_abi_on_a_side_stream_equals_reference_exactly(name):
    case = fic.BY_NAME[name]
    ref = fic.expected(case)
    b, _, h, w = case.flow.shape
    flow = torch.from_numpy(case.flow).to(DEV)
    outs = [torch.full_like(flow, float("nan")) for _ in range(2)]
    torch.cuda.synchronize(DEV)  # the inputs are in place before the side stream reads them
    stream = torch.cuda.Stream(DEV)
    lib = _native.load()
    with torch.cuda.device(DEV):
        for out in outs:
            st = lib.oflow_forward_interpolate_f32(flow.data_ptr(), b, h, w, out.data_ptr(),
                                                   ctypes.c_void_p(stream.cuda_stream))
            assert st == 0, lib.oflow_status_string(st)
    stream.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), ref), name
    assert torch.equal(outs[0], outs[1])


def test_op_refuses_what_it_cannot_run():
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        torch.ops.oflow.forward_interpolate(torch.zeros(2, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.oflow.forward_interpolate(torch.zeros(1, 2, 8, 8, device=DEV, dtype=torch.float16))
    flow = torch.randn(1, 2, 8, 8, device=DEV, requires_grad=True)
    out = forward_interpolate(flow)
    assert not out.requires_grad
    assert tuple(torch.ops.oflow.forward_interpolate(torch.zeros(0, 2, 8, 8, device=DEV)).shape) == (0, 2, 8, 8)


@pytest.mark.parametrize("b", [2, 1])
def test_flow_init_matches_oracle_on_gpu(b):
    """The warm-started forward of the default model (split encoders, split update; two pair lanes at B = 2) against
    the oracle model on the GPU given the same flow_init: SURVEY §8(c)'s bar on both outputs."""
    first = [x.to(DEV) for x in synthetic.synthetic_pair(b, 128, 160, seed=41)]
    second = [x.to(DEV) for x in synthetic.synthetic_pair(b, 128, 160, seed=42)]
    prod, orac = _model(RAFT), _model(oraft.RAFT)
    assert prod.update_impl == "split" and prod.encoder_impl == "split" and prod.pair_lanes == 2
    with torch.inference_mode():
        low0, _ = prod(*first, iters=4, test_mode=True)
        init = forward_interpolate(low0)
        assert init.shape == (b, 2, 16, 20) and float(init.abs().max()) > 0
        lo_p, up_p = prod(*second, iters=4, flow_init=init, test_mode=True)
        lo_o, up_o = orac(*second, iters=4, flow_init=init, test_mode=True)
        lo_c, up_c = prod(*second, iters=4, test_mode=True)
    for what, got, ref in (("low", lo_p, lo_o), ("up", up_p, up_o)):
        e = torch.norm(got - ref, dim=1)
        print(f"flow_init B={b} {what}: product vs oracle-on-GPU EPE mean {float(e.mean()):.2e} max {float(e.max()):.2e}")
        assert float(e.mean()) <= 1e-4 and float(e.max()) <= 1e-3, (what, float(e.mean()), float(e.max()))
    assert not torch.equal(lo_p, lo_c) and not torch.equal(up_p, up_c)  # the argument is not ignored


def _flo_bytes(flow: torch.Tensor) -> bytes:
    _, h, w = flow.shape
    return (np.array([MAGIC_NUMBER], np.float32).tobytes() + np.array([w, h], np.int32).tobytes()
            + flow.permute(1, 2, 0).contiguous().cpu().numpy().tobytes())


def test_predict_warm_start_equals_the_manual_chain(tmp_path):
    import predict
    from PIL import Image

    src = tmp_path / "frames"
    src.mkdir()
    frames = []
    for k in range(4):
        img, _ = synthetic.synthetic_pair(1, 128, 160, seed=50 + k)  # (the 4-level pyramid needs >= 128 x 128)
        arr = img[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()
        Image.fromarray(arr, "RGB").save(src / f"f{k}.png")
        frames.append(torch.from_numpy(arr).permute(2, 0, 1).float()[None].to(DEV))
    args = dict(iters=3, visualize=False, eval_mode=True, num_workers=0)
    assert predict.main(str(src), str(tmp_path / "warm"), warm_start=True, **args) == 3
    assert predict.main(str(src), str(tmp_path / "cold"), warm_start=False, **args) == 3
    assert predict.main(str(src), str(tmp_path / "default"), **args) == 3

    model = _model(RAFT)
    prev = None
    differ = 0
    for i in range(3):
        padder = InputPadder(frames[i].shape)
        p0, p1 = padder.pad(frames[i], frames[i + 1])
        with torch.inference_mode():
            init = forward_interpolate(prev) if prev is not None else None
            prev, up_w = model(p0, p1, iters=3, flow_init=init, test_mode=True)
            _, up_c = model(p0, p1, iters=3, test_mode=True)
        warm, cold = _flo_bytes(padder.unpad(up_w)[0]), _flo_bytes(padder.unpad(up_c)[0])
        name = f"{i:06d}.flo"
        assert (tmp_path / "warm" / name).read_bytes() == warm, name
        assert (tmp_path / "cold" / name).read_bytes() == cold, name
        assert (tmp_path / "default" / name).read_bytes() == cold, name
        differ += warm != cold
        if i == 0:
            assert warm == cold  # the first pair starts cold
    assert differ >= 1
