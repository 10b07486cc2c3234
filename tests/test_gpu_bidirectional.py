"""RAFT.forward_bidirectional on the GPU: the flow 0 -> 1 and the flow 1 -> 0 from one forward with the feature encoder
run once per image. Its defining semantics is the stacked forward ``model(cat(i0, i1), cat(i1, i0))`` split in halves:
the comparison is bit identity (per-pixel results cross neither pairs nor images), in every configuration ``forward``
has whose kernels are this project's (with ``encoder_impl = "module"`` MIOpen picks fnet's convolution solver by the batch
size, and the comparison is the end-to-end tolerance); gradients against the stacked forward's within test_gpu_raft.py's gradient bound. The counted-encoder test shows
that the shared path does what it claims: fnet sees 2 B images where the stacked forward feeds it 4 B. Then
predict.py's ``bidirectional`` / ``occlusion`` outputs.

Synthetic weights, 3 iterations, 128 x 160 frames (the smallest whose level 3 is still >= 2 px), B = 1 and B = 3 (an odd
lane split of the 6 pairs)."""
import numpy as np
import pytest
import torch

import optical_flow
from model import RAFT, InputPadder, synthetic
from model.extractor import SplitEncoder
from optical_flow import _native
from optical_flow.io.middlebury import MAGIC_NUMBER

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ITERS = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _model(**kw):
    m = RAFT(**kw).eval()
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    return m.to(DEV)


_FRAMES = {}


def _frames(b):
    if b not in _FRAMES:
        _FRAMES[b] = tuple(x.to(DEV) for x in synthetic.synthetic_pair(b, 128, 160, seed=70 + b))
    return _FRAMES[b]


def _stack(i0, i1):
    return torch.cat([i0, i1], dim=0), torch.cat([i1, i0], dim=0)


def _same(got, ref, what, exact=True):
    """Bit identity; with ``exact=False`` the project's end-to-end tolerance (mean EPE <= 1e-4 px, max
    <= 1e-3 px), for the one configuration whose convolutions are not this project's kernels."""
    assert got.shape == ref.shape, what
    e = torch.norm(got.float() - ref.float(), dim=1)
    print(f"{what}: EPE vs the reference forward mean {float(e.mean()):.2e} max {float(e.max()):.2e}, "
          f"bit-identical {torch.equal(got, ref)}")
    if exact:
        assert torch.equal(got, ref), what
    else:
        assert float(e.mean()) <= 1e-4 and float(e.max()) <= 1e-3, (what, float(e.mean()), float(e.max()))


# encoder_impl "module" runs fnet's convolutions through MIOpen, which picks its solver by the batch size: fnet's bits
# then depend on whether it sees B or 2 B images (measured: max EPE 2e-6 px), so that configuration alone is held to the
# end-to-end tolerance instead of bit identity (DESIGN.md §4 "Bidirectional forward"). Every native path is exact.
INEXACT = {"module-encoders"}
CONFIGS = {
    "default": ({}, {}),
    "alternate_corr": ({"alternate_corr": True}, {}),
    "module-encoders": ({}, {"encoder_impl": "module"}),
    "one-lane": ({}, {"pair_lanes": 1}),
    "patch-matrix-stem": ({}, {"stem_from_image": False}),
    "one-fnet-stream": ({}, {"fnet_streams": False, "stem_from_image": False}),
}


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_equals_the_stacked_forward(config, b):
    ctor, attrs = CONFIGS[config]
    exact = config not in INEXACT
    model = _model(**ctor)
    for k, v in attrs.items():
        assert hasattr(model, k)
        setattr(model, k, v)
    i0, i1 = _frames(b)
    s0, s1 = _stack(i0, i1)
    init_fw = torch.from_numpy(synthetic.hash_normal(91, (b, 2, 16, 20), 1.5)).to(DEV)
    init_bw = torch.from_numpy(synthetic.hash_normal(92, (b, 2, 16, 20), 1.5)).to(DEV)
    zeros = torch.zeros_like(init_fw)
    with torch.inference_mode():
        # test mode, cold
        (lo_f, up_f), (lo_b, up_b) = model.forward_bidirectional(i0, i1, iters=ITERS, test_mode=True)
        lo_s, up_s = model(s0, s1, iters=ITERS, test_mode=True)
        assert lo_f.shape == (b, 2, 16, 20) and up_b.shape == (b, 2, 128, 160)
        for got, ref, what in ((lo_f, lo_s[:b], "low fw"), (lo_b, lo_s[b:], "low bw"), (up_f, up_s[:b], "up fw"),
                               (up_b, up_s[b:], "up bw")):
            _same(got, ref, f"{config} B={b} cold {what}", exact)
        assert not torch.equal(up_f, up_b)
        # test mode with flow_init: both, and either one alone (None = zeros)
        for name, pair, stacked in (("both", (init_fw, init_bw), torch.cat([init_fw, init_bw])),
                                    ("fw only", (init_fw, None), torch.cat([init_fw, zeros])),
                                    ("bw only", (None, init_bw), torch.cat([zeros, init_bw]))):
            (lo_f2, up_f2), (lo_b2, up_b2) = model.forward_bidirectional(i0, i1, iters=ITERS, flow_init=pair, test_mode=True)
            lo_s2, up_s2 = model(s0, s1, iters=ITERS, flow_init=stacked, test_mode=True)
            _same(torch.cat([lo_f2, lo_b2]), lo_s2, f"{config} B={b} init {name} low", exact)
            _same(torch.cat([up_f2, up_b2]), up_s2, f"{config} B={b} init {name} up", exact)
            # an initialiser is not ignored, and it moves its own direction only (the pairs are independent)
            assert not torch.equal(up_f2 if pair[0] is not None else up_b2, up_f if pair[0] is not None else up_b), name
            if exact:
                assert torch.equal(up_f2, up_f) == (pair[0] is None) and torch.equal(up_b2, up_b) == (pair[1] is None), name
        (_, up_f3), (_, up_b3) = model.forward_bidirectional(i0, i1, iters=ITERS, flow_init=(None, None), test_mode=True)
        _same(torch.cat([up_f3, up_b3]), torch.cat([up_f, up_b]), f"{config} B={b} init (None, None)", exact)
        # list mode: every iteration's prediction
        preds_f, preds_b = model.forward_bidirectional(i0, i1, iters=ITERS)
        preds_s = model(s0, s1, iters=ITERS)
        assert len(preds_f) == len(preds_b) == len(preds_s) == ITERS
        for k in range(ITERS):
            _same(torch.cat([preds_f[k], preds_b[k]]), preds_s[k], f"{config} B={b} list {k}", exact)
        _same(torch.cat([preds_f[-1], preds_b[-1]]), torch.cat([up_f, up_b]), f"{config} B={b} list vs test mode", exact)
    model.check_range(DEV)


def test_gradients_equal_the_stacked_forward():
    """Under autograd (module encoders, canonical correlation): the gradient of the sum of both directions' last
    predictions with respect to fnet's stem weight, against the stacked forward's, within test_gpu_raft.py's bound for
    gradient comparisons (relative Frobenius error <= 1e-3)."""
    i0, i1 = _frames(1)
    s0, s1 = _stack(i0, i1)
    model = _model()
    model.train()
    for m in model.modules():  # eval-mode batch norm, as test_raft_training_gradients_match_oracle
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    keys = ("fnet.conv1.weight", "fnet.layer3.1.conv2.weight", "cnet.conv2.weight", "update_block.gru.convz1.weight")
    params = dict(model.named_parameters())
    preds_f, preds_b = model.forward_bidirectional(i0, i1, iters=ITERS)
    assert preds_f[-1].requires_grad and preds_b[-1].requires_grad
    (preds_f[-1].sum() + preds_b[-1].sum()).backward()
    got = {k: params[k].grad.detach().clone() for k in keys}
    model.zero_grad(set_to_none=True)
    preds_s = model(s0, s1, iters=ITERS)
    preds_s[-1].sum().backward()
    for k in keys:
        ref = params[k].grad
        rel = float((got[k] - ref).norm() / ref.norm())
        print(f"grad {k}: relative error vs the stacked forward {rel:.2e}")
        assert float(ref.norm()) > 0 and rel <= 1e-3, (k, rel)
    e = torch.norm(torch.cat([preds_f[-1], preds_b[-1]]).detach() - preds_s[-1].detach(), dim=1)
    assert float(e.mean()) <= 1e-4 and float(e.max()) <= 1e-3


@pytest.mark.parametrize("b", [1, 3])
def test_fnet_runs_once_per_image(b, monkeypatch):
    """SplitEncoder.__call__ image totals: the shared path feeds fnet 2 B images, the stacked forward 4 B; cnet 2 B in
    both."""
    model = _model()
    i0, i1 = _frames(b)
    counts = {}
    real = SplitEncoder.__call__

    def counting(self, x, *args, **kw):
        n = sum(int(t.shape[0]) for t in x) if isinstance(x, (tuple, list)) else int(x.shape[0])
        key = "fnet" if self.enc is model.fnet else "cnet" if self.enc is model.cnet else "other"
        counts[key] = counts.get(key, 0) + n
        return real(self, x, *args, **kw)

    monkeypatch.setattr(SplitEncoder, "__call__", counting)
    for streams in (True, False):
        model.fnet_streams = streams
        with torch.inference_mode():
            counts.clear()
            model.forward_bidirectional(i0, i1, iters=1, test_mode=True)
            assert counts == {"fnet": 2 * b, "cnet": 2 * b}, (streams, counts)
            counts.clear()
            model(*_stack(i0, i1), iters=1, test_mode=True)
            assert counts == {"fnet": 4 * b, "cnet": 2 * b}, (streams, counts)


def test_dropout_runs_the_stacked_forward():
    """fnet in train mode with dropout > 0: an image's features depend on its place in the batch, so the shared path
    would change the semantics; forward_bidirectional then is the stacked forward, random draws included."""
    model = _model(dropout=0.5)
    model.train()
    i0, i1 = _frames(1)
    with torch.no_grad():
        torch.manual_seed(5)
        preds_f, preds_b = model.forward_bidirectional(i0, i1, iters=1)
        torch.manual_seed(5)
        preds_s = model(*_stack(i0, i1), iters=1)
    assert torch.equal(torch.cat([preds_f[0], preds_b[0]]), preds_s[0])


def test_range_guard_raises_as_forward_does():
    i0, i1 = _frames(1)
    good = _model()
    with torch.inference_mode():
        ref = good.forward_bidirectional(i0, i1, iters=ITERS, test_mode=True)
    bad = _model()
    bad.range_guard = "sync"
    with torch.inference_mode():
        with pytest.raises(RuntimeError, match="fp16 range"):
            bad(i0 * 1e6, i1 * 1e6, iters=ITERS, test_mode=True)
        with pytest.raises(RuntimeError, match="fp16 range"):
            bad.forward_bidirectional(i0 * 1e6, i1 * 1e6, iters=ITERS, test_mode=True)
        got = good.forward_bidirectional(i0, i1, iters=ITERS, test_mode=True)  # flag cleared: a valid forward runs
    assert torch.equal(got[0][1], ref[0][1]) and torch.equal(got[1][1], ref[1][1])
    # deferred (the default): the snapshot of a bidirectional forward reports it
    lazy = _model()
    with torch.inference_mode():
        lazy.forward_bidirectional(i0 * 1e6, i1 * 1e6, iters=ITERS, test_mode=True)
        assert lazy.last_range_snapshot.overflowed()
        with pytest.raises(RuntimeError, match="fp16 range"):
            lazy.check_range(DEV)


# ---------------------------------------------------------------------------------------------------------- predict.py
def _flo_bytes(flow: torch.Tensor) -> bytes:
    _, h, w = flow.shape
    return (np.array([MAGIC_NUMBER], np.float32).tobytes() + np.array([w, h], np.int32).tobytes()
            + flow.permute(1, 2, 0).contiguous().cpu().numpy().tobytes())


def _read_flo(path) -> torch.Tensor:
    raw = path.read_bytes()
    w, h = np.frombuffer(raw[4:12], np.int32)
    return torch.from_numpy(np.frombuffer(raw[12:], np.float32).reshape(h, w, 2).copy()).permute(2, 0, 1)


def test_predict_bidirectional_and_occlusion(tmp_path):
    import predict
    from PIL import Image

    src = tmp_path / "frames"
    src.mkdir()
    frames = []
    for k in range(3):
        img, _ = synthetic.synthetic_pair(1, 128, 160, seed=80 + k)
        arr = img[0].permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()
        Image.fromarray(arr, "RGB").save(src / f"f{k}.png")
        frames.append(torch.from_numpy(arr).permute(2, 0, 1).float()[None].to(DEV))
    args = dict(iters=ITERS, visualize=False, eval_mode=True, num_workers=0)
    assert predict.main(str(src), str(tmp_path / "plain"), **args) == 2
    assert predict.main(str(src), str(tmp_path / "bidir"), bidirectional=True, **args) == 2
    assert predict.main(str(src), str(tmp_path / "occ"), occlusion=True, **args) == 2
    assert predict.main(str(src), str(tmp_path / "occ_warm"), occlusion=True, warm_start=True, **args) == 2

    def listing(name):
        return sorted(p.name for p in (tmp_path / name).iterdir())

    # without the flags: the files and bytes of before (the plain forward's flow, as test_gpu_forward_interpolate.py
    # holds predict.main to)
    assert listing("plain") == ["000000.flo", "000001.flo"]
    assert listing("bidir") == ["000000.flo", "000000_bw.flo", "000001.flo", "000001_bw.flo"]
    extra = [f"{i:06d}_{s}" for i in range(2) for s in ("bw.flo", "occ.png", "occ_bw.png")]
    assert listing("occ") == sorted(["000000.flo", "000001.flo"] + extra) and len(extra) == 6
    assert listing("occ_warm") == listing("occ")
    model = _model()
    for i in range(2):
        padder = InputPadder(frames[i].shape)
        p0, p1 = padder.pad(frames[i], frames[i + 1])
        with torch.inference_mode():
            _, up = model(p0, p1, iters=ITERS, test_mode=True)
            _, up_rev = model(p1, p0, iters=ITERS, test_mode=True)
            (_, bi_f), (_, bi_b) = model.forward_bidirectional(p0, p1, iters=ITERS, test_mode=True)
        assert (tmp_path / "plain" / f"{i:06d}.flo").read_bytes() == _flo_bytes(padder.unpad(up)[0])
        for run in ("bidir", "occ"):
            assert (tmp_path / run / f"{i:06d}.flo").read_bytes() == _flo_bytes(padder.unpad(bi_f)[0]), (run, i)
            assert (tmp_path / run / f"{i:06d}_bw.flo").read_bytes() == _flo_bytes(padder.unpad(bi_b)[0]), (run, i)
            assert (tmp_path / run / f"{i:06d}_bw.flo").stat().st_size == 12 + 128 * 160 * 8
        # the reverse flow is the reversed pair's plain prediction, and the forward flow the plain one
        fw_file, bw_file = (_read_flo(tmp_path / "occ" / f"{i:06d}{s}.flo").to(DEV) for s in ("", "_bw"))
        _same(bw_file[None], padder.unpad(up_rev), f"predict pair {i} _bw.flo vs the reversed pair's forward")
        _same(fw_file[None], padder.unpad(up), f"predict pair {i} .flo vs the plain forward")
        # the masks decode to the operator's output on the written flows
        m_fw, m_bw = optical_flow.fb_consistency(fw_file[None], bw_file[None], both=True)
        for suffix, m in (("occ", m_fw), ("occ_bw", m_bw)):
            png = Image.open(tmp_path / "occ" / f"{i:06d}_{suffix}.png")
            assert png.mode == "L" and png.size == (160, 128)
            arr = np.array(png)
            assert set(np.unique(arr).tolist()) <= {0, 255}
            assert np.array_equal(arr == 255, m[0, 0].cpu().numpy()), (i, suffix)
            print(f"pair {i} {suffix}: {float(m.float().mean()):.3f} occluded")
    # warm start: the first pair starts cold in both directions; the second pair's forward direction is warm-started
    # (differs), its reverse direction starts cold from the same forward batch
    assert (tmp_path / "occ_warm" / "000000.flo").read_bytes() == (tmp_path / "occ" / "000000.flo").read_bytes()
    assert (tmp_path / "occ_warm" / "000000_bw.flo").read_bytes() == (tmp_path / "occ" / "000000_bw.flo").read_bytes()
    assert (tmp_path / "occ_warm" / "000001.flo").read_bytes() != (tmp_path / "occ" / "000001.flo").read_bytes()
    assert (tmp_path / "occ_warm" / "000001_bw.flo").read_bytes() == (tmp_path / "occ" / "000001_bw.flo").read_bytes()
