"""Augmentation on the GPU (csrc/augment.hip through data.augmentor.*.augment_batch): every case of
tests/augment_cases.py, dense and sparse, equals the NumPy restatement exactly on all four outputs -- everything is
integer or once-rounded IEEE arithmetic in a fixed order, so zero tolerance is the criterion; a second run gives the
same bits; an augmented batch goes through RAFT.training_step."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import augment_cases as ac
from data.augmentor import FlowAugmentor, SparseFlowAugmentor
from model import RAFT, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OUTPUTS = ("img1", "img2", "flow", "valid")


def _gpu_run(case):
    (img1, img2, flow, valid), want, _ = ac.expected(case.name)
    t = lambda a: torch.from_numpy(a.copy()).to(DEV)  # noqa: E731
    aug = (SparseFlowAugmentor if case.sparse else FlowAugmentor)(case.crop)
    args = (t(img1), t(img2), t(flow), t(valid) if case.sparse else None)
    return aug, args, want


@pytest.mark.parametrize("name", [c.name for c in ac.CASES])
def test_augment_batch_equals_restatement(name):
    case = ac.BY_NAME[name]
    aug, args, want = _gpu_run(case)
    got = aug.augment_batch(*args, params=case.params)
    again = aug.augment_batch(*args, params=case.params)
    b, (ch, cw) = len(case.params), case.crop
    shapes = ((b, 3, ch, cw), (b, 3, ch, cw), (b, 2, ch, cw), (b, ch, cw))
    for what, g, g2, w, shape in zip(OUTPUTS, got, again, want, shapes):
        assert g.device == args[0].device and g.dtype == torch.float32 and g.is_contiguous(), (name, what)
        assert tuple(g.shape) == shape, (name, what)
        diff = g.cpu().numpy() != w
        print(f"{name}/{what}: {int(diff.sum())} of {diff.size} elements differ")
        assert np.array_equal(g.cpu().numpy(), w), (name, what, int(diff.sum()))
        assert torch.equal(g, g2), (name, what, "a second run differs")


def test_operator_on_a_side_stream_and_non_contiguous_inputs():
    case = ac.BY_NAME["batch3"]
    aug, (img1, img2, flow, _), want = _gpu_run(case)
    wide = torch.zeros(3, 120, 200, 3, dtype=torch.uint8, device=DEV)
    wide[:, :, 20:180] = img1
    view = wide[:, :, 20:180]
    assert not view.is_contiguous()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = aug.augment_batch(view, img2, flow, params=case.params)
    side.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


def test_operator_argument_errors_on_the_device():
    case = ac.BY_NAME["one_rect"]
    aug, (img1, img2, flow, _), _ = _gpu_run(case)
    from data.augmentor import AugmentParams

    rows = AugmentParams.to_tensor(case.params)
    op = torch.ops.oflow.augment_batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(img1, img2, flow, None, rows, 64, 96)  # the parameter rows are still on the host
    with pytest.raises(RuntimeError, match="augment_batch"):
        op(img1, img2, flow, None, rows.to(DEV)[:, :-1], 64, 96)
    with pytest.raises(ValueError, match="leaves"):
        aug.augment_batch(img1, img2, flow, params=[ac.P(y0=57, x0=0)])
    empty = op(img1[:0], img2[:0], flow[:0], None, rows.to(DEV)[:0], 64, 96)
    assert [tuple(o.shape) for o in empty] == [(0, 3, 64, 96), (0, 3, 64, 96), (0, 2, 64, 96), (0, 64, 96)]


def _train_once(model, batch):
    model.zero_grad(set_to_none=True)
    loss = model.training_step(batch, 0)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def test_training_step_on_an_augmented_batch():
    """An augmented batch of 2 is what RAFT.training_step takes. The model refuses frames under 128 x 128 (its fourth
    pyramid level would be under 2 pixels, whatever ``corr_levels`` says: CorrBlock is built with 4 levels, as in the
    reference), so the 64 x 96 crops are padded to 128 x 128 first -- frames by replication, flow and valid with zeros,
    so the padding carries no loss -- and a second batch is cropped at 128 x 128 and goes in as it is."""
    rng = np.random.default_rng(5)
    b, ht, wd = 2, 150, 180
    img0, img1 = synthetic.synthetic_pair(b, ht, wd, seed=3)  # (B, 3, H, W) fp32 levels in [0, 255]
    u8 = lambda x: x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
    flow = torch.from_numpy((rng.standard_normal((b, 2, ht, wd)) * 3).astype(np.float32)).to(DEV)
    model = RAFT(iters=2)
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(DEV).train()
    np.random.seed(11)
    torch.manual_seed(11)
    for ch, cw in ((64, 96), (128, 128)):
        batch = FlowAugmentor((ch, cw)).augment_batch(u8(img0), u8(img1), flow)
        assert [tuple(t.shape) for t in batch] == [(b, 3, ch, cw), (b, 3, ch, cw), (b, 2, ch, cw), (b, ch, cw)]
        assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in batch)
        assert float(batch[0].min()) >= 0 and float(batch[0].max()) <= 255 and float(batch[3].min()) == 1.0
        if (ch, cw) != (128, 128):
            pad = (0, 128 - cw, 0, 128 - ch)
            fr = [torch.nn.functional.pad(t, pad, mode="replicate") for t in batch[:2]]
            batch = (fr[0], fr[1], torch.nn.functional.pad(batch[2], pad), torch.nn.functional.pad(batch[3], pad))
            assert float(batch[3].sum()) == b * ch * cw
        _train_once(model, batch)
