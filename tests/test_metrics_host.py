"""optical_flow.metrics, model.raft.sequence_loss and RAFT's evaluation attributes without a GPU: the CPU path against
the reference's own outputs (tests/golden/metrics_small.npz, gen_metrics_goldens.py), the three new operators' Meta
kernels / argument checks / CPU refusal, and the metric classes' state handling (reset, several updates, state_dict,
a gloo world of 2). The GPU half is tests/test_gpu_metrics.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_cases as mc
from model import RAFT
from model.raft import sequence_loss
from optical_flow import _native, _ops
from optical_flow.metrics import AverageEndPointError, OutlierRatio, end_point_error

META = torch.device("meta")
# the reference sums fp32 terms with ATen's blocked sum, this build in float64: <= (log2 n + 4) * 2^-24 ~ 1.4e-6 apart
# for n <= 2^20 terms; 1e-5 relative is the bound the GPU tests use against the same golden
RTOL_GOLDEN = 1e-5


def _close(got, want, rtol=RTOL_GOLDEN):
    got, want = float(got), float(want)
    assert abs(got - want) <= rtol * abs(want), (got, want)


@pytest.mark.parametrize("name", list(mc.METRIC_CASES))
def test_cpu_metrics_match_the_reference(golden, name):
    g = golden("metrics_small")
    pred, target, valid = mc.metric_case(name)
    np.testing.assert_array_equal(np.stack([mc.checksum(pred), mc.checksum(target)]), g[f"{name}_checksum"])
    _close(end_point_error(pred, target), g[f"{name}_epe_mean"])
    epe_map = end_point_error(pred, target, reduce=False)
    assert tuple(epe_map.shape) == (pred.shape[0], *pred.shape[2:])
    np.testing.assert_array_equal(mc.checksum(epe_map), g[f"{name}_epe_map_checksum"])
    if f"{name}_epe_map" in g:
        np.testing.assert_array_equal(epe_map.numpy(), g[f"{name}_epe_map"])
    aepe, f1 = AverageEndPointError(), OutlierRatio()
    batch_epe, batch_f1 = aepe(pred, target, valid), f1(pred, target, valid)  # forward: update + the batch value
    assert batch_epe.dtype == torch.float32 and batch_epe.dim() == 0
    _close(batch_epe, g[f"{name}_aepe"])
    _close(batch_f1, g[f"{name}_f1"], rtol=1e-7)  # a ratio of two exact counts, rounded to fp32 once
    _close(aepe.compute(), g[f"{name}_aepe"])
    _close(f1.compute(), g[f"{name}_f1"], rtol=1e-7)
    assert int(aepe._state[1]) == int(g[f"{name}_total"])
    _close(AverageEndPointError()(pred, target), g[f"{name}_aepe_novalid"])
    _close(OutlierRatio()(pred, target), g[f"{name}_f1_novalid"], rtol=1e-7)


def test_thresholds_and_several_updates_match_the_reference(golden):
    g = golden("metrics_small")
    pred, target, valid = mc.metric_case("vec3")
    _close(OutlierRatio(abs_threshold=1.0, rel_threshold=0.1)(pred, target, valid), g["vec3_f1_abs1_rel10"], rtol=1e-7)
    aepe, f1 = AverageEndPointError(), OutlierRatio()
    for name in ("vec3", "vec30", "crop"):
        aepe.update(*mc.metric_case(name))
        f1.update(*mc.metric_case(name))
    _close(aepe.compute(), g["multi_aepe"])
    _close(f1.compute(), g["multi_f1"], rtol=1e-7)


def test_valid_kinds_select_the_same_pixels():
    """valid=None keeps everything; a float valid keeps values >= 0.5 ({0, 0.49} out, {0.5, 1} in); a bool valid and
    the equivalent float one agree; a (B, 1, H, W) valid is accepted."""
    pred, target, valid = mc.metric_case("tiny")
    assert sorted(set(valid.reshape(-1).tolist())) == pytest.approx([0.0, 0.49, 0.5, 1.0])
    keep = valid >= 0.5
    epe = torch.norm(pred - target, dim=1)
    m = AverageEndPointError()
    m.update(pred, target, valid)
    assert int(m._state[1]) == int(keep.sum()) and 0 < int(keep.sum()) < keep.numel()
    _close(m.compute(), epe[keep].double().mean(), rtol=1e-6)
    for v in (keep, keep.float(), keep.to(torch.uint8), keep[:, None]):
        other = AverageEndPointError()
        other.update(pred, target, v)
        assert torch.equal(other._state, m._state)
    none = AverageEndPointError()
    none.update(pred, target)
    assert int(none._state[1]) == epe.numel()


def test_empty_selection_is_nan_and_reset_clears():
    pred, target, _ = mc.metric_case("tiny")
    for cls in (AverageEndPointError, OutlierRatio):
        m = cls()
        assert torch.isnan(m.compute())  # nothing seen
        assert torch.isnan(m(pred, target, torch.zeros(2, 5, 7)))  # nothing selected: 0 / 0, as the reference
        assert torch.isnan(m.compute())
        m.update(pred, target)
        assert torch.isfinite(m.compute())
        m.reset()
        assert torch.isnan(m.compute()) and float(m._state.abs().sum()) == 0.0


def test_state_created_under_inference_mode_stays_usable():
    pred, target, valid = mc.metric_case("tiny")
    m = AverageEndPointError()
    with torch.inference_mode():
        m.update(pred, target, valid)
    m.update(pred, target, valid)  # in place, outside inference mode
    once = AverageEndPointError()
    once.update(pred, target, valid)
    assert torch.equal(m._state, 2 * once._state)
    m.reset()
    assert float(m._state.abs().sum()) == 0.0


def test_two_updates_equal_one_update_on_the_concatenation():
    a, b = mc.metric_case("vec3"), mc.metric_case("vec30")
    for cls in (AverageEndPointError, OutlierRatio):
        two, one = cls(), cls()
        two.update(a[0], a[1], a[2])
        two.update(b[0], b[1], b[2].float())
        one.update(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]), torch.cat([a[2], b[2].float()]))
        assert torch.equal(two._state[1:], one._state[1:])  # counts: exact
        _close(two._state[0], one._state[0], rtol=1e-12)  # the float64 sum, in another order
        _close(two.compute(), one.compute(), rtol=1e-7)


def test_other_dims_and_ranks():
    """A ``dim`` other than 1 and inputs that are not 4-D (the reference's torch.norm(dim=...) semantics)."""
    pred, target, valid = mc.metric_case("tiny")
    want_map = torch.norm(pred - target, dim=1)
    p_last, t_last = pred.permute(0, 2, 3, 1).contiguous(), target.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(end_point_error(p_last, t_last, dim=-1, reduce=False), want_map)
    m1, m2 = AverageEndPointError(dim=3), AverageEndPointError()
    m1.update(p_last, t_last, valid)
    m2.update(pred, target, valid)
    assert torch.equal(m1._state, m2._state)
    flat_p, flat_t = p_last.reshape(-1, 2), t_last.reshape(-1, 2)
    assert torch.equal(end_point_error(flat_p, flat_t, reduce=False), want_map.reshape(-1))
    _close(OutlierRatio(dim=1)(flat_p, flat_t, valid.reshape(-1)), OutlierRatio()(pred, target, valid), rtol=0)


@pytest.mark.parametrize("name", list(mc.LOSS_CASES))
def test_cpu_sequence_loss_matches_the_reference(golden, name):
    g = golden("metrics_small")
    preds, gt, valid = mc.loss_case(name)
    np.testing.assert_array_equal(
        np.stack([mc.checksum(gt), mc.checksum(valid)] + [mc.checksum(p) for p in preds]), g[f"{name}_checksum"])
    preds = [p.clone().requires_grad_() for p in preds]
    loss, metrics = sequence_loss(preds, gt, valid, gamma=mc.GAMMA, max_flow=mc.MAX_FLOW)
    assert set(metrics) == {"1px", "3px", "5px"} and all(isinstance(v, float) for v in metrics.values())
    _close(loss.detach(), g[f"{name}_loss"], rtol=1e-6)
    np.testing.assert_allclose([metrics["1px"], metrics["3px"], metrics["5px"]], g[f"{name}_px"], rtol=1e-7)
    loss.backward()
    idx = torch.from_numpy(g[f"{name}_grad_index"])
    for row, i in enumerate(g[f"{name}_grad_preds"]):
        np.testing.assert_allclose(preds[int(i)].grad.reshape(-1)[idx].numpy(), g[f"{name}_grad"][row], rtol=1e-6)
        np.testing.assert_allclose(mc.checksum(preds[int(i)].grad), g[f"{name}_grad_checksum"][row], rtol=1e-6)
    # nothing valid: the three shares are NaN, as the reference's mean of an empty selection
    _, none = sequence_loss([p.detach() for p in preds], gt, torch.zeros_like(valid))
    assert all(np.isnan(v) for v in none.values())


def test_ops_are_registered_with_meta_kernels():
    _native.load()
    for name in ("flow_error_stats", "sequence_loss", "sequence_loss_backward"):
        assert name in _ops.OPS
        assert getattr(torch.ops.oflow, name).default._schema.name == f"oflow::{name}"
    p = torch.empty(3, 2, 37, 130, device=META)
    acc = torch.empty(8, dtype=torch.float64, device=META)
    valid = torch.empty(3, 37, 130, device=META)
    assert tuple(torch.ops.oflow.flow_error_stats(p, p, valid, 3.0, 0.05, 0.0, acc, True).shape) == (3, 37, 130)
    assert torch.ops.oflow.flow_error_stats(p, p, None, 3.0, 0.05, 0.0, acc, False).numel() == 0
    preds = [torch.empty(3, 2, 37, 130, device=META, requires_grad=i != 1) for i in range(3)]
    loss, stats = torch.ops.oflow.sequence_loss(preds, p, valid, [0.64, 0.8, 1.0], 400.0)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    assert tuple(stats.shape) == (8,) and stats.dtype == torch.float64 and not stats.requires_grad
    loss.backward()  # the autograd formula is wired: gradients (as shapes) only where they are needed
    assert preds[0].grad.shape == preds[0].shape and preds[2].grad.shape == preds[2].shape and preds[1].grad is None
    grads = torch.ops.oflow.sequence_loss_backward(torch.empty((), device=META), [q.detach() for q in preds], p, valid,
                                                   [0.64, 0.8, 1.0], 400.0, [1, 0, 1])
    assert [tuple(t.shape) for t in grads] == [(3, 2, 37, 130), (0,), (3, 2, 37, 130)]


def test_op_argument_checks():
    _native.load()
    p = torch.empty(2, 2, 8, 8, device=META)
    acc = torch.empty(8, dtype=torch.float64, device=META)
    with pytest.raises(RuntimeError, match=r"must be equal \(B, 2, H, W\)"):
        torch.ops.oflow.flow_error_stats(p, torch.empty(2, 2, 8, 9, device=META), None, 3.0, 0.05, 0.0, acc, False)
    with pytest.raises(RuntimeError, match=r"must be equal \(B, 2, H, W\)"):
        torch.ops.oflow.flow_error_stats(torch.empty(2, 3, 8, 8, device=META), torch.empty(2, 3, 8, 8, device=META), None,
                                         3.0, 0.05, 0.0, acc, False)
    with pytest.raises(RuntimeError, match="one element per pixel"):
        torch.ops.oflow.flow_error_stats(p, p, torch.empty(2, 8, 7, device=META), 3.0, 0.05, 0.0, acc, False)
    with pytest.raises(RuntimeError, match=r"float64 \[8\]"):
        torch.ops.oflow.flow_error_stats(p, p, None, 3.0, 0.05, 0.0, torch.empty(8, device=META), False)
    valid = torch.empty(2, 8, 8, device=META)
    with pytest.raises(RuntimeError, match="number of flow predictions 0"):
        torch.ops.oflow.sequence_loss([], p, valid, [], 400.0)
    with pytest.raises(RuntimeError, match="number of flow predictions 33"):
        torch.ops.oflow.sequence_loss([p] * 33, p, valid, [1.0] * 33, 400.0)
    with pytest.raises(RuntimeError, match="1 weights for 2 predictions"):
        torch.ops.oflow.sequence_loss([p, p], p, valid, [1.0], 400.0)
    with pytest.raises(RuntimeError, match="gradient flags"):
        torch.ops.oflow.sequence_loss_backward(torch.empty((), device=META), [p, p], p, valid, [1.0, 1.0], 400.0, [1])


def test_raw_ops_refuse_cpu_tensors():
    """Only the raw operators refuse CPU tensors; the metric classes, end_point_error and sequence_loss run the torch
    composition there (the tests above)."""
    _native.load()
    p, valid, acc = torch.zeros(1, 2, 4, 4), torch.ones(1, 4, 4), torch.zeros(8, dtype=torch.float64)
    for call in (
        lambda: torch.ops.oflow.flow_error_stats(p, p, valid, 3.0, 0.05, 0.0, acc, False),
        lambda: torch.ops.oflow.sequence_loss([p], p, valid, [1.0], 400.0),
        lambda: torch.ops.oflow.sequence_loss_backward(torch.ones(()), [p], p, valid, [1.0], 400.0, [1]),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_c_abi_argument_errors_without_launch():
    lib = _native.load()
    fake = 4096
    args = [fake, 64, 32, 8, fake, 64, 32, 8, None, 0, 0, 0, 1, 4, 8, 3.0, 0.05, 0.0, None, fake, fake, None]
    bad = list(args); bad[0] = None
    assert lib.oflow_flow_error_stats_f32(*bad) == -1
    bad = list(args); bad[9] = 1  # a valid kind without a valid pointer
    assert lib.oflow_flow_error_stats_f32(*bad) == -1
    bad = list(args); bad[9] = 7
    assert lib.oflow_flow_error_stats_f32(*bad) == -6
    bad = list(args); bad[13] = 0
    assert lib.oflow_flow_error_stats_f32(*bad) == -2
    bad = list(args); bad[0] = fake + 2
    assert lib.oflow_flow_error_stats_f32(*bad) == -7
    import ctypes
    ptrs = (ctypes.c_void_p * 33)(*([fake] * 33))
    w = (ctypes.c_float * 33)(*([1.0] * 33))
    assert lib.oflow_sequence_loss_f32(ptrs, 33, w, fake, fake, 1, 1, 4, 8, 400.0, fake, fake, fake, None) == -2
    assert lib.oflow_sequence_loss_f32(ptrs, 2, w, fake, fake, 0, 1, 4, 8, 400.0, fake, fake, fake, None) == -6
    assert lib.oflow_sequence_loss_backward_f32(None, ptrs, ptrs, 2, w, fake, fake, 1, 1, 4, 8, 400.0, None) == -1


def test_raft_gains_metrics_without_new_state_dict_keys():
    model = RAFT()
    assert isinstance(model.epe_train, AverageEndPointError) and isinstance(model.epe_val, AverageEndPointError)
    assert isinstance(model.f1_val, OutlierRatio) and (model.f1_val.abs_threshold, model.f1_val.rel_threshold) == (3.0, 0.05)
    keys = set(model.state_dict())
    assert not [k for k in keys if k.startswith(("epe_", "f1_"))]
    assert {k.split(".")[0] for k in keys} == {"fnet", "cnet", "update_block"}
    pred, target, valid = mc.metric_case("tiny")
    model.epe_val.update(pred, target, valid)  # a live state is still neither buffer nor parameter
    assert set(model.state_dict()) == keys and not list(model.epe_val.buffers()) and not list(model.epe_val.parameters())
    state = model.epe_val._state
    model.half().float()
    assert model.epe_val._state is state and state.dtype == torch.float64
    assert callable(model.validation_step)


class _PixelwiseRAFT(RAFT):
    """RAFT with the forward replaced by a per-pixel function of the frames (the product's forward needs the GPU): what
    validation_step does around the forward -- padding, iters_val, test mode, unpadding, the metrics -- runs as is."""

    def forward(self, image0, image1, iters=12, flow_init=None, upsample=True, test_mode=False):
        assert test_mode and image0.shape[-2] % 8 == 0 and image0.shape[-1] % 8 == 0
        self.seen = (iters, tuple(image0.shape))
        return None, (image1[:, :2] - image0[:, 1:3]) * 0.05


def test_validate_on_cpu_tensors():
    from model import synthetic
    from validate import validate

    model = _PixelwiseRAFT(iters_val=7)
    model.train()
    img0, img1 = synthetic.synthetic_pair(2, 130, 132, seed=2)
    gt = torch.from_numpy(synthetic.hash_normal(71, (2, 2, 130, 132), 3.0))
    valid = mc.valid_of("float4", (2, 130, 132), 72)
    batches = [(img0[:1], img1[:1], gt[:1], valid[:1]), (img0[1:], img1[1:], gt[1:], valid[1:])]
    model.epe_val.update(gt, gt + 100.0)  # stale state: validate resets it
    got = validate(model, iter(batches), stage="kitti")
    assert model.seen == (7, (1, 3, 136, 136)) and model.training  # 'kitti' padding, iters_val, mode restored
    flow = (img1[:, :2] - img0[:, 1:3]) * 0.05  # replicate padding and cropping commute with a per-pixel function
    want_epe, want_f1 = AverageEndPointError()(flow, gt, valid), OutlierRatio()(flow, gt, valid)
    assert got["f1_val"] == float(want_f1) and 0.0 < got["f1_val"] < 1.0
    _close(got["epe_val"], want_epe, rtol=1e-6)
    assert int(model.epe_val._state[1]) == int((valid >= 0.5).sum())
    assert all(np.isnan(v) for v in validate(model, [], stage="sintel").values())  # no batch: 0 / 0


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _metric_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        aepe, f1, idle = AverageEndPointError(), OutlierRatio(), AverageEndPointError()
        pred, target, valid = mc.metric_case(("vec3", "vec30")[rank])
        aepe.update(pred, target, valid)
        f1.update(pred, target, valid)
        if rank == 0:
            idle.update(pred, target, valid)  # a metric only one rank ever updated
        local = aepe._state.clone()
        out = (float(aepe.compute()), float(f1.compute()), float(idle.compute()))
        q.put((rank, out, torch.equal(aepe._state, local)))
    finally:
        dist.destroy_process_group()


def test_compute_sums_the_state_over_a_gloo_world_of_two():
    """Each rank updates with a different batch; compute() on both ranks equals the single-process value over both
    batches (dist_reduce_fx="sum"), and leaves the rank's own state as it was."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_metric_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    aepe, f1, idle = AverageEndPointError(), OutlierRatio(), AverageEndPointError()
    for name in ("vec3", "vec30"):
        aepe.update(*mc.metric_case(name))
        f1.update(*mc.metric_case(name))
    idle.update(*mc.metric_case("vec3"))
    want = (float(aepe.compute()), float(f1.compute()), float(idle.compute()))
    for rank, got, state_kept in res:
        assert got == want and state_kept, (rank, got, want)
