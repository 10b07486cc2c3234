"""In-process A/B of the fused metrics / sequence-loss kernels (csrc/flow_metrics.hip) against the reference's torch
composition on the same GPU, at the shapes a user runs:

  (a) one metric update on Sintel x 8: pred / target (8, 2, 436, 1024), a float valid. Fused: flow_error_stats (one
      pass gives the EPE and the F1 statistics). Composition: AverageEndPointError.update and OutlierRatio.update as
      the reference writes them (optical_flow/metrics/epe.py:24-37, f1.py:34-50), whose boolean index synchronises.
  (b) sequence_loss forward + backward on 12 predictions (8, 2, 368, 496) (the training crop), fused op + native
      backward against the composition (methods/raft/model/raft.py:239-258) under autograd.

Each leg queues its launches behind a spin kernel (as bench.py's legs do) and brackets REPS calls with one event pair;
the composition's own host synchronisations stay in its time. Prints one JSON line per leg with the times, the
algorithmic bytes and the achieved TB/s of the fused kernels (peak HBM 8 TB/s, measured streaming read ~6.3 TB/s)."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "torch-optical-flow_amd"), os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from model import synthetic  # noqa: E402
from model.raft import sequence_loss, sequence_loss_torch  # noqa: E402
from optical_flow import _native  # noqa: E402
from optical_flow.metrics import _stats  # noqa: E402

DEV = torch.device("cuda", 0)
SPIN_CYCLES = 40_000_000
REPS, ROUNDS = 20, 5


def timed(fn, reps=REPS):
    """Median over ROUNDS of (one event pair around ``reps`` calls queued behind a spin kernel) / reps, in us."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(SPIN_CYCLES)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out)


def leg_metrics():
    b, h, w = 8, 436, 1024
    target = torch.from_numpy(synthetic.hash_normal(1, (b, 2, h, w), 20.0)).to(DEV)
    pred = target + torch.from_numpy(synthetic.hash_normal(2, (b, 2, h, w), 3.0)).to(DEV)
    valid = torch.from_numpy((synthetic.hash_uniform(3, b * h * w) < 0.7).astype("float32")).view(b, h, w).to(DEV)
    fused_state, torch_state = _stats.new_state(DEV), _stats.new_state(DEV)

    def fused():
        _stats.accumulate(fused_state, pred, target, valid, 1, 3.0, 0.05)

    def composition_epe():  # epe.py:29-37
        epe = torch.norm(pred - target, p=2, dim=1).view(-1)
        epe = epe[valid.view(-1) >= 0.5]
        torch_state[0] += epe.sum()
        torch_state[1] += epe.numel()

    def composition_f1():  # f1.py:37-50
        epe = torch.norm(pred - target, p=2, dim=1).view(-1)
        mag = torch.norm(target, p=2, dim=1).view(-1)
        outliers = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
        outliers = outliers[valid.view(-1) >= 0.5]
        torch_state[2] += outliers.sum()

    with torch.inference_mode():
        t_fused, t_epe, t_f1 = timed(fused), timed(composition_epe), timed(composition_f1)
        fused_state.zero_(), torch_state.zero_()
        fused(), composition_epe(), composition_f1()
        same = (fused_state[1:3] == torch_state[1:3]).all().item()
        rel = abs(fused_state[0].item() - torch_state[0].item()) / torch_state[0].item()
    nbytes = b * h * w * 20
    print(json.dumps({"leg": "metrics_update", "shape": [b, 2, h, w], "fused_us": round(t_fused[0], 2), "fused_min_us": round(t_fused[1], 2),
                      "composition_epe_us": round(t_epe[0], 2), "composition_f1_us": round(t_f1[0], 2),
                      "bytes": nbytes, "bytes_formula": "B*H*W*(2*8 + 4)", "fused_TBps": round(nbytes / (t_fused[0] * 1e-6) / 1e12, 3),
                      "counts_equal": bool(same), "sum_rel_diff": rel}), flush=True)


def leg_sequence_loss():
    n, b, h, w = 12, 8, 368, 496
    gt = torch.from_numpy(synthetic.hash_normal(11, (b, 2, h, w), 20.0)).to(DEV)
    preds = [(gt + torch.from_numpy(synthetic.hash_normal(20 + i, (b, 2, h, w), 4.0)).to(DEV)).requires_grad_() for i in range(n)]
    valid = torch.from_numpy((synthetic.hash_uniform(4, b * h * w) < 0.7).astype("float32")).view(b, h, w).to(DEV)
    weights = [0.8 ** (n - i - 1) for i in range(n)]

    def fused():
        loss, _ = _native.ops().sequence_loss(preds, gt, valid, weights, 400.0)
        loss.backward()

    def fused_forward():
        with torch.no_grad():
            _native.ops().sequence_loss(preds, gt, valid, weights, 400.0)

    def fused_api():  # with the three metrics' device-to-host copy, as a training step calls it
        loss, _ = sequence_loss(preds, gt, valid)
        loss.backward()

    def composition():  # with the reference's three .item() calls
        loss, _ = sequence_loss_torch(preds, gt, valid, weights, 400.0)
        loss.backward()

    def clear():
        for p in preds:
            p.grad = None

    res = {}
    for name, fn in (("fused", fused), ("fused_forward", fused_forward), ("fused_api", fused_api), ("composition", composition)):
        def step(fn=fn):
            clear()
            fn()
        res[name] = timed(step, reps=5)
    clear(); fused(); g_fused = [p.grad.clone() for p in preds]
    clear(); composition(); g_ref = [p.grad.clone() for p in preds]
    worst = max(float(((a - r).abs() / r.abs().clamp_min(1e-30)).max()) for a, r in zip(g_fused, g_ref))
    px = b * h * w
    fwd_bytes, bwd_bytes = px * (n * 8 + 8 + 4), px * (n * 8 + 8 + 4 + n * 8)
    print(json.dumps({"leg": "sequence_loss", "shape": [n, b, 2, h, w], "fused_fwd_bwd_us": round(res["fused"][0], 2),
                      "fused_forward_us": round(res["fused_forward"][0], 2), "fused_api_fwd_bwd_us": round(res["fused_api"][0], 2),
                      "composition_fwd_bwd_us": round(res["composition"][0], 2),
                      "forward_bytes": fwd_bytes, "forward_bytes_formula": "B*H*W*(N*8 + 8 + 4)",
                      "backward_bytes": bwd_bytes, "backward_bytes_formula": "B*H*W*(N*8 + 8 + 4 + N*8)",
                      "fused_forward_TBps": round(fwd_bytes / (res["fused_forward"][0] * 1e-6) / 1e12, 3),
                      "fused_fwd_bwd_TBps": round((fwd_bytes + bwd_bytes) / (res["fused"][0] * 1e-6) / 1e12, 3),
                      "grad_max_rel_diff": worst}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "run_metrics_ab.py measures on the GPU"
    _native.load()
    leg_metrics()
    leg_sequence_loss()
