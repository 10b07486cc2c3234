"""Bidirectional inference and the forward-backward consistency check, measured (DESIGN.md §4 "Bidirectional forward").

1. ``optical_flow.fb_consistency(both=True)`` (csrc/fb_consistency.hip) on ``--batch`` flow pairs of ``--height x
   --width``: masks only and masks + residuals, against an ATen composition of the same check (``F.grid_sample`` of the
   other flow at the pixel grid + flow, both directions), each timed with device events over windows of ``--reps``
   back-to-back calls, alternated window by window, median of ``--windows``. The native times are also given as bytes
   per second of the traffic the check cannot avoid: both flows read once, two masks (and two residual maps) written.
   A time per call over back-to-back launches is the kernel's time when the kernel outlasts its launch; the test flows
   are a translation plus smooth noise, so that the taps fall as they do on real flow.
2. One eager test-mode step of ``RAFT.forward_bidirectional`` against the stacked forward
   ``model(cat(i0, i1), cat(i1, i0))`` and against two separate forwards, ``--batch`` pairs, ``--iters`` refinements,
   frames padded by ``InputPadder``: the three alternated in one process, host clock around a device synchronise, median
   of ``--steps``; the outputs are compared first.

Needs a ROCm GPU; prints a table and writes one JSON line (default: profiles/bidirectional/bidirectional_bench.json).

    python tools/bidirectional_bench.py
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), REPO, os.path.join(REPO, "torch-optical-flow_amd"),
          os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_backward_bench import _alternate  # noqa: E402


def smooth_flows(b: int, h: int, w: int, dev):
    """(fw, bw): a translation per image and its inverse plus smooth noise of ~1 px (about half the pixels occluded)."""
    gen = torch.Generator(device=dev).manual_seed(3)
    t = torch.randn(b, 2, 1, 1, device=dev, generator=gen) * 6.0

    def noise():
        g = torch.randn(b, 2, h // 8 + 2, w // 8 + 2, device=dev, generator=gen)
        return F.interpolate(g, size=(h, w), mode="bilinear", align_corners=True)

    return (t + noise()).contiguous(), (-t + noise()).contiguous()


def aten_check(a, o, alpha: float, beta: float):
    """One direction of the check as an ATen composition (the masks agree with the kernel's except within rounding of
    the threshold; frame-edge handling by zero padding plus an explicit inside test)."""
    b, _, h, w = a.shape
    xs = torch.arange(w, device=a.device, dtype=torch.float32).view(1, 1, w)
    ys = torch.arange(h, device=a.device, dtype=torch.float32).view(1, h, 1)
    px, py = xs + a[:, 0], ys + a[:, 1]
    inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    grid = torch.stack([px * (2.0 / (w - 1)) - 1.0, py * (2.0 / (h - 1)) - 1.0], dim=-1)
    s = F.grid_sample(o, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    err = ((a + s) ** 2).sum(1, keepdim=True)
    thr = alpha * ((a * a).sum(1, keepdim=True) + (s * s).sum(1, keepdim=True)) + beta
    mask = ~(err <= thr) | ~inside.unsqueeze(1)
    return mask, torch.where(inside.unsqueeze(1), err, torch.full_like(err, float("inf")))


def bench_consistency(b: int, h: int, w: int, reps: int, windows: int):
    import optical_flow

    dev = torch.device("cuda", 0)
    fw, bw = smooth_flows(b, h, w, dev)
    (m_fw, e_fw), (m_bw, e_bw) = optical_flow.fb_consistency(fw, bw, both=True, return_error=True)
    a_fw, ae_fw = aten_check(fw, bw, 0.01, 0.5)
    a_bw, _ = aten_check(bw, fw, 0.01, 0.5)
    fin = torch.isfinite(e_fw) & torch.isfinite(ae_fw)
    agree = dict(mask_fw=float((m_fw == a_fw).float().mean()), mask_bw=float((m_bw == a_bw).float().mean()),
                 occluded_fw=float(m_fw.float().mean()), occluded_bw=float(m_bw.float().mean()),
                 max_err_diff=float((e_fw[fin] - ae_fw[fin]).abs().max()))
    t = _alternate({
        "native_masks": lambda: optical_flow.fb_consistency(fw, bw, both=True),
        "native_masks_errors": lambda: optical_flow.fb_consistency(fw, bw, both=True, return_error=True),
        "native_one_direction": lambda: optical_flow.fb_consistency(fw, bw),
        "aten": lambda: (aten_check(fw, bw, 0.01, 0.5), aten_check(bw, fw, 0.01, 0.5)),
    }, reps, windows)
    px = b * h * w
    gb = {"native_masks": (2 * 8 + 2) * px / 1e9, "native_masks_errors": (2 * 8 + 2 + 2 * 4) * px / 1e9,
          "native_one_direction": (2 * 8 + 1) * px / 1e9}
    rate = {k: gb[k] / t[k] for k in gb}  # GB / ms = TB/s
    print(f"fb_consistency {b} x {h} x {w}, both directions: masks {t['native_masks'] * 1e3:.1f} us "
          f"({rate['native_masks']:.2f} TB/s of 2 flows + 2 masks), masks + residuals {t['native_masks_errors'] * 1e3:.1f} us "
          f"({rate['native_masks_errors']:.2f} TB/s of 2 flows + 2 masks + 2 residuals), one direction "
          f"{t['native_one_direction'] * 1e3:.1f} us ({rate['native_one_direction']:.2f} TB/s); ATen composition, both "
          f"directions with residuals {t['aten'] * 1e3:.1f} us; masks equal on {agree['mask_fw']:.6f} / "
          f"{agree['mask_bw']:.6f} of the pixels, {agree['occluded_fw']:.3f} / {agree['occluded_bw']:.3f} occluded, "
          f"max |err - err_aten| {agree['max_err_diff']:.2e}", flush=True)
    return dict(b=b, h=h, w=w, ms=t, tbps=rate, agreement=agree)


def bench_step(b: int, height: int, width: int, iters: int, steps: int):
    from model import RAFT, InputPadder, synthetic

    dev = torch.device("cuda", 0)
    img0, img1 = synthetic.synthetic_pair(b, height, width, seed=5)
    padder = InputPadder(img0.shape)
    p0, p1 = (x.to(dev) for x in padder.pad(img0, img1))
    s0, s1 = torch.cat([p0, p1]), torch.cat([p1, p0])
    model = RAFT().eval()
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(dev)

    runs = {
        "shared": lambda: model.forward_bidirectional(p0, p1, iters=iters, test_mode=True),
        "stacked": lambda: model(s0, s1, iters=iters, test_mode=True),
        "two_forwards": lambda: (model(p0, p1, iters=iters, test_mode=True), model(p1, p0, iters=iters, test_mode=True)),
    }
    with torch.inference_mode():
        (_, up_f), (_, up_b) = runs["shared"]()
        _, up_s = runs["stacked"]()
        (_, up_1), (_, up_2) = runs["two_forwards"]()
        same = dict(shared_equals_stacked=bool(torch.equal(torch.cat([up_f, up_b]), up_s)),
                    max_diff_vs_two_forwards=float((torch.cat([up_f, up_b]) - torch.cat([up_1, up_2])).abs().max()))
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(steps):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
    model.check_range(dev)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in med:
        print(f"bidirectional step, {b} pairs of {p0.shape[-2]} x {p0.shape[-1]}, {iters} iterations, {k}: median of {steps} "
              f"{med[k]:.2f} ms (min {min(times[k]):.2f}, max {max(times[k]):.2f})", flush=True)
    print(f"shared / stacked = {med['shared'] / med['stacked']:.3f}, shared / two forwards = "
          f"{med['shared'] / med['two_forwards']:.3f}; shared equals stacked bit for bit: {same['shared_equals_stacked']}, "
          f"max |shared - two forwards| {same['max_diff_vs_two_forwards']:.2e} px", flush=True)
    return dict(pairs=b, height=int(p0.shape[-2]), width=int(p0.shape[-1]), iters=iters, median_ms=med, all_ms=times, outputs=same)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bidirectional", "bidirectional_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bidirectional_bench: needs a ROCm GPU")
    from optical_flow import _native

    _native.load()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    result = {}
    if not a.skip_kernel:
        result["fb_consistency"] = bench_consistency(a.batch, a.height, a.width, a.reps, a.windows)
    if not a.skip_step:
        result["step"] = bench_step(a.batch, a.height, a.width, a.iters, a.steps)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
