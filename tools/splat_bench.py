"""Forward warping (optical_flow.splat), measured (DESIGN.md §4 "splat").

Shapes: ``8 x 3 x 436 x 1024`` images and ``8 x 128 x 55 x 128`` features at 1/8 resolution, under a smooth flow (blurred
Gaussian noise of about 8 px). Per shape and mode ("sum", "avg", "linear", "soft"):

* the native forward (``torch.ops.oflow.splat``) and forward + backward (all three gradients), against
  (a) the fp32 ATen composition with ``index_add_`` (its backward by autograd), and
  (b) for "sum" only, the float-atomic route that existed before: the frame gradient of
  ``warp(x, normalize(flow), "bilinear", "zeros", align_corners=True)`` (csrc/warp_backward.hip);
  each timed with device events over windows of ``--reps`` back-to-back calls, alternated window by window, median of
  ``--windows``;
* the device time of every splat kernel from one profiled run (torch.profiler, median over the run's calls), and the
  scatter kernel's atomic bytes (8 bytes per tap inside the frame and accumulator plane) divided by its time, next to
  the guides' float-atomic rate of about 1.3 TB/s of added bytes for context;
* whether two native runs gave the same bits, and whether the float-atomic route did.

The accumulator layout is planar (csrc/splat.hip); no interleaved variant was built, so only planar is measured.
Needs a ROCm GPU; prints a table and writes one JSON line (default: profiles/splat/splat_bench.json).

    python tools/splat_bench.py
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), REPO, os.path.join(REPO, "torch-optical-flow_amd"),
          os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_backward_bench import _alternate  # noqa: E402

MODES = ("sum", "avg", "linear", "soft")
SHAPES = {"images": (8, 3, 436, 1024), "features": (8, 128, 55, 128)}
EPS = 1e-7


def smooth_flow(b: int, h: int, w: int, dev, px: float = 8.0):
    """Blurred Gaussian noise of about ``px`` pixels: noise on a grid 16 times coarser, bilinearly enlarged."""
    gen = torch.Generator(device=dev).manual_seed(11)
    g = torch.randn(b, 2, h // 16 + 2, w // 16 + 2, device=dev, generator=gen) * px
    return F.interpolate(g, size=(h, w), mode="bilinear", align_corners=True).contiguous()


def aten_splat(frame, flow, metric, mode: str):
    """(a): the operator as an fp32 ATen composition on the device, index_add_ for the scatter (float atomics)."""
    b, c, h, w = frame.shape
    hw = h * w
    px = torch.arange(w, device=frame.device, dtype=torch.float32).view(1, 1, w) + flow[:, 0]
    py = torch.arange(h, device=frame.device, dtype=torch.float32).view(1, h, 1) + flow[:, 1]
    keep = (px > -1) & (px < w) & (py > -1) & (py < h)
    pxs, pys = torch.where(keep, px, 0.0), torch.where(keep, py, 0.0)
    x0f, y0f = torch.floor(pxs.detach()), torch.floor(pys.detach())
    fx, fy = pxs - x0f, pys - y0f
    x0, y0 = x0f.long(), y0f.long()
    if mode == "linear":
        m = metric[:, 0]
    elif mode == "soft":
        m = torch.exp(metric[:, 0] - metric.detach().reshape(b, -1).amax(dim=1).view(b, 1, 1))
    else:
        m = torch.ones_like(px)
    f = frame.permute(1, 0, 2, 3).reshape(c, b * hw)
    num = torch.zeros((c, b * hw), device=frame.device)
    den = torch.zeros(b * hw, device=frame.device)
    base = (torch.arange(b, device=frame.device) * hw).view(b, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = keep & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            wm = torch.where(ok, ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)) * m, 0.0).reshape(-1)
            idx = (torch.where(ok, y * w + x, 0) + base).reshape(-1)
            den = den.index_add(0, idx, wm)
            num = num.index_add(1, idx, wm * f)
    out = num if mode == "sum" else num / (den + EPS)
    return out.view(c, b, h, w).permute(1, 0, 2, 3)


def kernel_times(fn, calls: int):
    """Median device time in microseconds of every kernel whose name contains 'splat', over ``calls`` calls of fn."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            if re.search(r"splat_\w+", ev.name):
                dur = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                per.setdefault(re.search(r"splat_\w+", ev.name).group(0), []).append(float(dur))
        return {k: statistics.median(v) for k, v in per.items()}
    except Exception as e:  # noqa: BLE001 (no profiler on this installation: the per-kernel rows are left out)
        print(f"per-kernel times unavailable: {type(e).__name__}: {e}", flush=True)
        return {}


def bench_shape(tag: str, shape, reps: int, windows: int):
    import optical_flow
    from optical_flow import _native

    ops = torch.ops.oflow
    dev = torch.device("cuda", 0)
    b, c, h, w = shape
    gen = torch.Generator(device=dev).manual_seed(5)
    frame = torch.rand(shape, device=dev, generator=gen)
    g = torch.randn(shape, device=dev, generator=gen)
    flow = smooth_flow(b, h, w, dev)
    raw = torch.randn((b, 1, h, w), device=dev, generator=gen)
    nflow = optical_flow.normalize(flow)
    # taps inside the frame: the scatter's atomics (an all-zero contribution is not added; none is expected here)
    px = torch.arange(w, device=dev).view(1, 1, w) + flow[:, 0]
    py = torch.arange(h, device=dev).view(1, h, 1) + flow[:, 1]
    keep = (px > -1) & (px < w) & (py > -1) & (py < h)
    x0, y0 = torch.floor(px), torch.floor(py)
    taps = sum(int((keep & (x0 + dx >= 0) & (x0 + dx < w) & (y0 + dy >= 0) & (y0 + dy < h)).sum())
               for dx in (0, 1) for dy in (0, 1))
    atomic_gb = taps * (c + 1) * 8 / 1e9
    rows = {}
    for mode in MODES:
        metric = {"linear": raw.abs(), "soft": raw}.get(mode)
        code = _native.SPLAT_MODES[mode]
        out, weight = ops.splat(frame, flow, metric, code)
        ref = aten_splat(frame, flow, metric, mode)
        agree = float((out - ref).abs().max() / ref.abs().max())
        same_bits = bool(torch.equal(ops.splat(frame, flow, metric, code)[0].view(torch.int32), out.view(torch.int32)))
        mask = [True, True, metric is not None]
        leaves = [t.clone().requires_grad_() for t in (frame, flow) + ((metric,) if metric is not None else ())]

        def aten_both():
            o = aten_splat(leaves[0], leaves[1], leaves[2] if metric is not None else None, mode)
            return torch.autograd.grad((o * g).sum(), leaves)

        def native_both():
            o, wt = ops.splat(frame, flow, metric, code)
            return ops.splat_backward(g, frame, flow, metric, o, wt, code, mask)

        fns = {"native_fwd": lambda: ops.splat(frame, flow, metric, code),
               "aten_fwd": lambda: aten_splat(frame, flow, metric, mode),
               "native_fwd_bwd": native_both, "aten_fwd_bwd": aten_both}
        if mode == "sum":
            fns["warp_grad_fwd"] = lambda: ops.grid_warp_backward(frame, frame, nflow, 0, 0, True, [True, False])
        t = _alternate(fns, reps, windows)
        row = dict(ms=t, rel_diff_vs_aten=agree, native_same_bits=same_bits)
        if mode == "sum":
            a, b2 = (ops.grid_warp_backward(frame, frame, nflow, 0, 0, True, [True, False])[0] for _ in range(2))
            row["warp_grad_same_bits"] = bool(torch.equal(a.view(torch.int32), b2.view(torch.int32)))
            row["rel_diff_vs_warp_grad"] = float((out - a).abs().max() / a.abs().max())
        kt = kernel_times(native_both, 20)
        row["kernel_us"] = kt
        scatter = next((v for k, v in kt.items() if "scatter" in k), None)
        row["atomic_gb"] = atomic_gb
        row["scatter_atomic_tbps"] = atomic_gb / (scatter * 1e-3) if scatter else None  # GB / ms = TB/s
        rows[mode] = row
        rate = f"{row['scatter_atomic_tbps']:.2f} TB/s of 64-bit integer adds" if scatter else "n/a"
        print(f"splat {tag} {b}x{c}x{h}x{w} {mode}: forward native {t['native_fwd'] * 1e3:.1f} us, ATen {t['aten_fwd'] * 1e3:.1f} us"
              + (f", warp-gradient route {t['warp_grad_fwd'] * 1e3:.1f} us" if mode == "sum" else "")
              + f"; forward + backward native {t['native_fwd_bwd'] * 1e3:.1f} us, ATen {t['aten_fwd_bwd'] * 1e3:.1f} us; "
              f"kernels (us) {({k: round(v, 1) for k, v in kt.items()})}; scatter atomics {atomic_gb * 1e3:.1f} MB -> {rate} "
              f"(float atomics: about 1.3 TB/s); max |native - ATen| / max {agree:.1e}; two native runs same bits: {same_bits}"
              + (f", two warp-gradient runs same bits: {row['warp_grad_same_bits']}" if mode == "sum" else ""), flush=True)
    return dict(shape=list(shape), taps=taps, layout="planar", modes=rows)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "splat", "splat_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splat_bench: needs a ROCm GPU")
    from optical_flow import _native

    _native.load()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    result = {tag: bench_shape(tag, shape, a.reps, a.windows) for tag, shape in SHAPES.items()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
