"""Native convolution backward (csrc/conv_backward.hip) against ATen / MIOpen on the update block's layers, and one
training step with ``RAFT.conv_backward_impl`` "native" against "aten" (DESIGN.md §4 "Convolution backward").

Per layer at ``--batch x --height/8 x --width/8``: the input gradient and the weight + bias gradient, timed with device
events over windows of ``--reps`` calls, the two implementations alternated window by window, median of ``--windows``.
ATen is timed after its first call, so MIOpen's find step is excluded. Whole step: forward + backward of
``training_step`` with ``--iters`` refinements, alternated, median of ``--steps``; the first (find) step of each is
reported separately. Needs a ROCm GPU; prints a table and one JSON line.

    python tools/conv_backward_bench.py --out profile.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "torch-optical-flow_amd"), os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

# (name, Cin, Cout, kh, kw, how many of it the block holds): update.py:31-161
LAYERS = [
    ("convc1", 324, 256, 1, 1, 1), ("convc2", 256, 192, 3, 3, 1), ("convf1", 2, 128, 7, 7, 1), ("convf2", 128, 64, 3, 3, 1),
    ("conv", 256, 126, 3, 3, 1), ("gru 1x5", 384, 128, 1, 5, 3), ("gru 5x1", 384, 128, 5, 1, 3),
    ("flow_head.conv1", 128, 256, 3, 3, 1), ("flow_head.conv2", 256, 2, 3, 3, 1), ("mask.0", 128, 256, 3, 3, 1),
    ("mask.2", 256, 576, 1, 1, 1),
]


def _window(fn, reps: int) -> float:
    """Milliseconds per call over one window of ``reps`` calls (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def _alternate(fns: dict, reps: int, windows: int) -> dict:
    for fn in fns.values():  # warm: code objects, MIOpen's find, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(_window(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}


def bench_layers(b: int, h: int, w: int, reps: int, windows: int):
    dev = torch.device("cuda", 0)
    ops = torch.ops.oflow
    rows = []
    for name, cin, cout, kh, kw, count in LAYERS:
        gen = torch.Generator(device=dev).manual_seed(cin * 1000 + cout)
        x = torch.randn(b, cin, h, w, device=dev, generator=gen)
        wt = torch.randn(cout, cin, kh, kw, device=dev, generator=gen) * 0.05
        g = torch.randn(b, cout, h, w, device=dev, generator=gen) * 1e-3
        pad = [kh // 2, kw // 2]

        def aten(mask):
            return lambda: torch.ops.aten.convolution_backward(g, x, wt, [cout], [1, 1], pad, [1, 1], False, [0, 0], 1, mask)

        dgrad = _alternate({"native": lambda: ops.conv2d_same_backward(g, x, wt, [True, False, False]),
                            "aten": aten([True, False, False])}, reps, windows)
        wgrad = _alternate({"native": lambda: ops.conv2d_same_backward(g, x, wt, [False, True, True]),
                            "aten": aten([False, True, True])}, reps, windows)
        # the two must agree before their times are compared
        n, a = ops.conv2d_same_backward(g, x, wt, [True, True, True]), aten([True, True, True])()
        rel = [float((p - q).norm() / q.norm()) for p, q in zip(n, a)]
        flops = 2.0 * b * h * w * cin * cout * kh * kw
        row = dict(layer=name, cin=cin, cout=cout, kh=kh, kw=kw, count=count, gflop=flops / 1e9,
                   dgrad_native_ms=dgrad["native"], dgrad_aten_ms=dgrad["aten"], wgrad_native_ms=wgrad["native"],
                   wgrad_aten_ms=wgrad["aten"], rel_dx=rel[0], rel_dw=rel[1], rel_db=rel[2])
        rows.append(row)
        print(f"{name:16s} {cin:3d}->{cout:3d} {kh}x{kw}  dgrad native {dgrad['native']:.3f} ms ({flops / dgrad['native'] / 1e9:6.1f} TF) "
              f"aten {dgrad['aten']:.3f} ms | wgrad+bias native {wgrad['native']:.3f} ms ({flops / wgrad['native'] / 1e9:6.1f} TF) "
              f"aten {wgrad['aten']:.3f} ms | rel diff dx {rel[0]:.1e} dw {rel[1]:.1e} db {rel[2]:.1e}", flush=True)
    tot = {k: sum(r[k] * r["count"] for r in rows) for k in ("dgrad_native_ms", "dgrad_aten_ms", "wgrad_native_ms", "wgrad_aten_ms")}
    tot["dgrad_native_ms"] -= rows[2]["dgrad_native_ms"]  # convf1's input, the detached flow, gets no gradient
    tot["dgrad_aten_ms"] -= rows[2]["dgrad_aten_ms"]
    print(f"one iteration's 15 convolutions (convf1 without dgrad): dgrad native {tot['dgrad_native_ms']:.3f} ms, aten "
          f"{tot['dgrad_aten_ms']:.3f} ms; wgrad+bias native {tot['wgrad_native_ms']:.3f} ms, aten {tot['wgrad_aten_ms']:.3f} ms", flush=True)
    return rows, tot


def bench_step(b: int, height: int, width: int, iters: int, steps: int):
    from model import RAFT, synthetic

    dev = torch.device("cuda", 0)
    img0, img1 = (t.to(dev) for t in synthetic.synthetic_pair(b, height, width, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (b, 2, height, width), 2.0)).to(dev)
    valid = torch.ones(b, height, width, device=dev)
    model = RAFT(iters=iters)
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(dev).train()
    model.freeze_bn()

    def step(impl):
        model.conv_backward_impl = impl
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = model.training_step((img0, img1, target, valid), 0)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.detach())

    first = {impl: step(impl) for impl in ("aten", "native")}
    print(f"training step {b}x{height}x{width}, {iters} iterations: first step aten {first['aten'][0]:.0f} ms, native "
          f"{first['native'][0]:.0f} ms (loss {first['aten'][1]:.6f} / {first['native'][1]:.6f})", flush=True)
    step("aten"), step("native")
    times = {"aten": [], "native": []}
    for _ in range(steps):
        for impl in times:
            times[impl].append(step(impl)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"training step: median of {steps}: aten {med['aten']:.1f} ms (min {min(times['aten']):.1f}, max {max(times['aten']):.1f}), "
          f"native {med['native']:.1f} ms (min {min(times['native']):.1f}, max {max(times['native']):.1f}); "
          f"native / aten = {med['native'] / med['aten']:.3f}", flush=True)
    return dict(first_ms={k: v[0] for k, v in first.items()}, median_ms=med, all_ms=times, peak_mem_gib=torch.cuda.max_memory_allocated() / 2**30)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=368)
    ap.add_argument("--width", type=int, default=496)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_backward_bench: needs a ROCm GPU")
    from optical_flow import _native

    _native.load()
    print(f"device: {torch.cuda.get_device_name(0)}; layers at {a.batch} x {a.height // 8} x {a.width // 8}", flush=True)
    rows, tot = bench_layers(a.batch, a.height // 8, a.width // 8, a.reps, a.windows)
    result = dict(batch=a.batch, h=a.height // 8, w=a.width // 8, layers=rows, iteration_ms=tot)
    if not a.skip_step:
        result["step"] = bench_step(a.batch, a.height, a.width, a.iters, a.steps)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
