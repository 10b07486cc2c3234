"""Native batch norm on batch statistics (csrc/batch_norm.hip, ``RAFT.batch_norm_impl = "native"``) against the module
+ ReLU (ATen / MIOpen) on cnet's three layer shapes, and one training step with cnet in train mode (no ``freeze_bn()``:
the Chairs stage) with all three switches native against all default (DESIGN.md §4 "Batch norm on batch statistics").

Per layer at cnet's training shape (``--batch`` images of ``--height x --width`` at 1/2, 1/4 and 1/8 resolution): the
forward as the encoder runs it under autograd (``enc_norm_act`` with the switch native, running statistics updated,
against ``relu(module(x))``) and the backward of both (all three gradients, both through ``torch.autograd.grad`` on a
retained graph, so both carry the autograd engine's host cost; the native op called directly is timed beside them), timed
with device events over windows of
``--reps`` calls, native and ATen alternated window by window, median of ``--windows``. ATen is timed after its first
calls, so MIOpen's find step is excluded. Each native time is also given as bytes per second of the traffic the
computation cannot avoid: the forward reads x twice (statistics, apply) and writes y; the backward reads grad_out and x
twice each (channel sums, apply) and writes dx. Both backends' y and dx are also compared with the float64 closed form
on the device. Whole step: forward + backward of ``training_step`` with ``--iters`` refinements, three settings
alternated (all default, ``batch_norm_impl`` alone, all three switches native), median of ``--steps``, with
``torch.cuda.max_memory_allocated`` of each; the first step of each setting (ATen's includes MIOpen's find) is reported
separately. Needs a ROCm GPU; prints a table and writes one JSON line (default:
profiles/batch_norm/batch_norm_bench.json).

    python tools/batch_norm_bench.py
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

from conv_backward_bench import _alternate  # noqa: E402

# (name, C, resolution divisor, how many of it cnet holds): extractor.py BasicEncoder
LAYERS = [("norm 64 @ 1/2", 64, 2, 5), ("norm 96 @ 1/4", 96, 4, 5), ("norm 128 @ 1/8", 128, 8, 5)]
# (encoder_backward_impl, conv_backward_impl, batch_norm_impl): all default, the new switch alone, all native
SETTINGS = {"default": ("aten", "aten", "aten"), "batch_norm_impl": ("aten", "aten", "native"),
            "all native": ("native", "native", "native")}


def bench_layers(b: int, height: int, width: int, reps: int, windows: int):
    from model import extractor as ext

    dev = torch.device("cuda", 0)
    ops = torch.ops.oflow
    rows = []
    for name, c, div, count in LAYERS:
        h, w = height // div, width // div
        gen = torch.Generator(device=dev).manual_seed(c)
        x = torch.randn(b, c, h, w, device=dev, generator=gen)
        g = torch.randn(b, c, h, w, device=dev, generator=gen) * 1e-3
        mods = {k: torch.nn.BatchNorm2d(c).to(dev).train() for k in ("native", "aten")}
        with torch.no_grad():
            for m in mods.values():
                m.weight.copy_(1 + 0.2 * torch.randn(c, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))
                m.bias.copy_(0.1 * torch.randn(c, device=dev, generator=torch.Generator(device=dev).manual_seed(2)))
        xr = x.clone().requires_grad_()
        fwd = _alternate({"native": lambda: ext.enc_norm_act(mods["native"], xr, True, "aten", "native"),
                          "aten": lambda: torch.relu(mods["aten"](xr))}, reps, windows)
        gamma, beta = mods["native"].weight.detach(), mods["native"].bias.detach()
        with torch.no_grad():
            y, mean, var = ops.batch_norm_act(x, gamma, beta, 1e-5, True)
        ya = torch.relu(mods["aten"](xr))  # the graph ATen's backward is timed on (threshold + batch norm backward)
        leaves = (xr, mods["aten"].weight, mods["aten"].bias)
        # both backwards through the autograd engine, as a training step runs them; the native op called directly is
        # timed too (no engine, no Python formula: nearer to its kernels' time)
        leaves_n = (xr, mods["native"].weight, mods["native"].bias)
        yn = ops.batch_norm_act(*leaves_n, 1e-5, True)[0]
        bwd = _alternate({"native": lambda: torch.autograd.grad(yn, leaves_n, g, retain_graph=True),
                          "aten": lambda: torch.autograd.grad(ya, leaves, g, retain_graph=True),
                          "native_direct": lambda: ops.batch_norm_act_backward(g, x, gamma, beta, mean, var, 1e-5, True,
                                                                               [True] * 3)}, reps, windows)
        got = ops.batch_norm_act_backward(g, x, gamma, beta, mean, var, 1e-5, True, [True] * 3)
        want = torch.autograd.grad(ya, leaves, g, retain_graph=True)
        rel = [float((p - q).norm() / q.norm()) for p, q in zip((y,) + tuple(got), (ya.detach(),) + tuple(want))]
        # both backends against the float64 closed form on the device (relative error norms of y and dx)
        x64, g64 = x.double(), g.double()
        mu = x64.mean(dim=(0, 2, 3), keepdim=True)
        r64 = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(dim=(0, 2, 3), keepdim=True) + 1e-5)
        xh = (x64 - mu) * r64
        y64 = torch.relu(xh * gamma.double().view(1, c, 1, 1) + beta.double().view(1, c, 1, 1))
        gm = g64 * (y64 > 0)
        dx64 = gamma.double().view(1, c, 1, 1) * r64 * (gm - gm.mean(dim=(0, 2, 3), keepdim=True)
                                                        - xh * (gm * xh).mean(dim=(0, 2, 3), keepdim=True))
        err = {k: float((t.double() - ref).norm() / ref.norm()) for k, t, ref in (
            ("y_native", y, y64), ("y_aten", ya.detach(), y64), ("dx_native", got[0], dx64), ("dx_aten", want[0], dx64))}
        del x64, g64, xh, y64, gm, dx64
        numel_gb = x.numel() * 4 / 1e9
        row = dict(layer=name, b=b, c=c, h=h, w=w, count=count, forward_native_ms=fwd["native"], forward_aten_ms=fwd["aten"],
                   backward_native_ms=bwd["native"], backward_aten_ms=bwd["aten"], backward_native_direct_ms=bwd["native_direct"],
                   forward_native_tbps=3 * numel_gb / fwd["native"], backward_native_tbps=5 * numel_gb / bwd["native"],
                   rel_y=rel[0], rel_dx=rel[1], rel_dgamma=rel[2], rel_dbeta=rel[3], err_vs_float64=err)
        rows.append(row)
        print(f"{name:15s} {b}x{c}x{h}x{w}  forward: native {fwd['native']:.3f} ms ({row['forward_native_tbps']:.2f} TB/s of "
              f"2 x + y) aten {fwd['aten']:.3f} ms | backward: native {bwd['native']:.3f} ms "
              f"({row['backward_native_tbps']:.2f} TB/s of 2 gy + 2 x + dx; op called directly {bwd['native_direct']:.3f} ms) aten "
              f"{bwd['aten']:.3f} ms | rel diff y {rel[0]:.1e} "
              f"dx {rel[1]:.1e} dgamma {rel[2]:.1e} dbeta {rel[3]:.1e} | against float64: y native {err['y_native']:.1e} aten "
              f"{err['y_aten']:.1e}, dx native {err['dx_native']:.1e} aten {err['dx_aten']:.1e}", flush=True)
    tot = {key: sum(r[key] * r["count"] for r in rows)
           for key in ("forward_native_ms", "forward_aten_ms", "backward_native_ms", "backward_aten_ms")}
    print(f"cnet's 15 batch norms at batch {b}: forward native {tot['forward_native_ms']:.3f} ms, aten "
          f"{tot['forward_aten_ms']:.3f} ms; backward native {tot['backward_native_ms']:.3f} ms, aten "
          f"{tot['backward_aten_ms']:.3f} ms", flush=True)
    return rows, tot


def bench_step(b: int, height: int, width: int, iters: int, steps: int):
    from model import RAFT, synthetic

    dev = torch.device("cuda", 0)
    img0, img1 = (t.to(dev) for t in synthetic.synthetic_pair(b, height, width, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (b, 2, height, width), 2.0)).to(dev)
    valid = torch.ones(b, height, width, device=dev)
    model = RAFT(iters=iters)
    model.load_state_dict(synthetic.synthetic_state_dict(model.state_dict()))
    model = model.to(dev).train()  # cnet's batch norm on batch statistics: no freeze_bn()

    def step(name):
        model.encoder_backward_impl, model.conv_backward_impl, model.batch_norm_impl = SETTINGS[name]
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss = model.training_step((img0, img1, target, valid), 0)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.detach()), torch.cuda.max_memory_allocated() / 2**30

    # all-native first: its first step holds no MIOpen backward find; the all-ATen one then pays every find
    first = {s: step(s) for s in reversed(list(SETTINGS))}
    for k, v in first.items():
        print(f"first step, {k}: {v[0]:.0f} ms (loss {v[1]:.6f})", flush=True)
    for s in SETTINGS:
        step(s)
    times, mem = {s: [] for s in SETTINGS}, {}
    for _ in range(steps):
        for s in SETTINGS:
            ms, _, gib = step(s)
            times[s].append(ms)
            mem[s] = gib
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in med:
        print(f"training step {b}x{height}x{width}, {iters} iterations, cnet in train mode, {k}: median of "
              f"{steps} {med[k]:.1f} ms (min {min(times[k]):.1f}, max {max(times[k]):.1f}), peak memory {mem[k]:.2f} GiB",
              flush=True)
    return dict(first_ms={k: v[0] for k, v in first.items()}, median_ms=med, all_ms=times, peak_mem_gib=mem)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=368)
    ap.add_argument("--width", type=int, default=496)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_norm", "batch_norm_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_norm_bench: needs a ROCm GPU")
    from optical_flow import _native

    _native.load()
    _native.ops()
    print(f"device: {torch.cuda.get_device_name(0)}; layers at cnet's batch {a.batch} of {a.height} x {a.width}", flush=True)
    result = dict(batch=a.batch, height=a.height, width=a.width)
    if not a.skip_layers:
        rows, tot = bench_layers(a.batch, a.height, a.width, a.reps, a.windows)
        result.update(layers=rows, layer_totals_ms=tot)
    if not a.skip_step:
        result["step"] = bench_step(a.batch, a.height, a.width, a.iters, a.steps)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
