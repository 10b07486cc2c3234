"""Native encoder backward (csrc/conv_backward.hip at stride 1 / 2, csrc/norm_backward.hip) against ATen / MIOpen on
the encoders' layers, and one training step for the four settings of ``RAFT.encoder_backward_impl`` and
``RAFT.conv_backward_impl`` (DESIGN.md §4 "Encoder backward").

Per layer at fnet's training shape (``2 * --batch`` images of ``--height x --width``; cnet sees half the batch): the
input gradient and the weight + bias gradient of each convolution, the backward of each norm layer (+ ReLU), timed with
device events over windows of ``--reps`` calls, native and ATen alternated window by window, median of ``--windows``.
ATen is timed after its first call, so MIOpen's find step is excluded. The stem's folded weight gradient is also timed
against the generic per-tap path on the same layer. Whole step: forward + backward of ``training_step`` with ``--iters``
refinements, the four settings alternated, median of ``--steps``, with ``torch.cuda.max_memory_allocated`` of each; the
first step of each setting (ATen's includes MIOpen's find) is reported separately. Needs a ROCm GPU; prints a table and
writes one JSON line (default: profiles/encoder_backward/encoder_backward_bench.json).

    python tools/encoder_backward_bench.py
"""
from __future__ import annotations

import argparse
import ctypes
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

# (name, Cin, Cout, k, stride, input-resolution divisor, how many of it one encoder holds): extractor.py BasicEncoder
CONVS = [
    ("stem 7x7/2", 3, 64, 7, 2, 1, 1), ("layer1 3x3", 64, 64, 3, 1, 2, 4), ("layer2 3x3/2", 64, 96, 3, 2, 2, 1),
    ("layer2 3x3", 96, 96, 3, 1, 4, 3), ("layer2 1x1/2", 64, 96, 1, 2, 2, 1), ("layer3 3x3/2", 96, 128, 3, 2, 4, 1),
    ("layer3 3x3", 128, 128, 3, 1, 8, 3), ("layer3 1x1/2", 96, 128, 1, 2, 4, 1), ("head 1x1", 128, 256, 1, 1, 8, 1),
]
# (name, C, resolution divisor, how many): 5 norm layers per resolution, all but the two projections' with a ReLU
NORMS = [("norm 64 @ 1/2", 64, 2, 5), ("norm 96 @ 1/4", 96, 4, 5), ("norm 128 @ 1/8", 128, 8, 5)]
SETTINGS = [("aten", "aten"), ("native", "aten"), ("aten", "native"), ("native", "native")]  # (encoder, update block)


def bench_convs(b: int, height: int, width: int, reps: int, windows: int):
    from optical_flow import _native

    dev = torch.device("cuda", 0)
    ops, lib = torch.ops.oflow, _native.load()
    rows = []
    for name, cin, cout, k, s, div, count in CONVS:
        h, w = height // div, width // div
        ho, wo = (h + s - 1) // s, (w + s - 1) // s
        gen = torch.Generator(device=dev).manual_seed(cin * 1000 + cout + k)
        x = torch.randn(b, cin, h, w, device=dev, generator=gen)
        wt = torch.randn(cout, cin, k, k, device=dev, generator=gen) * 0.05
        g = torch.randn(b, cout, ho, wo, device=dev, generator=gen) * 1e-3
        pad = [k // 2, k // 2]

        def aten(mask):
            return lambda: torch.ops.aten.convolution_backward(g, x, wt, [cout], [s, s], pad, [1, 1], False, [0, 0], 1, mask)

        stem = cin == 3  # the images need no gradient: nothing is launched for the stem's dgrad
        dgrad = {"native": 0.0, "aten": 0.0} if stem else _alternate(
            {"native": lambda: ops.conv2d_strided_backward(g, x, wt, s, [True, False, False]),
             "aten": aten([True, False, False])}, reps, windows)
        fns = {"native": lambda: ops.conv2d_strided_backward(g, x, wt, s, [False, True, True]),
               "aten": aten([False, True, True])}
        if stem:  # the generic per-tap path on the same layer, through the C ABI on the same stream
            dims = (b, cout, cin, h, w, k, k, s)
            ws = torch.empty(lib.oflow_conv2d_strided_backward_weight_workspace_floats(*dims), device=dev)
            gw, gb = torch.empty_like(wt), torch.empty(cout, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            fns["generic"] = lambda: lib.oflow_conv2d_strided_backward_weight_generic_f32(
                g.data_ptr(), x.data_ptr(), *dims, gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), st)
        wgrad = _alternate(fns, reps, windows)
        mask = [not stem, True, True]
        n, a = ops.conv2d_strided_backward(g, x, wt, s, mask), aten(mask)()
        rel = [float((p - q).norm() / q.norm()) if m else 0.0 for p, q, m in zip(n, a, mask)]
        flops = 2.0 * b * ho * wo * cin * cout * k * k
        row = dict(layer=name, cin=cin, cout=cout, k=k, stride=s, h=h, w=w, count=count, gflop=flops / 1e9,
                   dgrad_native_ms=dgrad["native"], dgrad_aten_ms=dgrad["aten"], wgrad_native_ms=wgrad["native"],
                   wgrad_aten_ms=wgrad["aten"], wgrad_generic_ms=wgrad.get("generic"), rel_dx=rel[0], rel_dw=rel[1],
                   rel_db=rel[2])
        rows.append(row)
        extra = f" (generic per-tap path {wgrad['generic']:.3f} ms)" if stem else ""
        print(f"{name:13s} {cin:3d}->{cout:3d} in {h}x{w}  dgrad native {dgrad['native']:.3f} ms aten {dgrad['aten']:.3f} ms | "
              f"wgrad+bias native {wgrad['native']:.3f} ms ({flops / wgrad['native'] / 1e9:6.1f} TF){extra} aten "
              f"{wgrad['aten']:.3f} ms | rel diff dx {rel[0]:.1e} dw {rel[1]:.1e} db {rel[2]:.1e}", flush=True)
    tot = {key: sum(r[key] * r["count"] for r in rows)
           for key in ("dgrad_native_ms", "dgrad_aten_ms", "wgrad_native_ms", "wgrad_aten_ms")}
    print(f"one encoder's 16 convolutions at batch {b}: dgrad native {tot['dgrad_native_ms']:.3f} ms, aten "
          f"{tot['dgrad_aten_ms']:.3f} ms; wgrad+bias native {tot['wgrad_native_ms']:.3f} ms, aten {tot['wgrad_aten_ms']:.3f} ms",
          flush=True)
    return rows, tot


def bench_norms(b: int, height: int, width: int, reps: int, windows: int):
    dev = torch.device("cuda", 0)
    ops = torch.ops.oflow
    rows = []
    for name, c, div, count in NORMS:
        h, w = height // div, width // div
        gen = torch.Generator(device=dev).manual_seed(c)
        x = torch.randn(b, c, h, w, device=dev, generator=gen)
        g = torch.randn(b, c, h, w, device=dev, generator=gen) * 1e-3
        gamma, beta, rm = (torch.randn(c, device=dev, generator=gen) for _ in range(3))
        rv = torch.rand(c, device=dev, generator=gen) + 0.5
        # ATen: the backward of relu(norm(x)) as autograd runs it, from a retained graph (threshold + norm backward)
        xi = x.clone().requires_grad_()
        yi = torch.relu(torch.nn.functional.instance_norm(xi))
        xb, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        yb = torch.relu(torch.nn.functional.batch_norm(xb, rm, rv, gr, br, False, 0.1, 1e-5))
        inst = _alternate({"native": lambda: ops.instance_norm_act_backward(g, x, 1e-5, True),
                           "aten": lambda: torch.autograd.grad(yi, xi, g, retain_graph=True)}, reps, windows)
        bn = _alternate({"native": lambda: ops.frozen_batch_norm_act_backward(g, x, gamma, beta, rm, rv, 1e-5, True, [True] * 3),
                         "aten": lambda: torch.autograd.grad(yb, (xb, gr, br), g, retain_graph=True)}, reps, windows)
        rel_i = float((ops.instance_norm_act_backward(g, x, 1e-5, True) - torch.autograd.grad(yi, xi, g, retain_graph=True)[0]).norm()
                      / torch.autograd.grad(yi, xi, g, retain_graph=True)[0].norm())
        gbytes = 3.0 * x.numel() * 4 / 1e9  # read gy, x; write dx
        rows.append(dict(layer=name, c=c, h=h, w=w, count=count, instance_native_ms=inst["native"],
                         instance_aten_ms=inst["aten"], frozen_bn_native_ms=bn["native"], frozen_bn_aten_ms=bn["aten"],
                         rel_instance_dx=rel_i))
        print(f"{name:15s} {b}x{c}x{h}x{w}  instance norm + relu: native {inst['native']:.3f} ms "
              f"({gbytes / inst['native']:.2f} TB/s of gy + x + dx) aten {inst['aten']:.3f} ms | frozen batch norm + relu: native "
              f"{bn['native']:.3f} ms ({gbytes / bn['native']:.2f} TB/s) aten {bn['aten']:.3f} ms | rel diff dx {rel_i:.1e}",
              flush=True)
    return rows


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

    def step(setting):
        model.encoder_backward_impl, model.conv_backward_impl = setting
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss = model.training_step((img0, img1, target, valid), 0)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss.detach()), torch.cuda.max_memory_allocated() / 2**30

    key = lambda s: f"encoder={s[0]},update={s[1]}"  # noqa: E731
    # all-native first: its first step holds no MIOpen backward find; the all-ATen one then pays every find
    first = {key(s): step(s) for s in reversed(SETTINGS)}
    for k, v in first.items():
        print(f"first step {k}: {v[0]:.0f} ms (loss {v[1]:.6f})", flush=True)
    for s in SETTINGS:
        step(s)
    times, mem = {key(s): [] for s in SETTINGS}, {}
    for _ in range(steps):
        for s in SETTINGS:
            ms, _, gib = step(s)
            times[key(s)].append(ms)
            mem[key(s)] = gib
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in med:
        print(f"training step {b}x{height}x{width}, {iters} iterations, {k}: median of {steps} {med[k]:.1f} ms "
              f"(min {min(times[k]):.1f}, max {max(times[k]):.1f}), peak memory {mem[k]:.2f} GiB", flush=True)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "encoder_backward", "encoder_backward_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_backward_bench: needs a ROCm GPU")
    from optical_flow import _native

    _native.load()
    nb = 2 * a.batch  # fnet runs both frames as one batch
    print(f"device: {torch.cuda.get_device_name(0)}; layers at fnet's batch {nb} of {a.height} x {a.width}", flush=True)
    result = dict(batch=a.batch, encoder_batch=nb, height=a.height, width=a.width)
    if not a.skip_layers:
        rows, tot = bench_convs(nb, a.height, a.width, a.reps, a.windows)
        result.update(convs=rows, conv_totals_ms=tot, norms=bench_norms(nb, a.height, a.width, a.reps, a.windows))
    if not a.skip_step:
        result["step"] = bench_step(a.batch, a.height, a.width, a.iters, a.steps)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
