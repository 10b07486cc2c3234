"""The unsupervised losses (optical_flow.losses), measured (DESIGN.md §4 "losses").

Shapes: ``8 x 3 x 436 x 1024`` (Sintel) and ``8 x 3 x 368 x 496`` (a Chairs crop), frames of integer levels with the
second frame a noisy copy, a 70 % mask. Per shape:

* the native census forward and forward + backward (both frame gradients) against the package's torch composition on
  the same GPU (tests/losses_cases.py: fp64 differences rounded to fp32, closed-form derivative; not plain fp32 ATen),
  each timed with device events over windows of ``--reps`` back-to-back calls, alternated window by window, median of
  ``--windows``, and ``torch.cuda.max_memory_allocated`` of one forward + backward of each;
* the same for the smoothness loss (order 1 and 2);
* the census backward kernel alone through the C ABI, taking s from the forward's map against recomputing it
  (``d_s_map = NULL``): the save-or-recompute decision;
* a 12-prediction ``unsupervised_sequence_loss``, forward + backward, native against the same sum over the compositions.

The native and the composed results are compared before their times are. Needs a ROCm GPU; prints a table and writes
one JSON line (default: profiles/losses/losses_bench.json).

    python tools/losses_bench.py
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "torch-optical-flow_amd"),
          os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import losses_cases as lc  # noqa: E402
from conv_backward_bench import _alternate  # noqa: E402

SHAPES = {"sintel": (8, 3, 436, 1024), "chairs": (8, 3, 368, 496)}


def inputs(shape, dev):
    b, c, h, w = shape
    gen = torch.Generator(device=dev).manual_seed(h * 10000 + w)
    f0 = torch.randint(0, 256, shape, device=dev, generator=gen).float()
    f0 = torch.nn.functional.avg_pool2d(f0, 5, stride=1, padding=2).round()  # (neighbouring levels correlate)
    f1 = (f0 + 4.0 * torch.randn(shape, device=dev, generator=gen)).clamp(0, 255)
    mask = torch.rand((b, 1, h, w), device=dev, generator=gen) < 0.7
    flow = 2.0 * torch.randn((b, 2, h, w), device=dev, generator=gen)
    return f0, f1, mask, flow


def peak_mib(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


def bench_shape(name, shape, reps, windows, seq_preds, dev):
    from model.raft import unsupervised_sequence_loss
    from optical_flow import _native, census_loss, normalize, smoothness_loss, warp

    b, c, h, w = shape
    f0, f1, mask, flow = inputs(shape, dev)
    row = dict(shape=name, dims=list(shape))

    def native_census(backward):
        def run():
            a, bb = f0.detach().requires_grad_(backward), f1.detach().requires_grad_(backward)
            loss = census_loss(a, bb, mask)
            return (loss, *torch.autograd.grad(loss, [a, bb])) if backward else (loss,)
        return run

    def composed_census(backward):
        def run():
            a, bb = f0.detach().requires_grad_(backward), f1.detach().requires_grad_(backward)
            with torch.set_grad_enabled(backward):
                loss, _ = lc.census_compose(a, bb, mask, 7, 255.0)
            return (loss, *torch.autograd.grad(loss, [a, bb])) if backward else (loss,)
        return run

    n, a = native_census(True)(), composed_census(True)()
    row["census_rel_diff"] = [abs(float(n[0].detach()) - float(a[0].detach())) / float(a[0].detach())] + \
        [float((p - q).norm() / q.norm()) for p, q in zip(n[1:], a[1:])]
    del n, a
    fwd = _alternate({"native": native_census(False), "torch": composed_census(False)}, reps, windows)
    both = _alternate({"native": native_census(True), "torch": composed_census(True)}, reps, windows)
    row.update(census_fwd_native_ms=fwd["native"], census_fwd_torch_ms=fwd["torch"], census_fb_native_ms=both["native"],
               census_fb_torch_ms=both["torch"], census_fb_native_mib=peak_mib(native_census(True), dev),
               census_fb_torch_mib=peak_mib(composed_census(True), dev))
    print(f"{name} {shape}: census fwd native {fwd['native']:.3f} ms torch {fwd['torch']:.3f} ms | fwd+bwd native "
          f"{both['native']:.3f} ms torch {both['torch']:.3f} ms ({both['torch'] / both['native']:.1f} x) | peak native "
          f"{row['census_fb_native_mib']:.0f} MiB torch {row['census_fb_torch_mib']:.0f} MiB | rel diff "
          f"{['%.1e' % v for v in row['census_rel_diff']]}", flush=True)

    # the backward kernel alone: s from the forward's map against s recomputed
    lib = _native.load()
    ws = torch.empty(lib.oflow_census_loss_workspace_bytes(b, h, w) // 8, device=dev, dtype=torch.float64)
    s_map, loss = torch.empty((b, 1, h, w), device=dev), torch.empty(1, device=dev)
    sum_m, gl = torch.empty(1, device=dev, dtype=torch.float64), torch.ones(1, device=dev)
    g0, g1 = torch.empty_like(f0), torch.empty_like(f1)
    f1c = f1.contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p, F = (lambda t: None if t is None else t.data_ptr()), ctypes.c_float

    def forward(with_map):
        return lambda: lib.oflow_census_loss_f32(p(f0), p(f1c), p(mask), 2, b, c, h, w, 7, F(255.0),
                                                 p(s_map) if with_map else None, p(ws), p(loss), p(sum_m), st)

    def backward(saved):
        return lambda: lib.oflow_census_loss_backward_f32(p(gl), p(f0), p(f1c), p(mask), 2, p(s_map) if saved else None,
                                                          p(sum_m), b, c, h, w, 7, F(255.0), p(g0), p(g1), st)

    assert forward(True)() == 0
    k = _alternate({"fwd_map": forward(True), "fwd_nomap": forward(False), "bwd_saved": backward(True),
                    "bwd_recomputed": backward(False)}, reps, windows)
    row.update({"kernel_" + key + "_ms": v for key, v in k.items()})
    print(f"{name}: kernels through the C ABI: forward with map {k['fwd_map']:.3f} ms, without {k['fwd_nomap']:.3f} ms; "
          f"backward from the saved map {k['bwd_saved']:.3f} ms, recomputing s {k['bwd_recomputed']:.3f} ms", flush=True)

    for order in (1, 2):
        def native_smooth():
            fl = flow.detach().requires_grad_()
            loss = smoothness_loss(fl, f0, order)
            return loss, *torch.autograd.grad(loss, [fl])

        def composed_smooth():
            fl = flow.detach().requires_grad_()
            loss = lc.smooth_compose(fl, f0, order, 150.0, 255.0)
            return loss, *torch.autograd.grad(loss, [fl])

        n, a = native_smooth(), composed_smooth()
        rel = [abs(float(n[0].detach()) - float(a[0].detach())) / float(a[0].detach()),
               float((n[1] - a[1]).norm() / a[1].norm())]
        del n, a
        t = _alternate({"native": native_smooth, "torch": composed_smooth}, reps, windows)
        row.update({f"smooth{order}_fb_native_ms": t["native"], f"smooth{order}_fb_torch_ms": t["torch"],
                    f"smooth{order}_fb_native_mib": peak_mib(native_smooth, dev),
                    f"smooth{order}_fb_torch_mib": peak_mib(composed_smooth, dev), f"smooth{order}_rel_diff": rel})
        print(f"{name}: smoothness order {order} fwd+bwd native {t['native']:.3f} ms torch {t['torch']:.3f} ms | peak native "
              f"{row[f'smooth{order}_fb_native_mib']:.0f} MiB torch {row[f'smooth{order}_fb_torch_mib']:.0f} MiB | rel diff "
              f"{['%.1e' % v for v in rel]}", flush=True)

    # a 12-prediction sequence loss, forward + backward
    flows = [flow + 0.1 * i for i in range(seq_preds)]

    def native_seq():
        preds = [f.detach().requires_grad_() for f in flows]
        loss = unsupervised_sequence_loss(preds, f0, f1, mask)
        return loss, *torch.autograd.grad(loss, preds)

    def composed_seq():
        preds = [f.detach().requires_grad_() for f in flows]
        loss = 0.0
        for i, fl in enumerate(preds):
            warped = warp(f1, normalize(fl), align_corners=True)
            term = lc.census_compose(f0, warped, mask, 7, 255.0)[0] + lc.smooth_compose(fl, f0, 1, 150.0, 255.0)
            loss = loss + 0.8 ** (seq_preds - 1 - i) * term
        return loss, *torch.autograd.grad(loss, preds)

    n, a = native_seq(), composed_seq()
    row["seq_rel_diff"] = abs(float(n[0].detach()) - float(a[0].detach())) / float(a[0].detach())
    del n, a
    t = _alternate({"native": native_seq, "torch": composed_seq}, max(1, reps // 4), windows)
    row.update(seq_preds=seq_preds, seq_fb_native_ms=t["native"], seq_fb_torch_ms=t["torch"],
               seq_fb_native_mib=peak_mib(native_seq, dev), seq_fb_torch_mib=peak_mib(composed_seq, dev))
    print(f"{name}: {seq_preds}-prediction unsupervised_sequence_loss fwd+bwd native {t['native']:.3f} ms torch "
          f"{t['torch']:.3f} ms ({t['torch'] / t['native']:.1f} x) | peak native {row['seq_fb_native_mib']:.0f} MiB torch "
          f"{row['seq_fb_torch_mib']:.0f} MiB | loss rel diff {row['seq_rel_diff']:.1e}", flush=True)
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--preds", type=int, default=12)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "losses", "losses_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "losses_bench needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    rows = [bench_shape(name, SHAPES[name], args.reps, args.windows, args.preds, dev) for name in args.shapes]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, rows=rows)) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
