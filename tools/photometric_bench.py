"""The photometric losses (optical_flow.losses.ssim_loss / charbonnier_loss), measured (DESIGN.md §4 "losses").

Shapes: ``8 x 3 x 436 x 1024`` (Sintel) and ``8 x 3 x 368 x 496`` (a Chairs crop), frames of integer levels with the
second frame a noisy copy, a 70 % mask. Per shape, for the SSIM loss at window 3 (box) and window 11 (Gaussian, sigma
1.5), forward and forward + backward (both frame gradients), time and ``torch.cuda.max_memory_allocated``:

* the native op;
* the package's torch composition on the same GPU (tests/photometric_cases.py: the kernel's arithmetic step by step,
  one shifted plane per window offset; it is the CPU path, written for accuracy, and slow at window 11);
* the SSIM people usually write, ``textbook_ssim`` below: five depthwise ``conv2d`` passes per frame pair and the plain
  quotient in fp32 under ATen autograd. It is the fair speed baseline; it does not have the contract's accuracy on
  near-identical frames.

The same for the Charbonnier loss (alpha 0.45), native against its composition. Each pair is timed with device events
over windows of back-to-back calls, alternated window by window, median of the windows; the native and the composed
results are compared before their times are. Needs a ROCm GPU; prints a table and writes one JSON line (default:
profiles/photometric/photometric_bench.json).

    python tools/photometric_bench.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "torch-optical-flow_amd"),
          os.path.join(REPO, "torch-optical-flow_amd", "methods", "raft")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_backward_bench import _alternate  # noqa: E402
from losses_bench import SHAPES, inputs, peak_mib  # noqa: E402

WINDOWS = ((3, None), (11, 1.5))


def textbook_ssim(f0, f1, mask, weights, c1, c2):
    """(1 - SSIM) / 2 averaged under the mask, the way it is usually written: E[x], E[y], E[x^2], E[y^2], E[xy] by a
    depthwise "valid" conv2d each, the plain quotient, fp32, ATen autograd."""
    c = f0.shape[1]
    w1 = torch.tensor(weights, device=f0.device, dtype=f0.dtype)
    kernel = (w1[:, None] * w1[None, :]).expand(c, 1, -1, -1).contiguous()
    filt = lambda t: F.conv2d(t, kernel, groups=c)  # noqa: E731
    mx, my = filt(f0), filt(f1)
    vx, vy, cxy = filt(f0 * f0) - mx * mx, filt(f1 * f1) - my * my, filt(f0 * f1) - mx * my
    ssim = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    d = (0.5 * (1 - ssim)).mean(dim=1, keepdim=True)
    r = len(weights) // 2
    m = mask[:, :, r:mask.shape[2] - r, r:mask.shape[3] - r].to(d.dtype)
    return (m * d).sum() / (m.sum() + 1e-6)


def bench_shape(name, shape, reps, windows, dev):
    from optical_flow import charbonnier_loss, ssim_loss
    from optical_flow.losses import charbonnier_loss_torch, ssim_loss_torch, ssim_window

    f0, f1, mask, _ = inputs(shape, dev)
    row = dict(shape=name, dims=list(shape))

    def runner(fn, backward):
        def run():
            a, b = f0.detach().requires_grad_(backward), f1.detach().requires_grad_(backward)
            with torch.set_grad_enabled(backward):
                loss = fn(a, b)
            return (loss, *torch.autograd.grad(loss, [a, b])) if backward else (loss,)
        return run

    def compare(n, a):
        return [abs(float(n[0].detach()) - float(a[0].detach())) / float(a[0].detach())] + \
            [float((p - q).norm() / q.norm()) for p, q in zip(n[1:], a[1:])]

    for window, sigma in WINDOWS:
        wt = ssim_window(window, sigma)
        c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
        fns = {"native": lambda a, b: ssim_loss(a, b, mask, window, sigma),
               "composition": lambda a, b: ssim_loss_torch(a, b, mask, wt, c1, c2)[0],
               "conv2d": lambda a, b: textbook_ssim(a, b, mask, wt, c1, c2)}
        key = f"ssim{window}"
        n, a, t = (runner(fns[k], True)() for k in ("native", "composition", "conv2d"))
        row[key + "_rel_diff_composition"], row[key + "_rel_diff_conv2d"] = compare(n, a), compare(n, t)
        del n, a, t
        for tag, backward in (("fwd", False), ("fb", True)):
            fast = _alternate({k: runner(fns[k], backward) for k in ("native", "conv2d")}, reps, windows)
            slow = _alternate({"composition": runner(fns["composition"], backward)}, 1, 3)
            for k, v in {**fast, **slow}.items():
                row[f"{key}_{tag}_{k}_ms"] = v
        for k in fns:
            row[f"{key}_fb_{k}_mib"] = peak_mib(runner(fns[k], True), dev)
        print(f"{name} {shape} ssim window {window} sigma {sigma}: "
              + " | ".join(f"{tag} native {row[f'{key}_{tag}_native_ms']:.3f} ms conv2d {row[f'{key}_{tag}_conv2d_ms']:.3f} ms "
                           f"composition {row[f'{key}_{tag}_composition_ms']:.1f} ms" for tag in ("fwd", "fb"))
              + " | fwd+bwd peak " + " ".join(f"{k} {row[f'{key}_fb_{k}_mib']:.0f} MiB" for k in fns)
              + f" | rel diff vs composition {['%.1e' % v for v in row[key + '_rel_diff_composition']]}"
              + f" vs conv2d {['%.1e' % v for v in row[key + '_rel_diff_conv2d']]}", flush=True)

    alpha = 0.45
    fns = {"native": lambda a, b: charbonnier_loss(a, b, mask, 1e-3, alpha),
           "composition": lambda a, b: charbonnier_loss_torch(a, b, mask, 1e-3, alpha, 255.0)}
    n, a = (runner(fns[k], True)() for k in fns)
    row["charb_rel_diff"] = compare(n, a)
    del n, a
    for tag, backward in (("fwd", False), ("fb", True)):
        for k, v in _alternate({k: runner(fns[k], backward) for k in fns}, reps, windows).items():
            row[f"charb_{tag}_{k}_ms"] = v
    for k in fns:
        row[f"charb_fb_{k}_mib"] = peak_mib(runner(fns[k], True), dev)
    print(f"{name} {shape} charbonnier alpha {alpha}: "
          + " | ".join(f"{tag} native {row[f'charb_{tag}_native_ms']:.3f} ms composition {row[f'charb_{tag}_composition_ms']:.3f} ms"
                       for tag in ("fwd", "fb"))
          + f" | fwd+bwd peak native {row['charb_fb_native_mib']:.0f} MiB composition {row['charb_fb_composition_mib']:.0f} MiB"
          + f" | rel diff {['%.1e' % v for v in row['charb_rel_diff']]}", flush=True)
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "photometric", "photometric_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "photometric_bench needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    rows = [bench_shape(name, SHAPES[name], args.reps, args.windows, dev) for name in args.shapes]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(dict(device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, rows=rows)) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
