"""Generate tests/golden/metrics_small.npz by running the REFERENCE's metrics and sequence loss (CPU, fp32).

Runs only where /root/reference exists; exits 0 with a message elsewhere. The reference is imported by file path, as
gen_goldens.py does; its imports of ``torchmetrics`` / ``pytorch_lightning`` / ``wandb`` are met by stand-in modules
registered here. The ``torchmetrics.Metric`` stand-in is functional, because the metric classes do their work through
it: ``add_state`` sets the attribute, calling the metric updates it and returns ``compute()``. Nothing from the
reference is copied into the repository; only its outputs and checksums of the inputs are written. The inputs come from
tests/metrics_cases.py (the repository's hash generators), which the tests re-run bit for bit.

Usage:  python tests/golden/gen_metrics_goldens.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def _load_by_path(name: str, path: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _load_by_path("oflow_metrics_cases", os.path.join(TESTS, "metrics_cases.py"))


def _install_stand_ins() -> None:
    class Metric(nn.Module):
        """What the reference's metrics use of torchmetrics.Metric, in one process: states are attributes holding
        their defaults, a call is update() followed by compute()."""

        def add_state(self, name, default, dist_reduce_fx=None):
            setattr(self, name, default.clone())

        def forward(self, *args, **kwargs):
            self.update(*args, **kwargs)
            return self.compute()

    class LightningModule(nn.Module):
        def save_hyperparameters(self):
            self.hparams = types.SimpleNamespace(
                **{k: v for k, v in sys._getframe(1).f_locals.items() if k not in ("self", "__class__")})

    mods = {name: types.ModuleType(name) for name in ("torchmetrics", "pytorch_lightning", "pytorch_lightning.loggers", "wandb")}
    mods["torchmetrics"].Metric = Metric
    mods["pytorch_lightning"].LightningModule = LightningModule
    mods["pytorch_lightning"].loggers = mods["pytorch_lightning.loggers"]
    mods["pytorch_lightning.loggers"].WandbLogger = type("WandbLogger", (), {})
    mods["wandb"].Image = type("Image", (), {})
    for name, mod in mods.items():
        sys.modules.setdefault(name, mod)


def main() -> int:
    if not os.path.isdir(REF):
        print("gen_metrics_goldens: /root/reference absent; the fixture is committed, nothing to do")
        return 0
    _install_stand_ins()
    sys.path[:0] = [os.path.join(REF, "methods", "raft"), REF]
    from model.raft import sequence_loss  # the reference's
    from optical_flow.metrics import AverageEndPointError, OutlierRatio
    from optical_flow.metrics.epe import end_point_error

    out = {}
    for name in cases.METRIC_CASES:
        pred, target, valid = cases.metric_case(name)
        valid = None if valid is None else valid.contiguous()  # (the reference flattens it with .view(-1))
        out[f"{name}_checksum"] = np.stack([cases.checksum(pred), cases.checksum(target)])
        out[f"{name}_epe_mean"] = end_point_error(pred, target).numpy()
        epe_map = end_point_error(pred, target, reduce=False)
        if epe_map.numel() <= 4096:
            out[f"{name}_epe_map"] = epe_map.numpy()
        out[f"{name}_epe_map_checksum"] = cases.checksum(epe_map)
        aepe, f1 = AverageEndPointError(), OutlierRatio()
        out[f"{name}_aepe"] = aepe(pred, target, valid).numpy()
        out[f"{name}_f1"] = f1(pred, target, valid).numpy()
        out[f"{name}_total"] = np.array(int(aepe.total), dtype=np.int64)
        out[f"{name}_aepe_novalid"] = AverageEndPointError()(pred, target).numpy()
        out[f"{name}_f1_novalid"] = OutlierRatio()(pred, target).numpy()
    # a tighter outlier definition, and several updates of one metric
    pred, target, valid = cases.metric_case("vec3")
    out["vec3_f1_abs1_rel10"] = OutlierRatio(abs_threshold=1.0, rel_threshold=0.1)(pred, target, valid).numpy()
    aepe, f1 = AverageEndPointError(), OutlierRatio()
    for name in ("vec3", "vec30", "crop"):
        pred, target, valid = cases.metric_case(name)
        aepe.update(pred, target, valid.contiguous())
        f1.update(pred, target, valid.contiguous())
    out["multi_aepe"] = aepe.compute().numpy()
    out["multi_f1"] = f1.compute().numpy()

    for name in cases.LOSS_CASES:
        preds, gt, valid = cases.loss_case(name)
        preds = [p.clone().requires_grad_() for p in preds]
        loss, metrics = sequence_loss(preds, gt, valid, gamma=cases.GAMMA, max_flow=cases.MAX_FLOW)
        loss.backward()
        out[f"{name}_checksum"] = np.stack([cases.checksum(gt), cases.checksum(valid)] + [cases.checksum(p) for p in preds])
        out[f"{name}_loss"] = loss.detach().numpy()
        out[f"{name}_px"] = np.array([metrics["1px"], metrics["3px"], metrics["5px"]], dtype=np.float64)
        idx = torch.tensor(cases.grad_probe_indices(gt.numel()))
        which = sorted({0, len(preds) // 2, len(preds) - 1})
        out[f"{name}_grad_preds"] = np.array(which, dtype=np.int64)
        out[f"{name}_grad_index"] = idx.numpy()
        out[f"{name}_grad"] = np.stack([preds[i].grad.reshape(-1)[idx].numpy() for i in which])
        out[f"{name}_grad_checksum"] = np.stack([cases.checksum(preds[i].grad) for i in which])
    np.savez_compressed(os.path.join(HERE, "metrics_small.npz"), **out)
    print("wrote metrics_small.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "metrics_small.npz")), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
