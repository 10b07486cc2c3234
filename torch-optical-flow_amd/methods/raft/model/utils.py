"""``model.utils`` drop-in (reference: methods/raft/model/utils.py:38-91), plus ``forward_interpolate``, the warm-start
initialiser of upstream RAFT's video mode that produces ``RAFT.forward``'s ``flow_init``."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from optical_flow import _native


class InputPadder:
    """Pads images such that dimensions are divisible by 8 (`utils.py:38-61`): replicate padding, symmetric in
    'sintel' mode, left/right + bottom only in every other mode (Q10)."""

    def __init__(self, dims: Sequence[int], mode: str = "sintel") -> None:
        self.ht, self.wd = dims[-2:]
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs: Tensor) -> List[Tensor]:
        # GPU fp32 frames (the inference inputs): every frame in one native launch (oflow_replicate_pad_f32, a copy,
        # bit-exact); anything else (CPU, autograd, other dtypes) through F.pad as the reference
        if (1 <= len(inputs) <= 4 and all(isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32
                                          and x.dim() >= 2 and x.shape == inputs[0].shape for x in inputs)
                and not (torch.is_grad_enabled() and any(x.requires_grad for x in inputs))):
            return _native.replicate_pad(inputs, self._pad)
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x: Tensor) -> Tensor:
        ht, wd = x.shape[-2:]
        c = [self._pad[2], ht - self._pad[3], self._pad[0], wd - self._pad[1]]
        return x[..., c[0] : c[1], c[2] : c[3]]


def bilinear_sampler(
    img: Tensor, coords: Tensor, mode: str = "bilinear", mask: bool = False
) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """grid_sample with pixel coordinates, align_corners=True, zeros padding (`utils.py:64-80`); like the
    reference it ignores ``mode``. Sampling runs on the gfx950 ``grid_sample`` kernel."""
    h, w = img.shape[-2:]
    xgrid, ygrid = coords.split([1, 1], dim=-1)
    xgrid = 2 * xgrid / (w - 1) - 1
    ygrid = 2 * ygrid / (h - 1) - 1
    grid = torch.cat([xgrid, ygrid], dim=-1)
    out = _native.grid_sample(img, grid, "bilinear", "zeros", True)
    if mask:
        m = (xgrid > -1) & (ygrid > -1) & (xgrid < 1) & (ygrid < 1)
        return out, m.float()
    return out


def coords_grid(batch: int, ht: int, wd: int, device: Optional[torch.device] = None) -> Tensor:
    """(B, 2, ht, wd) fp32, channel 0 = x (column index), channel 1 = y (row index) (`utils.py:83-86`).
    ``device`` (an addition) builds it in place instead of on the CPU + copy (`raft.py:68-69`)."""
    ys, xs = torch.meshgrid(
        torch.arange(ht, device=device, dtype=torch.float32),
        torch.arange(wd, device=device, dtype=torch.float32),
        indexing="ij",
    )
    return torch.stack((xs, ys), dim=0)[None].repeat(batch, 1, 1, 1)


def forward_interpolate(flow: Tensor) -> Tensor:
    """The warm-start initialiser of RAFT's video mode: ``flow`` -- (2, H, W) as upstream RAFT's ``forward_interpolate``
    takes it, or (B, 2, H, W); fp32, channel 0 = dx, 1 = dy, in practice the low-resolution flow a test-mode forward
    returns first -- projected forward along itself, to be passed as ``flow_init`` of the next pair of the sequence.

    Per image, with all selection arithmetic in float64: source pixel ``s = y * W + x`` lands at ``(x + dx[s], y + dy[s])``
    and counts iff ``0 < x1 < W and 0 < y1 < H`` (a NaN or infinite flow never lands); every grid pixel takes the fp32
    flow of the landed source with the least squared distance to it, ties to the lowest ``s``; an image in which nothing
    lands gives zeros (a cold start). Where no two candidates tie this is scipy's ``griddata(method="nearest")`` of
    upstream bit for bit. Same shape, dtype and device as the input, which is detached: the result carries no gradient.

    GPU tensors run one kernel on the current stream (``torch.ops.oflow.forward_interpolate``, no host sync); CPU tensors
    run the same selection as a plain torch float64 composition."""
    if not isinstance(flow, Tensor):
        raise TypeError(f"forward_interpolate: flow must be a torch.Tensor, got {type(flow).__name__}")
    if flow.dtype != torch.float32:
        raise TypeError(f"forward_interpolate: flow must be float32, got {flow.dtype}")
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise ValueError(f"forward_interpolate: flow must be (2, H, W) or (B, 2, H, W), got {tuple(flow.shape)}")
    fl = flow.detach()
    fl = fl[None] if flow.dim() == 3 else fl
    out = _native.forward_interpolate(fl) if fl.is_cuda else _forward_interpolate_torch(fl)
    return out[0] if flow.dim() == 3 else out


def _forward_interpolate_torch(flow: Tensor) -> Tensor:
    """``forward_interpolate`` of a (B, 2, H, W) fp32 tensor in plain torch (the CPU path): explicit float64 squared
    distances ``dx * dx + dy * dy`` (each operation rounded once) from a chunk of queries to the landed sources in
    index order, and ``argmin``, which returns the first minimum: the lowest source index."""
    b, _, h, w = flow.shape
    n = h * w
    out = torch.zeros((b, 2, n), dtype=torch.float32, device=flow.device)
    s = torch.arange(n, device=flow.device)
    qx, qy = (s % max(w, 1)).double(), (s // max(w, 1)).double()
    for i in range(b):
        f = flow[i].reshape(2, n)
        x1, y1 = qx + f[0].double(), qy + f[1].double()
        landed = ((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)).nonzero().squeeze(1)  # ascending source indices
        if landed.numel() == 0:
            continue  # nothing landed: zeros
        lx, ly = x1[landed], y1[landed]
        chunk = max(1, (1 << 22) // landed.numel())  # <= 32 MiB per float64 temporary
        for q0 in range(0, n, chunk):
            dx = qx[q0:q0 + chunk, None] - lx[None]
            dy = qy[q0:q0 + chunk, None] - ly[None]
            out[i, :, q0:q0 + chunk] = f[:, landed[(dx * dx + dy * dy).argmin(dim=1)]]
    return out.view(b, 2, h, w)


def upflow8(flow: Tensor, mode: str = "bilinear") -> Tensor:
    """8x bilinear upsampling of a flow field, magnitudes x8 (`utils.py:89-91`)."""
    new_size = (8 * flow.shape[2], 8 * flow.shape[3])
    return 8 * F.interpolate(flow, size=new_size, mode=mode, align_corners=True)
