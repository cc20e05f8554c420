"""RandomResizedCrop box sampling (``--random-resized-crop``), pure torch and free of host syncs.

The published rule (Szegedy et al., "Going deeper with convolutions"; the usual ImageNet ResNet recipe): per sample,
up to ``TRIES`` times draw a target area as a uniform fraction ``scale`` of the image and an aspect ratio
log-uniform in ``ratio``; the first draw whose box fits the image wins, at a uniform position; when none fits, the
centre crop at the aspect clamped into ``ratio``. It is vectorised over the batch here -- all tries of all samples
are drawn at once and the first fitting one selected with tensor ops -- so the boxes can be made on the compute
device from a device generator while the host runs ahead. The boxes feed ``ops.misc.rrc_normalize_u8`` (one fused
HIP kernel: crop, antialiased resize, normalise, flip) or the torch backend of ``data.loader.InputTransform``.

Boxes are int32 ``[B, 4]`` rows ``(top, left, h, w)``. The arithmetic is float64 so that it equals a plain
per-sample loop in Python floats on the same uniforms.
"""

from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch

TRIES = 10
DEFAULT_SCALE = (0.08, 1.0)
DEFAULT_RATIO = (3.0 / 4.0, 4.0 / 3.0)


def check_ranges(scale: Sequence[float], ratio: Sequence[float]) -> None:
    """ValueError unless 0 < scale[0] <= scale[1] <= 1 and 0 < ratio[0] <= ratio[1]."""
    if len(scale) != 2 or not (0.0 < scale[0] <= scale[1] <= 1.0):
        raise ValueError(f"scale range {tuple(scale)}: need 0 < lo <= hi <= 1 (fractions of the image area)")
    if len(ratio) != 2 or not (0.0 < ratio[0] <= ratio[1]) or not math.isfinite(ratio[1]):
        raise ValueError(f"aspect ratio range {tuple(ratio)}: need 0 < lo <= hi")


def boxes_from_uniforms(u_area: torch.Tensor, u_logr: torch.Tensor, u_pos: torch.Tensor, Hs: int, Ws: int,
                        scale: Sequence[float] = DEFAULT_SCALE,
                        ratio: Sequence[float] = DEFAULT_RATIO) -> torch.Tensor:
    """Boxes from uniforms in [0, 1): ``u_area`` / ``u_logr`` [B, T] (try t's area and log-aspect draws), ``u_pos``
    [B, 2] (top, left) -> int32 [B, 4] = (top, left, h, w)."""
    check_ranges(scale, ratio)
    f64 = torch.float64
    ua, ul, up = u_area.to(f64), u_logr.to(f64), u_pos.to(f64)
    area = float(Hs * Ws) * (scale[0] + (scale[1] - scale[0]) * ua)
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    aspect = torch.exp(lr0 + (lr1 - lr0) * ul)
    w = torch.round(torch.sqrt(area * aspect)).to(torch.int64)
    h = torch.round(torch.sqrt(area / aspect)).to(torch.int64)
    fits = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)  # [B, T]
    first = torch.argmax(fits.to(torch.uint8), dim=1, keepdim=True)  # the first fitting try (0 when none fits)
    any_fit = fits.any(dim=1)
    # no try fits: the centre crop at the image's aspect clamped into `ratio`
    in_ratio = Ws / Hs
    if in_ratio < ratio[0]:
        fw, fh = Ws, min(Hs, int(round(Ws / ratio[0])))
    elif in_ratio > ratio[1]:
        fh, fw = Hs, min(Ws, int(round(Hs * ratio[1])))
    else:
        fw, fh = Ws, Hs
    fw, fh = max(fw, 1), max(fh, 1)
    wb = torch.where(any_fit, w.gather(1, first).squeeze(1), torch.full_like(first.squeeze(1), fw))
    hb = torch.where(any_fit, h.gather(1, first).squeeze(1), torch.full_like(first.squeeze(1), fh))
    top = torch.floor(up[:, 0] * (Hs - hb + 1).to(f64)).to(torch.int64)
    left = torch.floor(up[:, 1] * (Ws - wb + 1).to(f64)).to(torch.int64)
    top = torch.where(any_fit, top, (Hs - hb) // 2)
    left = torch.where(any_fit, left, (Ws - wb) // 2)
    top = torch.minimum(top.clamp_min(0), Hs - hb)
    left = torch.minimum(left.clamp_min(0), Ws - wb)
    return torch.stack([top, left, hb, wb], 1).to(torch.int32).contiguous()


def sample_boxes(B: int, Hs: int, Ws: int, scale: Sequence[float] = DEFAULT_SCALE,
                 ratio: Sequence[float] = DEFAULT_RATIO, generator: torch.Generator = None,
                 device=None) -> torch.Tensor:
    """``B`` boxes in an ``Hs`` x ``Ws`` image: the uniforms are drawn on ``device`` from ``generator`` (one launch,
    no host sync) and handed to :func:`boxes_from_uniforms`."""
    u = torch.rand((B, 2 * TRIES + 2), generator=generator, device=device, dtype=torch.float32)
    return boxes_from_uniforms(u[:, :TRIES], u[:, TRIES:2 * TRIES], u[:, 2 * TRIES:], Hs, Ws, scale, ratio)


def center_box(Hs: int, Ws: int, frac: float) -> Tuple[int, int, int, int]:
    """(top, left, h, w) of the centred ``round(frac * Hs)`` x ``round(frac * Ws)`` box."""
    if not (0.0 < frac <= 1.0):
        raise ValueError(f"centre crop fraction {frac}: need 0 < frac <= 1")
    h = min(Hs, max(1, int(round(frac * Hs))))
    w = min(Ws, max(1, int(round(frac * Ws))))
    return ((Hs - h) // 2, (Ws - w) // 2, h, w)
