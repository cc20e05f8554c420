"""TrivialAugmentWide (``--trivialaugment``; Mueller and Hutter, "TrivialAugment: Tuning-free Yet State-of-the-Art
Data Augmentation"): a table of draws over the 14 ops of ``data/randaug.py``, and the stage that applies them.

Every training image goes through ONE op, chosen uniformly from the 14, at a magnitude bin drawn uniformly from 0 ..
30, with a random sign where the op is signed -- torchvision's ``TrivialAugmentWide``. The ops, their integer rules and
both backends (``ops.misc.randaug_u8`` and ``randaug_torch``) are RandAugment's, unchanged: the stage only draws other
rows ``(op, a0 .. a6)``, ``params`` int32 [B, 1, 8]. With ``f = bin / 30``:

===================================== ==========================================
op                                    argument
===================================== ==========================================
ShearX / ShearY                       s = +-0.99 f
TranslateX                            t = +-round(32 f W / 224) whole pixels
TranslateY                            the same with H
Rotate                                theta = +-135 f degrees
Brightness, Color, Contrast,          F = round(256 (1 +- 0.99 f))
Sharpness
Posterize                             bits = 8 - round(bin / 5): 8 .. 2
Solarize                              a0 = ceil(255 (1 - f))
Identity, AutoContrast, Equalize      none
===================================== ==========================================

The translation is torchvision's: up to 32 pixels of a 224-pixel image. The stage runs on the batch as stored, ahead
of the crop, so the 32 pixels are scaled to the stored size (``32 W / 224``): after a crop that resamples the stored
image to 224 pixels they are 32 pixels of the model input for a full-size box, and more for a smaller one.
"""

from __future__ import annotations

import functools
import math
from typing import List, Optional

import torch

from .randaug import (AUTOCONTRAST, BRIGHTNESS, COLOR, CONTRAST, EQUALIZE, IDENTITY, NUM_OPS, POSTERIZE, ROTATE,
                      SHARPNESS, SHEAR_X, SHEAR_Y, SOLARIZE, TRANSLATE_X, TRANSLATE_Y, affine_args, randaug_torch)

NUM_BINS = 31


def ta_op_args(op: int, bin_: int, negative: bool, H: int, W: int) -> List[int]:
    """``(a0 .. a6)`` of op ``op`` at bin ``bin_`` (0 .. 30) with the given sign, for ``H`` x ``W`` images (Python
    floats)."""
    if int(bin_) != bin_ or not (0 <= bin_ < NUM_BINS):
        raise ValueError(f"bin {bin_}: 0 .. {NUM_BINS - 1}")
    f = bin_ / (NUM_BINS - 1)
    sg = -1.0 if negative else 1.0
    if op == SHEAR_X:
        return affine_args(1.0, sg * 0.99 * f, 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return affine_args(1.0, 0.0, 0.0, sg * 0.99 * f, 1.0, 0.0)
    if op == TRANSLATE_X:
        return affine_args(1.0, 0.0, -2.0 * sg * round(32.0 * f * W / 224.0), 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return affine_args(1.0, 0.0, 0.0, 0.0, 1.0, -2.0 * sg * round(32.0 * f * H / 224.0))
    if op == ROTATE:
        th = math.radians(sg * 135.0 * f)
        return affine_args(math.cos(th), -math.sin(th), 0.0, math.sin(th), math.cos(th), 0.0)
    if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        return [int(round(256.0 * (1.0 + sg * 0.99 * f)))] + [0] * 6
    if op == POSTERIZE:
        bits = 8 - int(round(bin_ / 5.0))
        return [(0xFF << (8 - bits)) & 0xFF] + [0] * 6
    if op == SOLARIZE:
        return [int(math.ceil(255.0 * (1.0 - f)))] + [0] * 6
    if op in (IDENTITY, AUTOCONTRAST, EQUALIZE):
        return [0] * 7
    raise ValueError(f"op {op}: 0 .. {NUM_OPS - 1}")


@functools.lru_cache(maxsize=16)
def _table(H: int, W: int, device: str) -> torch.Tensor:
    """int32 [31, 14, 2, 7]: ``(a0 .. a6)`` of every bin and op with the positive (0) and the negative (1) sign, on
    ``device`` (made once per image size and device: the draws then index it without touching the host)."""
    rows = [[[ta_op_args(op, b, neg, H, W) for neg in (False, True)] for op in range(NUM_OPS)]
            for b in range(NUM_BINS)]
    return torch.tensor(rows, dtype=torch.int32).to(device)


def params_from_uniforms(u_op: torch.Tensor, u_bin: torch.Tensor, u_sign: torch.Tensor, H: int,
                         W: int) -> torch.Tensor:
    """``params`` int32 [..., 8] from uniforms in [0, 1) of equal shape: ``op = min(13, floor(14 u_op))``, ``bin =
    min(30, floor(31 u_bin))``, the negative sign where ``u_sign < 0.5`` (ignored by the ops that have none)."""
    op = torch.floor(u_op.to(torch.float64) * NUM_OPS).to(torch.int64).clamp(0, NUM_OPS - 1)
    b = torch.floor(u_bin.to(torch.float64) * NUM_BINS).to(torch.int64).clamp(0, NUM_BINS - 1)
    neg = (u_sign.to(torch.float64) < 0.5).to(torch.int64)
    args = _table(int(H), int(W), str(u_op.device))[b, op, neg]
    return torch.cat([op.to(torch.int32).unsqueeze(-1), args], -1).contiguous()


def sample_params(B: int, H: int, W: int, generator: Optional[torch.Generator] = None, device=None) -> torch.Tensor:
    """``params [B, 1, 8]`` for ``B`` images of ``H`` x ``W`` pixels: the uniforms are drawn on ``device`` from
    ``generator`` (one ``torch.rand`` launch, no host sync) and handed to :func:`params_from_uniforms`."""
    u = torch.rand((B, 1, 3), generator=generator, device=device, dtype=torch.float32)
    return params_from_uniforms(u[..., 0], u[..., 1], u[..., 2], H, W)


class TrivialAugmentWide:
    """TrivialAugmentWide of every training batch: ``ta(u8) -> u8`` on the uint8 NHWC batch as stored -- the
    interface of :class:`~imagent_amd.data.randaug.RandAugment`, for ``InputTransform(randaug=...)``.

    ``backend`` ``hip`` / ``hip_f32``: ``ops.misc.randaug_u8``. ``torch``: ``randaug_torch`` -- the ``--kernels torch``
    / CPU path and the oracle of the tests. The draws come from a generator of the stage's own on the compute device,
    reseeded from (seed, rank, epoch) by :meth:`set_epoch`, so a resumed epoch repeats them."""

    num_ops = 1

    def __init__(self, backend: str, fill: int = 128, seed: int = 0, rank: int = 0):
        if backend not in ("hip", "hip_f32", "torch"):
            raise ValueError(f"backend {backend!r}: hip, hip_f32 or torch")
        if int(fill) != fill or not (0 <= fill <= 255):
            raise ValueError(f"fill {fill}: need 0 <= V <= 255")
        self.backend, self.fill = backend, int(fill)
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0
        self._gen = None

    def _epoch_seed(self) -> int:
        # other constants than the crop's, the mixer's, RandAugment's and the eraser's streams of draws
        return (self.seed * 0xC6BC2796 + self.rank * 0x8A5CD789 + self.epoch * 0xF1357AEA + 43) % (2 ** 63 - 1)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        if self._gen is not None:
            self._gen.manual_seed(self._epoch_seed())

    def _generator(self, device) -> torch.Generator:
        if self._gen is None or self._gen.device != torch.device(device):
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._epoch_seed())
        return self._gen

    def draw(self, B: int, H: int, W: int, device) -> torch.Tensor:
        """The next batch's ``params [B, 1, 8]`` from the stage's generator."""
        return sample_params(B, H, W, self._generator(device), device)

    def __call__(self, u8: torch.Tensor, params: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``params``: explicit draws instead of the stage's own (comparing backends on identical draws)."""
        B, H, W, _ = u8.shape
        if params is None:
            params = self.draw(B, H, W, u8.device)
        params = params.to(device=u8.device, dtype=torch.int32)
        if self.backend in ("hip", "hip_f32"):
            from ..ops.misc import randaug_u8
            return randaug_u8(u8.contiguous(), params, self.fill)
        return randaug_torch(u8, params, self.fill)
