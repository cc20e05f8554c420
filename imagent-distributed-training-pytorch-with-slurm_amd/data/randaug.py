"""RandAugment (``--randaugment``; Cubuk et al., "RandAugment: Practical automated data augmentation with a reduced
search space"): the definition in integer arithmetic, the per-sample draws, pure torch and free of host syncs, and
the stage that applies them to the uint8 batch.

Every training image goes through ``L`` layers. A layer is one op of the table below, chosen uniformly (no apply
probability), at magnitude ``m`` of 31 bins (0 .. 30) with a random sign where the op is signed -- torchvision's
``RandAugment``. Every float step of the usual implementations is replaced by a stated integer rule, so the HIP
kernels (``csrc/kernels/randaug.hip`` through ``ops.misc.randaug_u8``) and :func:`randaug_torch` agree bit for bit.

The draws are one int32 tensor ``params [B, L, 8]``, rows ``(op, a0 .. a6)``; both backends read nothing else. Layers
apply in order: layer l sees layer l - 1's output, also for its whole-image statistics. With ``f = m / 30``:

== ===================== ===================================================================== ======
id op                    argument (float64 on the host, then rounded as stated)                signed
== ===================== ===================================================================== ======
0  Identity
1  ShearX                s = +-0.3 f, M = [[1, s], [0, 1]]                                     yes
2  ShearY                s = +-0.3 f, M = [[1, 0], [s, 1]]                                     yes
3  TranslateX            t = +-round(150 / 331 f W) whole pixels, the content moves by +t      yes
4  TranslateY            the same with H                                                       yes
5  Rotate                theta = +-30 f degrees, counter-clockwise as displayed,               yes
                         M = [[cos, -sin], [sin, cos]]
6  Brightness            F = round(256 (1 +- 0.9 f)), d = 0                                    yes
7  Color (saturation)    the same F, d = the pixel's gray                                      yes
8  Contrast              the same F, d = the image's mean gray                                 yes
9  Sharpness             the same F, d = the pixel of the smoothed image                       yes
10 Posterize             a0 = (0xFF << (8 - bits)) & 0xFF, bits = 8 - round(4 f)
11 Solarize              a0 = ceil(255 (1 - f))
12 AutoContrast
13 Equalize
== ===================== ===================================================================== ======

Affine ops (1 - 5): ``M`` maps an output pixel to its source (the inverse map), ``a0 .. a5 = round(65536 (m00, m01,
m02, m10, m11, m12))`` in doubled, centred pixel units. For output pixel (x, y): ``X = 2x - (W - 1)``, ``Y = 2y -
(H - 1)``, ``sx = (m00 X + m01 Y + m02 + (W << 16)) >> 17``, ``sy = (m10 X + m11 Y + m12 + (H << 16)) >> 17`` in
64-bit integers with an arithmetic shift (floor); the output is source pixel (sx, sy) where that lies in the image,
else the fill colour (nearest neighbour). A translation by t pixels is ``m02 = -2 t 65536``; the identity matrix
gives ``sx = x``.

Colour ops: ``blend(v, d, F) = clamp((F v + (256 - F) d + 128) >> 8, 0, 255)`` per channel (F may exceed 256, the
shift is arithmetic), ``gray = (77 r + 150 g + 29 b + 128) >> 8``, the mean gray ``(sum + n / 2) / n`` over the
image's ``n = H W`` pixels, the smoothed image ``(3x3 sum + 4 centre + 6) / 13`` inside and the pixel itself on the
first and last row and column (an image with H < 3 or W < 3 is unchanged by Sharpness).

Posterize: ``v & a0``. Solarize: ``255 - v`` where ``v >= a0``; at ``m = 0`` the threshold is 255, so a pixel of 255
becomes 0 -- as in PIL and torchvision, and kept. AutoContrast, per channel with the image's extremes lo, hi:
unchanged when ``lo == hi``, else ``((v - lo) 255 + (hi - lo) / 2) / (hi - lo)``. Equalize, per channel with
histogram h and ``last`` the count of the highest non-empty bin: ``step = (n - last) / 255``; unchanged when ``step
== 0``, else ``lut[i] = min(255, (sum_{j < i} h[j] + step / 2) / step)``. All divisions are integer divisions of
non-negative operands.

The stage runs on the batch as stored, ahead of the crop (``data.loader.InputTransform(randaug=...)``).
"""

from __future__ import annotations

import functools
import math
from typing import List, Optional

import torch

NUM_OPS = 14
MAX_MAGNITUDE = 30
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(NUM_OPS)
OP_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
            "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
ONE = 65536  # the affine matrices' fixed point


def check_randaug(num_ops: int, magnitude: int) -> None:
    """ValueError unless 1 <= num_ops <= 4 and 0 <= magnitude <= 30 (both whole numbers)."""
    if int(num_ops) != num_ops or not (1 <= num_ops <= 4):
        raise ValueError(f"{num_ops} ops per image: need 1 <= N <= 4")
    if int(magnitude) != magnitude or not (0 <= magnitude <= MAX_MAGNITUDE):
        raise ValueError(f"magnitude {magnitude}: need 0 <= M <= {MAX_MAGNITUDE}")


def affine_args(m00: float, m01: float, m02: float, m10: float, m11: float, m12: float) -> List[int]:
    """``(a0 .. a6)`` of an affine op from its inverse map in doubled, centred pixel units."""
    return [int(round(ONE * v)) for v in (m00, m01, m02, m10, m11, m12)] + [0]


def op_args(op: int, magnitude: int, negative: bool, H: int, W: int) -> List[int]:
    """``(a0 .. a6)`` of op ``op`` at ``magnitude`` with the given sign, for ``H`` x ``W`` images (Python floats)."""
    f = magnitude / MAX_MAGNITUDE
    sg = -1.0 if negative else 1.0
    if op == SHEAR_X:
        return affine_args(1.0, sg * 0.3 * f, 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return affine_args(1.0, 0.0, 0.0, sg * 0.3 * f, 1.0, 0.0)
    if op == TRANSLATE_X:
        return affine_args(1.0, 0.0, -2.0 * sg * round(150.0 / 331.0 * f * W), 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return affine_args(1.0, 0.0, 0.0, 0.0, 1.0, -2.0 * sg * round(150.0 / 331.0 * f * H))
    if op == ROTATE:
        th = math.radians(sg * 30.0 * f)
        return affine_args(math.cos(th), -math.sin(th), 0.0, math.sin(th), math.cos(th), 0.0)
    if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        return [int(round(256.0 * (1.0 + sg * 0.9 * f)))] + [0] * 6
    if op == POSTERIZE:
        bits = 8 - int(round(4.0 * f))
        return [(0xFF << (8 - bits)) & 0xFF] + [0] * 6
    if op == SOLARIZE:
        return [int(math.ceil(255.0 * (1.0 - f)))] + [0] * 6
    if op in (IDENTITY, AUTOCONTRAST, EQUALIZE):
        return [0] * 7
    raise ValueError(f"op {op}: 0 .. {NUM_OPS - 1}")


@functools.lru_cache(maxsize=16)
def _level_table(magnitude: int, H: int, W: int, device: str) -> torch.Tensor:
    """int32 [14, 2, 7]: ``(a0 .. a6)`` of every op with the positive (0) and the negative (1) sign, on ``device``
    (made once per magnitude, image size and device: the draws then index it without touching the host)."""
    rows = [[op_args(op, magnitude, neg, H, W) for neg in (False, True)] for op in range(NUM_OPS)]
    return torch.tensor(rows, dtype=torch.int32).to(device)


def params_from_uniforms(u_op: torch.Tensor, u_sign: torch.Tensor, magnitude: int, H: int, W: int) -> torch.Tensor:
    """``params`` int32 [..., 8] from uniforms in [0, 1) of equal shape: ``op = min(13, floor(14 u_op))``, the
    negative sign where ``u_sign < 0.5`` (ignored by the ops that have none)."""
    check_randaug(1, magnitude)
    op = torch.floor(u_op.to(torch.float64) * NUM_OPS).to(torch.int64).clamp(0, NUM_OPS - 1)
    neg = (u_sign.to(torch.float64) < 0.5).to(torch.int64)
    table = _level_table(int(magnitude), int(H), int(W), str(u_op.device))
    args = table[op, neg]
    return torch.cat([op.to(torch.int32).unsqueeze(-1), args], -1).contiguous()


def sample_params(B: int, L: int, magnitude: int, H: int, W: int, generator: Optional[torch.Generator] = None,
                  device=None) -> torch.Tensor:
    """``params [B, L, 8]`` for ``B`` images of ``H`` x ``W`` pixels: the uniforms are drawn on ``device`` from
    ``generator`` (one ``torch.rand`` launch, no host sync) and handed to :func:`params_from_uniforms`."""
    check_randaug(L, magnitude)
    u = torch.rand((B, L, 2), generator=generator, device=device, dtype=torch.float32)
    return params_from_uniforms(u[..., 0], u[..., 1], magnitude, H, W)


def _blend(v: torch.Tensor, d, F: torch.Tensor) -> torch.Tensor:
    return ((F * v + (256 - F) * d + 128) >> 8).clamp(0, 255)


def _layer_torch(x: torch.Tensor, p: torch.Tensor, fill: int) -> torch.Tensor:
    """One layer on int64 ``x`` [B, H, W, 3] with rows ``p`` int64 [B, 8]: every op's result for the whole batch,
    each sample taking its own op's (no data-dependent control flow, so no host sync)."""
    B, H, W, _ = x.shape
    n = H * W
    dev = x.device
    op = p[:, 0].view(B, 1, 1, 1)
    a0 = p[:, 1].view(B, 1, 1, 1)
    # affine: gather the source pixel
    a = [p[:, 1 + i].view(B, 1, 1) for i in range(6)]
    X = (2 * torch.arange(W, device=dev, dtype=torch.int64) - (W - 1)).view(1, 1, W)
    Y = (2 * torch.arange(H, device=dev, dtype=torch.int64) - (H - 1)).view(1, H, 1)
    sx = (a[0] * X + a[1] * Y + a[2] + (W << 16)) >> 17
    sy = (a[3] * X + a[4] * Y + a[5] + (H << 16)) >> 17
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    idx = (sy.clamp(0, H - 1) * W + sx.clamp(0, W - 1)).view(B, n, 1).expand(B, n, 3)
    affine = torch.where(inside.unsqueeze(-1), x.reshape(B, n, 3).gather(1, idx).view(B, H, W, 3),
                         torch.full_like(x, int(fill)))
    # colour: blends against 0, the gray, the mean gray, the smoothed image
    gray = (77 * x[..., 0:1] + 150 * x[..., 1:2] + 29 * x[..., 2:3] + 128) >> 8
    mean = ((gray.sum(dim=(1, 2, 3)) + n // 2) // n).view(B, 1, 1, 1)
    smooth = x.clone()
    if H >= 3 and W >= 3:
        s = 4 * x[:, 1:-1, 1:-1] + 6
        for dy in range(3):
            for dx in range(3):
                s = s + x[:, dy:H - 2 + dy, dx:W - 2 + dx]
        smooth[:, 1:-1, 1:-1] = s // 13
    # AutoContrast
    flat = x.reshape(B, n, 3)
    lo = flat.amin(dim=1).view(B, 1, 1, 3)
    hi = flat.amax(dim=1).view(B, 1, 1, 3)
    span = hi - lo
    auto = torch.where(span > 0, ((x - lo) * 255 + span // 2) // span.clamp_min(1), x)
    # Equalize
    chan = flat.permute(0, 2, 1).contiguous()  # [B, 3, n]
    hist = torch.zeros((B, 3, 256), dtype=torch.int64, device=dev).scatter_add_(2, chan, torch.ones_like(chan))
    bins = torch.arange(256, device=dev, dtype=torch.int64)
    top = torch.where(hist > 0, bins, torch.zeros_like(bins)).amax(dim=2, keepdim=True)  # highest non-empty bin
    step = (n - hist.gather(2, top)) // 255
    lut = ((hist.cumsum(2) - hist + step // 2) // step.clamp_min(1)).clamp_max(255)
    eq = torch.where(step > 0, lut.gather(2, chan), chan).permute(0, 2, 1).reshape(B, H, W, 3)
    out = x
    for ops, res in (((SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE), affine),
                     ((BRIGHTNESS,), _blend(x, 0, a0)), ((COLOR,), _blend(x, gray, a0)),
                     ((CONTRAST,), _blend(x, mean, a0)), ((SHARPNESS,), _blend(x, smooth, a0)),
                     ((POSTERIZE,), x & a0 & 0xFF), ((SOLARIZE,), torch.where(x >= a0, 255 - x, x)),
                     ((AUTOCONTRAST,), auto), ((EQUALIZE,), eq)):
        sel = op == ops[0]
        for o in ops[1:]:
            sel = sel | (op == o)
        out = torch.where(sel, res, out)
    return out


def randaug_torch(u8: torch.Tensor, params: torch.Tensor, fill: int = 128) -> torch.Tensor:
    """The definition in torch integer ops: uint8 NHWC ``u8`` [B, H, W, 3] through the layers of ``params`` int32
    [B, L, 8] -> uint8 [B, H, W, 3] (a new tensor). The ``--kernels torch`` / CPU backend and the oracle of the
    tests. An op id outside the table leaves the image as it is. Solarize at magnitude 0 (threshold 255) turns a
    pixel of 255 into 0, as PIL and torchvision do."""
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8:
        raise ValueError(f"randaug_torch: images {tuple(u8.shape)} {u8.dtype} (uint8 [B, H, W, 3])")
    B = u8.shape[0]
    if params.dim() != 3 or params.shape[0] != B or params.shape[2] != 8:
        raise ValueError(f"randaug_torch: params {tuple(params.shape)}, expected ({B}, L, 8)")
    x = u8.to(torch.int64)
    if u8.numel() == 0:
        return u8.clone()
    p = params.to(device=u8.device, dtype=torch.int64)
    for layer in range(p.shape[1]):
        x = _layer_torch(x, p[:, layer], fill)
    return x.to(torch.uint8).contiguous()


class RandAugment:
    """RandAugment of every training batch: ``ra(u8) -> u8`` on the uint8 NHWC batch as stored.

    ``backend`` ``hip`` / ``hip_f32``: ``ops.misc.randaug_u8`` (the stage never sees the model's dtype). ``torch``:
    :func:`randaug_torch` -- the ``--kernels torch`` / CPU path and the oracle of the tests. The draws come from a
    generator of the stage's own on the compute device, reseeded from (seed, rank, epoch) by :meth:`set_epoch`, so a
    resumed epoch repeats them."""

    def __init__(self, backend: str, num_ops: int = 2, magnitude: int = 9, fill: int = 128, seed: int = 0,
                 rank: int = 0):
        check_randaug(num_ops, magnitude)
        if backend not in ("hip", "hip_f32", "torch"):
            raise ValueError(f"backend {backend!r}: hip, hip_f32 or torch")
        if int(fill) != fill or not (0 <= fill <= 255):
            raise ValueError(f"fill {fill}: need 0 <= V <= 255")
        self.backend = backend
        self.num_ops, self.magnitude, self.fill = int(num_ops), int(magnitude), int(fill)
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0
        self._gen = None

    def _epoch_seed(self) -> int:
        # other constants than InputTransform._epoch_seed and BatchMixer._epoch_seed: the three streams of draws of
        # an epoch are unrelated
        return (self.seed * 0xA24BAED5 + self.rank * 0x9FB21C65 + self.epoch * 0xE7037ED1 + 13) % (2 ** 63 - 1)

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
        """The next batch's ``params [B, L, 8]`` from the stage's generator."""
        return sample_params(B, self.num_ops, self.magnitude, H, W, self._generator(device), device)

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
