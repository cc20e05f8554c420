"""Random Erasing (``--random-erase``; Zhong et al., "Random Erasing Data Augmentation"): the per-sample draws, pure
torch and free of host syncs, the counter-based noise of the ``pixel`` mode as integer arithmetic, and the stage that
applies both to the model input.

A training sample is erased with probability ``p``: ``N`` boxes, each found as torchvision's ``RandomErasing`` finds
its one box -- up to 10 attempts of an area share uniform over ``scale`` (divided by ``N``: timm's ``max_count``) and
an aspect ratio h / w log-uniform over ``ratio``, the first attempt that fits inside the image wins -- are overwritten
with ``value`` (``const``; in normalised units, so 0 is the mean colour) or with an independent N(0, 1) draw per
element (``pixel``, timm). The stage runs on the model input, after the normalise / crop kernel and before Mixup /
CutMix, as both libraries erase in the per-sample transform and mix in the collate.

The draws are ``boxes`` int32 [B, N, 4] = (top, left, h, w) on the model-input grid, (0, 0, 0, 0) the empty box, and
``keys`` int32 [B, 2], the per-sample key of the noise generator. They feed ``ops.misc.erase_boxes`` (one HIP kernel,
in place) or :func:`erase_torch`. The box arithmetic is float64 so that it equals a plain per-sample loop in Python
floats on the same uniforms.

The noise is defined once, in integers, so both backends form the same 32-bit words: for sample ``b`` and pixel ``q = y
W + x``, ``(r0, r1, r2, r3) = Philox4x32-10(counter = (q, 0, 0, 0), key = keys[b] read as uint32)`` (Salmon et al.,
"Parallel Random Numbers: As Easy as 1, 2, 3"), then Box-Muller: ``u = ((r0 >> 8) + 1) 2^-24`` in (0, 1], ``v = (r1 >>
8) 2^-24``, channel 0 ``sqrt(-2 ln u) cos(2 pi v)``, channel 1 the sine, channel 2 the cosine form on ``(r2, r3)``. It
depends on the sample's key and the pixel alone: overlapping boxes of a sample write equal values.
"""

from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

ATTEMPTS = 10
MAX_COUNT = 4
MODES = ("const", "pixel")
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def check_erase(p: float, scale: Sequence[float], ratio: Sequence[float], count: int = 1, mode: str = "const",
                value: float = 0.0) -> None:
    """ValueError unless ``0 <= p <= 1``, ``0 < scale[0] <= scale[1] <= 1``, ``0 < ratio[0] <= ratio[1]``, ``1 <=
    count <= 4``, the mode is ``const`` or ``pixel`` and the value is finite."""
    if not (0.0 <= p <= 1.0):
        raise ValueError(f"probability {p}: need 0 <= P <= 1")
    if len(scale) != 2 or not (0.0 < scale[0] <= scale[1] <= 1.0):
        raise ValueError(f"scale {tuple(scale)}: need 0 < LO <= HI <= 1")
    if len(ratio) != 2 or not (0.0 < ratio[0] <= ratio[1]) or not math.isfinite(ratio[1]):
        raise ValueError(f"ratio {tuple(ratio)}: need 0 < LO <= HI")
    if int(count) != count or not (1 <= count <= MAX_COUNT):
        raise ValueError(f"{count} boxes per sample: need 1 <= N <= {MAX_COUNT}")
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: const or pixel")
    if not math.isfinite(value):
        raise ValueError(f"value {value}: need a finite number")


def params_from_uniforms(u_apply: torch.Tensor, u: torch.Tensor, H: int, W: int, p: float, scale: Sequence[float],
                         ratio: Sequence[float]) -> torch.Tensor:
    """``boxes`` int32 [B, N, 4] from uniforms in [0, 1): ``u_apply`` [B] (the sample is erased where ``u_apply <
    p``) and ``u`` [B, N, 10, 4] = (area, ratio, top, left) of each of a box's 10 attempts. Per attempt ``area = H W
    (s0 + u0 (s1 - s0)) / N``, ``ar = exp(ln r0 + u1 (ln r1 - ln r0))``, ``h = round(sqrt(area ar))``, ``w =
    round(sqrt(area / ar))``, valid when ``h < H and w < W`` (torchvision's test), ``top = min(H - h, floor(u2 (H - h
    + 1)))`` and ``left`` likewise. The box is the first valid attempt; with none, or with ``h`` or ``w`` 0, the empty
    box."""
    f64, i64 = torch.float64, torch.int64
    N = u.shape[1]
    if u.dim() != 4 or u.shape[0] != u_apply.shape[0] or u.shape[2] != ATTEMPTS or u.shape[3] != 4:
        raise ValueError(f"uniforms {tuple(u.shape)}, expected ({u_apply.shape[0]}, N, {ATTEMPTS}, 4)")
    u = u.to(f64)
    s0, s1 = float(scale[0]), float(scale[1])
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    area = H * W * (s0 + u[..., 0] * (s1 - s0)) / N
    ar = torch.exp(l0 + u[..., 1] * (l1 - l0))
    h = torch.round(torch.sqrt(area * ar)).to(i64)
    w = torch.round(torch.sqrt(area / ar)).to(i64)
    valid = (h < H) & (w < W)
    top = torch.floor(u[..., 2] * (H - h + 1).to(f64)).to(i64).clamp_max(H - h)
    left = torch.floor(u[..., 3] * (W - w + 1).to(f64)).to(i64).clamp_max(W - w)
    # the first valid attempt: the largest of valid * (10 - attempt), which no two attempts share
    rank = valid.to(i64) * (ATTEMPTS - torch.arange(ATTEMPTS, device=u.device, dtype=i64))
    first = rank.argmax(-1, keepdim=True)
    pick = lambda t: t.gather(-1, first).squeeze(-1)  # noqa: E731
    bt, bl, bh, bw = pick(top), pick(left), pick(h), pick(w)
    keep = pick(valid) & (bh > 0) & (bw > 0) & (u_apply.to(f64) < p).unsqueeze(-1)
    boxes = torch.stack([bt, bl, bh, bw], -1)
    return torch.where(keep.unsqueeze(-1), boxes, torch.zeros_like(boxes)).to(torch.int32).contiguous()


def erase_params(B: int, H: int, W: int, p: float, scale: Sequence[float] = (0.02, 0.33),
                 ratio: Sequence[float] = (0.3, 3.3), count: int = 1, generator: Optional[torch.Generator] = None,
                 device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(boxes, keys)`` for a batch of ``B`` samples of ``H`` x ``W`` pixels, drawn on ``device`` from ``generator``
    (a handful of launches, no host sync): the uniforms go to :func:`params_from_uniforms`, the keys are uniform over
    the whole int32 range."""
    check_erase(p, scale, ratio, count)
    u_apply = torch.rand((B,), generator=generator, device=device, dtype=torch.float32)
    u = torch.rand((B, count, ATTEMPTS, 4), generator=generator, device=device, dtype=torch.float32)
    keys = torch.randint(-2 ** 31, 2 ** 31, (B, 2), generator=generator, device=device, dtype=torch.int64)
    return params_from_uniforms(u_apply, u, H, W, p, scale, ratio), keys.to(torch.int32).contiguous()


# ------------------------------------------------------------------ the noise
def _mulhilo(m: int, a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(high, low) 32-bit words of ``m a`` for int64 ``a`` in [0, 2^32): the product split into 16-bit halves, so no
    intermediate passes 2^49."""
    mh, ml = m >> 16, m & 0xFFFF
    ah, al = a >> 16, a & 0xFFFF
    lo, m1, m2, hi = al * ml, ah * ml, al * mh, ah * mh
    mid = (lo >> 16) + (m1 & 0xFFFF) + (m2 & 0xFFFF)
    return hi + (m1 >> 16) + (m2 >> 16) + (mid >> 16), ((mid & 0xFFFF) << 16) | (lo & 0xFFFF)


def philox4x32_10(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Philox4x32-10 in int64 tensors: ``counter`` [..., 4] and ``key`` [..., 2] (any integer dtype, read as uint32
    words; broadcast against each other) -> int64 [..., 4], each word in [0, 2^32)."""
    c = counter.to(torch.int64) & _M32
    k = key.to(torch.int64) & _M32
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        h0, l0 = _mulhilo(PHILOX_M0, c0)
        h1, l1 = _mulhilo(PHILOX_M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return torch.stack(torch.broadcast_tensors(c0, c1, c2, c3), -1)


def noise_words(keys: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The Philox words of every pixel of every sample: int64 [B, H, W, 4] from ``keys`` int32 [B, 2]."""
    q = torch.arange(H * W, device=keys.device, dtype=torch.int64).view(1, H * W, 1)
    counter = torch.cat([q, torch.zeros((1, H * W, 3), device=keys.device, dtype=torch.int64)], -1)
    return philox4x32_10(counter, keys.view(-1, 1, 2)).view(-1, H, W, 4)


def normals_from_words(r: torch.Tensor) -> torch.Tensor:
    """float64 [..., 3]: the three channels' N(0, 1) values of the words ``r`` int64 [..., 4] (Box-Muller, the module
    docstring's rule, evaluated in float64)."""
    f64 = torch.float64
    u0, v0 = ((r[..., 0] >> 8) + 1).to(f64) * 2.0 ** -24, (r[..., 1] >> 8).to(f64) * 2.0 ** -24
    u1, v1 = ((r[..., 2] >> 8) + 1).to(f64) * 2.0 ** -24, (r[..., 3] >> 8).to(f64) * 2.0 ** -24
    rad0, rad1 = torch.sqrt(-2.0 * torch.log(u0)), torch.sqrt(-2.0 * torch.log(u1))
    return torch.stack([rad0 * torch.cos(2.0 * math.pi * v0), rad0 * torch.sin(2.0 * math.pi * v0),
                        rad1 * torch.cos(2.0 * math.pi * v1)], -1)


def erase_torch(x: torch.Tensor, boxes: torch.Tensor, keys: Optional[torch.Tensor], mode: str = "const",
                value: float = 0.0) -> torch.Tensor:
    """The definition in PyTorch ops on NCHW ``x`` [B, 3, H, W] (a new tensor): inside every box of ``boxes`` int32
    [B, N, 4] an element becomes ``value`` (taken as fp32, then rounded to ``x``'s dtype) or, in ``pixel`` mode, its
    noise value, formed in float64 from the Philox words and rounded to ``x``'s dtype. The ``--kernels torch`` / CPU
    path and the oracle of the tests; it forms the noise of the whole batch, erased or not."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: const or pixel")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"erase_torch: x {tuple(x.shape)} (NCHW with 3 channels)")
    B, _, H, W = x.shape
    if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4:
        raise ValueError(f"erase_torch: boxes {tuple(boxes.shape)}, expected ({B}, N, 4)")
    boxes = boxes.to(device=x.device, dtype=torch.int64)
    rows = torch.arange(H, device=x.device).view(1, 1, H, 1)
    cols = torch.arange(W, device=x.device).view(1, 1, 1, W)
    t, lf, h, w = (boxes[:, :, i].view(B, -1, 1, 1) for i in range(4))
    inside = ((rows >= t) & (rows < t + h) & (cols >= lf) & (cols < lf + w) & (h > 0) & (w > 0)).any(1, keepdim=True)
    if mode == "pixel":
        if keys is None or tuple(keys.shape) != (B, 2):
            raise ValueError(f"erase_torch: pixel mode needs keys of shape ({B}, 2)")
        fill = normals_from_words(noise_words(keys.to(x.device), H, W)).permute(0, 3, 1, 2).to(x.dtype)
    else:
        fill = torch.tensor(float(value), dtype=torch.float32, device=x.device).to(x.dtype)
    return torch.where(inside, fill, x).contiguous()


class BatchEraser:
    """Random Erasing of every training batch: ``eraser(x) -> x``.

    ``backend`` ``hip`` / ``hip_f32``: ``x`` is the model input as the normalise kernels leave it (NHWC [B, H, W, Cp],
    bf16 / fp32), written in place by ``ops.misc.erase_boxes``. ``torch``: NCHW, :func:`erase_torch` -- the
    ``--kernels torch`` path and the oracle of the tests. The draws come from a generator of the stage's own on the
    compute device, reseeded from (seed, rank, epoch) by :meth:`set_epoch`, so a resumed epoch repeats them."""

    def __init__(self, backend: str, p: float, scale: Sequence[float] = (0.02, 0.33),
                 ratio: Sequence[float] = (0.3, 3.3), count: int = 1, mode: str = "const", value: float = 0.0,
                 seed: int = 0, rank: int = 0):
        check_erase(p, scale, ratio, count, mode, value)
        if backend not in ("hip", "hip_f32", "torch"):
            raise ValueError(f"backend {backend!r}: hip, hip_f32 or torch")
        self.backend = backend
        self.p, self.count, self.mode, self.value = float(p), int(count), mode, float(value)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0
        self._gen = None

    def _epoch_seed(self) -> int:
        # other constants than InputTransform's, BatchMixer's and RandAugment's: the streams of draws of an epoch
        # are unrelated
        return (self.seed * 0xB5297A4D + self.rank * 0x68E31DA4 + self.epoch * 0x1B56C4E9 + 29) % (2 ** 63 - 1)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        if self._gen is not None:
            self._gen.manual_seed(self._epoch_seed())

    def _generator(self, device) -> torch.Generator:
        if self._gen is None or self._gen.device != torch.device(device):
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._epoch_seed())
        return self._gen

    def draw(self, B: int, H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """The next batch's ``(boxes, keys)`` from the stage's generator."""
        return erase_params(B, H, W, self.p, self.scale, self.ratio, self.count, self._generator(device), device)

    def __call__(self, x: torch.Tensor, params=None) -> torch.Tensor:
        """``params``: explicit ``(boxes, keys)`` instead of the stage's own draws (comparing backends on identical
        draws)."""
        nhwc = self.backend in ("hip", "hip_f32")
        B = x.shape[0]
        H, W = (x.shape[1], x.shape[2]) if nhwc else (x.shape[2], x.shape[3])
        boxes, keys = params if params is not None else self.draw(B, H, W, x.device)
        boxes = boxes.to(device=x.device, dtype=torch.int32)
        keys = keys.to(device=x.device, dtype=torch.int32)
        if nhwc:
            from ..ops.misc import erase_boxes
            return erase_boxes(x, boxes, keys, self.mode, self.value)
        return erase_torch(x, boxes, keys, self.mode, self.value)
