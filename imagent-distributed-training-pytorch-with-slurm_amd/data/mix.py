"""Mixup and CutMix (``--mixup`` / ``--cutmix``): the per-sample draws, pure torch and free of host syncs, and the
batch mixer that applies them.

Mixup (Zhang et al., "mixup: Beyond Empirical Risk Minimization"): a sample becomes ``lam x + (1 - lam) x'`` with its
partner ``x'`` from the same batch, ``lam ~ Beta(alpha, alpha)``. CutMix (Yun et al., "CutMix: Regularization Strategy
to Train Strong Classifiers with Localizable Features"): a box of the partner is pasted into the sample -- the
published rule: ``r = sqrt(1 - lam)``, a box of ``int(H r)`` x ``int(W r)`` around a centre uniform over the image,
clipped to the image, and ``lam`` replaced by the share of the sample's own pixels that remain. Either way the loss
is taken against both labels, weighted ``lam`` and ``1 - lam`` (``ops.misc.XentPairFn``).

The draws are ``pair`` int32 [B] (a permutation of the batch; ``pair[i] == i`` is legal), ``lam`` float32 [B] and
``boxes`` int32 [B, 4] = (top, left, h, w) on the model-input grid. A Mixup sample and a sample that is not mixed
carry the empty box (0, 0, 0, 0), the latter with ``lam = 1``. They feed ``ops.misc.mix_pairs`` (one HIP kernel)
or the torch backend of :class:`BatchMixer`. The box arithmetic is float64 so that it equals a plain per-sample
loop in Python floats on the same inputs; the Beta draw is float64 because in float32 both gamma variates of a
small alpha (0.2) underflow to 0 far too often.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch


def check_mix(mixup_alpha: float, cutmix_alpha: float, prob: float, switch_prob: float) -> None:
    """ValueError unless both alphas are >= 0 and both probabilities lie in [0, 1]."""
    if not (mixup_alpha >= 0.0) or not (cutmix_alpha >= 0.0):
        raise ValueError(f"alphas ({mixup_alpha}, {cutmix_alpha}): need alpha >= 0 (0 switches the kind off)")
    if not (0.0 <= prob <= 1.0) or not (0.0 <= switch_prob <= 1.0):
        raise ValueError(f"probabilities ({prob}, {switch_prob}): need 0 <= p <= 1")


def kinds_from_uniforms(u_mix: torch.Tensor, u_kind: torch.Tensor, mixup_alpha: float, cutmix_alpha: float,
                        prob: float, switch_prob: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mixed, cut) bool [B] from uniforms in [0, 1): a sample is mixed with probability ``prob``; a mixed sample is
    CutMix with probability ``switch_prob`` when both alphas are > 0, else always the kind whose alpha is > 0."""
    mixed = u_mix < prob
    if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
        cut = u_kind < switch_prob
    else:
        cut = torch.full_like(mixed, cutmix_alpha > 0.0)
    if not (mixup_alpha > 0.0 or cutmix_alpha > 0.0):
        mixed = torch.zeros_like(mixed)
    return mixed, cut & mixed


def params_from_uniforms(mixed: torch.Tensor, cut: torch.Tensor, u_pos: torch.Tensor, lam: torch.Tensor,
                         pair: torch.Tensor, H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The draws as the kernels take them, from each sample's kind (``mixed`` / ``cut`` bool [B]), the box centre's
    uniforms ``u_pos`` [B, 2] (row, column) in [0, 1), the Beta draw ``lam`` [B] and ``pair`` [B]:
    ``(pair int32 [B], lam float32 [B], boxes int32 [B, 4])``. A CutMix sample gets the published box and the
    adjusted ``lam = 1 - h w / (H W)`` of the clipped box; a box clipped to nothing becomes the empty box with
    ``lam = 1``. Mixup samples keep ``lam`` and get the empty box, samples that are not mixed ``lam = 1``."""
    f64, i64 = torch.float64, torch.int64
    lam = lam.to(f64)
    r = torch.sqrt((1.0 - lam).clamp_min(0.0))
    ch = torch.floor(H * r).to(i64)
    cw = torch.floor(W * r).to(i64)
    cy = torch.floor(u_pos[:, 0].to(f64) * H).to(i64).clamp_max(H - 1)
    cx = torch.floor(u_pos[:, 1].to(f64) * W).to(i64).clamp_max(W - 1)
    y0, y1 = (cy - ch // 2).clamp(0, H), (cy + ch // 2).clamp(0, H)
    x0, x1 = (cx - cw // 2).clamp(0, W), (cx + cw // 2).clamp(0, W)
    bh, bw = y1 - y0, x1 - x0
    boxed = cut & (bh > 0) & (bw > 0)
    zero = torch.zeros_like(bh)
    boxes = torch.stack([torch.where(boxed, y0, zero), torch.where(boxed, x0, zero), torch.where(boxed, bh, zero),
                         torch.where(boxed, bw, zero)], 1)
    lam_box = 1.0 - (bh * bw).to(f64) / float(H * W)
    one = torch.ones_like(lam)
    lam = torch.where(boxed, lam_box, torch.where(mixed & ~cut, lam, one))
    return pair.to(torch.int32).contiguous(), lam.to(torch.float32).contiguous(), boxes.to(torch.int32).contiguous()


def beta_draws(alpha: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``Beta(alpha, alpha)`` per element of ``alpha`` (float64, > 0) as ``g1 / (g1 + g2)`` of two gamma variates
    drawn from ``generator``; 0.5 where both are 0 (possible for a tiny alpha even in float64), so never a NaN."""
    g = torch._standard_gamma(torch.stack([alpha, alpha]).to(torch.float64), generator=generator)
    s = g[0] + g[1]
    ok = s > 0
    return torch.where(ok, g[0] / torch.where(ok, s, torch.ones_like(s)), torch.full_like(s, 0.5))


def mix_params(B: int, H: int, W: int, mixup_alpha: float, cutmix_alpha: float, prob: float = 1.0,
               switch_prob: float = 0.5, generator: Optional[torch.Generator] = None,
               device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(pair, lam, boxes)`` for a batch of ``B`` samples of ``H`` x ``W`` pixels, drawn on ``device`` from
    ``generator`` (a handful of launches, no host sync) and handed to :func:`params_from_uniforms`."""
    check_mix(mixup_alpha, cutmix_alpha, prob, switch_prob)
    u = torch.rand((B, 4), generator=generator, device=device, dtype=torch.float32)
    mixed, cut = kinds_from_uniforms(u[:, 0], u[:, 1], mixup_alpha, cutmix_alpha, prob, switch_prob)
    # every sample draws at its kind's alpha (a kind that is off never occurs; its alpha only has to be valid)
    a_mix = mixup_alpha if mixup_alpha > 0.0 else cutmix_alpha
    a_cut = cutmix_alpha if cutmix_alpha > 0.0 else mixup_alpha
    if a_mix > 0.0:
        alpha = torch.where(cut, torch.full((B,), a_cut, dtype=torch.float64, device=u.device),
                            torch.full((B,), a_mix, dtype=torch.float64, device=u.device))
        lam = beta_draws(alpha, generator)
    else:
        lam = torch.ones(B, dtype=torch.float64, device=u.device)
    pair = torch.randperm(B, generator=generator, device=u.device)
    return params_from_uniforms(mixed, cut, u[:, 2:4], lam, pair, H, W)


class BatchMixer:
    """Mixup / CutMix of every training batch: ``mixer(x, y) -> (x_mixed, (y, y[pair], lam))``.

    ``backend`` ``hip`` / ``hip_f32``: ``x`` is the model input as the normalise kernels leave it (NHWC
    [B, H, W, Cp], bf16 / fp32) and goes through ``ops.misc.mix_pairs``. ``torch``: NCHW, PyTorch ops -- the
    ``--kernels torch`` path and the oracle of the tests. The draws come from a generator of the mixer's own on the
    compute device, reseeded from (seed, rank, epoch) by :meth:`set_epoch`, so a resumed epoch repeats them."""

    def __init__(self, backend: str, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, seed: int = 0, rank: int = 0):
        check_mix(mixup_alpha, cutmix_alpha, prob, switch_prob)
        if backend not in ("hip", "hip_f32", "torch"):
            raise ValueError(f"backend {backend!r}: hip, hip_f32 or torch")
        self.backend = backend
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0
        self._gen = None

    def _epoch_seed(self) -> int:
        # other constants than InputTransform._epoch_seed: the crop boxes and the mix draws of an epoch are unrelated
        return (self.seed * 0xD6E8FEB9 + self.rank * 0xCA5A8263 + self.epoch * 0x94D049BB + 7) % (2 ** 63 - 1)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        if self._gen is not None:
            self._gen.manual_seed(self._epoch_seed())

    def _generator(self, device) -> torch.Generator:
        if self._gen is None or self._gen.device != torch.device(device):
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._epoch_seed())
        return self._gen

    def draw(self, B: int, H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The next batch's ``(pair, lam, boxes)`` from the mixer's generator."""
        return mix_params(B, H, W, self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob,
                          self._generator(device), device)

    def __call__(self, x: torch.Tensor, y: torch.Tensor, params=None):
        """``params``: explicit ``(pair, lam, boxes)`` instead of the mixer's own draws (comparing backends on
        identical draws)."""
        nhwc = self.backend in ("hip", "hip_f32")
        B = x.shape[0]
        H, W = (x.shape[1], x.shape[2]) if nhwc else (x.shape[2], x.shape[3])
        pair, lam, boxes = params if params is not None else self.draw(B, H, W, x.device)
        pair = pair.to(device=x.device, dtype=torch.int32)
        lam = lam.to(device=x.device, dtype=torch.float32)
        boxes = boxes.to(device=x.device, dtype=torch.int32)
        if nhwc:
            from ..ops.misc import mix_pairs
            out = mix_pairs(x, pair, lam, boxes)
        else:
            out = mix_torch(x, pair, lam, boxes)
        return out, (y, y.index_select(0, pair), lam)


def mix_torch(x: torch.Tensor, pair: torch.Tensor, lam: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """The definition in PyTorch ops on NCHW ``x``: ``lam x + (1 - lam) x[pair]`` in fp32 for a sample with an
    empty box, the partner's pixels inside a non-empty one."""
    B, _, H, W = x.shape
    xp = x.index_select(0, pair)
    l = lam.to(torch.float32).view(B, 1, 1, 1)
    blend = (l * x.float() + (1.0 - l) * xp.float()).to(x.dtype)
    t, lf, h, w = (boxes[:, i].view(B, 1, 1, 1) for i in range(4))
    rows = torch.arange(H, device=x.device).view(1, 1, H, 1)
    cols = torch.arange(W, device=x.device).view(1, 1, 1, W)
    inside = (rows >= t) & (rows < t + h) & (cols >= lf) & (cols < lf + w)
    boxed = (h > 0) & (w > 0)
    return torch.where(boxed, torch.where(inside, xp, x), blend).contiguous()
