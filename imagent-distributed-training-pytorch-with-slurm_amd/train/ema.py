"""Exponential moving average of the weights (``--model-ema DECAY``).

The modern ImageNet recipe (timm, torchvision's reference scripts) evaluates
and ships an average of the weights: with Mixup / CutMix the raw weights are
noisy from step to step. Once per optimizer step, with ``p'`` the parameter
after the step::

    E += (1 - d_t) * (p' - E)        # lerp form: E == p' is a fixed point

``d_t = DECAY``, or with ``--model-ema-warmup`` timm's ramp
``min(DECAY, (1 + t) / (10 + t))`` over the ``t`` updates already done. The
host forms ``1 - d_t`` in double precision and rounds it once to fp32: the
kernels and the CPU path take that one number.

The average is one more flat fp32 arena ``E`` with the offsets of
``ParamArena.P``:

* every optimizer runs ``imk_ema_flat`` over ``(E, P)`` after its step: one
  elementwise launch, no ``_foreach_lerp_`` over 161 tensors and no second
  model (fused into the SGD launch it measured no faster than the two
  launches, ``profiles/model_ema.md``, so the SGD kernel stays as it was);
* the BatchNorm running statistics are averaged with the same ``d_t`` into a
  flat side buffer (``model.buffers()`` order, float buffers only;
  ``num_batches_tracked`` is not averaged) by one launch over a descriptor
  table;
* evaluation swaps ``P <-> E`` and the buffers IN PLACE (every descriptor
  table and shadow keeps its pointers), validates through the unchanged eval
  forward, and swaps back: two swaps restore every bit.

On CPU (or ``native=False``) the same math runs as flat torch ops.
"""

from __future__ import annotations

import struct
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn

from ..models.arena import ParamArena


def check_decay(decay: float) -> None:
    if not (0.0 < decay < 1.0):
        raise ValueError(f"need 0 < DECAY < 1, got {decay}")


def _f32(x: float) -> float:
    """``x`` rounded once to fp32 (what a float kernel argument holds), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


class ModelEma:
    def __init__(self, arena: ParamArena, model: nn.Module, decay: float, warmup: bool = False,
                 native: Optional[bool] = None, refresh: Optional[Callable[[], None]] = None):
        """``refresh``: what re-derives the compute copies after the weights changed under the model
        (``NativeState.refresh_shadows``: transposes, stem pad, fp8 re-quantisation); the swap kernel itself
        writes the bf16 shadow."""
        check_decay(decay)
        self.arena, self.decay, self.warmup = arena, float(decay), bool(warmup)
        self.native = arena.P.is_cuda if native is None else native
        self.refresh = refresh
        self.updates = 0
        self.E = arena.P.detach().clone()
        named = [(n, b) for n, b in model.named_buffers() if b.dtype == torch.float32]
        self.buf_names = [n for n, _ in named]
        self.bufs: List[torch.Tensor] = [b for _, b in named]
        self.buf_offsets, off = [], 0
        for b in self.bufs:
            self.buf_offsets.append(off)
            off += b.numel()
        self.B = torch.cat([b.detach().reshape(-1) for b in self.bufs]).to(arena.P.device) if self.bufs \
            else torch.zeros(0, dtype=torch.float32, device=arena.P.device)
        self._table = None

    # ------------------------------------------------------------------
    def decay_at(self, t: int) -> float:
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    def omd(self) -> float:
        """This step's ``1 - d_t``: formed in double precision, rounded once to fp32."""
        return _f32(1.0 - self.decay_at(self.updates))

    def _buf_slice(self, i: int) -> torch.Tensor:
        o = self.buf_offsets[i]
        return self.B[o:o + self.bufs[i].numel()]

    def _bufs_kernel(self, omd: float, swap: bool) -> None:
        from ..ops.misc import ema_buf_table, ema_bufs
        if self._table is None:  # the buffers' storage never moves (the BatchNorm tables hold it too)
            self._table = ema_buf_table(self.bufs, self.buf_offsets, self.B.device)
            self._max_n = max(b.numel() for b in self.bufs)
        ema_bufs(self._table, len(self.bufs), self._max_n, self.B, omd, swap)

    @torch.no_grad()
    def update_buffers(self) -> None:
        """The buffer half of an update, and the update count (:meth:`update` ends with it)."""
        w = self.omd()
        if self.bufs:
            if self.native:
                self._bufs_kernel(w, False)
            else:
                cur = torch.cat([b.reshape(-1) for b in self.bufs])
                self.B.add_(cur - self.B, alpha=w)
        self.updates += 1

    @torch.no_grad()
    def update(self) -> None:
        """One update after an optimizer step: the flat arena, then the buffers."""
        w = self.omd()
        if self.native:
            from ..ops.misc import ema_flat
            ema_flat(self.E, self.arena.P, w)
        else:
            self.E.add_(self.arena.P - self.E, alpha=w)
        self.update_buffers()

    @torch.no_grad()
    def swap(self) -> None:
        """``P <-> E`` and buffers <-> their averages, in place; the compute copies follow. Call it twice."""
        ar = self.arena
        if self.native:
            from ..ops.misc import ema_swap
            ema_swap(ar.P, self.E, ar.S)
            if self.bufs:
                self._bufs_kernel(0.0, True)
        else:
            tmp = ar.P.clone()
            ar.P.copy_(self.E)
            self.E.copy_(tmp)
            if ar.S is not None:
                ar.S.copy_(ar.P)
            for i, b in enumerate(self.bufs):
                s = self._buf_slice(i)
                tmp = b.detach().clone()
                b.copy_(s.view_as(b))
                s.copy_(tmp.reshape(-1))
        if self.refresh is not None:
            self.refresh()

    # the one-time bucket re-layout moves P: E follows it like the optimizer's momentum
    def flats(self) -> List[torch.Tensor]:
        return [self.E]

    def set_flats(self, flats: List[torch.Tensor]) -> None:
        if flats:
            self.E = flats[0]

    # checkpointing: keyed by parameter / buffer name (layout-independent); tensors, numbers and strings only
    def state_dict(self) -> Dict:
        ar = self.arena
        return {"decay": self.decay, "warmup": int(self.warmup), "updates": self.updates,
                "params": {n: ar.flat_slice(self.E, i).detach().cpu().clone() for i, n in enumerate(ar.names)},
                "buffers": {n: self._buf_slice(i).detach().cpu().clone() for i, n in enumerate(self.buf_names)}}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict) -> None:
        ar = self.arena
        for i, n in enumerate(ar.names):
            ar.flat_slice(self.E, i).copy_(sd["params"][n].to(self.E.device).reshape(-1))
        for i, n in enumerate(self.buf_names):
            self._buf_slice(i).copy_(sd["buffers"][n].to(self.B.device).reshape(-1))
        self.updates = int(sd.get("updates", 0))
