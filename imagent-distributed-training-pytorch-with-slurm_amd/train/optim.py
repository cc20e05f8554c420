"""Optimizers over the flat parameter arena.

Reference: ``SGD(model.parameters(), lr, momentum=0.9, weight_decay=1e-4)``
(``imagenet.py:325``) plus the commented-out alternatives Adagrad, RMSprop,
Adadelta, Adam, ASGD, custom Nadam(schedule_decay=4e-3) and custom FR
(``imagenet.py:326-340``; the ``custom_optimizers`` module is missing from the
reference, quirk Q5).

* :class:`FlatSGD` - torch.optim.SGD math ([torch] optim/sgd.py:343-380,
  incl. the first-step ``buf = grad`` rule, dampening and nesterov) as ONE
  fused HIP launch over the whole arena that also rewrites the bf16 compute
  shadow; on CPU the same math in flat torch ops.
* :class:`FlatAdam` - torch.optim.Adam / AdamW math as ONE fused HIP launch
  over the arena (``m``, ``v`` are two more flat arenas), shadow included.
* :class:`FlatLAMB` - LAMB, the other layer-wise large-batch optimizer: two
  or three launches over a per-tensor descriptor table and a chunk table.
* every other optimizer is the stock ``torch.optim`` class over the arena
  views (updates land in the arena) followed by a shadow refresh.
  ``nadam`` maps Keras' ``schedule_decay`` to torch's ``momentum_decay`` (the
  same psi in mu_t = beta1 * (1 - 0.5 * 0.96 ** (t * psi))).
* :class:`FlatLARS` - LARS for the large-batch (8192) configuration.
* ``fr`` is deliberately absent: the reference never defines it.
* every optimizer has an optional ``ema`` attribute (:class:`~imagent_amd.train.ema.ModelEma`, ``--model-ema``)
  and updates it once after its own step.
"""

from __future__ import annotations

import math
import struct
from typing import Callable, Dict, List, Optional

import torch

from ..models.arena import ParamArena


class FlatSGD:
    def __init__(self, arena: ParamArena, lr: float, momentum: float = 0.9, dampening: float = 0.0,
                 weight_decay: float = 1e-4, nesterov: bool = False, native: Optional[bool] = None,
                 after_step: Optional[Callable[[], None]] = None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.arena = arena
        self.native = arena.P.is_cuda if native is None else native
        self.after_step = after_step
        self.param_groups = [dict(lr=lr, momentum=momentum, dampening=dampening,
                                  weight_decay=weight_decay, nesterov=nesterov)]
        self.buf: Optional[torch.Tensor] = None
        self.steps = 0
        self.grad_scale = 1.0
        self.ema = None  # train/ema.py ModelEma: updated once per step()

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.arena.zero_grad()

    def flats(self) -> List[torch.Tensor]:
        return [self.buf] if self.buf is not None else []

    def set_flats(self, flats: List[torch.Tensor]) -> None:
        if flats:
            self.buf = flats[0]

    @torch.no_grad()
    def step(self) -> None:
        g = self.param_groups[0]
        lr, mu, damp, wd, nest = g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]
        ar = self.arena
        first = self.buf is None
        if first and mu != 0:
            self.buf = torch.zeros_like(ar.P)
        if self.native:
            from ..ops.misc import sgd_flat
            sgd_flat(ar.P, ar.G, self.buf, ar.S, lr, mu, damp, wd, nest, first, self.grad_scale)
        else:
            d = ar.G.mul(self.grad_scale) if self.grad_scale != 1.0 else ar.G.clone()
            if wd != 0:
                d.add_(ar.P, alpha=wd)
            if mu != 0:
                if first:
                    self.buf.copy_(d)
                else:
                    self.buf.mul_(mu).add_(d, alpha=1 - damp)
                d = d.add(self.buf, alpha=mu) if nest else self.buf
            ar.P.add_(d, alpha=-lr)
            if ar.S is not None:
                ar.S.copy_(ar.P)
        if self.ema is not None:
            self.ema.update()
        self.steps += 1
        if self.after_step is not None:
            self.after_step()

    # checkpointing: momentum keyed by parameter name (layout-independent)
    def state_dict(self) -> Dict:
        ar = self.arena
        mom = {}
        if self.buf is not None:
            for i, n in enumerate(ar.names):
                mom[n] = ar.flat_slice(self.buf, i).detach().cpu().clone()
        return {"kind": "sgd", "param_groups": [dict(x) for x in self.param_groups], "steps": self.steps,
                "momentum": mom}

    def load_state_dict(self, sd: Dict) -> None:
        self.param_groups = [dict(x) for x in sd["param_groups"]]
        self.steps = sd.get("steps", 0)
        mom = sd.get("momentum", {})
        ar = self.arena
        if mom:
            self.buf = torch.zeros_like(ar.P)
            for i, n in enumerate(ar.names):
                ar.flat_slice(self.buf, i).copy_(mom[n].to(ar.P.device).reshape(-1))
        else:
            self.buf = None


class FlatLARS(FlatSGD):
    """LARS (You, Gitman, Ginsburg 2017) for large-batch runs (the fp8 8192
    config): per tensor trust = eta * ||w|| / (||g|| + wd * ||w||),
    v = mu * v + lr * trust * (g + wd * w), w -= v. One-dimensional tensors
    (BatchNorm affine, biases) are neither adapted nor decayed. On the GPU it
    is two launches over a per-tensor descriptor table (csrc/kernels/optim.hip);
    on CPU the same math per tensor."""

    def __init__(self, arena: ParamArena, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 eta: float = 1e-3, native: Optional[bool] = None, after_step: Optional[Callable[[], None]] = None):
        super().__init__(arena, lr, momentum, 0.0, weight_decay, False, native, after_step)
        self.param_groups[0]["eta"] = eta
        self._descs = None

    def _build_descs(self):
        import ctypes as C

        from ..ops import _lib
        ar = self.arena
        T = len(ar.params)
        d = (_lib.LarsDesc * T)()
        for i in range(T):
            o, n = ar.offsets[i], ar.numels[i]
            d[i].p = ar.P[o:o + n].data_ptr()
            d[i].g = ar.G[o:o + n].data_ptr()
            d[i].buf = self.buf[o:o + n].data_ptr()
            d[i].shadow = ar.S[o:o + n].data_ptr() if ar.S is not None else None
            d[i].n = n
            d[i].adapt = 1 if len(ar.shapes[i]) > 1 else 0
        self._descs = torch.frombuffer(bytearray(bytes(memoryview(d))), dtype=torch.uint8).to(ar.P.device)
        self._norms = torch.zeros(2 * T, dtype=torch.float32, device=ar.P.device)
        self._key = (ar.P.data_ptr(), ar.G.data_ptr(), self.buf.data_ptr())
        self._max_n = max(ar.numels)
        del C

    @torch.no_grad()
    def step(self) -> None:
        g = self.param_groups[0]
        lr, mu, wd, eta = g["lr"], g["momentum"], g["weight_decay"], g["eta"]
        ar = self.arena
        first = self.buf is None
        if first:
            self.buf = torch.zeros_like(ar.P)
        if self.native:
            from ..ops import _lib
            if self._descs is None or self._key != (ar.P.data_ptr(), ar.G.data_ptr(), self.buf.data_ptr()):
                self._build_descs()  # (re)built after a bucket re-layout moved the arenas
            _lib.check(_lib.kernels().imk_lars_step(self._descs.data_ptr(), len(ar.params), self._max_n,
                                                    self._norms.data_ptr(), lr, mu, wd, eta, self.grad_scale,
                                                    1 if first else 0, _lib.stream_ptr()), "lars step")
        else:
            for i in range(len(ar.params)):
                w, gr, v = ar.flat_slice(ar.P, i), ar.flat_slice(ar.G, i) * self.grad_scale, \
                    ar.flat_slice(self.buf, i)
                adapt = len(ar.shapes[i]) > 1
                trust, wdt = 1.0, 0.0
                if adapt:
                    wdt = wd
                    wn, gn = w.norm().item(), gr.norm().item()
                    if wn > 0 and gn > 0:
                        trust = eta * wn / (gn + wd * wn)
                d = gr + wdt * w
                if first:
                    v.copy_(lr * trust * d)
                else:
                    v.mul_(mu).add_(d, alpha=lr * trust)
                w.sub_(v)
            if ar.S is not None:
                ar.S.copy_(ar.P)
        if self.ema is not None:
            self.ema.update()
        self.steps += 1
        if self.after_step is not None:
            self.after_step()

    def state_dict(self) -> Dict:
        sd = super().state_dict()
        sd["kind"] = "lars"
        return sd


def _f32(x: float) -> float:
    """``x`` rounded once to fp32 (what a float kernel argument holds), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


class _FlatMoments:
    """What FlatAdam and FlatLAMB share: two flat fp32 moment arenas ``m`` / ``v`` with the offsets of
    ``arena.P`` (created at the first step), and FlatSGD's contract around them -- ``param_groups[0]["lr"]``,
    ``grad_scale``, ``steps``, one ``ema.update()`` and ``after_step()`` per step, ``flats()`` / ``set_flats()`` for
    the bucket re-layout, a checkpoint keyed by parameter name."""

    kind = ""

    def __init__(self, arena: ParamArena, native: Optional[bool], after_step: Optional[Callable[[], None]], **group):
        b1, b2 = group["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"need 0 <= beta < 1, got betas {group['betas']}")
        if not group["eps"] > 0.0:
            raise ValueError(f"need eps > 0, got {group['eps']}")  # (0 / (0 + eps) keeps the arena padding zero)
        self.arena = arena
        self.native = arena.P.is_cuda if native is None else native
        self.after_step = after_step
        self.param_groups = [dict(group, betas=(float(b1), float(b2)))]
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        self.steps = 0
        self.grad_scale = 1.0
        self.ema = None  # train/ema.py ModelEma: updated once per step()

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.arena.zero_grad()

    def flats(self) -> List[torch.Tensor]:
        return [self.m, self.v] if self.m is not None else []

    def set_flats(self, flats: List[torch.Tensor]) -> None:
        if flats:
            self.m, self.v = flats[0], flats[1]

    def _begin(self) -> int:
        """The moments, and this step's 1-based count ``t`` of the bias corrections."""
        if self.m is None:
            self.m, self.v = torch.zeros_like(self.arena.P), torch.zeros_like(self.arena.P)
        return self.steps + 1

    def _finish(self) -> None:
        if self.ema is not None:
            self.ema.update()
        self.steps += 1
        if self.after_step is not None:
            self.after_step()

    def state_dict(self) -> Dict:
        ar = self.arena
        m, v = {}, {}
        if self.m is not None:
            for i, n in enumerate(ar.names):
                m[n] = ar.flat_slice(self.m, i).detach().cpu().clone()
                v[n] = ar.flat_slice(self.v, i).detach().cpu().clone()
        groups = [dict(x, betas=list(x["betas"])) for x in self.param_groups]
        return {"kind": self.kind, "param_groups": groups, "steps": self.steps, "m": m, "v": v}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict) -> None:
        self.param_groups = [dict(x, betas=tuple(x["betas"])) for x in sd["param_groups"]]
        self.steps = sd.get("steps", 0)
        m, v = sd.get("m", {}), sd.get("v", {})
        ar = self.arena
        if m:
            self.m, self.v = torch.zeros_like(ar.P), torch.zeros_like(ar.P)
            for i, n in enumerate(ar.names):
                ar.flat_slice(self.m, i).copy_(m[n].to(ar.P.device).reshape(-1))
                ar.flat_slice(self.v, i).copy_(v[n].to(ar.P.device).reshape(-1))
        else:
            self.m = self.v = None


class FlatAdam(_FlatMoments):
    """torch.optim.Adam (``decoupled=False``: L2 weight decay folded into the gradient) and torch.optim.AdamW
    (``decoupled=True``: ``p *= 1 - lr * wd``) as ONE fused HIP launch over the flat arena that also writes the bf16
    shadow (csrc/kernels/optim.hip ``imk_adam_flat``); on CPU (or ``native=False``) the same formulas in flat torch
    ops. The step-dependent scalars -- ``lr / (1 - beta1^t)``, ``1 / sqrt(1 - beta2^t)`` -- are formed in double on
    the host and rounded once to fp32, so the launch does not capture into a HIP graph."""

    kind = "adam"

    def __init__(self, arena: ParamArena, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-4, decoupled: bool = False, native: Optional[bool] = None,
                 after_step: Optional[Callable[[], None]] = None):
        super().__init__(arena, native, after_step, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         decoupled=bool(decoupled))

    @torch.no_grad()
    def step(self) -> None:
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd, dec = g["lr"], g["betas"], g["eps"], g["weight_decay"], g["decoupled"]
        ar = self.arena
        t = self._begin()
        step_size, rbc2 = _f32(lr / (1.0 - b1 ** t)), _f32(1.0 / math.sqrt(1.0 - b2 ** t))
        omb1, omb2, lr_wd = _f32(1.0 - b1), _f32(1.0 - b2), _f32(1.0 - lr * wd)
        if self.native:
            from ..ops.misc import adam_flat
            adam_flat(ar.P, ar.G, self.m, self.v, ar.S, step_size, rbc2, eps, b2, omb1, omb2, wd, lr_wd, dec,
                      self.grad_scale)
        else:
            d = ar.G.mul(self.grad_scale) if self.grad_scale != 1.0 else ar.G.clone()
            if dec:
                ar.P.mul_(lr_wd)
            elif wd != 0:
                d.add_(ar.P, alpha=wd)
            self.m.add_(d - self.m, alpha=omb1)
            self.v.mul_(b2).addcmul_(d, d, value=omb2)
            ar.P.addcdiv_(self.m, self.v.sqrt().mul_(rbc2).add_(eps), value=-step_size)
            if ar.S is not None:
                ar.S.copy_(ar.P)
        self._finish()

    @torch.no_grad()
    def load_state_dict(self, sd: Dict) -> None:
        if sd.get("kind") != "torch":
            return super().load_state_dict(sd)
        # a --resume file of the stock torch.optim.Adam / AdamW route: index i is arena.params[i]
        tsd = sd["state"]
        tg, g = tsd["param_groups"][0], self.param_groups[0]
        g.update(lr=tg["lr"], betas=tuple(tg["betas"]), eps=tg["eps"], weight_decay=tg["weight_decay"])
        if "decoupled_weight_decay" in tg:
            g["decoupled"] = bool(tg["decoupled_weight_decay"])
        ar = self.arena
        state = tsd.get("state", {})
        self.steps = sd.get("steps", 0)
        if not state:
            self.m = self.v = None
            return
        self.m, self.v = torch.zeros_like(ar.P), torch.zeros_like(ar.P)
        for i in range(len(ar.params)):
            s = state[i]
            ar.view(self.m, i).copy_(s["exp_avg"].to(ar.P.device))
            ar.view(self.v, i).copy_(s["exp_avg_sq"].to(ar.P.device))
        self.steps = int(state[0]["step"])


class FlatLAMB(_FlatMoments):
    """LAMB (You et al. 2019) in the form of apex FusedLAMB / timm Lamb with the usual no-decay filter: with the
    gradient clipped to a global norm of ``max_grad_norm`` (0: off), Adam's bias-corrected quotient plus the decay,
    ``r = m_hat / (sqrt(v_hat) + eps) + wd * w``, scaled per tensor by the trust ratio ``||w|| / ||r||`` (1 where
    either norm is 0). One-dimensional tensors (BatchNorm affine, biases) get neither trust ratio nor decay, as in
    :class:`FlatLARS`. On the GPU a memset and two launches (three with clipping) over a per-tensor descriptor
    table and a fixed-size chunk table (csrc/kernels/optim.hip ``imk_lamb_step``), no host sync; on CPU the same
    math per tensor. The norms are float-atomic sums on the GPU: the trust ratios vary in their last bits from run
    to run, as LARS's do."""

    kind = "lamb"

    def __init__(self, arena: ParamArena, lr: float, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 1e-4, max_grad_norm: float = 1.0, native: Optional[bool] = None,
                 after_step: Optional[Callable[[], None]] = None):
        if max_grad_norm < 0:
            raise ValueError(f"need max_grad_norm >= 0 (0: no clipping), got {max_grad_norm}")
        super().__init__(arena, native, after_step, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         max_grad_norm=float(max_grad_norm))
        self._table = None
        self._key = None

    def launches(self) -> int:
        return 3 if self.param_groups[0]["max_grad_norm"] > 0 else 2

    @torch.no_grad()
    def step(self) -> None:
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd, mgn = g["lr"], g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"]
        ar = self.arena
        t = self._begin()
        c1, c2 = _f32(1.0 / (1.0 - b1 ** t)), _f32(1.0 / math.sqrt(1.0 - b2 ** t))
        omb1, omb2 = _f32(1.0 - b1), _f32(1.0 - b2)
        gs = self.grad_scale
        if self.native:
            from ..ops.misc import lamb_step, lamb_table
            key = (ar.P.data_ptr(), ar.G.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                   ar.S.data_ptr() if ar.S is not None else 0)
            if self._table is None or self._key != key:
                self._table, self._key = lamb_table(ar, self.m, self.v), key  # (re)built when the arenas moved
            lamb_step(self._table, lr, b2, omb1, omb2, c1, c2, eps, wd, mgn, gs)
        else:
            # norms accumulated in float64: a float32 sum over the whole arena drops the small gradients' squares
            # (ResNet-18's first step measured 0.3 % low), the kernels' tree of block sums does not
            def norm(x):
                return torch.linalg.vector_norm(x, dtype=torch.float64).item()
            c = 1.0
            if mgn > 0:
                gn = gs * norm(ar.G)
                if gn > mgn:
                    c = mgn / gn
            for i in range(len(ar.params)):
                w, m, v = ar.flat_slice(ar.P, i), ar.flat_slice(self.m, i), ar.flat_slice(self.v, i)
                d = ar.flat_slice(ar.G, i) * (gs * c)
                adapt = len(ar.shapes[i]) > 1
                m.add_(d - m, alpha=omb1)
                v.mul_(b2).addcmul_(d, d, value=omb2)
                r = (m * c1).div_(v.sqrt().mul_(c2).add_(eps))
                trust = 1.0
                if adapt:
                    r.add_(w, alpha=wd)
                    wn, rn = norm(w), norm(r)
                    if wn > 0 and rn > 0:
                        trust = wn / rn
                w.sub_(r, alpha=lr * trust)
            if ar.S is not None:
                ar.S.copy_(ar.P)
        self._finish()


class TorchOptimizer:
    """A stock torch.optim optimizer over the arena views + shadow refresh."""

    def __init__(self, arena: ParamArena, opt: torch.optim.Optimizer,
                 after_step: Optional[Callable[[], None]] = None, full_refresh: Optional[Callable] = None):
        self.arena, self.opt = arena, opt
        self.after_step = after_step
        self.full_refresh = full_refresh
        self.steps = 0
        self.ema = None  # train/ema.py ModelEma

    @property
    def param_groups(self):
        return self.opt.param_groups

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    def flats(self):
        return []

    def set_flats(self, flats):
        pass

    def step(self):
        self.opt.step()
        self.steps += 1
        if self.full_refresh is not None:
            self.full_refresh()
        if self.ema is not None:
            self.ema.update()

    def state_dict(self):
        return {"kind": "torch", "state": self.opt.state_dict(), "steps": self.steps}

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd["state"])
        self.steps = sd.get("steps", 0)


def build_optimizer(name: str, arena: ParamArena, lr: float, momentum: float = 0.9,
                    weight_decay: float = 1e-4, nesterov: bool = False,
                    after_step: Optional[Callable[[], None]] = None,
                    full_refresh: Optional[Callable[[], None]] = None, **kw):
    name = name.lower()
    params = arena.params
    if name == "sgd":
        return FlatSGD(arena, lr, momentum, kw.get("dampening", 0.0), weight_decay, nesterov,
                       after_step=after_step)
    if name == "lars":
        return FlatLARS(arena, lr, momentum, weight_decay, eta=kw.get("lars_eta", 1e-3), after_step=after_step)
    betas = tuple(kw.get("betas") or (0.9, 0.999))
    eps = kw.get("opt_eps")
    if name in ("adam", "adamw"):
        return FlatAdam(arena, lr, betas, 1e-8 if eps is None else eps, weight_decay, decoupled=name == "adamw",
                        after_step=after_step)
    if name == "lamb":
        return FlatLAMB(arena, lr, betas, 1e-6 if eps is None else eps, weight_decay,
                        max_grad_norm=kw.get("lamb_max_grad_norm", 1.0), after_step=after_step)
    if name == "adagrad":
        o = torch.optim.Adagrad(params, lr=lr, lr_decay=0, weight_decay=weight_decay,
                                initial_accumulator_value=0, eps=1e-10)
    elif name == "rmsprop":
        o = torch.optim.RMSprop(params, lr=lr, alpha=0.99, eps=1e-8, weight_decay=weight_decay,
                                momentum=momentum, centered=False)
    elif name == "adadelta":
        o = torch.optim.Adadelta(params, lr=lr, rho=0.9, eps=1e-6, weight_decay=weight_decay)
    elif name == "asgd":
        o = torch.optim.ASGD(params, lr=lr, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=weight_decay)
    elif name == "nadam":
        o = torch.optim.NAdam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay,
                              momentum_decay=kw.get("schedule_decay", 4e-3))
    elif name == "fr":
        raise ValueError("optimizer 'FR' comes from the reference's missing custom_optimizers "
                         "module (imagenet.py:36) and is not specified anywhere; not implemented")
    else:
        raise ValueError(f"unknown optimizer {name!r}")
    return TorchOptimizer(arena, o, after_step, full_refresh)
