"""Squeeze-and-excitation block tail on the HIP kernels of ``csrc/kernels/se.hip`` (NHWC bf16).

The tail of an SE block is ``out = relu(s[n,c] * bn(a) + idt)`` with the gate ``s = sigmoid(fc2(relu(fc1(z))))``
computed from the block's own pooled output ``z = mean_hw bn(a)``. With the training BatchNorm as a per-channel
affine ``u = sc * a + sh`` (``bn_scale_shift``) the mean is taken of the raw conv output (``z = sc * X1 / HW + sh``),
so the forward is one extra streaming pass (:func:`se_squeeze`), one small launch (:func:`se_excite_fwd`) and the
tail pass (:func:`se_scale_add_relu`). The backward makes the two passes of the unfused BatchNorm tail:
:func:`se_bwd_reduce` writes ``g = dout * [out > 0]`` with the per-(n, c) sums ``G1 = sum g``, ``G2 = sum g a``; the
gate's backward, the four SE gradients and the BatchNorm's two reductions follow from those sums without touching
the tensor again (:func:`se_excite_bwd`), and :func:`se_bn_apply_bwd` is the apply pass. No kernel uses a float atomic:
two calls on the same inputs give the same bits.

The SE state (X1, z, h, s, G1, G2, dpool, partials) comes from torch's caching allocator per call.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .bn import bn_scale_shift
from .grad_sink import notify_ready


def _nhwc(a: torch.Tensor) -> Tuple[int, int, int]:
    if a.dim() != 4 or a.dtype != torch.bfloat16 or not a.is_contiguous():
        raise ValueError(f"se: expected a contiguous NHWC bf16 tensor, got {tuple(a.shape)} {a.dtype}")
    return a.shape[0], a.shape[1] * a.shape[2], a.shape[3]


def _f32(n: int, like: torch.Tensor) -> Optional[torch.Tensor]:
    return torch.empty(n, device=like.device, dtype=torch.float32) if n else None


def se_squeeze(a: torch.Tensor) -> torch.Tensor:
    """X1 [N, C] fp32 = sum over the pixels of ``a`` [N, H, W, C], in a fixed order."""
    N, HW, C = _nhwc(a)
    k = _lib.kernels()
    X1 = torch.empty((N, C), device=a.device, dtype=torch.float32)
    part = _f32(k.imk_se_reduce_floats(N, HW, C, 1), a)
    _lib.check(k.imk_se_squeeze(a.data_ptr(), X1.data_ptr(), _lib.ptr(part), N, HW, C, _lib.stream_ptr()),
               "se squeeze")
    return X1


def se_excite_fwd(X1: torch.Tensor, ss: Optional[torch.Tensor], se, HW: int):
    """(z [N, C], h [N, R], s [N, C]) fp32: z = ss[0] * X1 / HW + ss[1] (``ss`` None: X1 / HW),
    h = relu(fc1 z), s = sigmoid(fc2 h), the GEMMs on the bf16 MFMA: the weights are the arena's bf16 shadows, z and h
    enter as three bf16 terms each (their fp32 values, so the ReLU masks of h and of the output are the fp32 gate's)."""
    N, C = X1.shape
    R = se.reduced
    z, s = torch.empty_like(X1), torch.empty_like(X1)
    h = torch.empty((N, R), device=X1.device, dtype=torch.float32)
    _lib.check(_lib.kernels().imk_se_excite_fwd(
        X1.data_ptr(), _lib.ptr(ss), se.fc1.w_bf16.data_ptr(), se.fc1.bias.data_ptr(), se.fc2.w_bf16.data_ptr(),
        se.fc2.bias.data_ptr(), z.data_ptr(), h.data_ptr(), s.data_ptr(), N, HW, C, R, _lib.stream_ptr()),
        "se excite fwd")
    return z, h, s


def se_scale_add_relu(a: torch.Tensor, ss: Optional[torch.Tensor], s: torch.Tensor, idt: torch.Tensor) -> torch.Tensor:
    """relu(s[n, c] * (ss[0] * a + ss[1]) + idt) as bf16 (``ss`` None: the identity affine)."""
    N, HW, C = _nhwc(a)
    if idt.shape != a.shape or idt.dtype != a.dtype or not idt.is_contiguous():
        raise ValueError(f"se: shortcut {tuple(idt.shape)} {idt.dtype} does not match {tuple(a.shape)}")
    out = torch.empty_like(a)
    _lib.check(_lib.kernels().imk_se_scale_add_relu(a.data_ptr(), idt.data_ptr(), _lib.ptr(ss), s.data_ptr(),
                                                    out.data_ptr(), N, HW, C, _lib.stream_ptr()), "se scale add relu")
    return out


def se_bwd_reduce(dout: torch.Tensor, out: torch.Tensor, a: torch.Tensor):
    """(g, G) of one pass over dout, out and a: g = dout * [out > 0] (bf16), G [2, N, C] fp32 = (sum g, sum g a)."""
    N, HW, C = _nhwc(a)
    k = _lib.kernels()
    g = torch.empty_like(a)
    G = torch.empty((2, N, C), device=a.device, dtype=torch.float32)
    part = _f32(k.imk_se_reduce_floats(N, HW, C, 2), a)
    _lib.check(k.imk_se_bwd_reduce(dout.data_ptr(), out.data_ptr(), a.data_ptr(), g.data_ptr(), G.data_ptr(),
                                   _lib.ptr(part), N, HW, C, _lib.stream_ptr()), "se bwd reduce")
    return g, G


def se_excite_bwd(G, X1, ss, z, h, s, bn, se, HW: int):
    """Everything of the backward that does not scale with HW: (dpool [N, C], bsum [2, C] = (sum du, sum du xhat)).
    The gradients of fc1 / fc2 (weights and biases) and of the BatchNorm's gamma / beta are added into their fp32
    slots of the gradient arena and the reducer is told."""
    N, C = X1.shape
    R = se.reduced
    k = _lib.kernels()
    ws = _f32(k.imk_se_excite_bwd_floats(N, C, R), X1)
    dpool = torch.empty_like(X1)
    bsum = torch.empty((2, C), device=X1.device, dtype=torch.float32)
    f1, f2 = se.fc1, se.fc2
    _lib.check(k.imk_se_excite_bwd(
        G.data_ptr(), X1.data_ptr(), ss.data_ptr(), bn.work.save.data_ptr(), z.data_ptr(), h.data_ptr(), s.data_ptr(),
        f1.w_bf16.data_ptr(), f2.w_bf16.data_ptr(), ws.data_ptr(), dpool.data_ptr(), bsum.data_ptr(),
        f1.weight.grad.data_ptr(), f1.bias.grad.data_ptr(), f2.weight.grad.data_ptr(), f2.bias.grad.data_ptr(),
        bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), N, HW, C, R, _lib.stream_ptr()), "se excite bwd")
    for p in (bn.weight, bn.bias, f2.weight, f2.bias, f1.weight, f1.bias):
        notify_ready(p)
    return dpool, bsum


def se_bn_apply_bwd(g, a, s, dpool, ss, bn, bsum) -> torch.Tensor:
    """dA = sc (du - sum du / M - xhat sum du xhat / M) with du = s g + dpool recomputed per element."""
    N, HW, C = _nhwc(a)
    dA = torch.empty_like(a)
    _lib.check(_lib.kernels().imk_se_bn_apply_bwd(g.data_ptr(), a.data_ptr(), s.data_ptr(), dpool.data_ptr(),
                                                  ss.data_ptr(), bn.work.save.data_ptr(), bsum.data_ptr(),
                                                  dA.data_ptr(), N, HW, C, _lib.stream_ptr()), "se bn apply bwd")
    return dA


def se_tail_forward(a: torch.Tensor, bn, idt: torch.Tensor, se):
    """Training forward of an SE block's tail: ``a`` the last conv's raw output (its statistics in ``bn.work.slab``),
    ``idt`` the shortcut. Returns (out, saved) with ``saved`` what :func:`se_tail_backward` needs."""
    N, HW, C = _nhwc(a)
    ss = bn_scale_shift(a, bn)  # one launch: leaves bn.work.save / stats as bn_act_forward does
    X1 = se_squeeze(a)
    z, h, s = se_excite_fwd(X1, ss, se, HW)
    out = se_scale_add_relu(a, ss, s, idt)
    return out, (a, out, ss, X1, z, h, s)


def se_tail_backward(dout: torch.Tensor, saved, bn, se):
    """(dA, g): the gradient of the last conv's output and of the shortcut (``g = dout * [out > 0]``)."""
    a, out, ss, X1, z, h, s = saved
    HW = a.shape[1] * a.shape[2]
    g, G = se_bwd_reduce(dout.contiguous(), out, a)
    dpool, bsum = se_excite_bwd(G, X1, ss, z, h, s, bn, se, HW)
    return se_bn_apply_bwd(g, a, s, dpool, ss, bn, bsum), g


def se_gate_eval(u: torch.Tensor, idt: torch.Tensor, se) -> torch.Tensor:
    """Inference: ``u`` is the last conv's output with the folded BatchNorm applied in its epilogue."""
    N, HW, C = _nhwc(u)
    _, _, s = se_excite_fwd(se_squeeze(u), None, se, HW)
    return se_scale_add_relu(u, None, s, idt)


class SETailFn(torch.autograd.Function):
    """The tail as an autograd node over (a, idt): the per-op path (``NativeState.fused_blocks = False``)."""

    @staticmethod
    def forward(ctx, a, idt, bn, se):
        out, saved = se_tail_forward(a, bn, idt, se)
        ctx.bn, ctx.se, ctx.state = bn, se, saved[2:]
        ctx.save_for_backward(a, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        dA, g = se_tail_backward(dout, tuple(ctx.saved_tensors) + tuple(ctx.state), ctx.bn, ctx.se)
        return dA, g, None, None
