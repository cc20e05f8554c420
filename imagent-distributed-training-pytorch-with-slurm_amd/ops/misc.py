"""Pooling, loss + metrics, optimizer and input kernels (Python side)."""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .conv import conv_out_size


# ----------------------------------------------------------------- pooling
class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        N, H, W, Cc = x.shape
        OH, OW = conv_out_size(H, k, s, p), conv_out_size(W, k, s, p)
        y = torch.empty((N, OH, OW, Cc), device=x.device, dtype=x.dtype)
        idx = torch.empty((N, OH, OW, Cc), device=x.device, dtype=torch.uint8)
        _lib.check(_lib.kernels().imk_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W,
                                                  Cc, OH, OW, k, s, p, _lib.stream_ptr()), "maxpool")
        ctx.save_for_backward(idx)
        ctx.geom = (N, H, W, Cc, OH, OW, k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, H, W, Cc, OH, OW, k, s, p = ctx.geom
        dx = torch.empty((N, H, W, Cc), device=dy.device, dtype=torch.bfloat16)
        _lib.check(_lib.kernels().imk_maxpool_bwd(dy.contiguous().data_ptr(), idx.data_ptr(),
                                                  dx.data_ptr(), N, H, W, Cc, OH, OW, k, s, p,
                                                  _lib.stream_ptr()), "maxpool bwd")
        return dx, None, None, None


class BNReluPoolFn(torch.autograd.Function):
    """y = maxpool(relu(bn(x))) for the stem, fused both ways: the forward pools
    bf16(relu(bn(x))) straight from the BN input (``imk_maxpool_fwd_bn``: the
    BN output is never written), the backward stores the ReLU-masked BN
    upstream gradient and reduces the BN-backward sums in the same pass
    (``imk_maxpool_bwd_bnr``), then one BN apply pass -- instead of BN forward
    + pool forward and pool backward + BN reduce + BN apply.
    Reference ops: torchvision resnet ``bn1 -> relu -> maxpool``
    (/root/reference/imagenet.py:312)."""

    @staticmethod
    def forward(ctx, x, bn, k, s, p):
        from .bn import stats_finalize
        N, H, W, Cc = x.shape
        OH, OW = conv_out_size(H, k, s, p), conv_out_size(W, k, s, p)
        y = torch.empty((N, OH, OW, Cc), device=x.device, dtype=x.dtype)
        idx = torch.empty((N, OH, OW, Cc), device=x.device, dtype=torch.uint8)
        w = bn.work
        stats_finalize(w, N * H * W)  # conv-epilogue slab -> (mean, var) (also read by the running-stat update)
        _lib.check(_lib.kernels().imk_maxpool_fwd_bn(
            x.data_ptr(), w.stats.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), w.save.data_ptr(),
            y.data_ptr(), idx.data_ptr(), None, N, H, W, Cc, OH, OW, k, s, p, bn.eps, _lib.stream_ptr()),
            "bn + maxpool")
        ctx.save_for_backward(x, idx)
        ctx.bn = bn
        ctx.geom = (N, H, W, Cc, OH, OW, k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .bn import bn_apply_backward
        x, idx = ctx.saved_tensors
        bn = ctx.bn
        N, H, W, Cc, OH, OW, k, s, p = ctx.geom
        g = torch.empty((N, H, W, Cc), device=dy.device, dtype=torch.bfloat16)
        w = bn.work
        _lib.check(_lib.kernels().imk_maxpool_bwd_bnr(
            dy.contiguous().data_ptr(), idx.data_ptr(), g.data_ptr(), x.data_ptr(), None, w.save.data_ptr(),
            bn.weight.data_ptr(), bn.bias.data_ptr(), w.scratch.data_ptr(), N, H, W, Cc, OH, OW, k, s, p,
            _lib.stream_ptr()), "maxpool bwd + bn reduce")
        dx, _ = bn_apply_backward(g, x, None, bn, None, 0)
        from . import streams
        streams.flush_deferred()  # layer1's conv1 weight gradient, after this BN pass
        return dx, None, None, None, None


class StemFn(torch.autograd.Function):
    """The 224-px stem -- conv1 (7x7 / 2) -> bn1 -> ReLU -> maxpool -- as ONE autograd node, so that the stem BN's
    backward apply pass never runs: the pool backward stores the ReLU-masked gradient g and reduces the BN sums
    (as BNReluPoolFn), ``imk_bn_bwd_coef`` turns them into dx = A g + B x + c (and dgamma / dbeta), and the stem's
    band weight gradient applies that on its operand staging (``ops.conv.stem_wgrad_bnx``) -- the stem conv's
    input (the image) needs no gradient, so dx is never materialised (one read of g and x and one write of dx
    less: 3 x 3.3 GB at 2048 img/GPU). Reference ops: torchvision resnet ``conv1 -> bn1 -> relu -> maxpool``
    (/root/reference/imagenet.py:312, backward :128)."""

    @staticmethod
    def forward(ctx, img, weight, conv, bn, k, s, p):
        from .bn import stats_finalize
        from .conv import igemm_fwd
        x = igemm_fwd(img, conv.w_bf16, conv.stride, conv.padding, conv.kh, conv.kw, stats=bn.work, stem=True)
        N, H, W, Cc = x.shape
        OH, OW = conv_out_size(H, k, s, p), conv_out_size(W, k, s, p)
        y = torch.empty((N, OH, OW, Cc), device=x.device, dtype=x.dtype)
        idx = torch.empty((N, OH, OW, Cc), device=x.device, dtype=torch.uint8)
        # the BN input at each window's argmax: the pool backward's ReLU mask and BN sums come from it
        # instead of a read of x (4x its bytes): pool backward 2,034 -> 1,772 us, pool forward 1,052 -> 1,167 us
        # at 2048 img; in-step 17,130 / 17,181 vs 17,091 / 17,169 img/s (same box)
        xsel = torch.empty_like(y)
        w = bn.work
        stats_finalize(w, N * H * W)
        _lib.check(_lib.kernels().imk_maxpool_fwd_bn(
            x.data_ptr(), w.stats.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), w.save.data_ptr(),
            y.data_ptr(), idx.data_ptr(), xsel.data_ptr(), N, H, W, Cc, OH, OW, k, s, p, bn.eps,
            _lib.stream_ptr()), "bn + maxpool")
        ctx.save_for_backward(img, x, idx, xsel)
        ctx.mods = (conv, bn)
        ctx.geom = (N, H, W, Cc, OH, OW, k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import streams
        from .conv import stem_wgrad_bnx
        from .grad_sink import notify_ready
        img, x, idx, xsel = ctx.saved_tensors
        conv, bn = ctx.mods
        N, H, W, Cc, OH, OW, k, s, p = ctx.geom
        g = torch.empty((N, H, W, Cc), device=dy.device, dtype=torch.bfloat16)
        w = bn.work
        kern = _lib.kernels()
        _lib.check(kern.imk_maxpool_bwd_bnr(
            dy.contiguous().data_ptr(), idx.data_ptr(), g.data_ptr(), x.data_ptr(), xsel.data_ptr(), w.save.data_ptr(),
            bn.weight.data_ptr(), bn.bias.data_ptr(), w.scratch.data_ptr(), N, H, W, Cc, OH, OW, k, s, p,
            _lib.stream_ptr()), "maxpool bwd + bn reduce")
        coef = torch.empty((3, Cc), device=dy.device, dtype=torch.float32)
        _lib.check(kern.imk_bn_bwd_coef(w.scratch.data_ptr(), w.save.data_ptr(), bn.weight.data_ptr(),
                                        bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), coef.data_ptr(),
                                        N * H * W, Cc, _lib.stream_ptr()), "stem bn bwd coef")
        notify_ready(bn.weight)
        notify_ready(bn.bias)
        streams.flush_deferred()  # layer1's conv1 weight gradient (queued behind this BN's backward)
        side = streams.side_stream(dy.device)
        if side is not None:
            streams.wait(side, torch.cuda.current_stream(dy.device))
        with torch.cuda.stream(side) if side is not None else _NullCtx():
            gp = conv.grad_pad
            ok = stem_wgrad_bnx(g, img, gp, x, coef, conv.stride, conv.padding, conv.kh, conv.kw)
            assert ok, "StemFn needs the band stem's shape (models.native checks it)"
            gw = conv.weight.grad
            _lib.check(kern.imk_stem_grad_fold(gp.data_ptr(), gw.data_ptr(), gp.shape[0], conv.in_channels,
                                               conv.kh, conv.kw, _lib.stream_ptr()), "stem grad fold")
            notify_ready(conv.weight)
        if side is not None:
            streams.protect(g, img, x, coef)
            streams.ensure_join_after_backward()
        return None, None, None, None, None, None, None


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def stem_fused_ok(img: torch.Tensor, conv) -> bool:
    """Does StemFn cover this stem (the band kernels' shape: 224-px 4-channel input, 7x7 / 2 / 3, 64 channels)?"""
    return (img.dim() == 4 and img.shape[1] == 224 and img.shape[2] == 224 and img.shape[3] == 4 and
            conv.kh == 7 and conv.kw == 7 and conv.stride == 2 and conv.padding == 3 and conv.out_channels == 64 and
            getattr(conv, "grad_pad", None) is not None)


def maxpool_eval(x, k, s, p):
    N, H, W, Cc = x.shape
    OH, OW = conv_out_size(H, k, s, p), conv_out_size(W, k, s, p)
    y = torch.empty((N, OH, OW, Cc), device=x.device, dtype=x.dtype)
    _lib.check(_lib.kernels().imk_maxpool_fwd(x.data_ptr(), y.data_ptr(), None, N, H, W, Cc, OH, OW,
                                              k, s, p, _lib.stream_ptr()), "maxpool")
    return y


class AvgPoolFn(torch.autograd.Function):
    """Global average pool NHWC [N,H,W,C] -> [N,C] (AdaptiveAvgPool2d((1,1)) + flatten)."""

    @staticmethod
    def forward(ctx, x):
        N, H, W, Cc = x.shape
        y = torch.empty((N, Cc), device=x.device, dtype=x.dtype)
        _lib.check(_lib.kernels().imk_avgpool_fwd(x.data_ptr(), y.data_ptr(), N, H * W, Cc,
                                                  _lib.stream_ptr()), "avgpool")
        ctx.shape = (N, H, W, Cc)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, Cc = ctx.shape
        dx = torch.empty((N, H, W, Cc), device=dy.device, dtype=torch.bfloat16)
        _lib.check(_lib.kernels().imk_avgpool_bwd(dy.to(torch.bfloat16).contiguous().data_ptr(),
                                                  dx.data_ptr(), N, H * W, Cc, _lib.stream_ptr()),
                   "avgpool bwd")
        return dx


# ------------------------------------------------------------ loss+metrics
class XentFn(torch.autograd.Function):
    """Mean softmax cross-entropy (nn.CrossEntropyLoss, imagenet.py:323) with
    fused top-1/top-5 counting into a device metrics vector
    ``[loss_sum, top1_hits, top5_hits, rows]`` - no host sync per step."""

    @staticmethod
    def forward(ctx, logits, labels, metrics, smoothing):
        logits = logits.contiguous()
        B, NC = logits.shape
        lse = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)  # cleared by imk_xent_fwd
        _lib.check(_lib.kernels().imk_xent_fwd(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(),
                                               loss.data_ptr(), _lib.ptr(metrics), B, NC,
                                               float(smoothing), _lib.stream_ptr()), "xent")
        ctx.save_for_backward(logits, labels, lse)
        ctx.smoothing = smoothing
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, labels, lse = ctx.saved_tensors
        B, NC = logits.shape
        g = gout.to(torch.float32).contiguous()
        # the logits' own dtype (fp32): autograd would otherwise cast a bf16 gradient back with an ATen copy; the
        # linear layer's backward rounds it to bf16 with its own kernel
        dz = torch.empty((B, NC), device=logits.device, dtype=logits.dtype)
        fn = _lib.kernels().imk_xent_bwd_f32 if logits.dtype == torch.float32 else _lib.kernels().imk_xent_bwd
        _lib.check(fn(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), g.data_ptr(), dz.data_ptr(), B, NC,
                      float(ctx.smoothing), _lib.stream_ptr()), "xent bwd")
        return dz, None, None, None


class XentPairFn(torch.autograd.Function):
    """The two-label form of :class:`XentFn` for Mixup / CutMix batches (``data/mix.py``): row b's target is
    ``(1 - eps) (lam[b] 1[ya[b]] + (1 - lam[b]) 1[yb[b]]) + eps / NC``; top-1 / top-5 count against the label with
    the larger weight (``ya`` when ``lam >= 0.5``). ``lam == 1`` gives ``XentFn`` on ``ya`` (``lse`` and the
    gradient bit for bit). ``ya`` / ``yb`` int64 [B], ``lam`` float32 [B]. One Function for the bf16 and the fp32
    kernel path: the gradient kernel follows the logits' dtype, as ``XentFn.backward``."""

    @staticmethod
    def forward(ctx, logits, ya, yb, lam, metrics, smoothing):
        logits = logits.contiguous()
        B, NC = logits.shape
        if ya.shape != (B,) or yb.shape != (B,) or lam.shape != (B,):
            raise ValueError(f"XentPairFn: ya {tuple(ya.shape)}, yb {tuple(yb.shape)}, lam {tuple(lam.shape)} for "
                             f"{B} rows")
        ya, yb = ya.to(torch.int64).contiguous(), yb.to(torch.int64).contiguous()
        lam = lam.to(torch.float32).contiguous()
        lse = torch.empty(B, device=logits.device, dtype=torch.float32)
        loss = torch.empty((), device=logits.device, dtype=torch.float32)  # cleared by imk_xent_pair_fwd
        _lib.check(_lib.kernels().imk_xent_pair_fwd(logits.data_ptr(), ya.data_ptr(), yb.data_ptr(), lam.data_ptr(),
                                                    lse.data_ptr(), loss.data_ptr(), _lib.ptr(metrics), B, NC,
                                                    float(smoothing), _lib.stream_ptr()), "xent pair")
        ctx.save_for_backward(logits, ya, yb, lam, lse)
        ctx.smoothing = smoothing
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, ya, yb, lam, lse = ctx.saved_tensors
        B, NC = logits.shape
        g = gout.to(torch.float32).contiguous()
        dz = torch.empty((B, NC), device=logits.device, dtype=logits.dtype)  # (XentFn.backward on the dtype)
        k = _lib.kernels()
        fn = k.imk_xent_pair_bwd_f32 if logits.dtype == torch.float32 else k.imk_xent_pair_bwd
        _lib.check(fn(logits.data_ptr(), ya.data_ptr(), yb.data_ptr(), lam.data_ptr(), lse.data_ptr(), g.data_ptr(),
                      dz.data_ptr(), B, NC, float(ctx.smoothing), _lib.stream_ptr()), "xent pair bwd")
        return dz, None, None, None, None, None


# -------------------------------------------------------------------- SGD
def sgd_flat(p: torch.Tensor, g: torch.Tensor, buf: Optional[torch.Tensor],
             shadow: Optional[torch.Tensor], lr: float, momentum: float, dampening: float,
             weight_decay: float, nesterov: bool, first: bool, grad_scale: float = 1.0) -> None:
    _lib.check(_lib.kernels().imk_sgd(p.data_ptr(), g.data_ptr(), _lib.ptr(buf), _lib.ptr(shadow),
                                      p.numel(), lr, momentum, dampening, weight_decay,
                                      1 if nesterov else 0, 1 if first else 0, grad_scale,
                                      _lib.stream_ptr()), "sgd")


def adam_flat(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, shadow: Optional[torch.Tensor],
              step_size: float, rbc2: float, eps: float, beta2: float, omb1: float, omb2: float, weight_decay: float,
              lr_wd: float, decoupled: bool, grad_scale: float = 1.0) -> None:
    """One Adam / AdamW step over the flat arenas (csrc/kernels/optim.hip adam_kernel): ``step_size = lr / (1 -
    beta1^t)``, ``rbc2 = 1 / sqrt(1 - beta2^t)``, ``omb = 1 - beta``, ``lr_wd = 1 - lr * weight_decay`` (read by the
    decoupled form only). ``g`` is read only; ``shadow`` (bf16, may be None) becomes ``bf16(p)``."""
    n = p.numel()
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.data_ptr() % 16 == 0
    assert shadow is None or (shadow.dtype == torch.bfloat16 and shadow.numel() == n and shadow.is_contiguous()
                              and shadow.data_ptr() % 8 == 0)
    _lib.check(_lib.kernels().imk_adam_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _lib.ptr(shadow),
                                            n, step_size, rbc2, eps, beta2, omb1, omb2, weight_decay, lr_wd,
                                            1 if decoupled else 0, grad_scale, _lib.stream_ptr()), "adam")


def lamb_chunk() -> int:
    """Elements per chunk (= per block) of the LAMB kernels."""
    return _lib.kernels().imk_optim_const(0)


class LambTable:
    """The device tables of :func:`lamb_step` over a :class:`~imagent_amd.models.arena.ParamArena` (see
    :func:`lamb_table`). ``norms`` after a step: ``sum w^2`` [T], ``sum r^2`` [T], ``sum g^2`` (0 with clipping
    off)."""

    def __init__(self, descs, chunks, norms, count, nchunks, g_flat):
        self.descs, self.chunks, self.norms = descs, chunks, norms
        self.count, self.nchunks, self.g_flat = count, nchunks, g_flat


def lamb_table(arena, m: torch.Tensor, v: torch.Tensor) -> LambTable:
    """Descriptor ``i`` is parameter ``i`` of ``arena`` with its slices of ``m`` and ``v`` (flat, ``arena.P``'s
    offsets); ``adapt`` = more than one dimension. Beside it the chunk table: ``(tensor, first element)`` per
    :func:`lamb_chunk` elements, tensor after tensor, a chunk never spanning two tensors."""
    P, G, S = arena.P, arena.G, arena.S
    T, chunk = len(arena.params), lamb_chunk()
    for t in (P, G, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == arena.total
        assert t.data_ptr() % 16 == 0
    assert S is None or (S.numel() == arena.total and S.data_ptr() % 8 == 0)
    d = (_lib.LambDesc * T)()
    rows = []
    for i in range(T):
        o, n = arena.offsets[i], arena.numels[i]
        assert o % 4 == 0 and 0 <= o and o + n <= arena.total  # f32x4 body from the first element of every slice
        d[i].p, d[i].g = P[o:o + n].data_ptr(), G[o:o + n].data_ptr()
        d[i].m, d[i].v = m[o:o + n].data_ptr(), v[o:o + n].data_ptr()
        d[i].shadow = S[o:o + n].data_ptr() if S is not None else None
        d[i].n = n
        d[i].adapt = 1 if len(arena.shapes[i]) > 1 else 0
        rows += [(i, f) for f in range(0, n, chunk)]
    dev = P.device
    descs = torch.frombuffer(bytearray(bytes(memoryview(d))), dtype=torch.uint8).to(dev)
    chunks = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(dev)
    norms = torch.zeros(2 * T + 1, dtype=torch.float32, device=dev)
    return LambTable(descs, chunks, norms, T, len(rows), G)


def lamb_step(tab: LambTable, lr: float, beta2: float, omb1: float, omb2: float, c1: float, c2: float, eps: float,
              weight_decay: float, max_grad_norm: float, grad_scale: float = 1.0) -> None:
    """One LAMB step over ``tab`` (csrc/kernels/optim.hip): a memset of the norms and two launches, three with
    ``max_grad_norm > 0`` (the global gradient norm). ``c1 = 1 / (1 - beta1^t)``, ``c2 = 1 / sqrt(1 - beta2^t)``."""
    _lib.check(_lib.kernels().imk_lamb_step(tab.descs.data_ptr(), tab.count, tab.chunks.data_ptr(), tab.nchunks,
                                            tab.g_flat.data_ptr(), tab.g_flat.numel(), tab.norms.data_ptr(), lr,
                                            beta2, omb1, omb2, c1, c2, eps, weight_decay, max_grad_norm, grad_scale,
                                            _lib.stream_ptr()), "lamb step")


def ema_flat(e: torch.Tensor, p: torch.Tensor, omd: float) -> None:
    """``e += omd * (p - e)`` over two flat fp32 arenas of one length."""
    assert e.numel() == p.numel() and e.dtype == p.dtype == torch.float32
    assert e.is_contiguous() and p.is_contiguous()
    _lib.check(_lib.kernels().imk_ema_flat(e.data_ptr(), p.data_ptr(), e.numel(), omd, _lib.stream_ptr()), "ema")


def ema_swap(p: torch.Tensor, e: torch.Tensor, shadow: Optional[torch.Tensor]) -> None:
    """``p <-> e`` in place and ``shadow = bf16(new p)`` (``shadow`` may be None)."""
    assert e.numel() == p.numel() and e.dtype == p.dtype == torch.float32
    assert e.is_contiguous() and p.is_contiguous()
    assert shadow is None or (shadow.numel() == p.numel() and shadow.dtype == torch.bfloat16)
    _lib.check(_lib.kernels().imk_ema_swap(p.data_ptr(), e.data_ptr(), _lib.ptr(shadow), p.numel(),
                                           _lib.stream_ptr()), "ema swap")


def ema_buf_table(bufs, offsets, device) -> torch.Tensor:
    """The device descriptor table of :func:`ema_bufs`: buffer ``i`` averages into ``flat[offsets[i]:][:numel]``."""
    d = (_lib.EmaBufDesc * len(bufs))()
    for q, b, o in zip(d, bufs, offsets):
        assert b.dtype == torch.float32 and b.is_contiguous()
        q.buf, q.off, q.n = b.data_ptr(), o, b.numel()
    return torch.frombuffer(bytearray(bytes(memoryview(d))), dtype=torch.uint8).to(device)


def ema_bufs(table: torch.Tensor, count: int, max_n: int, flat: torch.Tensor, omd: float, swap: bool) -> None:
    """One launch over ``table`` (:func:`ema_buf_table`): the average of every buffer into ``flat``, or
    (``swap``) buffer <-> average in place."""
    _lib.check(_lib.kernels().imk_ema_bufs(table.data_ptr(), count, max_n, flat.data_ptr(), omd, 1 if swap else 0,
                                           _lib.stream_ptr()), "ema buffers")


def cast_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    _lib.check(_lib.kernels().imk_cast_bf16(src.data_ptr(), dst.data_ptr(), src.numel(),
                                            _lib.stream_ptr()), "cast")


def uncast_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    """bf16 ``src`` -> fp32 ``dst`` (same numel) on the current stream."""
    _lib.check(_lib.kernels().imk_uncast_bf16(src.data_ptr(), dst.data_ptr(), src.numel(),
                                              _lib.stream_ptr()), "uncast")


class TransposePlan:
    """Batched ``[Co][T][Ci] -> [Ci][T][Co]`` re-layout of every conv's bf16
    weight shadow into its dgrad shadow: one launch per optimizer step."""

    def __init__(self, items: Sequence[tuple], device):
        descs = (_lib.TDesc * max(1, len(items)))()
        tile = 0
        for i, (src, dst, Co, T, Ci) in enumerate(items):
            descs[i].src, descs[i].dst = src.data_ptr(), dst.data_ptr()
            descs[i].Co, descs[i].T, descs[i].Ci, descs[i].tile0 = Co, T, Ci, tile
            tile += ((Co + 31) // 32) * ((Ci + 31) // 32) * T
        raw = bytes(memoryview(descs))[: C.sizeof(_lib.TDesc) * len(items)]
        self.n = len(items)
        self.tiles = tile
        self.desc = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device) if items else None

    def run(self) -> None:
        if self.n:
            _lib.check(_lib.kernels().imk_transpose_batched(self.desc.data_ptr(), self.n, self.tiles,
                                                            _lib.stream_ptr()), "transpose")


# -------------------------------------------------------------- normalize
def resize_normalize_u8(images: torch.Tensor, out_hw, cpad: int, mean: Sequence[float], std: Sequence[float],
                        flip: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B, Hs, Ws, 3] -> bf16 NHWC [B, H, W, cpad]: bilinear resample to (H, W) (half-pixel centres,
    ``F.interpolate(mode='bilinear', align_corners=False)``) fused with (x/255 - mean)/std -- the records stored
    smaller than the model input (``--record-resize``), resized on the GPU instead of on the host
    (imagenet.py:281's Resize, moved after the gather)."""
    B, Hs, Ws, _ = images.shape
    H, W = out_hw
    if out is None:
        out = torch.empty((B, H, W, cpad), device=images.device, dtype=torch.bfloat16)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.kernels().imk_resize_normalize_u8(images.data_ptr(), out.data_ptr(), _lib.ptr(flip), B, Hs, Ws,
                                                      H, W, cpad, C.cast(m, C.c_void_p), C.cast(s, C.c_void_p),
                                                      _lib.stream_ptr()), "resize + normalize")
    return out


def rrc_normalize_u8(images: torch.Tensor, out_hw, cpad: int, mean: Sequence[float], std: Sequence[float],
                     boxes: torch.Tensor, flip: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     dtype=torch.bfloat16) -> torch.Tensor:
    """uint8 [B, Hs, Ws, 3] -> NHWC [B, H, W, cpad] (bf16 or fp32): every sample's box ``boxes[b] = (top, left, h,
    w)`` resampled to (H, W) with the antialiased triangle filter -- ``F.interpolate(crop, (H, W), mode='bilinear',
    antialias=True, align_corners=False)``, "crop, then resize" -- fused with (x/255 - mean)/std and an optional
    horizontal flip (RandomResizedCrop, ``data/augment.py``; csrc/kernels/misc.hip rrc_normalize_kernel).
    ``boxes`` on the host are checked here (ValueError for a box outside the image) and copied; boxes on the device
    are not synchronised on -- the kernel clamps them into the image, so no value reads out of bounds."""
    B, Hs, Ws, _ = images.shape
    H, W = out_hw
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"rrc_normalize_u8: dtype {dtype} (bf16 or fp32)")
    if boxes.dim() != 2 or tuple(boxes.shape) != (B, 4):
        raise ValueError(f"rrc_normalize_u8: boxes {tuple(boxes.shape)}, expected ({B}, 4)")
    if not boxes.is_cuda:
        bx = boxes.to(torch.int64)
        t, l, h, w = bx.unbind(1)
        bad = (t < 0) | (l < 0) | (h < 1) | (w < 1) | (t + h > Hs) | (l + w > Ws)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise ValueError(f"rrc_normalize_u8: box {i} = {bx[i].tolist()} (top, left, h, w) lies outside the "
                             f"{Hs}x{Ws} image")
    boxes = boxes.to(device=images.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty((B, H, W, cpad), device=images.device, dtype=dtype)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.kernels().imk_rrc_normalize_u8(images.data_ptr(), out.data_ptr(), boxes.data_ptr(), _lib.ptr(flip),
                                                   B, Hs, Ws, H, W, cpad, C.cast(m, C.c_void_p),
                                                   C.cast(s, C.c_void_p), 1 if out.dtype == torch.float32 else 0,
                                                   _lib.stream_ptr()), "random-resized-crop + normalize")
    return out


def mix_pairs(x: torch.Tensor, pair: torch.Tensor, lam: torch.Tensor, boxes: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mixup / CutMix of a batch with itself, one HIP kernel (csrc/kernels/misc.hip mix_pairs_kernel): ``x`` NHWC
    [B, H, W, Cp] (bf16 or fp32, Cp 4 or 8, as the normalise kernels leave it), ``pair`` int32 [B] the partner of
    each sample, ``lam`` float32 [B], ``boxes`` int32 [B, 4] = (top, left, h, w). A sample with a non-empty box
    takes its partner's pixels inside the box (a bit-exact select); one with an empty box becomes
    ``lam x[b] + (1 - lam) x[pair[b]]`` (fp32 arithmetic, round-to-nearest-even to bf16; ``lam`` 1 / 0 copy bit for
    bit). Out of place: ``out`` must not alias ``x``. The draws come from ``data/mix.py``; nothing here
    synchronises with the host."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"mix_pairs: x {tuple(x.shape)} {x.dtype} (contiguous NHWC, bf16 or fp32)")
    B, H, W, Cp = x.shape
    if Cp not in (4, 8):
        raise ValueError(f"mix_pairs: {Cp} channels (the padded 4 or 8 of the model input)")
    if tuple(pair.shape) != (B,) or tuple(lam.shape) != (B,) or tuple(boxes.shape) != (B, 4):
        raise ValueError(f"mix_pairs: pair {tuple(pair.shape)}, lam {tuple(lam.shape)}, boxes {tuple(boxes.shape)} "
                         f"for {B} samples")
    pair = pair.to(device=x.device, dtype=torch.int32).contiguous()
    lam = lam.to(device=x.device, dtype=torch.float32).contiguous()
    boxes = boxes.to(device=x.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty_like(x)
    else:
        nb = x.numel() * x.element_size()
        if out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous() or \
                (out.data_ptr() < x.data_ptr() + nb and x.data_ptr() < out.data_ptr() + nb):
            raise ValueError("mix_pairs: out must be a contiguous tensor of x's shape and dtype that does not "
                             "overlap x")
    if x.numel() == 0:
        return out
    _lib.check(_lib.kernels().imk_mix_pairs(x.data_ptr(), out.data_ptr(), pair.data_ptr(), lam.data_ptr(),
                                            boxes.data_ptr(), B, H, W, Cp, 1 if x.dtype == torch.float32 else 0,
                                            _lib.stream_ptr()), "mix pairs")
    return out


def erase_boxes(x: torch.Tensor, boxes: torch.Tensor, keys: Optional[torch.Tensor], mode: str = "const",
                value: float = 0.0) -> torch.Tensor:
    """Random Erasing of a batch **in place**, one HIP kernel (csrc/kernels/erase.hip erase_boxes_kernel): ``x`` NHWC
    [B, H, W, Cp] (bf16 or fp32, Cp 4 or 8, as the normalise kernels leave it), ``boxes`` int32 [B, N, 4] = (top,
    left, h, w), ``keys`` int32 [B, 2] (``pixel`` mode; may be None in ``const`` mode). Inside a box channels 0 .. 2
    become ``value`` (``const``; taken as fp32, round-to-nearest-even to bf16) or the pixel's N(0, 1) noise
    (``pixel``: Philox4x32-10 on (key, pixel) through Box-Muller, ``data/erase.py``), the pad channels zero; nothing
    outside the boxes is touched, and the work follows the boxes' area. Returns ``x``. The draws come from
    ``data/erase.py``; nothing here synchronises with the host."""
    if x.dim() != 4 or not x.is_contiguous() or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"erase_boxes: x {tuple(x.shape)} {x.dtype} (contiguous NHWC, bf16 or fp32)")
    B, H, W, Cp = x.shape
    if Cp not in (4, 8):
        raise ValueError(f"erase_boxes: {Cp} channels (the padded 4 or 8 of the model input)")
    if mode not in ("const", "pixel"):
        raise ValueError(f"erase_boxes: mode {mode!r} (const or pixel)")
    if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[1] < 1 or boxes.shape[2] != 4:
        raise ValueError(f"erase_boxes: boxes {tuple(boxes.shape)}, expected ({B}, N, 4)")
    if mode == "pixel" and (keys is None or tuple(keys.shape) != (B, 2)):
        raise ValueError(f"erase_boxes: pixel mode needs keys of shape ({B}, 2)")
    boxes = boxes.to(device=x.device, dtype=torch.int32).contiguous()
    if keys is not None:
        keys = keys.to(device=x.device, dtype=torch.int32).contiguous()
    if x.numel() == 0:
        return x
    _lib.check(_lib.kernels().imk_erase_boxes(x.data_ptr(), boxes.data_ptr(), _lib.ptr(keys), B, boxes.shape[1], H, W,
                                              Cp, 1 if x.dtype == torch.float32 else 0, 1 if mode == "pixel" else 0,
                                              float(value), _lib.stream_ptr()), "erase boxes")
    return x


def randaug_u8(images: torch.Tensor, params: torch.Tensor, fill: int = 128) -> torch.Tensor:
    """RandAugment of a uint8 NHWC batch [B, H, W, 3] (csrc/kernels/randaug.hip): ``params`` int32 [B, L, 8], rows
    ``(op, a0 .. a6)`` as ``data/randaug.py`` draws them, its L layers applied in order -- per layer one statistics
    launch (the histograms of the images whose op needs the whole image) and one apply launch, from one buffer into
    the other. Bit for bit ``data.randaug.randaug_torch``. ``images`` is never written; the result is a new tensor.
    The stage is blind to the model's dtype, so the ``hip`` and ``hip_f32`` backends share it. The histogram scratch
    and the two buffers come from the caching allocator and go back to it; nothing here synchronises with the
    host."""
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8 or not images.is_contiguous():
        raise ValueError(f"randaug_u8: images {tuple(images.shape)} {images.dtype} (contiguous uint8 [B, H, W, 3])")
    B, H, W, _ = images.shape
    if params.dim() != 3 or params.shape[0] != B or params.shape[1] < 1 or params.shape[2] != 8:
        raise ValueError(f"randaug_u8: params {tuple(params.shape)}, expected ({B}, L, 8)")
    if not (0 <= int(fill) <= 255):
        raise ValueError(f"randaug_u8: fill {fill} (0 .. 255)")
    params = params.to(device=images.device, dtype=torch.int32).contiguous()
    L = params.shape[1]
    src, dst = images, torch.empty_like(images)
    if B == 0 or H == 0 or W == 0:
        return dst
    hist = torch.empty((B, 4, 256), dtype=torch.int32, device=images.device)
    k, st = _lib.kernels(), _lib.stream_ptr()
    for layer in range(L):
        _lib.check(k.imk_randaug_stats(src.data_ptr(), params.data_ptr(), hist.data_ptr(), B, H, W, L, layer, st),
                   "randaugment statistics")
        _lib.check(k.imk_randaug_apply(src.data_ptr(), dst.data_ptr(), params.data_ptr(), hist.data_ptr(), B, H, W,
                                       L, layer, int(fill), st), "randaugment apply")
        if layer + 1 < L:  # the next layer reads what this one wrote, into the other buffer (never into `images`)
            src, dst = dst, (src if src is not images else torch.empty_like(images))
    return dst


def normalize_u8(images: torch.Tensor, out_hw, cpad: int, mean: Sequence[float], std: Sequence[float],
                 crop: Optional[torch.Tensor] = None, flip: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B, Hs, Ws, 3] -> bf16 NHWC [B, H, W, cpad]: (x/255 - mean)/std
    (ToTensor + Normalize of imagenet.py:280-283, on the GPU)."""
    B, Hs, Ws, _ = images.shape
    H, W = out_hw
    if out is None:
        out = torch.empty((B, H, W, cpad), device=images.device, dtype=torch.bfloat16)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _lib.check(_lib.kernels().imk_normalize_u8(images.data_ptr(), out.data_ptr(), _lib.ptr(crop),
                                               _lib.ptr(flip), B, Hs, Ws, H, W, cpad,
                                               C.cast(m, C.c_void_p), C.cast(s, C.c_void_p),
                                               _lib.stream_ptr()), "normalize")
    return out
