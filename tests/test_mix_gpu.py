"""Mixup / CutMix on the GPU (--mixup / --cutmix): ``ops.misc.mix_pairs`` (csrc/kernels/misc.hip mix_pairs_kernel)
against its definition, past 2^31 bytes, the two-label loss kernels against ``F.cross_entropy`` with soft targets in
float64, the two backends of ``BatchMixer`` on identical draws, and three trainer steps on both kernel paths.

mix_pairs: a sample with a non-empty box, and a blend with lam 0 or 1, is a select and is compared bit for bit. Every
other blended element obeys ``|out - r| <= 2^-8 |r| + 2^-22 (|lam a| + |(1 - lam) b|)`` with ``r`` formed in float64
from the fp32 ``lam`` and the stored inputs: bf16's half ulp, and the three fp32 roundings (two products, one sum; the
fp32 ``1 - lam`` is a fourth, at most 2^-25). fp32 outputs: the second term alone. Shapes: the 5 x 7 and 16 x 16
samples fit one chunk of the kernel (5 x 7 x 4 bf16 samples are 280 bytes, no multiple of 16: the 8-byte vectors);
33 x 70 and 33 x 71 span two to five chunks with a tail, the latter on the 8-byte path in bf16."""

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 5, 7, 4), (3, 5, 7, 8), (4, 16, 16, 4), (3, 33, 70, 4), (3, 33, 71, 4)]


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _cases(H, W):
    """(lam, box) per sample: the blends, then boxes (their lam is ignored by the kernel, as a CutMix sample's lam
    only enters the loss)."""
    return [(0.0, (0, 0, 0, 0)), (1.0, (0, 0, 0, 0)), (0.5, (0, 0, 0, 0)), (0.3, (0, 0, 0, 0)),
            (0.7, (0, 0, 0, 5)),                 # empty: h = 0
            (0.9, (2, 3, 1, 1)),                 # one pixel, at an odd column
            (0.9, (1, 1, 3, 2)),                 # starts at an odd column: straddles a 16-byte vector of two pixels
            (0.9, (1, 2, 2, 3)),                 # ends at an odd column
            (0.9, (0, 2, 2, 3)),                 # touches the top
            (0.9, (H - 2, 1, 2, 3)),             # the bottom
            (0.9, (1, 0, 3, 2)),                 # the left
            (0.9, (1, W - 2, 3, 2)),             # the right: the vector after the box's last holds the next row's start
            (0.9, (0, W - 1, H, 1)),             # the last column, every row
            (0.9, (0, 0, H, W))]                 # the whole image


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _reference(x, pair, lam, boxes):
    """x: CPU NHWC tensor. -> (r float64 [B,H,W,C], exact bool [B], bound float64 [B,H,W,C])"""
    B, H, W, _ = x.shape
    xd = x.double().numpy()
    r, bound, exact = np.empty_like(xd), np.zeros_like(xd), np.zeros(B, dtype=bool)
    for b in range(B):
        a, p = xd[b], xd[int(pair[b])]
        t, l, h, w = (int(v) for v in boxes[b])
        lm = float(lam[b])  # the fp32 value, exactly
        if h > 0 and w > 0:
            r[b] = a
            r[b, t:t + h, l:l + w] = p[t:t + h, l:l + w]
            exact[b] = True
        elif lm in (0.0, 1.0):
            r[b] = a if lm == 1.0 else p
            exact[b] = True
        else:
            r[b] = lm * a + (1.0 - lm) * p
            bound[b] = 2.0 ** -22 * (np.abs(lm * a) + np.abs((1.0 - lm) * p))
            if x.dtype == torch.bfloat16:
                bound[b] += 2.0 ** -8 * np.abs(r[b])
    return r, exact, bound


def _check(out, x, pair, lam, boxes):
    r, exact, bound = _reference(x.cpu(), pair.cpu(), lam.cpu(), boxes.cpu())
    o = out.cpu()
    rt = torch.from_numpy(r).to(x.dtype)  # exact for the select samples: r holds stored values
    for b in range(x.shape[0]):
        if exact[b]:
            assert torch.equal(_bits(o[b]), _bits(rt[b])), f"sample {b}: lam {float(lam[b])} box {boxes[b].tolist()}"
        else:
            err = np.abs(o[b].double().numpy() - r[b])
            worst = (err - bound[b]).max()
            assert (err <= bound[b]).all(), f"sample {b}: lam {float(lam[b])}, {worst:.3e} over the bound"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_pairs_matches_definition(shape, dtype):
    from imagent_amd.ops.misc import mix_pairs
    B, H, W, Cp = shape
    g = torch.Generator().manual_seed(B * 1000 + H * W + Cp)
    x = torch.randn(shape, generator=g)
    x[..., 3:] = 0  # padding channels
    x[0, 0, 0, 0], x[1, 0, 1, 1] = -0.0, 0.0  # a copy keeps the sign of zero
    x = x.to(dtype).to(DEV)
    cases = _cases(H, W)
    n = len(cases)
    pair = torch.tensor([(i + 1) % B for i in range(B)], dtype=torch.int32)
    pair[1] = 1  # a fixed point
    for launch in range(n):  # sample i takes case launch + i: every case meets every sample, the fixed point too
        sel = [cases[(launch + i) % n] for i in range(B)]
        lam = torch.tensor([c[0] for c in sel], dtype=torch.float32)
        boxes = torch.tensor([c[1] for c in sel], dtype=torch.int32)
        out = mix_pairs(x, pair.to(DEV), lam.to(DEV), boxes.to(DEV))
        assert out.shape == x.shape and out.dtype == x.dtype and out.data_ptr() != x.data_ptr()
        _check(out, x, pair, lam, boxes)
        assert not out[..., 3:].any(), "padding channels"


def test_mix_pairs_arguments():
    from imagent_amd.ops.misc import mix_pairs
    x = torch.zeros((2, 4, 4, 4), device=DEV, dtype=torch.bfloat16)
    pair = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    lam = torch.ones(2, device=DEV)
    boxes = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="overlap"):
        mix_pairs(x, pair, lam, boxes, out=x)
    with pytest.raises(ValueError, match="channels"):
        mix_pairs(torch.zeros((2, 4, 4, 3), device=DEV, dtype=torch.bfloat16), pair, lam, boxes)
    with pytest.raises(ValueError, match="samples"):
        mix_pairs(x, pair[:1], lam, boxes)
    # a partner outside the batch is clamped into it, not read out of bounds
    x = torch.randn((2, 4, 4, 4), device=DEV).to(torch.bfloat16)
    out = mix_pairs(x, torch.tensor([7, -3], dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV), boxes)
    assert torch.equal(out[0], x[1]) and torch.equal(out[1], x[0])


def test_past_2gb():
    """Three 9500 x 9500 x 4 bf16 samples (2.17 GB): the last sample, partnered with the first, as a blend and as a
    box, equals the same call on the two-sample tensor that holds just those two."""
    from imagent_amd.ops.misc import mix_pairs
    H = W = 9500
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.empty((3, H, W, 4), device=DEV, dtype=torch.bfloat16)
    for i in range(3):
        x[i] = torch.randn((H, W, 4), device=DEV, generator=g, dtype=torch.float32)
    assert x.numel() * 2 > 2 ** 31
    xs = torch.stack([x[2], x[0]])
    pair, ps = torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV), torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    box = [1001, 4001, 5000, 3333]
    for lam, bx in ((0.3, [0, 0, 0, 0]), (0.5, box)):
        l3, b3 = torch.full((3,), lam, device=DEV), torch.tensor([bx] * 3, dtype=torch.int32, device=DEV)
        big = mix_pairs(x, pair, l3, b3)[2]
        small = mix_pairs(xs, ps, l3[:2].contiguous(), b3[:2].contiguous())[0]
        assert torch.equal(_bits(big), _bits(small)), f"lam {lam} box {bx}"
        t, l, h, w = box
        if bx[2]:  # and it is the select: a corner inside, a corner outside
            assert torch.equal(big[t:t + h, l:l + w], x[0, t:t + h, l:l + w]) and torch.equal(big[:t], x[2, :t])
            assert torch.equal(big[t + h:], x[2, t + h:]) and torch.equal(big[:, :l], x[2, :, :l])
        del big, small


# ------------------------------------------------------------------ the two-label loss
@functools.lru_cache(maxsize=None)
def _loss_case(B, NC):
    g = torch.Generator().manual_seed(B * 7 + NC)
    z = torch.randn((B, NC), generator=g) * 3
    ya, yb = torch.randint(0, NC, (B,), generator=g), torch.randint(0, NC, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1], lam[2], lam[3] = 1.0, 0.0, 0.5, 0.25
    ya[0], yb[1], ya[2], yb[3] = z[0].argmax(), z[1].argmax(), z[2].argmax(), z[3].topk(3).indices[2]  # forced hits
    ya[4] = yb[4]  # both labels the same class
    return z.to(DEV), ya.to(DEV), yb.to(DEV), lam.to(DEV)


def _loss_reference(z, ya, yb, lam, eps):
    NC = z.shape[1]
    zr = z.double().requires_grad_(True)
    l = lam.double().unsqueeze(1)
    soft = l * F.one_hot(ya, NC).double() + (1 - l) * F.one_hot(yb, NC).double()
    ref = F.cross_entropy(zr, soft, label_smoothing=eps)
    ref.backward()
    return ref.item(), zr.grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,NC", [(5, 10), (5, 257), (64, 1000)])
def test_pair_loss_matches_soft_target_cross_entropy(B, NC, eps):
    from imagent_amd.ops import _lib
    from imagent_amd.ops.misc import XentPairFn
    z, ya, yb, lam = _loss_case(B, NC)
    ref, gref = _loss_reference(z, ya, yb, lam, eps)
    met = torch.zeros(4, device=DEV)
    za = z.clone().requires_grad_(True)
    loss = XentPairFn.apply(za, ya, yb, lam, met, eps)
    loss.backward()
    print(f"loss {loss.item():.6f} ref {ref:.6f}; fp32 dz rel {rel(za.grad, gref):.2e}")
    assert abs(loss.item() - ref) < 1e-4
    assert za.grad.dtype == torch.float32 and rel(za.grad, gref) < 1e-4  # the fp32 path's gradient kernel
    # the bf16 path's gradient kernel (bf16 dz, as imk_xent_bwd)
    lse = torch.logsumexp(z, 1).float().contiguous()
    one = torch.ones((), device=DEV)
    dzb = torch.empty((B, NC), device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.kernels().imk_xent_pair_bwd(z.data_ptr(), ya.data_ptr(), yb.data_ptr(), lam.data_ptr(),
                                                lse.data_ptr(), one.data_ptr(), dzb.data_ptr(), B, NC, eps,
                                                _lib.stream_ptr()), "xent pair bwd")
    print(f"bf16 dz rel {rel(dzb, gref):.2e}")
    assert rel(dzb, gref) < 1e-2
    # metrics: top-1 / top-5 against the dominant label, rows, loss sum
    dom = torch.where(lam >= 0.5, ya, yb)
    top5 = z.topk(5, 1).indices
    assert met[1].item() == (top5[:, 0] == dom).sum().item() >= 2
    assert met[2].item() == (top5 == dom[:, None]).any(1).sum().item() >= 3
    assert met[3].item() == B
    assert abs(met[0].item() - ref * B) < 1e-2


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,NC", [(5, 10), (5, 257), (64, 1000)])
def test_pair_loss_with_lam_one_is_the_one_label_loss(B, NC, eps):
    """lam = 1 everywhere: lse and dz bit-identical to XentFn / XentF32Fn on ya, whatever yb holds."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.f32 import XentF32Fn
    from imagent_amd.ops.misc import XentFn, XentPairFn
    z, ya, yb, _ = _loss_case(B, NC)
    lam = torch.ones(B, device=DEV)
    outs = []
    for fn, args in ((XentPairFn, (ya, yb, lam)), (XentFn, (ya,)), (XentF32Fn, (ya,))):
        met = torch.zeros(4, device=DEV)
        za = z.clone().requires_grad_(True)
        loss = fn.apply(za, *args, met, eps)
        lse = loss.grad_fn.saved_tensors[-1].clone()
        loss.backward()
        outs.append((loss.item(), lse, za.grad.clone(), met))
    for other in outs[1:]:
        assert torch.equal(_bits(outs[0][1]), _bits(other[1])), "lse"
        assert torch.equal(_bits(outs[0][2]), _bits(other[2])), "dz"
        # (the mean loss is summed with atomics, in any order: the loss tolerance, not bits)
        assert abs(outs[0][0] - other[0]) < 1e-4 and torch.equal(outs[0][3][1:], other[3][1:])
    # and the bf16 gradient kernels
    k, lse, one = _lib.kernels(), outs[0][1], torch.ones((), device=DEV)
    d1 = torch.empty((B, NC), device=DEV, dtype=torch.bfloat16)
    d2 = torch.empty_like(d1)
    _lib.check(k.imk_xent_pair_bwd(z.data_ptr(), ya.data_ptr(), yb.data_ptr(), lam.data_ptr(), lse.data_ptr(),
                                   one.data_ptr(), d1.data_ptr(), B, NC, eps, _lib.stream_ptr()), "xent pair bwd")
    _lib.check(k.imk_xent_bwd(z.data_ptr(), ya.data_ptr(), lse.data_ptr(), one.data_ptr(), d2.data_ptr(), B, NC, eps,
                              _lib.stream_ptr()), "xent bwd")
    assert torch.equal(_bits(d1), _bits(d2))


# ------------------------------------------------------------------ the two backends of BatchMixer
@pytest.mark.parametrize("backend,dtype", [("hip", torch.bfloat16), ("hip_f32", torch.float32)])
def test_backends_agree(backend, dtype):
    from imagent_amd.data.mix import BatchMixer
    B, H, W, Cp = 6, 12, 10, 4
    g = torch.Generator().manual_seed(3)
    xc = torch.randn((B, 3, H, W), generator=g).to(dtype)          # NCHW, the torch backend's layout
    xn = torch.zeros((B, H, W, Cp), dtype=dtype)
    xn[..., :3] = xc.permute(0, 2, 3, 1)
    y = torch.arange(B)
    pair = torch.tensor([3, 2, 1, 0, 4, 0], dtype=torch.int32)
    lam = torch.tensor([0.3, 0.85, 1.0, 0.0, 0.5, 0.6], dtype=torch.float32)
    boxes = torch.tensor([[0, 0, 0, 0], [2, 3, 5, 4], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 12, 3]],
                         dtype=torch.int32)
    params = (pair.to(DEV), lam.to(DEV), boxes.to(DEV))
    oh, (ya, yb, lh) = BatchMixer(backend, 0.2, 1.0)(xn.to(DEV), y.to(DEV), params=params)
    ot, (ta, tb, lt) = BatchMixer("torch", 0.2, 1.0)(xc.to(DEV), y.to(DEV), params=params)
    assert torch.equal(ya, ta) and torch.equal(yb, tb) and torch.equal(lh, lt) and torch.equal(yb.cpu(), y[pair.long()])
    _check(oh, xn, pair, lam, boxes)                                 # the kernel against the definition
    r, exact, bound = _reference(xn, pair, lam, boxes)
    tn = ot.permute(0, 2, 3, 1).cpu().double().numpy()               # the torch backend against it, same bound
    assert (np.abs(tn - r[..., :3]) <= bound[..., :3]).all()
    assert not oh[..., 3:].any()
    # own draws: two mixers at the same epoch give identical draws and outputs
    outs = []
    for _ in range(2):
        m = BatchMixer(backend, 0.2, 1.0, seed=11, rank=1)
        m.set_epoch(4)
        d = m.draw(B, H, W, DEV)
        m.set_epoch(4)
        outs.append((d, m(xn.to(DEV), y.to(DEV))))
    (d0, (x0, t0)), (d1, (x1, t1)) = outs
    assert all(torch.equal(a, b) for a, b in zip(d0, d1)) and all(t.is_cuda for t in d0)
    assert torch.equal(_bits(x0), _bits(x1)) and all(torch.equal(a, b) for a, b in zip(t0, t1))
    assert torch.equal(t0[2], d0[1])  # the call drew what draw() drew after the same set_epoch


# ------------------------------------------------------------------ trainer
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_trainer_three_steps(tmp_path, monkeypatch, dtype):
    """(100 classes: the fp32 kernel path takes class counts that are a multiple of 4.)"""
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    args = ["--arch", "resnet18", "--image-size", "64", "--data", "synthetic", "--synthetic-train-size", "64",
            "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "100", "--quiet-banner", "--tb-dir", "",
            "--kernels", "hip", "--launcher", "single", "--mixup", "0.2", "--cutmix", "1.0", "--max-steps", "3",
            "--dtype", dtype, "--log-interval", "0"]
    tr = Trainer(build_parser().parse_args(args))
    try:
        assert tr.mixer is not None and tr.mixer.backend == ("hip" if dtype == "bf16" else "hip_f32")
        seen = []
        loss_fn = tr.step.loss
        monkeypatch.setattr(tr.step, "loss", lambda logits, y: (seen.append(type(y)), loss_fn(logits, y))[1])
        train, val = tr._loaders(0)
        loss, t1, t5, _ = tr.train_epoch(0, train)
        assert math.isfinite(loss) and loss > 0, loss
        assert tr.metrics.buf[3].item() == 24 and tr.last_train_images == 24
        assert seen == [tuple] * 3
        del seen[:]
        vloss, v1, v5, _ = tr.validate(val)   # the plain one-label path
        assert seen == [torch.Tensor] * 2 and math.isfinite(vloss) and tr.metrics.buf[3].item() == 16
    finally:
        tr.close()
