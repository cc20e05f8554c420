"""Grouped 3x3 convolution kernels (conv_group.hip; ResNeXt's conv2) against fp64 on the CPU, and one ResNeXt-50
training step against the torch backend.

Operands are small integers (exact_ref.py): every product sum is exact in fp32 while |sum| < 2^24, so the forward and
the dgrad must equal the fp64 ``F.conv2d`` / ``F.conv_transpose2d`` (``groups=``) result rounded once to bf16 bit for
bit, and the weight gradient into a zeroed fp32 slot must equal fp64 exactly (integer atomics do not depend on order).
"""

import copy

import pytest
import torch
import torch.nn.functional as F

from exact_ref import assert_out_exact, ints, out_size, shifted_stats_ref, ternary, ternary_density

pytestmark = pytest.mark.gpu
DEV = "cuda"

WIDTHS = [(64, 4), (128, 8), (64, 16), (64, 32), (128, 32), (128, 64)]  # (C, channels per group)
NHW = [(2, 14, 14), (1, 9, 11), (3, 7, 7)]  # even; no multiple of any tile, odd stride-2 output; the smallest map


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _ref(x, w, dy, stride, groups):
    """fp64 on the CPU: y, dx (both NHWC) and dw [C][3][3][cg] of x [N,H,W,C], w [C,3,3,cg], dy [N,OH,OW,C]."""
    wt = w.double().permute(0, 3, 1, 2)  # [C, cg, 3, 3]
    H, W = x.shape[1], x.shape[2]
    y = F.conv2d(_nchw(x), wt, None, stride, 1, 1, groups)
    opad = (H - ((dy.shape[1] - 1) * stride + 1), W - ((dy.shape[2] - 1) * stride + 1))
    dx = F.conv_transpose2d(_nchw(dy), wt, None, stride, 1, opad, groups)
    dw = torch.nn.grad.conv2d_weight(_nchw(x), wt.shape, _nchw(dy), stride, 1, 1, groups)
    return y.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1)


def _transposed(w, groups):
    """wt[g cg + ci][ky][kx][co in group] = w[g cg + co in group][ky][kx][ci]."""
    Cc, _, _, cg = w.shape
    return w.view(groups, cg, 3, 3, cg).permute(0, 4, 2, 3, 1).reshape(Cc, 3, 3, cg).contiguous()


def _run(x, w, dy, stride, groups):
    from imagent_amd.ops.conv import gconv_dgrad, gconv_fwd, gconv_wgrad
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y = gconv_fwd(xd, wd, stride, groups)
    dx = gconv_dgrad(dyd, _transposed(wd, groups), (x.shape[1], x.shape[2]), stride, groups)
    dw = torch.zeros(w.shape, device=DEV)
    gconv_wgrad(dyd, xd, dw, stride, groups)
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), dw.cpu()


def _check(got, ref):
    y, dx, dw = got
    ry, rdx, rdw = ref
    assert max(ry.abs().max(), rdx.abs().max(), rdw.abs().max()).item() < 2 ** 24  # the exactness precondition
    assert torch.equal(y, ry.to(torch.bfloat16)), (y.double() - ry).abs().max().item()
    assert torch.equal(dx, rdx.to(torch.bfloat16)), (dx.double() - rdx).abs().max().item()
    assert torch.equal(dw.double(), rdw), (dw.double() - rdw).abs().max().item()


@pytest.mark.parametrize("nhw", NHW, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,cg", WIDTHS)
def test_gconv_exact(C, cg, stride, nhw):
    N, H, W = nhw
    x = ints((N, H, W, C), -4, 4, 1)
    w = ints((C, 3, 3, cg), -2, 2, 2)
    dy = ints((N, out_size(H, 3, stride, 1), out_size(W, 3, stride, 1), C), -4, 4, 3)
    _check(_run(x, w, dy, stride, C // cg), _ref(x, w, dy, stride, C // cg))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cg,co,ci", [(4, 5, 2), (4, 63, 0), (8, 17, 7), (8, 8, 3)])
def test_gconv_one_hot_weight_stays_in_its_group(cg, co, ci, stride):
    """One nonzero weight: inside a 16-channel MFMA tile that spans 16 / cg groups, nothing may leak into the other
    groups' channels (forward: only output channel co; dgrad: only input channel ci of co's group; wgrad: one row)."""
    C, (N, H, W) = 64, NHW[0]
    g = co // cg
    x = ints((N, H, W, C), -4, 4, 4)
    dy = ints((N, out_size(H, 3, stride, 1), out_size(W, 3, stride, 1), C), -4, 4, 5)
    w = torch.zeros(C, 3, 3, cg, dtype=torch.bfloat16)
    w[co, 0, 2, ci] = 3
    got = _run(x, w, dy, stride, C // cg)
    _check(got, _ref(x, w, dy, stride, C // cg))
    keep = torch.zeros(C, dtype=torch.bool)
    keep[co] = True
    assert got[0][..., co].abs().sum() > 0 and not got[0][..., ~keep].any()
    keep[co], keep[g * cg + ci] = False, True
    assert got[1][..., g * cg + ci].abs().sum() > 0 and not got[1][..., ~keep].any()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,cg", WIDTHS)
def test_gconv_epilogues(C, cg, stride):
    """Training epilogue: the BatchNorm slab of one launch, folded by stats_finalize, against the fp64 mean and biased
    variance of the stored values around an integer shift. Eval epilogue: affine (power-of-two scale, integer shift) +
    ReLU. Ternary operands keep every output an integer of magnitude <= 256: rounded and unrounded values agree.

    Tolerance (M values per channel): the fp32 accumulation bound M 2^-24 sum|v| on the sum and M 2^-24 relative on
    the sum of squares; as (mean, variance) = (shift + S1 / M, S2 / M - (S1 / M)^2) that is 2^-24 sum|v| on the mean
    and 2^-24 S2 + 2 |S1 / M| 2^-24 sum|d| on the variance."""
    from imagent_amd.models.resnet import BNWork
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import stats_finalize
    from imagent_amd.ops.conv import gconv_fwd
    N, H, W = NHW[0]
    d = ternary_density(9 * cg)
    x, w = ternary((N, H, W, C), d, 6), ternary((C, 3, 3, cg), d, 7)
    ref = F.conv2d(_nchw(x), w.double().permute(0, 3, 1, 2), None, stride, 1, 1, C // cg).permute(0, 2, 3, 1)
    assert_out_exact(ref)
    M = ref.numel() // C
    work = BNWork(torch.zeros(_lib.STAT_SLOTS, 2, C, device=DEV), torch.zeros(2, C, device=DEV),
                  torch.zeros(2, C, device=DEV), None)
    shift = ints((C,), -3, 3, 8, dtype=torch.float32)
    work.save[0].copy_(shift)
    y = gconv_fwd(x.to(DEV), w.to(DEV), stride, C // cg, stats=work)
    stats_finalize(work, M)
    sc = torch.tensor([0.5, 2.0, -1.0, 4.0]).repeat(C // 4)
    sh = ints((C,), -5, 5, 9, dtype=torch.float32)
    ye = gconv_fwd(x.to(DEV), w.to(DEV), stride, C // cg, affine=torch.stack([sc, sh]).to(DEV), relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref)
    assert torch.equal(ye.cpu().double(), (ref * sc.double() + sh.double()).clamp_min(0).to(torch.bfloat16).double())
    S = shifted_stats_ref(ref, shift)
    dabs = (ref.reshape(-1, C) - shift.double()).abs().sum(0)
    mean, var = shift.double() + S[0] / M, S[1] / M - (S[0] / M) ** 2
    got = work.stats.cpu().double()
    print("mean err", (got[0] - mean).abs().max().item(), "var err", (got[1] - var).abs().max().item())
    assert ((got[0] - mean).abs() <= 2.0 ** -24 * ref.reshape(-1, C).abs().sum(0)).all()
    assert ((got[1] - var).abs() <= 2.0 ** -24 * (S[1] + 2 * (S[0] / M).abs() * dabs)).all()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _grads(model, x, lab, autocast=False):
    for p in model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x)
    F.cross_entropy(logits.float(), lab).backward()
    return logits.float(), {n: p.grad.float().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-op"])
def test_resnext50_step_matches_torch(fused):
    """One training step of resnext50_32x4d (16 classes, 64x64, batch 4) and the eval logits against the torch backend
    from the same bf16-rounded weights -- the comparison and tolerances of test_model_gpu.py's
    test_hip_vs_torch_forward_backward: per tensor, the relative L2 distance to the fp32 oracle is at most 2x the
    distance of PyTorch's own bf16 autocast, or 5e-2 (logits, gradients, eval logits) / 2e-2 (running statistics)."""
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops.misc import normalize_u8
    torch.manual_seed(0)
    ref = resnet.build("resnext50_32x4d", num_classes=16).to(DEV)
    model = copy.deepcopy(ref)
    st = bind_native(model, DEV)
    st.fused_blocks = fused
    with torch.no_grad():
        for p_ref, p in zip(ref.parameters(), model.parameters()):
            p_ref.copy_(p.to(torch.bfloat16).float())
    ref_bf = copy.deepcopy(ref)
    B, H = 4, 64
    low = torch.rand(B, 3, 8, 8, device=DEV)
    img = (F.interpolate(low, size=(H, H), mode="bicubic", align_corners=False).clamp(0, 1) * 255)
    img = img.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    lab = torch.randint(0, 16, (B,), device=DEV)
    x = normalize_u8(img, (H, H), 4, (0.5,) * 3, (0.5,) * 3)
    xr = x[..., :3].float().permute(0, 3, 1, 2).contiguous()
    for m in (model, ref, ref_bf):
        m.train()
    st.arena.zero_grad()
    logits = model(x)
    F.cross_entropy(logits, lab).backward()
    l32, g32 = _grads(ref, xr, lab)
    lbf, gbf = _grads(ref_bf, xr, lab, autocast=True)
    assert _rel(logits, l32) < max(5e-2, 2.0 * _rel(lbf, l32))
    bad = [(n, _rel(p.grad, g32[n]), _rel(gbf[n], g32[n])) for n, p in model.named_parameters()
           if _rel(p.grad, g32[n]) > max(0.05, 2.0 * _rel(gbf[n], g32[n]))]
    assert not bad, bad
    for (n1, b1), (_, b2), (_, b3) in zip(model.named_buffers(), ref.named_buffers(), ref_bf.named_buffers()):
        if "num_batches_tracked" not in n1:
            assert _rel(b1, b2) < max(2e-2, 2.0 * _rel(b3, b2)), n1
    for m in (model, ref, ref_bf):
        m.eval()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ebf = _rel(ref_bf(xr).float(), ref(xr))
        assert _rel(model(x), ref(xr)) < max(5e-2, 2.0 * ebf)
