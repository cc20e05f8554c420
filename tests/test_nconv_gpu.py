"""Narrow 3x3 convolution kernels (conv_narrow.hip; the ResNet-D deep stem) against fp64 on the CPU.

Operands are small integers (exact_ref.py): every product sum is exact in fp32 while |sum| < 2^24, so the forward and
the dgrad must equal the fp64 result rounded once to bf16 bit for bit, and the weight gradient (fp32 partials folded in
a fixed order) must equal fp64 exactly.

Maps: 5x7 (odd, smaller than one band), 16x16 (whole bands), 33x18 (crosses the 8-row band boundary with a remainder).
The kernels' band is 8 output rows x 32 output columns, so 33x18 has one width tile: 17x67 is the smallest map whose
output crosses both a band and a width-tile boundary with a remainder at stride 1 (17x67 -> 32 + 32 + 3 columns) and at
stride 2 (9x34 -> 32 + 2 columns).
"""

import pytest
import torch
import torch.nn.functional as F

from exact_ref import assert_out_exact, ints, out_size, shifted_stats_ref, ternary, ternary_density

pytestmark = pytest.mark.gpu
DEV = "cuda"

CONVS = [(4, 32, 2), (32, 32, 1), (32, 64, 1)]  # (Ci, Co, stride): conv A, B, C of the stem
MAPS = [(5, 7), (16, 16), (33, 18), (17, 67)]
N = 2
_ids = dict(ids=lambda s: "x".join(map(str, s)))


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _ref(x, w, dy, stride):
    """fp64 on the CPU: y, dx (NHWC) and dw [Co][3][3][Ci] of x [N,H,W,Ci], w [Co,3,3,Ci], dy [N,OH,OW,Co]."""
    wt = w.double().permute(0, 3, 1, 2)
    H, W = x.shape[1], x.shape[2]
    y = F.conv2d(_nchw(x), wt, None, stride, 1)
    opad = (H - ((dy.shape[1] - 1) * stride + 1), W - ((dy.shape[2] - 1) * stride + 1))
    dx = F.conv_transpose2d(_nchw(dy), wt, None, stride, 1, opad)
    dw = torch.nn.grad.conv2d_weight(_nchw(x), wt.shape, _nchw(dy), stride, 1)
    return y.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1)


def _run(x, w, dy, stride):
    """(y, dx or None, dw) of the narrow kernels; the image conv (stride 2) has no input gradient."""
    from imagent_amd.ops.conv import nconv_dgrad, nconv_fwd, nconv_wgrad
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y = nconv_fwd(xd, wd, stride)
    dx = nconv_dgrad(dyd, wd.permute(3, 1, 2, 0).contiguous()) if stride == 1 else None
    dw = torch.zeros(w.shape, device=DEV)
    nconv_wgrad(dyd, xd, dw, stride)
    torch.cuda.synchronize()
    return y.cpu(), None if dx is None else dx.cpu(), dw.cpu()


def _check(got, ref):
    assert max(r.abs().max() for r in ref).item() < 2 ** 24  # the exactness precondition
    assert torch.equal(got[0], ref[0].to(torch.bfloat16)), (got[0].double() - ref[0]).abs().max().item()
    if got[1] is not None:
        assert torch.equal(got[1], ref[1].to(torch.bfloat16)), (got[1].double() - ref[1]).abs().max().item()
    assert torch.equal(got[2].double(), ref[2]), (got[2].double() - ref[2]).abs().max().item()


def _dy_shape(H, W, Co, stride):
    return (N, out_size(H, 3, stride, 1), out_size(W, 3, stride, 1), Co)


@pytest.mark.parametrize("hw", MAPS, **_ids)
@pytest.mark.parametrize("conv", CONVS, **_ids)
def test_nconv_exact(conv, hw):
    (Ci, Co, stride), (H, W) = conv, hw
    x, w = ints((N, H, W, Ci), -4, 4, 1), ints((Co, 3, 3, Ci), -2, 2, 2)
    dy = ints(_dy_shape(H, W, Co, stride), -4, 4, 3)
    _check(_run(x, w, dy, stride), _ref(x, w, dy, stride))


def test_nconv_image_weights_with_three_channels():
    """The model's conv A: a [32,3,3,3] shadow and gradient slot against the 4-channel image (channel 3 ignored)."""
    from imagent_amd.ops.conv import nconv_fwd, nconv_wgrad
    H, W = MAPS[2]
    x, w = ints((N, H, W, 4), -4, 4, 1), ints((32, 3, 3, 3), -2, 2, 2)
    dy = ints(_dy_shape(H, W, 32, 2), -4, 4, 3)
    ry, _, rdw = _ref(x[..., :3], w, dy, 2)
    dw = torch.zeros(w.shape, device=DEV)  # [Co][3][3][3] in memory, passed as the parameter's [Co,3,3,3] grad view
    nconv_wgrad(dy.to(DEV), x.to(DEV), dw.permute(0, 3, 1, 2), 2)
    assert torch.equal(nconv_fwd(x.to(DEV), w.to(DEV), 2).cpu(), ry.to(torch.bfloat16))
    assert torch.equal(dw.cpu().double(), rdw)


@pytest.mark.parametrize("conv", CONVS, **_ids)
def test_nconv_wgrad_is_bitwise_repeatable(conv):
    """Random bf16 operands (no exact sum): the fixed-order fold gives the same bits twice, and accumulates."""
    from imagent_amd.ops.conv import nconv_wgrad
    (Ci, Co, stride), (H, W) = conv, MAPS[3]
    g = torch.Generator().manual_seed(4)
    x = torch.randn((N, H, W, Ci), generator=g).to(torch.bfloat16).to(DEV)
    dy = torch.randn(_dy_shape(H, W, Co, stride), generator=g).to(torch.bfloat16).to(DEV)
    a, b = torch.zeros(Co, 3, 3, Ci, device=DEV), torch.zeros(Co, 3, 3, Ci, device=DEV)
    nconv_wgrad(dy, x, a, stride)
    nconv_wgrad(dy, x, b, stride)
    assert torch.equal(a, b) and a.abs().sum() > 0
    nconv_wgrad(dy, x, b, stride)
    assert torch.equal(b, a + a)


@pytest.mark.parametrize("end", [0, -1], ids=["first", "last"])
@pytest.mark.parametrize("tap", [(0, 0), (0, 2), (1, 1), (2, 0), (2, 2)], **_ids)
@pytest.mark.parametrize("conv", CONVS, **_ids)
def test_nconv_one_hot(conv, tap, end):
    """One nonzero weight (co, tap, ci) moves one input pixel to one output pixel and channel (mirrored taps and
    fragment lanes); the dgrad moves one dy pixel back, the wgrad has one nonzero entry."""
    (Ci, Co, stride), (H, W), (ky, kx) = conv, MAPS[0], tap
    ci, co = (Ci + end) % Ci, (Co + end) % Co
    w = torch.zeros(Co, 3, 3, Ci, dtype=torch.bfloat16)
    w[co, ky, kx, ci] = 3
    oy, ox = 1, 2  # an interior output pixel: input (oy s - 1 + ky, ox s - 1 + kx) is inside 5x7 for both strides
    x = torch.zeros(N, H, W, Ci, dtype=torch.bfloat16)
    x[1, oy * stride - 1 + ky, ox * stride - 1 + kx, ci] = 2
    dy = torch.zeros(_dy_shape(H, W, Co, stride), dtype=torch.bfloat16)
    dy[1, oy, ox, co] = 5
    got, ref = _run(x, w, dy, stride), _ref(x, w, dy, stride)
    _check(got, ref)
    assert got[0][1, oy, ox, co] == 6 and got[0].count_nonzero() == 1
    assert got[2][co, ky, kx, ci] == 10 and got[2].count_nonzero() == 1
    if got[1] is not None:
        assert got[1][1, oy - 1 + ky, ox - 1 + kx, ci] == 15 and got[1].count_nonzero() == 1


@pytest.mark.parametrize("conv", CONVS, **_ids)
def test_nconv_epilogues(conv):
    """Training epilogue: the BatchNorm slab of one launch, folded by stats_finalize, against the fp64 mean and biased
    variance of the STORED values around an integer shift; eval epilogue: affine (power-of-two scale, integer shift) +
    ReLU. Ternary operands keep every output an integer of magnitude <= 256: rounded and unrounded values agree.
    Tolerance as test_gconv_epilogues (M values per channel, fp32 accumulation): 2^-24 sum|v| on the mean and
    2^-24 S2 + 2 |S1 / M| 2^-24 sum|d| on the variance."""
    from imagent_amd.models.resnet import BNWork
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import stats_finalize
    from imagent_amd.ops.conv import nconv_fwd
    (Ci, Co, stride), (H, W) = conv, MAPS[3]
    d = ternary_density(9 * Ci)
    x, w = ternary((N, H, W, Ci), d, 6), ternary((Co, 3, 3, Ci), d, 7)
    ref = F.conv2d(_nchw(x), w.double().permute(0, 3, 1, 2), None, stride, 1).permute(0, 2, 3, 1)
    assert_out_exact(ref)
    M = ref.numel() // Co
    work = BNWork(torch.zeros(_lib.STAT_SLOTS, 2, Co, device=DEV), torch.zeros(2, Co, device=DEV),
                  torch.zeros(2, Co, device=DEV), None)
    shift = ints((Co,), -3, 3, 8, dtype=torch.float32)
    work.save[0].copy_(shift)
    y = nconv_fwd(x.to(DEV), w.to(DEV), stride, stats=work)
    stats_finalize(work, M)
    sc = torch.tensor([0.5, 2.0, -1.0, 4.0]).repeat(Co // 4)
    sh = ints((Co,), -5, 5, 9, dtype=torch.float32)
    ye = nconv_fwd(x.to(DEV), w.to(DEV), stride, affine=torch.stack([sc, sh]).to(DEV), relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref)
    assert torch.equal(ye.cpu().double(), (ref * sc.double() + sh.double()).clamp_min(0).to(torch.bfloat16).double())
    S = shifted_stats_ref(ref, shift)
    dabs = (ref.reshape(-1, Co) - shift.double()).abs().sum(0)
    mean, var = shift.double() + S[0] / M, S[1] / M - (S[0] / M) ** 2
    got = work.stats.cpu().double()
    print("mean err", (got[0] - mean).abs().max().item(), "var err", (got[1] - var).abs().max().item())
    assert ((got[0] - mean).abs() <= 2.0 ** -24 * ref.reshape(-1, Co).abs().sum(0)).all()
    assert ((got[1] - var).abs() <= 2.0 ** -24 * (S[1] + 2 * (S[0] / M).abs() * dabs)).all()
