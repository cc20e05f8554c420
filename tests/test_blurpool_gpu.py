"""The anti-aliased archs' BlurPool (blurpool.hip) against its definition in fp64: ``F.pad`` reflect 1 + the depthwise
[1,2,1]^T [1,2,1] / 16 conv at stride 2, and that conv's autograd for the backward. Inputs and upstream gradients are
integers in [-4, 4]: every output and input gradient is a multiple of 1/16 below 8, exact in fp32 and bf16, so both
directions must agree bit for bit. The fused form pools relu(sc x + sh) with sc in {1/2, 1, 2, -1, -2} and integer sh
in [-2, 2]: exact with or without FMA, the output still exact in bf16. Shapes: the 2x2 minimum (both reflections land
on the same pixels), odd and even extents in each axis, 72 channels (no multiple of 64), output maps of 7 and 17 rows
(more than one 4-row band, a short last band) and enough chunks for more than one block."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 2), (3, 5), (7, 6), (8, 9), (14, 14), (33, 31)]


def _definition(x):  # NCHW
    C = x.shape[1]
    k = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype)
    filt = (k[:, None] * k[None, :] / 16).view(1, 1, 3, 3)
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), filt.expand(C, 1, 3, 3), stride=2, groups=C)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [8, 72, 256])
def test_blurpool_matches_definition(C, hw):
    from imagent_amd.ops.misc import BlurPoolFn
    (H, W), N = hw, 2
    g = torch.Generator().manual_seed(C + 100 * H + W)
    x = _ints((N, C, H, W), -4, 4, g).requires_grad_()
    ref = _definition(x)
    dy = _ints(ref.shape, -4, 4, g)
    ref.backward(dy)
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV).requires_grad_()
    y = BlurPoolFn.apply(xd)
    y.backward(dy.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV))
    assert y.shape == (N, (H + 1) // 2, (W + 1) // 2, C)
    assert torch.equal(y.detach().cpu().double(), ref.detach().permute(0, 2, 3, 1))
    assert torch.equal(xd.grad.cpu().double(), x.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [8, 72, 256])
def test_blurpool_fused_bn_relu_matches_definition(C, hw):
    from imagent_amd.ops.misc import blurpool_fwd
    (H, W), N = hw, 2
    g = torch.Generator().manual_seed(7 + C + 100 * H + W)
    x = _ints((N, C, H, W), -4, 4, g)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0, -2.0], dtype=torch.double)[torch.randint(0, 5, (C,), generator=g)]
    sh = _ints((C,), -2, 2, g)
    ref = _definition(F.relu(sc.view(1, C, 1, 1) * x + sh.view(1, C, 1, 1)))
    ss = torch.stack([sc, sh]).float().contiguous().to(DEV)
    y = blurpool_fwd(x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV), ss)
    assert torch.equal(y.cpu().double(), ref.permute(0, 2, 3, 1))
