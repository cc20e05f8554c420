"""The 2x2 / stride-2 average pool of the ResNet-D shortcut (avgpool2.hip; ceil_mode, count_include_pad=False) against
``F.avg_pool2d`` in fp64. Inputs are multiples of 1/4 below 8: sums of up to four of them and their quotients by 1, 2
or 4 are exact in fp32 and in bf16, so both directions must agree bit for bit (odd maps: the last window holds 2 or 1
pixels)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("hw", [(8, 8), (9, 9), (7, 10)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", [64, 256])
def test_avgpool2_matches_torch(C, hw):
    from imagent_amd.ops.misc import AvgPool2Fn
    (H, W), N = hw, 2
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randint(-4, 5, (N, H, W, C), generator=g).double() / 4).requires_grad_()  # sums stay multiples of 1/16
    ref = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False)
    dy = torch.randint(-8, 9, ref.shape, generator=g).double() / 4
    ref.backward(dy)
    xd = x.detach().to(torch.bfloat16).to(DEV).requires_grad_()
    y = AvgPool2Fn.apply(xd)
    y.backward(dy.permute(0, 2, 3, 1).to(torch.bfloat16).to(DEV))
    assert y.shape == (N, (H + 1) // 2, (W + 1) // 2, C)
    assert torch.equal(y.detach().cpu().double(), ref.detach().permute(0, 2, 3, 1))
    assert torch.equal(xd.grad.cpu().double(), x.grad)
