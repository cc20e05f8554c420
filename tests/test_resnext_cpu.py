"""ResNeXt archs without a GPU: torchvision's state-dict keys, shapes and parameter counts, the grouped Conv2d's torch
forward, and the command line's refusal of the fp32 HIP path."""

import pytest
import torch
import torch.nn.functional as F

# (groups, width_per_group, layers, parameters) of torchvision.models.resnext*
ARCHS = {"resnext50_32x4d": (32, 4, [3, 4, 6, 3], 25_028_904),
         "resnext101_64x4d": (64, 4, [3, 4, 23, 3], 83_455_272),
         "resnext101_32x8d": (32, 8, [3, 4, 23, 3], 88_791_336)}


@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_state_dict_matches_torchvision(arch):
    from imagent_amd.models import resnet
    groups, wpg, layers, count = ARCHS[arch]
    m = resnet.build(arch)
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == count
    assert list(sd) == list(resnet.build("resnet50" if layers[2] == 6 else "resnet101").state_dict())  # same module tree
    inplanes = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), layers), 1):
        width = int(planes * wpg / 64) * groups
        for b in range(n):
            k = f"layer{li}.{b}."
            assert tuple(sd[k + "conv1.weight"].shape) == (width, inplanes, 1, 1)
            assert tuple(sd[k + "conv2.weight"].shape) == (width, width // groups, 3, 3)
            assert tuple(sd[k + "conv3.weight"].shape) == (planes * 4, width, 1, 1)
            assert tuple(sd[k + "bn2.running_var"].shape) == (width,)
            inplanes = planes * 4


@pytest.mark.parametrize("stride", [1, 2])
def test_grouped_conv2d_forward_torch(stride):
    from imagent_amd.models.resnet import Conv2d
    torch.manual_seed(0)
    c = Conv2d(32, 32, 3, stride, 1, groups=8)
    assert tuple(c.weight.shape) == (32, 4, 3, 3)
    x = torch.randn(2, 32, 9, 11)
    assert torch.equal(c.forward_torch(x), F.conv2d(x, c.weight, None, stride, 1, 1, 8))
    with pytest.raises(ValueError):
        Conv2d(30, 32, 3, 1, 1, groups=8)


@pytest.mark.parametrize("kernels", ["hip", "auto"])
def test_cli_refuses_fp32_with_a_grouped_arch(kernels):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    a = build_parser().parse_args(["--data", "synthetic", "--arch", "resnext50_32x4d", "--dtype", "fp32",
                                   "--kernels", kernels])
    with pytest.raises(SystemExit) as e:
        Trainer(a)
    assert "resnext50_32x4d" in str(e.value) and "--dtype fp32" in str(e.value)
