"""SE-ResNet / SE-ResNeXt without a GPU: the archs build with timm's parameter names and counts, the torch backend
runs a step, the command line takes the names and refuses the fp8 / fp32 HIP paths."""

import pytest
import torch
import torch.nn.functional as F

COUNTS = {"seresnet50": 28_088_024, "seresnext50_32x4d": 27_559_896}  # at 1000 classes


def test_se_archs_build_with_their_parameter_counts():
    from imagent_amd.models import resnet
    assert set(resnet.SE_ARCHS) == {"se" + a for a in resnet.ARCHS if not a.startswith("se")}
    assert all(a in resnet.ARCHS for a in resnet.SE_ARCHS)
    for arch in resnet.SE_ARCHS:
        m = resnet.build(arch, num_classes=10)
        assert all(b.se is not None for b in m.blocks())
        assert not any(isinstance(mod, resnet.Conv2d) for b in m.blocks() for mod in b.se.modules())
    for arch, count in COUNTS.items():
        assert sum(p.numel() for p in resnet.build(arch).parameters()) == count
    assert all(b.se is None for b in resnet.build("resnet18", num_classes=10).blocks())


@pytest.mark.parametrize("arch", ["seresnet18", "seresnext50_32x4d"])
def test_se_state_dict_keys_and_shapes(arch):
    from imagent_amd.models import resnet
    m = resnet.build(arch, num_classes=10)
    sd = m.state_dict()
    plain = resnet.build(arch[2:], num_classes=10).state_dict()
    assert [k for k in sd if ".se." not in k] == list(plain)
    n = 0
    for li in range(1, 5):
        for i, b in enumerate(getattr(m, f"layer{li}")):
            C = b.convs_bns()[-1][0].out_channels
            R = max(8, C // 16)
            k = f"layer{li}.{i}.se."
            assert tuple(sd[k + "fc1.weight"].shape) == (R, C, 1, 1) and tuple(sd[k + "fc1.bias"].shape) == (R,)
            assert tuple(sd[k + "fc2.weight"].shape) == (C, R, 1, 1) and tuple(sd[k + "fc2.bias"].shape) == (C,)
            assert not sd[k + "fc1.bias"].any() and not sd[k + "fc2.bias"].any() and sd[k + "fc1.weight"].std() > 0
            n += 4
    assert n == len(sd) - len(plain)


def test_se_torch_backend_step():
    """The torch backend's block tail is relu(s * bn(a) + shortcut) with s from the pooled bn(a): one block against
    the formula written out, and a whole-model step that reaches every SE parameter."""
    from imagent_amd.models import resnet
    torch.manual_seed(0)
    m = resnet.build("seresnet18", num_classes=10)
    b = m.layer2[0]
    with torch.no_grad():
        b.se.fc1.bias.normal_()
        b.se.fc2.bias.normal_()
    x = torch.randn(2, 64, 8, 8)
    u = b.bn2.forward_torch(b.conv2.forward_torch(F.relu(b.bn1.forward_torch(b.conv1.forward_torch(x)))))
    z = u.mean((2, 3))
    h = F.relu(z @ b.se.fc1.weight.flatten(1).t() + b.se.fc1.bias)
    s = torch.sigmoid(h @ b.se.fc2.weight.flatten(1).t() + b.se.fc2.bias)
    idt = b.downsample[1].forward_torch(b.downsample[0].forward_torch(x))
    want = F.relu(s[:, :, None, None] * u + idt)
    assert torch.allclose(b.forward_torch(x), want, atol=1e-5)
    y = m(torch.randn(2, 3, 64, 64))
    F.cross_entropy(y, torch.tensor([1, 2])).backward()
    assert tuple(y.shape) == (2, 10)
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for n, p in m.named_parameters() if ".se." in n)


@pytest.mark.parametrize("dtype", ["fp32", "fp8"])
@pytest.mark.parametrize("kernels", ["hip", "auto"])
def test_cli_takes_se_archs_and_refuses_other_dtypes_on_hip(kernels, dtype):
    from imagent_amd.cli import build_parser
    from imagent_amd.models.resnet import SE_ARCHS
    from imagent_amd.train.engine import Trainer
    for arch in SE_ARCHS:
        assert build_parser().parse_args(["--data", "synthetic", "--arch", arch]).arch == arch
    a = build_parser().parse_args(["--data", "synthetic", "--arch", "seresnet50", "--dtype", dtype,
                                   "--kernels", kernels])
    with pytest.raises(SystemExit) as e:
        Trainer(a)
    assert "seresnet50" in str(e.value) and f"--dtype {dtype}" in str(e.value) and "bf16" in str(e.value)
