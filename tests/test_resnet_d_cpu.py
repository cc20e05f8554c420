"""ResNet-D without a GPU: the archs build with timm's parameter names and counts (stem_type='deep', stem_width=32,
avg_down=True), the torch backend runs a step, the command line takes the names and refuses the fp8 / fp32 HIP paths."""

import pytest
import torch
import torch.nn.functional as F

from imagent_amd.models import resnet


@pytest.mark.parametrize("arch,count", [("resnet18d", 11_708_744), ("resnet50d", 25_576_264),
                                        ("seresnet50d", 28_088_024 + 19_232)])
def test_parameter_counts(arch, count):
    assert sum(p.numel() for p in resnet.build(arch).parameters()) == count


@pytest.mark.parametrize("arch,base", [("resnet18d", "resnet18"), ("seresnext50d_32x4d", "seresnext50_32x4d")])
def test_keys_and_shapes(arch, base):
    sd, sb = resnet.build(arch).state_dict(), resnet.build(base).state_dict()
    stem = {"conv1.0.weight": (32, 3, 3, 3), "conv1.1.weight": (32,), "conv1.3.weight": (32, 32, 3, 3),
            "conv1.4.weight": (32,), "conv1.6.weight": (64, 32, 3, 3), "bn1.weight": (64,)}
    for k, shape in stem.items():
        assert tuple(sd[k].shape) == shape, k
    assert {k.split(".")[1] for k in sd if k.startswith("conv1.")} == {"0", "1", "3", "4", "6"}
    for k, v in sb.items():  # downsample.0 / .1 -> .1 / .2 with the base's shapes: the conv is stride 1, same weights
        if ".downsample." in k:
            head, idx, tail = k.rsplit(".", 2)
            assert sd[f"{head}.{int(idx) + 1}.{tail}"].shape == v.shape, k
    assert not any(".downsample.0." in k for k in sd)
    rest = [k for k in sd if not k.startswith("conv1.") and ".downsample." not in k]
    assert rest == [k for k in sb if k != "conv1.weight" and ".downsample." not in k]
    assert all(sd[k].shape == sb[k].shape for k in rest)
    names = [n for n, _ in resnet.build(arch).named_modules() if n.endswith(("conv1.1", "conv1.4")) or n == "bn1"]
    assert names == ["conv1.1", "conv1.4", "bn1"]  # batchnorms() order: the running-statistics rows follow it


@pytest.mark.parametrize("block", ["basic", "bottleneck"])
def test_stride2_block_formula_at_odd_map(block):
    torch.manual_seed(0)
    m = resnet.build("resnet18d" if block == "basic" else "resnet50d").double()
    b = m.layer2[0]
    x = torch.randn(2, b.conv1.in_channels, 9, 9, dtype=torch.double)
    sc = b.shortcut()
    assert sc.conv is b.downsample[1] and sc.bn is b.downsample[2] and sc.conv.stride == 1 and sc.pool is not None
    idt = sc.bn.forward_torch(F.conv2d(F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False), sc.conv.weight))
    out = x
    for conv, bn, relu in b.convs_bns():
        out = bn.forward_torch(conv.forward_torch(out))
        out = F.relu(out) if relu else out
    want = F.relu(out + idt)
    assert want.shape[-2:] == (5, 5)
    torch.testing.assert_close(b.forward_torch(x), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("arch", ["resnet18d", "seresnext50d_32x4d"])
def test_torch_step_gives_every_parameter_a_gradient(arch):
    torch.manual_seed(0)
    m = resnet.build(arch, num_classes=10).train()
    F.cross_entropy(m(torch.randn(2, 3, 72, 72)), torch.tensor([1, 7])).backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in m.parameters())
    assert int(m.conv1[1].num_batches_tracked) == 1 and resnet.build("resnet50d").layer1[0].shortcut().pool is None


@pytest.mark.parametrize("dtype", ["fp32", "fp8"])
@pytest.mark.parametrize("kernels", ["hip", "auto"])
def test_cli_takes_d_archs_and_refuses_other_dtypes_on_hip(kernels, dtype):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    assert len(resnet.D_ARCHS) == 16 and set(resnet.SE_ARCHS) == {"se" + a for a in resnet.ARCHS if a[:2] != "se"}
    for arch in resnet.D_ARCHS:
        assert build_parser().parse_args(["--data", "synthetic", "--arch", arch]).arch == arch
    a = build_parser().parse_args(["--data", "synthetic", "--arch", "resnext50d_32x4d", "--dtype", dtype,
                                   "--kernels", kernels])
    with pytest.raises(SystemExit) as e:
        Trainer(a)
    assert "resnext50d_32x4d" in str(e.value) and f"--dtype {dtype}" in str(e.value) and "bf16" in str(e.value)
