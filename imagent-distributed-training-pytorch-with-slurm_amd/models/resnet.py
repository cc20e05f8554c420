"""ResNet-18/34/50/101/152 and ResNeXt-50 32x4d / -101 32x8d / -101 64x4d with torchvision-identical parameter names,
and their squeeze-and-excitation variants (``seresnet*`` / ``seresnext*``: a channel gate ``se`` after each block's
last BatchNorm, parameter names ``layerL.i.se.fc1.weight`` .. as in timm), and the ResNet-D variants of all of them
(``resnet50d``, ``resnext50d_32x4d``, ``seresnet50d`` ..: timm's ``stem_type='deep', stem_width=32, avg_down=True`` --
``conv1`` is a Sequential of three 3x3 convs, a downsampling shortcut is pool -> 1x1 stride-1 conv -> BN under
``downsample.0/.1/.2``), and the anti-aliased variants of all of those (``resnetblur50``, ``resnetaa50d``,
``seresnextaa101d_32x8d`` ..: timm's ``aa_layer`` -- the conv that carried a block's stride runs at stride 1 and a
parameter-free pool halves the map after its BatchNorm + ReLU; same keys, shapes and counts as the base arch).

The reference instantiates ``torchvision.models.resnet18(pretrained=False,
num_classes=1000)`` (``/root/reference/imagenet.py:312``); torchvision is not
available here, and the compute path is ours, so the family is re-declared
with the same module tree (``conv1, bn1, layer{1..4}.{i}.conv{1,2,3},
bn{1,2,3}, downsample.{0,1}, fc``), the same shapes and the same init
(kaiming-normal fan_out for convs, BN weight 1 / bias 0, nn.Linear default for
fc). ``state_dict()`` therefore matches torchvision key-for-key (122 keys for
ResNet-18, 320 for ResNet-50) and loads into it directly.
Bottleneck is v1.5 (stride on the 3x3 conv), as in torchvision.

Two execution backends share these parameters:

* ``backend='hip'``  - NHWC bf16 activations through the hand-written
  MI355X kernels (ops/*): MFMA implicit-GEMM convs with BN statistics fused
  into their epilogue, fused BN(+add)(+ReLU), fp32 master weights in a flat
  arena with bf16 shadows.
* ``backend='hip_f32'`` - NHWC fp32 through the fp32 kernels (models/native_f32.py),
  the reference's own precision.
* ``backend='torch'`` - NCHW through stock PyTorch ops: the numerical oracle
  for the kernel tests and the path used on CPU (gloo) runs.
"""

from __future__ import annotations

import math
from typing import Callable, List, Optional, Type, Union

import torch
import torch.nn as nn
import torch.nn.functional as F


# --------------------------------------------------------------------------
# parameter-holding modules (torchvision names, our own forward)
# --------------------------------------------------------------------------

class Conv2d(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, stride: int = 1, padding: int = 0, groups: int = 1):
        super().__init__()
        if cin % groups or cout % groups:
            raise ValueError(f"Conv2d: {cin} -> {cout} channels do not split into {groups} groups")
        self.in_channels, self.out_channels = cin, cout
        self.kh = self.kw = k
        self.stride, self.padding, self.groups = stride, padding, groups
        w = torch.empty(cout, cin // groups, k, k)
        nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
        self.weight = nn.Parameter(w.contiguous(memory_format=torch.channels_last))
        # bf16 shadows bound by ResNet.bind_native()
        self.w_bf16: Optional[torch.Tensor] = None
        self.wt_bf16: Optional[torch.Tensor] = None

    def forward_torch(self, x):
        return F.conv2d(x, self.weight.to(x.dtype), None, self.stride, self.padding, 1, self.groups)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size=({self.kh}, {self.kw}), "
                f"stride=({self.stride}, {self.stride}), padding=({self.padding}, {self.padding})" +
                (f", groups={self.groups}" if self.groups > 1 else ""))


class BatchNorm2d(nn.Module):
    def __init__(self, c: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.work = None  # BNWork, bound by ResNet.bind_native()

    def forward_torch(self, x):
        if self.training:
            self.num_batches_tracked.add_(1)
        return F.batch_norm(x, self.running_mean, self.running_var, self.weight.to(x.dtype),
                            self.bias.to(x.dtype), self.training, self.momentum, self.eps)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}"


class Linear(nn.Module):
    def __init__(self, fin: int, fout: int):
        super().__init__()
        self.in_features, self.out_features = fin, fout
        w = torch.empty(fout, fin)
        b = torch.empty(fout)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))  # nn.Linear.reset_parameters
        bound = 1 / math.sqrt(fin)
        nn.init.uniform_(b, -bound, bound)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(b)
        self.w_bf16: Optional[torch.Tensor] = None
        self.wt_bf16: Optional[torch.Tensor] = None

    def forward_torch(self, x):
        return F.linear(x, self.weight.to(x.dtype), self.bias.to(x.dtype))


class SEConv(nn.Module):
    """One 1x1 conv with bias of the SE gate: parameters only. Deliberately not a :class:`Conv2d`: ``ResNet.convs()``,
    the dgrad transpose plan, the fp8 quantiser and ``conv_wgrad`` never see it (ops/se.py runs the gate)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        w = torch.empty(cout, cin, 1, 1)
        nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(cout))
        self.w_bf16: Optional[torch.Tensor] = None  # [cout * cin] bf16 shadow bound by ResNet.bind_native()


class SEModule(nn.Module):
    """Squeeze-and-excitation gate: s = sigmoid(fc2(relu(fc1(mean_hw x)))), R = max(8, C // 16) reduced channels."""

    def __init__(self, channels: int):
        super().__init__()
        self.channels, self.reduced = channels, max(8, channels // 16)
        self.fc1 = SEConv(channels, self.reduced)
        self.fc2 = SEConv(self.reduced, channels)

    def forward_torch(self, x):
        z = x.mean((2, 3), keepdim=True)
        h = F.relu(F.conv2d(z, self.fc1.weight.to(x.dtype), self.fc1.bias.to(x.dtype)))
        return x * torch.sigmoid(F.conv2d(h, self.fc2.weight.to(x.dtype), self.fc2.bias.to(x.dtype)))


class AvgPool2(nn.Module):
    """The ResNet-D shortcut's pool: ``AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)``; no parameters. Also
    the pool of the ``aa`` archs' stride-2 points (timm ``aa_layer=nn.AvgPool2d``; equal to it on even maps)."""

    kind = "avg"

    def forward_torch(self, x):
        return F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)


class BlurPool2(nn.Module):
    """The anti-aliased archs' BlurPool (timm ``BlurPool2d(filt_size=3, stride=2)``): depthwise [1,2,1]^T [1,2,1] / 16
    at stride 2 over the reflect-padded map. No parameters and no buffer (timm's filter is a non-persistent one): no
    state-dict key, nothing for the weight average or the buffer broadcast to carry."""

    kind = "blur"

    def forward_torch(self, x):
        from ..ops.misc import blurpool_torch
        return blurpool_torch(x)


def _aa_pool(aa: Optional[str]) -> Optional[nn.Module]:
    """The pool of an anti-aliased downsampling point: ``"blur"`` BlurPool, ``"avg"`` the 2x2 average pool."""
    if aa not in (None, "blur", "avg"):
        raise ValueError(f"aa must be None, 'blur' or 'avg', got {aa!r}")
    return None if aa is None else (BlurPool2() if aa == "blur" else AvgPool2())


class Shortcut:
    """A downsampling block's shortcut as its parts, whatever their indices in ``downsample``: ``pool`` (the D archs'
    2x2 average pool in front of the conv, or None), the 1x1 ``conv`` and its BatchNorm ``bn``."""

    __slots__ = ("pool", "conv", "bn")

    def __init__(self, seq: nn.Sequential):
        # torchvision: downsample.0 conv, .1 BN; the D archs (timm avg_down): .0 pool / identity, .1 conv, .2 BN
        self.conv, self.bn = seq[-2], seq[-1]
        self.pool = seq[0] if isinstance(seq[0], AvgPool2) else None

    def forward_torch(self, x):
        if self.pool is not None:
            x = self.pool.forward_torch(x)
        return self.bn.forward_torch(self.conv.forward_torch(x))


class BNWork:
    """Per-BN device workspace (views into one arena zeroed once per step)."""

    __slots__ = ("slab", "stats", "save", "scratch")

    def __init__(self, slab, stats, save, scratch):
        # slab [STAT_SLOTS, 2, C]: conv-epilogue (sum, sumsq) partials (zeroed per step)
        # stats [2, C]: folded sums; save [2, C]: (mean, invstd); scratch [3, C]: bwd sums
        self.slab, self.stats, self.save, self.scratch = slab, stats, save, scratch


# --------------------------------------------------------------------------
# blocks
# --------------------------------------------------------------------------

class BasicBlock(nn.Module):
    expansion = 1

    aa_after = 0  # an anti-aliased block's pool follows the (conv1, bn1) pair

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, width_per_group=64, se=False, aa=None):
        super().__init__()
        if groups != 1 or width_per_group != 64:
            raise ValueError("BasicBlock only supports groups=1 and width_per_group=64")
        # anti-aliased (stride-2 blocks only): conv1 at stride 1, the pool after bn1 + ReLU
        self.aa = _aa_pool(aa) if stride == 2 else None
        self.conv1 = Conv2d(inplanes, planes, 3, 1 if self.aa is not None else stride, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, 1, 1)
        self.bn2 = BatchNorm2d(planes)
        self.se = SEModule(planes) if se else None
        self.downsample = downsample
        self.stride = stride

    def convs_bns(self):
        return [(self.conv1, self.bn1, True), (self.conv2, self.bn2, False)]

    def shortcut(self) -> Optional["Shortcut"]:
        return None if self.downsample is None else Shortcut(self.downsample)

    def pool(self):
        """(pool module, index of the (conv, bn) pair whose ReLU it follows) of an anti-aliased block, else None."""
        return None if self.aa is None else (self.aa, self.aa_after)

    def forward_torch(self, x):
        out = F.relu(self.bn1.forward_torch(self.conv1.forward_torch(x)))
        if self.aa is not None:
            out = self.aa.forward_torch(out)
        out = self.bn2.forward_torch(self.conv2.forward_torch(out))
        if self.se is not None:
            out = self.se.forward_torch(out)
        idt = x if self.downsample is None else self.shortcut().forward_torch(x)
        return F.relu(out + idt)


class Bottleneck(nn.Module):
    expansion = 4

    aa_after = 1  # an anti-aliased block's pool follows the (conv2, bn2) pair

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, width_per_group=64, se=False, aa=None):
        super().__init__()
        width = int(planes * width_per_group / 64) * groups  # torchvision's rule (ResNeXt: groups > 1)
        self.conv1 = Conv2d(inplanes, width, 1)
        self.bn1 = BatchNorm2d(width)
        # anti-aliased (stride-2 blocks only): conv2 at stride 1, the pool after bn2 + ReLU
        self.aa = _aa_pool(aa) if stride == 2 else None
        self.conv2 = Conv2d(width, width, 3, 1 if self.aa is not None else stride, 1, groups=groups)
        self.bn2 = BatchNorm2d(width)
        self.conv3 = Conv2d(width, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.se = SEModule(planes * 4) if se else None
        self.downsample = downsample
        self.stride = stride

    def convs_bns(self):
        return [(self.conv1, self.bn1, True), (self.conv2, self.bn2, True), (self.conv3, self.bn3, False)]

    def shortcut(self) -> Optional["Shortcut"]:
        return None if self.downsample is None else Shortcut(self.downsample)

    def pool(self):
        """(pool module, index of the (conv, bn) pair whose ReLU it follows) of an anti-aliased block, else None."""
        return None if self.aa is None else (self.aa, self.aa_after)

    def forward_torch(self, x):
        out = F.relu(self.bn1.forward_torch(self.conv1.forward_torch(x)))
        out = F.relu(self.bn2.forward_torch(self.conv2.forward_torch(out)))
        if self.aa is not None:
            out = self.aa.forward_torch(out)
        out = self.bn3.forward_torch(self.conv3.forward_torch(out))
        if self.se is not None:
            out = self.se.forward_torch(out)
        idt = x if self.downsample is None else self.shortcut().forward_torch(x)
        return F.relu(out + idt)


# --------------------------------------------------------------------------
# ResNet
# --------------------------------------------------------------------------

class ResNet(nn.Module):
    # NHWC input channels on the HIP path (3 real + 1 zero): the stem kernel
    # reads the 7 taps x 4 channels of a kernel row as one contiguous segment
    STEM_CPAD = 4

    def __init__(self, block: Type[Union[BasicBlock, Bottleneck]], layers: List[int],
                 num_classes: int = 1000, zero_init_residual: bool = False, groups: int = 1,
                 width_per_group: int = 64, se: bool = False, deep: bool = False, aa: Optional[str] = None):
        super().__init__()
        self.block = block
        # anti-aliased (timm aa_layer): "blur" BlurPool / "avg" the 2x2 average pool at every stride-2 point; the
        # stem's max-pool becomes max-pool(3, 1, 1) -> BlurPool, or the average pool alone
        self.aa = aa
        self.stem_pool = _aa_pool(aa)
        self.groups, self.width_per_group, self.se = groups, width_per_group, se
        # ResNet-D (timm stem_type='deep', stem_width=32, avg_down=True): three 3x3 stem convs, pooled shortcuts
        self.deep = deep
        self.inplanes = 64
        if deep:  # (indices 2 and 5: the parameter-free ReLUs of timm's Sequential)
            self.conv1 = nn.Sequential(Conv2d(3, 32, 3, 2, 1), BatchNorm2d(32), nn.ReLU(), Conv2d(32, 32, 3, 1, 1),
                                       BatchNorm2d(32), nn.ReLU(), Conv2d(32, 64, 3, 1, 1))
        else:
            self.conv1 = Conv2d(3, 64, 7, 2, 3)
        self.bn1 = BatchNorm2d(64)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.fc = Linear(512 * block.expansion, num_classes)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)
                elif isinstance(m, BasicBlock):
                    nn.init.zeros_(m.bn2.weight)
        self.backend = "torch"
        self.native = None  # NativeState when bound

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if (stride != 1 or self.inplanes != planes * block.expansion) and self.deep:
            downsample = nn.Sequential(AvgPool2() if stride != 1 else nn.Identity(),
                                       Conv2d(self.inplanes, planes * block.expansion, 1, 1),
                                       BatchNorm2d(planes * block.expansion))
        elif stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(Conv2d(self.inplanes, planes * block.expansion, 1, stride),
                                       BatchNorm2d(planes * block.expansion))
        gw = dict(groups=self.groups, width_per_group=self.width_per_group, se=self.se)
        layers = [block(self.inplanes, planes, stride, downsample, aa=self.aa, **gw)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, **gw))
        return nn.Sequential(*layers)

    def blocks(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for b in layer:
                yield b

    def stem(self):
        """The stem's (conv, BatchNorm) pairs in forward order; each BatchNorm is followed by a ReLU."""
        if not self.deep:
            return [(self.conv1, self.bn1)]
        return [(self.conv1[0], self.conv1[1]), (self.conv1[3], self.conv1[4]), (self.conv1[6], self.bn1)]

    def batchnorms(self) -> List[BatchNorm2d]:
        return [m for m in self.modules() if isinstance(m, BatchNorm2d)]

    def convs(self) -> List[Conv2d]:
        return [m for m in self.modules() if isinstance(m, Conv2d)]

    # ---------------------------------------------------------------- torch
    def forward_torch(self, x):
        for conv, bn in self.stem():
            x = F.relu(bn.forward_torch(conv.forward_torch(x)))
        if self.aa == "blur":
            x = self.stem_pool.forward_torch(F.max_pool2d(x, 3, 1, 1))
        elif self.aa == "avg":
            x = self.stem_pool.forward_torch(x)
        else:
            x = F.max_pool2d(x, 3, 2, 1)
        for b in self.blocks():
            x = b.forward_torch(x)
        x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
        return self.fc.forward_torch(x)

    # ------------------------------------------------------------------ hip
    def forward(self, x):
        if self.backend == "hip":
            from .native import forward_hip
            return forward_hip(self, x)
        if self.backend == "hip_f32":
            from .native_f32 import forward_hip_f32
            return forward_hip_f32(self, x)
        return self.forward_torch(x)


def _resnet(block, layers, **kw) -> ResNet:
    return ResNet(block, layers, **kw)


def resnet18(**kw) -> ResNet:
    return _resnet(BasicBlock, [2, 2, 2, 2], **kw)


def resnet34(**kw) -> ResNet:
    return _resnet(BasicBlock, [3, 4, 6, 3], **kw)


def resnet50(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 6, 3], **kw)


def resnet101(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 23, 3], **kw)


def resnet152(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 8, 36, 3], **kw)


def resnext50_32x4d(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 6, 3], groups=32, width_per_group=4, **kw)


def resnext101_32x8d(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 23, 3], groups=32, width_per_group=8, **kw)


def resnext101_64x4d(**kw) -> ResNet:
    return _resnet(Bottleneck, [3, 4, 23, 3], groups=64, width_per_group=4, **kw)


def _se(fn: Callable[..., ResNet]) -> Callable[..., ResNet]:
    return lambda **kw: fn(se=True, **kw)


def _d(fn: Callable[..., ResNet]) -> Callable[..., ResNet]:
    return lambda **kw: fn(deep=True, **kw)


def d_name(name: str) -> str:
    """timm's name of the D variant: the ``d`` follows the depth (``resnet50d``, ``resnext50d_32x4d``)."""
    head, sep, tail = name.partition("_")
    return head + "d" + sep + tail


def _aa(fn: Callable[..., ResNet], kind: str) -> Callable[..., ResNet]:
    return lambda **kw: fn(aa=kind, **kw)


def aa_name(name: str, tag: str) -> str:
    """timm's name of an anti-aliased variant: ``blur`` / ``aa`` follows the ``resnet`` / ``resnext`` head
    (``resnetblur50``, ``resnetaa50d``, ``resnextblur50_32x4d``)."""
    head = "resnext" if name.startswith("resnext") else "resnet"
    if not name.startswith(head):
        raise ValueError(f"aa_name: {name!r} does not start with resnet / resnext")
    return head + tag + name[len(head):]


ARCHS = {"resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50, "resnet101": resnet101,
         "resnet152": resnet152, "resnext50_32x4d": resnext50_32x4d, "resnext101_32x8d": resnext101_32x8d,
         "resnext101_64x4d": resnext101_64x4d}
_PLAIN_D = tuple(d_name(name) for name in ARCHS)
ARCHS.update({d_name(name): _d(fn) for name, fn in list(ARCHS.items())})
_PLAIN_AA = tuple(aa_name(name, tag) for name in ARCHS for tag in ("blur", "aa"))
ARCHS.update({aa_name(name, tag): _aa(fn, kind) for name, fn in list(ARCHS.items())
              for tag, kind in (("blur", "blur"), ("aa", "avg"))})
ARCHS.update({"se" + name: _se(fn) for name, fn in list(ARCHS.items())})
# the grouped-bottleneck archs: bf16 HIP kernels (ops/conv.py gconv_*) or the torch backend, no fp32 HIP path
GROUPED_ARCHS = tuple(a for a in ARCHS if "resnext" in a)
# the squeeze-and-excitation archs: bf16 HIP kernels (ops/se.py) or the torch backend, no fp8 / fp32 HIP path
SE_ARCHS = tuple(a for a in ARCHS if a.startswith("se"))
# the ResNet-D archs (deep 3x3 stem, average-pool shortcut): bf16 HIP kernels (ops/conv.py nconv_*, ops/misc.py
# avgpool2_*) or the torch backend, no fp8 / fp32 HIP path
D_ARCHS = _PLAIN_D + tuple("se" + a for a in _PLAIN_D)
# the anti-aliased archs (BlurPool / average pool at the stride-2 points): bf16 HIP kernels (ops/misc.py blurpool_*,
# avgpool2_*) or the torch backend, no fp8 / fp32 HIP path
AA_ARCHS = _PLAIN_AA + tuple("se" + a for a in _PLAIN_AA)


def build(arch: str, num_classes: int = 1000, **kw) -> ResNet:
    if arch not in ARCHS:
        raise ValueError(f"unknown arch {arch!r}; choose from {sorted(ARCHS)}")
    return ARCHS[arch](num_classes=num_classes, **kw)
