"""--fp8-wgrad on the command line (no GPU): it parses, the Trainer rejects it without --dtype fp8 --kernels hip, and
its environment switch is documented."""

import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*extra):
    from imagent_amd.cli import build_parser
    return build_parser().parse_args(["--data", "synthetic", "--arch", "resnet18", *extra])


def test_fp8_wgrad_parses():
    assert _args().fp8_wgrad is False
    a = _args("--dtype", "fp8", "--kernels", "hip", "--fp8-wgrad")
    assert a.fp8_wgrad is True and a.dtype == "fp8"


@pytest.mark.parametrize("extra", [("--dtype", "bf16", "--kernels", "hip"), ("--dtype", "fp8", "--kernels", "torch"),
                                   ("--dtype", "bf16",)], ids=["bf16", "torch", "bf16-auto"])
def test_trainer_rejects_fp8_wgrad_without_fp8_hip(extra):
    from imagent_amd.train.engine import Trainer
    with pytest.raises(SystemExit) as e:
        Trainer(_args("--fp8-wgrad", *extra))
    assert "--fp8-wgrad" in str(e.value) and "--dtype fp8" in str(e.value)


def test_fp8_wgrad_ok_rule():
    """The static rule on ResNet-50's convs: the thirteen 3x3 convs of layers 2-4, layer 4's conv1 and conv3 and the
    layer-3 / layer-4 downsample convs (21; a bound model drops those without an e5m2 gradient copy)."""
    from imagent_amd.models import resnet
    from imagent_amd.ops.block import fp8_dgrad_ok, fp8_fwd_ok, fp8_wgrad_ok
    m = resnet.build("resnet50", num_classes=10)
    ok = [c for c in m.convs() if fp8_wgrad_ok(c)]
    assert len(ok) == 21
    for c in ok:
        assert fp8_fwd_ok(c) and fp8_dgrad_ok(c) and c.in_channels % 128 == 0 and c.out_channels % 128 == 0
    assert sum(c.kh == 3 for c in ok) == 13
    assert not fp8_wgrad_ok(m.conv1)


def test_switch_is_documented():
    with open(os.path.join(ROOT, "docs", "PARITY.md")) as f:
        rows = [ln for ln in f if ln.startswith("| `IMAGENT_FP8_WGRAD`")]
    assert len(rows) == 1
