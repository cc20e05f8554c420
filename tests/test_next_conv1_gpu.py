"""The next bottleneck's conv1 computed by conv3's fused-output launch (conv_stream.hip IG_NEXT1,
``igemm_fwd(next1=)``, ``IMAGENT_NEXT_CONV1``).

Kernel: the fused call (K = 64 -> 256 with affine, residual, ReLU, mask bits and ``next1``) against the same call
without ``next1`` followed by the stand-alone 256 -> 64 conv on its output: the block output, its mask bytes and the
second output must be bit-identical; the second output's statistics slab is held to an fp64 sum of the stored values
(relative error < 1e-3, the bound tests/test_conv_shapes_gpu.py::test_production_conv_shape uses for the same sums).
Model: ResNet-50 forward + backward against the fp32 model with the switch on, the conv1 launches that disappear,
and a stale hand-over that must be ignored.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# N, H, W: M = 9 (one partial group, most waves idle), 147 (a 3-row tail group), 6,272 (every wave one or two
# groups), 75,264 (more groups than resident waves x prefetch depth: the ring wraps)
SHAPES = [(1, 3, 3), (3, 7, 7), (2, 56, 56), (24, 56, 56)]


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


class _Work:
    """A BatchNorm workspace as igemm_fwd(stats=) reads it: the slab and the shift (``save[:C]``)."""

    def __init__(self, c, shift):
        from imagent_amd.ops import _lib
        self.slab = torch.zeros(_lib.STAT_SLOTS, 2, c, device=DEV)
        self.save = torch.zeros(2, c, device=DEV)
        self.save[0] = shift


def _operands(N, H, W, downsample):
    torch.manual_seed(N * 1000 + H)
    h = torch.randn(N, H, W, 64, device=DEV).to(torch.bfloat16)
    w3 = (torch.randn(256, 1, 1, 64, device=DEV) * (2.0 / 64) ** 0.5).to(torch.bfloat16)
    w1 = (torch.randn(64, 1, 1, 256, device=DEV) * (2.0 / 256) ** 0.5).to(torch.bfloat16)
    res = torch.randn(N, H, W, 256, device=DEV).to(torch.bfloat16)
    aff = torch.stack([torch.empty(256, device=DEV).uniform_(0.5, 1.5), torch.empty(256, device=DEV).uniform_(-0.5, 0.5)])
    rsc = torch.empty(256, device=DEV).uniform_(0.5, 1.5) if downsample else None
    return h, w3, w1, res, aff.contiguous(), rsc


def _fused(h, w3, res, aff, rsc, **kw):
    from imagent_amd.ops.conv import igemm_fwd
    out = torch.empty_like(res)
    ym = torch.zeros(out.numel() // 8, device=DEV, dtype=torch.uint8)
    r = igemm_fwd(h, w3, 1, 0, 1, 1, out=out, affine=aff, relu=True, res=res, maskout=ym, res_scale=rsc, **kw)
    return out, ym, (r[1] if isinstance(r, tuple) else None)


@pytest.mark.parametrize("downsample", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{h}x{w}" for n, h, w in SHAPES])
def test_next_conv1_bit_identical(shape, downsample):
    from imagent_amd.ops.conv import igemm_fwd
    N, H, W = shape
    h, w3, w1, res, aff, rsc = _operands(N, H, W, downsample)
    out0, ym0, _ = _fused(h, w3, res, aff, rsc)
    a0 = igemm_fwd(out0, w1, 1, 0, 1, 1)
    a64 = a0.double().reshape(-1, 64)
    for shift in (torch.zeros(64, device=DEV), torch.randn(64, device=DEV) * 0.5):
        wk = _Work(64, shift)
        out1, ym1, a1 = _fused(h, w3, res, aff, rsc, next1=(w1, wk))
        torch.cuda.synchronize()
        assert torch.equal(out1, out0)
        assert torch.equal(ym1, ym0)
        assert a1.shape == a0.shape and torch.equal(a1, a0)
        # the same sums from the stand-alone conv's epilogue, and both against fp64
        wk0 = _Work(64, shift)
        igemm_fwd(out0, w1, 1, 0, 1, 1, stats=wk0)
        d = a64 - shift.double()
        tot, tot0 = wk.slab.sum(0), wk0.slab.sum(0)
        e1, e2 = rel(tot[0], d.sum(0)), rel(tot[1], (d * d).sum(0))
        print(f"M={N * H * W} shift={'0' if not shift.any() else 'rand'}: sum {e1:.2e} sumsq {e2:.2e} "
              f"(stand-alone {rel(tot0[0], d.sum(0)):.2e} {rel(tot0[1], (d * d).sum(0)):.2e})")
        assert e1 < 1e-3 and e2 < 1e-3, (e1, e2)
    # statistics optional
    _, _, a2 = _fused(h, w3, res, aff, rsc, next1=(w1, None))
    assert torch.equal(a2, a0)


def test_next_conv1_uncovered_shape_is_an_error():
    """next1 on shapes the mode does not cover (K = 128, 512 output channels; a 128-channel next conv): the call
    raises, no other kernel runs."""
    from imagent_amd.ops.conv import igemm_fwd
    h = torch.randn(2, 8, 8, 128, device=DEV).to(torch.bfloat16)
    w3 = (torch.randn(512, 1, 1, 128, device=DEV) * 0.1).to(torch.bfloat16)
    w1 = (torch.randn(128, 1, 1, 512, device=DEV) * 0.1).to(torch.bfloat16)
    res = torch.randn(2, 8, 8, 512, device=DEV).to(torch.bfloat16)
    aff = torch.ones(2, 512, device=DEV)
    ym = torch.zeros(res.numel() // 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="failed with code -12"):
        igemm_fwd(h, w3, 1, 0, 1, 1, out=torch.empty_like(res), affine=aff, relu=True, res=res, maskout=ym,
                  next1=(w1, None))
    h, w3, _, res, aff, _ = _operands(1, 4, 4, False)
    w1 = (torch.randn(128, 1, 1, 256, device=DEV) * 0.1).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="failed with code -12"):
        _fused(h, w3, res, aff, None, next1=(w1, None))
    # without the fused-output epilogue
    with pytest.raises(RuntimeError, match="failed with code -12"):
        igemm_fwd(h, w3, 1, 0, 1, 1, next1=((torch.randn(64, 1, 1, 256, device=DEV) * 0.1).to(torch.bfloat16), None))
    torch.cuda.synchronize()


def _profiled(fn):
    """Run fn under torch.profiler; the conv kernel names it launched (as test_conv_shapes_gpu._kernels)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type.name == "CUDA" and "conv_stream" in e.name]


_CONV1 = "conv_stream_kernel<256, 64, 2, 0"   # the stand-alone 256 -> 64 / 128 conv1
_FUSED = "conv_stream_kernel<64, 256, 1, 5"   # conv3's fused output + the next conv1


def test_next_conv1_model_matches_torch(monkeypatch):
    """ResNet-50 forward + backward against the fp32 PyTorch model (test_hip_vs_torch_forward_backward and its
    bounds) with IMAGENT_NEXT_CONV1 off, then on. On: the second and third layer-1 blocks launch no conv1 -- no
    256 -> 64 conv is called, the step has two stand-alone 256-input conv1 launches fewer -- and their predecessors'
    conv3 launches carry it."""
    from test_model_gpu import test_hip_vs_torch_forward_backward
    from imagent_amd.ops import block
    monkeypatch.setattr(block, "_GRAM", True)
    monkeypatch.setattr(block, "_GRAM_NOX", True)
    monkeypatch.setattr(block, "_GRAM_FWD", True)
    monkeypatch.setattr(block, "_GRAM_MIN_ROWS", 0)  # every block, at this test's 16 x 64 x 64 input
    calls = []
    real = block._fwd8
    monkeypatch.setattr(block, "_fwd8", lambda conv, *a: calls.append((conv.in_channels, conv.out_channels,
                                                                         conv.kh)) or real(conv, *a))
    seen = {}
    for on in (False, True):
        monkeypatch.setattr(block, "_NEXT1", on)
        del calls[:]
        _, names = _profiled(lambda: test_hip_vs_torch_forward_backward("resnet50", True))
        seen[on] = (sum(_CONV1 in n for n in names), sum(_FUSED in n for n in names), calls.count((256, 64, 1)))
        print(f"switch {on}: (stand-alone <256, 64> launches, fused launches, 256 -> 64 conv1 calls) = {seen[on]}")
    assert seen[False][1:] == (0, 2) and seen[True][1:] == (2, 0), seen
    assert seen[False][0] - seen[True][0] == 2, seen


def test_stale_hand_over_is_ignored(monkeypatch):
    """A block whose input is not the tensor its predecessor's launch computed conv1 from runs its own conv1 (and
    starts bn1's statistics afresh); fed that very tensor it launches none."""
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops import _lib, block
    monkeypatch.setattr(block, "_GRAM_MIN_ROWS", 0)
    torch.manual_seed(0)
    model = resnet.build("resnet50", num_classes=10).to(DEV)
    st = bind_native(model, DEV)
    model.train()
    b0, b1 = model.layer1[0], model.layer1[1]
    x = torch.relu(torch.randn(4, 16, 16, 64, device=DEV)).to(torch.bfloat16)

    def two(on, same):
        monkeypatch.setattr(block, "_NEXT1", on)
        _lib.zero_(st.zero_ws)
        o0 = block.BlockFn.apply(x, b0)
        assert (b1._next1_in is not None) == on
        x1 = o0 if same else o0.clone()
        o1, names = _profiled(lambda: block.BlockFn.apply(x1, b1))
        assert b1._next1_in is None
        return o0, o1, sum(_CONV1 in n for n in names)

    # bound: the arms differ by the summation order of the BatchNorm statistics' atomics, which moves bf16
    # roundings by one unit (2^-8 relative per element at most, over two blocks); a hand-over taken wrongly, or
    # statistics counted twice (mean and E[x^2] doubled), changes the normalised activations by O(1). 1e-2, the
    # bound the conv tests hold bf16 outputs to, separates the two
    _, ref, n = two(False, True)
    assert n == 1
    _, o1, n = two(True, True)
    print(f"hand-over taken: {n} conv1 launches, rel {rel(o1, ref):.2e}")
    assert n == 0 and rel(o1, ref) < 1e-2, (n, rel(o1, ref))
    _, o1, n = two(True, False)  # another tensor with the same values: conv1 runs, the statistics are not doubled
    print(f"hand-over stale: {n} conv1 launches, rel {rel(o1, ref):.2e}")
    assert n == 1 and rel(o1, ref) < 1e-2, (n, rel(o1, ref))
