"""The kernels a conv call launches are the ones csrc/kernels/conv_plan.h plans, in order -- one case per kernel family
and mode, plus both two-launch splits -- and, where tests/exact_ref.py has a reference for the form, the result
equals it. tests/test_conv_plan.py holds the plan to the recorded dispatch table on the CPU; this is the other half:
imk_conv_igemm launches what the plan says.

Every imk_conv_igemm call of a case is intercepted (ops.conv._igemm_call), its plan read from the host runtime with the
device's CU count, and the planned kernel names compared with the names the profiler saw.
"""

import ctypes as C
import os
import sys

import pytest
import torch

import test_epilogue_exact_gpu as E
from exact_ref import dgrad_ref, fwd_ref, kernel_names, out_size, stem_form, ternary, ternary_density
from test_conv_exact_gpu import _check_fwd, _fwd_preconditions, _slab

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import conv_dispatch_grid as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(a, tile, cus=None):
    """(return code, [kernel name], [images]) of one imk_conv_igemm call"""
    from imagent_amd.ops import _lib
    rt = _lib.runtime()
    out = (C.c_int32 * rt.imr_conv_plan_out_ints())()
    deep = int(os.environ.get("IMAGENT_V3_DEEP", "0") or 0) != 0
    assert rt.imr_conv_plan(C.byref(a), tile, cus or _cus(), int(deep), out) == 0
    per = (len(out) - 2) // 2
    parts = [2 + i * per for i in range(out[1])]
    assert all(out[o + 2] == 1 for o in parts)  # in its family's list
    return out[0], [C.string_at(C.addressof(out) + 4 * (o + 3)).decode() for o in parts], [out[o + 1] for o in parts]


def planned(fn, monkeypatch):
    """fn() under the profiler: (its result, the kernel names that ran, the names planned), both in launch order"""
    from imagent_amd.ops import conv
    want, call = [], conv._igemm_call

    def spy(a, tile, st, what):
        rc, names, _ = _plan(a, tile)
        assert rc == 0, (what, rc)
        want.extend(names)
        call(a, tile, st, what)

    monkeypatch.setattr(conv, "_igemm_call", spy)
    out, ran = kernel_names(fn)
    ran = [n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for n in ran]
    print(f"planned {want}\nran     {ran}")
    assert ran == want and want
    return out, ran


def _fwd(shape, monkeypatch, family, tile=0, chunked=False):
    """a forward with statistics against the fp64 reference, the whole output and the slab"""
    from imagent_amd.ops.conv import igemm_fwd
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    d = ternary_density(k * k * Ci, N * OH * OH)
    x, w = ternary((N, H, H, Ci), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    slab = _slab(Co)
    y, ran = planned(lambda: igemm_fwd(x, w, s, p, k, k, stats=slab, tile=tile), monkeypatch)
    assert all(n.startswith(family) for n in ran), ran
    ref = torch.cat([fwd_ref(x[sl], w, s, p) for sl in E._chunks(N, H * H)]) if chunked else fwd_ref(x, w, s, p)
    _fwd_preconditions(ref)
    _check_fwd(y, slab, ref)
    return ran


def test_register_staged(monkeypatch):
    assert _fwd((7, 64, 14, 64, 3, 1, 1), monkeypatch, "igemm_rs_kernel") == ["igemm_rs_kernel<128, 64, 1, 0, 2>"]


def test_lds_dma_ring(monkeypatch):
    _fwd((5, 72, 11, 200, 3, 2, 1), monkeypatch, "igemm_dma_kernel")  # C % 64 != 0


def test_v3(monkeypatch):
    _fwd((7, 128, 14, 256, 3, 1, 1), monkeypatch, "igemm_v3_kernel")


def test_stream_plain(monkeypatch):
    ran = _fwd((5, 256, 13, 1024, 1, 1, 0), monkeypatch, "conv_stream_kernel")  # 256 -> 1024 1x1: never a tiled kernel
    assert ran == ["conv_stream_kernel<256, 128, 2, 0, false, false, 0>"]


def test_halo_forward(monkeypatch):
    _fwd((3, 64, 56, 64, 3, 1, 1), monkeypatch, "halo3x3_kernel<56, 4, 0>")


def _smallest_split(Ci):
    """smallest batch at which the Ci -> 256 3x3 conv at 14 x 14 is split in two launches on this device"""
    from imagent_amd.ops import _lib
    for N in range(2, 4096):
        a = G.fwd(N, Ci, 14, 256, 3, 1, 1, **G.STATS)
        s = _lib.IGemmArgs()
        for f in G.INTS:
            setattr(s, f, a[f])
        for f in G.PTRS:
            setattr(s, f, 4096 if a[f] else None)
        rc, names, imgs = _plan(s, 0)
        if len(names) == 2:
            return N, names, imgs
    raise AssertionError("no split below 4096 images")


@pytest.mark.parametrize("Ci,family", [(256, "igemm_v3_kernel"), (96, "igemm_dma_kernel")], ids=["v3", "dma"])
def test_two_launch_split(Ci, family, monkeypatch):
    """the smallest batch the plan splits: whole rounds of 256x256 tiles, then the remaining images on 128x128 tiles
    (C % 64 != 0 keeps the conv on the LDS-DMA ring)"""
    N, names, imgs = _smallest_split(Ci)
    print(f"{Ci} -> 256 3x3 @14: split at N = {N}, images {imgs}, {names}")
    assert sum(imgs) == N and f"{family}<256, 256," in names[0] and f"{family}<128, 128," in names[1]
    ran = _fwd((N, Ci, 14, 256, 3, 1, 1), monkeypatch, family, chunked=True)
    assert ran == names


@pytest.mark.parametrize("tile,kernel", [(0, "stem_band_kernel<4>"),
                                         (23, "conv_stream_kernel<224, 64, 2, 0, true, false, 0>")], ids=["band", "stream"])
def test_stem(tile, kernel, monkeypatch):
    from imagent_amd.ops.conv import igemm_fwd
    N, H, Co = 3, 224, 64
    d = ternary_density(147, N * 112 * 112)
    x = stem_form(ternary((N, H, H, 4), d, 1, DEV))
    w = stem_form(ternary((Co, 7, 7, 4), d, 2, DEV))
    ref = fwd_ref(x, w, 2, 3)
    _fwd_preconditions(ref)
    wrow = torch.zeros(Co, 7, 32, dtype=torch.bfloat16, device=DEV)
    wrow[:, :, :28] = w.reshape(Co, 7, 28)
    slab = _slab(Co)
    y, ran = planned(lambda: igemm_fwd(x, wrow, 2, 3, 7, 7, stats=slab, stem=True, tile=tile), monkeypatch)
    assert ran == [kernel]
    _check_fwd(y, slab, ref)


BNB = [("stream-mode1", (5, 256, 13, 64, 1, 1, 0), "y_mask", "conv_stream_kernel<64, 128, 3, 1,"),
       ("stream-mode2", (5, 256, 13, 64, 1, 1, 0), "x_mask", "conv_stream_kernel<64, 128, 3, 2,"),
       ("stream-mode3", (5, 256, 13, 64, 1, 1, 0), "x2", "conv_stream_kernel<64, 128, 3, 3,"),
       ("halo-epi1", (3, 64, 56, 64, 3, 1, 1), "y_mask", "halo3x3_kernel<56, 4, 1>"),
       ("halo-epi2", (3, 64, 56, 64, 3, 1, 1), "x2", "halo3x3_kernel<56, 4, 2>")]


@pytest.mark.parametrize("shape,variant,kernel", [b[1:] for b in BNB], ids=[b[0] for b in BNB])
def test_fused_bn_backward(shape, variant, kernel, monkeypatch):
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    N, Ci, H, Co, k, s, p = shape
    o = E._bnb_operands(shape, variant)
    f = BNBwdFuse(o.x, o.bn, y=o.bits, x2=o.x2, bn2=o.bn2)
    got, ran = planned(lambda: igemm_dgrad(o.dy, o.wt, (H, H), s, p, k, k, bnb=f), monkeypatch)
    assert len(ran) == 1 and ran[0].startswith(kernel), ran
    E._bnb_check(o, shape, got)


@pytest.mark.parametrize("next1", [False, True], ids=["stream-mode4", "stream-mode5"])
def test_fused_output(next1, monkeypatch):
    """affine + residual + ReLU + mask bits on the 64 -> 256 streaming kernel, alone and with the next conv1"""
    from exact_ref import DYADIC, assert_bf16_exact, dyadic, fused_out_ref, halves, ints, mask_bytes
    from imagent_amd.ops.conv import igemm_fwd
    N, H, K, Co = 5, 13, 64, 256
    x, w = E._fwd_operands(N, H, K, Co)
    aff = torch.stack([dyadic(Co, 10, DYADIC, DEV), halves(Co, -2, 2, 11, DEV)]).contiguous()
    res = ints((N, H, H, Co), -3, 3, 12, DEV)
    out = torch.full_like(res, float("nan"))
    ym = torch.zeros(out.numel() // 8, device=DEV, dtype=torch.uint8)
    w2 = ternary((64, 1, 1, Co), ternary_density(Co), 7, DEV) if next1 else None
    r, ran = planned(lambda: igemm_fwd(x, w, 1, 0, 1, 1, out=out, affine=aff, relu=True, res=res, maskout=ym,
                                       next1=(w2, None) if next1 else None), monkeypatch)
    assert ran == [f"conv_stream_kernel<64, 256, {1 if next1 else 2}, {5 if next1 else 4}, false, false, 0>"]
    ref = fused_out_ref(fwd_ref(x, w, 1, 0), aff, res, None, relu=True)
    assert_bf16_exact(ref)
    E._eq("out", out.double(), ref)
    E._eq("mask bytes", ym, mask_bytes(ref > 0))
    if next1:  # bit for bit the stand-alone conv on the stored output
        assert torch.equal(r[1], igemm_fwd(out, w2, 1, 0, 1, 1))


@pytest.mark.parametrize("shape,kernel", [((7, 64, 14, 192, 3, 1, 1), "igemm_dma_kernel<128, 128, 2, 2, 1, 4, 2, 1, 0, 128>"),
                                          ((5, 128, 13, 256, 3, 1, 1), "igemm_v3_kernel<128, 128, 2, 2, 4, 128, 1, 0, false>")],
                         ids=["dma-fp8", "v3-fp8"])
def test_fp8_forward(shape, kernel, monkeypatch):
    from imagent_amd.ops.conv import igemm_fwd
    N, Ci, H, Co, k, s, p = shape
    d = ternary_density(k * k * Ci, N * H * H)
    x, w = ternary((N, H, H, Ci), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    x8, w8 = x.float().to(torch.float8_e4m3fn), w.float().to(torch.float8_e4m3fn)
    ref = fwd_ref(x, w, s, p)
    _fwd_preconditions(ref)
    slab = _slab(Co)
    ex, ew = E._e(0, 0)
    y, ran = planned(lambda: igemm_fwd(x8.view(torch.uint8), w8.view(torch.uint8), s, p, k, k, stats=slab,
                                       fp8=(ex, ew)), monkeypatch)
    assert ran == [kernel]
    _check_fwd(y, slab, ref)


def test_stride2_dgrad_launches_in_order(monkeypatch):
    """four parity classes of different sizes: four planned launches, the profiler's order"""
    from imagent_amd.ops.conv import igemm_dgrad
    shape = (5, 128, 13, 256, 3, 2, 1)
    N, Ci, H, Co, k, s, p = shape
    d = ternary_density(k * k * Co)
    dy, w = ternary((N, 7, 7, Co), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    out, ran = planned(lambda: igemm_dgrad(dy, w.permute(3, 1, 2, 0).contiguous(), (H, H), s, p, k, k), monkeypatch)
    assert len(ran) == 4
    E._eq("dx", out.double(), dgrad_ref(dy, w, (H, H), s, p))
