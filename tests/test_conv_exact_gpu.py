"""Bit-exact forward and dgrad: every conv kernel on ternary operands must EQUAL the fp64 reference, over ALL images,
and the forward's statistics slab must hold exactly the reference's per-channel sum and sum of squares.

Operands are in {-1, 0, 1} with a nonzero density set from K = taps x C (exact_ref.ternary_density), and each case
first checks on the reference alone that |y| <= 256 (an exact bf16 integer) and that a channel's sum(y * y) stays
below 2^23 (exact fp32 partial sums in any order). The existing relative-L2 checks look at four images of a large
batch and allow 1e-3 on the statistics; here a row written or counted twice, a padding tap that is not zero or a
tile past its image range is an inequality. Shapes are (N, Ci, H, Co, k, stride, pad).

The fused epilogues (fused output, BN backward, the ``xbn`` operand) and the fp8 forward and dgrad are integer-closed
too once the BatchNorm constants are dyadic: tests/test_epilogue_exact_gpu.py holds them to the same equality.
Measured results and the kernels the default dispatch launched: profiles/exact_tests.md.
"""

import functools
import re

import pytest
import torch

from exact_ref import (assert_out_exact, dgrad_ref, fwd_ref, ints, kernel_names, out_size, short_names, stem_form, ternary,
                       ternary_density)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _id(s):
    return "x".join(map(str, s))


def _launch(fn):
    """fn(), with an existing -10x return (a tile / epilogue pair the entry does not take) as a skip."""
    try:
        return fn()
    except RuntimeError as e:
        m = re.search(r"failed with code (-10\d)$", str(e))
        if m is None:
            raise
        pytest.skip(f"unsupported tile / epilogue pair ({m.group(1)})")


@functools.lru_cache(maxsize=3)
def _fwd_case(shape):
    """(x, w, fp64 reference) of a shape, shared and never modified; preconditions checked on the reference."""
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    d = ternary_density(k * k * Ci, N * OH * OH)
    x = ternary((N, H, H, Ci), d, 1, DEV)
    w = ternary((Co, k, k, Ci), d, 2, DEV)
    ref = fwd_ref(x, w, s, p)
    _fwd_preconditions(ref)
    return x, w, ref


def _fwd_preconditions(ref):
    assert_out_exact(ref)
    assert ref.any()
    assert (ref * ref).reshape(-1, ref.shape[-1]).sum(0).max().item() < 2 ** 23


def _check_fwd(y, slab, ref):
    torch.cuda.synchronize()
    bad = (y.double() != ref).sum().item()
    assert bad == 0, f"y: {bad} of {ref.numel()} elements differ, first at {(y.double() != ref).nonzero()[0].tolist()}"
    r2 = ref.reshape(-1, ref.shape[-1])
    want = torch.stack([r2.sum(0), (r2 * r2).sum(0)])
    got = slab.sum(0).double()
    assert torch.equal(got, want), f"statistics: max |sum diff| {(got[0] - want[0]).abs().max().item()}, " \
                                   f"max |sumsq diff| {(got[1] - want[1]).abs().max().item()}"


def _slab(Co):
    from imagent_amd.ops import _lib
    return torch.zeros(_lib.STAT_SLOTS, 2, Co, device=DEV)


def _fwd_tile(shape, tile, epi):
    from imagent_amd.ops.conv import igemm_fwd
    _, _, _, Co, k, s, p = shape
    x, w, ref = _fwd_case(shape)
    slab = _slab(Co)
    y = _launch(lambda: igemm_fwd(x, w, s, p, k, k, stats=slab, tile=tile, epi=epi))
    _check_fwd(y, slab, ref)


# ---- explicit tiles: the register-staged and LDS-DMA ring tiles (ragged M / N / K on the second shape)
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("shape", [(7, 64, 14, 128, 3, 1, 1), (5, 72, 11, 200, 3, 2, 1), (5, 256, 9, 320, 1, 1, 0)],
                         ids=_id)
def test_fwd_explicit_tiles(shape, tile, epi):
    _fwd_tile(shape, tile, epi)


# ---- the v3 main loop (conv_igemm_v3.h): 256x256 / 128x128 / 256x128, tap-inner, the deeper rings. It has the
# staged epilogue only (never epi 1); epi 0 picks it for more than four 64-deep K tiles, so the K = 256 shape with
# epi 0 is the entry's -105
@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("tile", [17, 18, 19, 27, 28, 29, 30, 31, 32])
@pytest.mark.parametrize("shape", [(7, 128, 14, 256, 3, 1, 1), (5, 256, 9, 512, 1, 1, 0)], ids=_id)
def test_fwd_v3_tiles(shape, tile, epi):
    _fwd_tile(shape, tile, epi)


# ---- the streaming short-K 1x1 kernel's 256 / 128 / 64-channel slices
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("tile", [20, 21, 22])
@pytest.mark.parametrize("shape", [(9, 64, 13, 256, 1, 1, 0), (9, 128, 13, 512, 1, 1, 0)], ids=_id)
def test_fwd_stream_slices(shape, tile, epi):
    _fwd_tile(shape, tile, epi)


@pytest.mark.parametrize("shape", [(3, 64, 56, 64, 3, 1, 1), (1, 64, 112, 64, 3, 1, 1)], ids=_id)
def test_fwd_halo(shape):
    """The halo-tiled 64 -> 64 3x3 (conv_halo.hip), the default dispatch at these shapes: halo3x3_kernel<56, 4> and
    <112, 2> (layer 1 of a 448-pixel input)."""
    from imagent_amd.ops.conv import igemm_fwd
    x, w, ref = _fwd_case(shape)
    slab = _slab(64)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 1, 3, 3, stats=slab))
    print(f"fwd {shape}: {short_names(names)}")
    assert any(f"halo3x3_kernel<{shape[2]}, " in n for n in names), names
    _check_fwd(y, slab, ref)


@pytest.mark.parametrize("tile", [0, 23], ids=["band", "stream"])
def test_fwd_stem(tile):
    """The 224-px 7x7 / 2 stem: 4-channel input (channel 3 zero), [Co][KH][32] weight rows."""
    from imagent_amd.ops.conv import igemm_fwd
    N, H, Co = 3, 224, 64
    OH = out_size(H, 7, 2, 3)
    d = ternary_density(147, N * OH * OH)
    x = stem_form(ternary((N, H, H, 4), d, 1, DEV))
    w = stem_form(ternary((Co, 7, 7, 4), d, 2, DEV))
    ref = fwd_ref(x, w, 2, 3)
    _fwd_preconditions(ref)
    wrow = torch.zeros(Co, 7, 32, dtype=torch.bfloat16, device=DEV)
    wrow[:, :, :28] = w.reshape(Co, 7, 28)
    slab = _slab(Co)
    y = igemm_fwd(x, wrow, 2, 3, 7, 7, stats=slab, stem=True, tile=tile)
    _check_fwd(y, slab, ref)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_fwd_auto_big_tile_without_split():
    """M = 49,147: 192 tiles of 256x256, less than one round of a 256-CU device -- one launch."""
    from imagent_amd.ops.conv import igemm_fwd
    shape = (1003, 128, 7, 256, 3, 1, 1)
    x, w, ref = _fwd_case(shape)
    slab = _slab(256)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 1, 3, 3, stats=slab))
    names = short_names(names)
    print(f"fwd {shape}: {names}")
    assert any("igemm_v3_kernel<256, 256" in n for n in names), names
    if _cus() == 256:
        assert len(names) == 1, names
    _check_fwd(y, slab, ref)


def test_fwd_auto_tail_split():
    """M = 69,580: 272 tiles = one round of 256 plus 16, so images [0, 1337) run on 256x256 tiles and [1337, 1420) on
    128x128 tiles (conv_igemm.hip tail_split_images). The main part's M = 65,513 is ragged: its last tile's rows
    past 65,513 are the tail part's first rows, which must be neither written nor counted twice. Every image is
    compared, the ones around the boundary included."""
    from imagent_amd.ops.conv import igemm_fwd
    if _cus() != 256:
        pytest.skip(f"the split point is derived for 256 CUs; this device reports {_cus()}")
    shape = (1420, 128, 7, 256, 3, 1, 1)
    x, w, ref = _fwd_case(shape)
    slab = _slab(256)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 1, 3, 3, stats=slab))
    names = short_names(names)
    print(f"fwd {shape}: {names}")
    assert any("igemm_v3_kernel<256, 256" in n for n in names), names
    assert any("igemm_v3_kernel<128, 128" in n for n in names), names
    _check_fwd(y, slab, ref)


# ---- dgrad, plain and accumulating into an integer-valued out; (5, 128, 13, ...) stride 2 on an odd image: all four
# parity classes with different sizes; the strided 1x1 leaves three classes without a tap
@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("shape", [(7, 64, 14, 128, 3, 1, 1), (5, 128, 13, 256, 3, 2, 1), (5, 256, 10, 512, 1, 2, 0),
                                   (1003, 256, 7, 128, 3, 1, 1)], ids=_id)
def test_dgrad(shape, accumulate):
    from imagent_amd.ops.conv import igemm_dgrad
    N, Ci, H, Co, k, s, p = shape
    dy, wt, ref = _dgrad_case(shape)
    if accumulate:
        base = ints((N, H, H, Ci), -8, 8, 3, DEV)
        assert_out_exact(ref, base)
        out = base.clone()
        want = base.double() + ref
        _, names = kernel_names(lambda: igemm_dgrad(dy, wt, (H, H), s, p, k, k, out=out, accumulate=True))
    else:
        want = ref
        out, names = kernel_names(lambda: igemm_dgrad(dy, wt, (H, H), s, p, k, k))
    print(f"dgrad {shape} {'accumulate' if accumulate else 'plain'}: {short_names(names)}")
    bad = (out.double() != want).sum().item()
    assert bad == 0, f"{bad} of {want.numel()} elements differ, first at {(out.double() != want).nonzero()[0].tolist()}"


# ---- dgrad through explicit tiles with the staged epilogue, as tests/test_kernels_gpu.py runs them
@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("tile", [2, 8, 17, 18, 19])
@pytest.mark.parametrize("shape", [(7, 64, 14, 128, 3, 1, 1), (5, 128, 13, 256, 3, 2, 1), (5, 256, 10, 512, 1, 2, 0)],
                         ids=_id)
def test_dgrad_explicit_tiles(shape, tile, accumulate):
    from imagent_amd.ops.conv import igemm_dgrad
    N, Ci, H, Co, k, s, p = shape
    dy, wt, ref = _dgrad_case(shape)
    base = ints((N, H, H, Ci), -8, 8, 3, DEV) if accumulate else \
        torch.zeros(N, H, H, Ci, dtype=torch.bfloat16, device=DEV)
    assert_out_exact(ref, base)
    out = base.clone() if accumulate else None
    out = _launch(lambda: igemm_dgrad(dy, wt, (H, H), s, p, k, k, out=out, accumulate=accumulate, tile=tile, epi=2))
    torch.cuda.synchronize()
    want = base.double() + ref
    bad = (out.double() != want).sum().item()
    assert bad == 0, f"{bad} of {want.numel()} elements differ, first at {(out.double() != want).nonzero()[0].tolist()}"


@functools.lru_cache(maxsize=1)
def _dgrad_case(shape):
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    d = ternary_density(k * k * Co)
    dy = ternary((N, OH, OH, Co), d, 1, DEV)
    w = ternary((Co, k, k, Ci), d, 2, DEV)
    ref = dgrad_ref(dy, w, (H, H), s, p)
    assert_out_exact(ref)
    assert ref.any()
    return dy, w.permute(3, 1, 2, 0).contiguous(), ref  # wt [Ci][KH][KW][Co]
