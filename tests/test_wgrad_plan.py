"""The weight-gradient launchers' split-K planner (csrc/kernels/conv_wgrad_plan.h, exported from the host runtime as
imr_wgrad_plan) against transcriptions of the three formulas it replaced -- the register-staged launcher's, the
LDS-DMA launcher's (2-byte operands) and the fp8 launcher's (1-byte operands) -- and its invariants, without a GPU.

The subtle part is the loop that halves a split until its dY rows and X images stay below 2^31 bytes (the kernels
address them by 32-bit offsets from the split's base); on the GPU only tests/test_large_tensors_gpu.py reaches it.
"""

import ctypes as C
import itertools

import pytest

from imagent_amd.ops import _lib

LIM = 1 << 31


@pytest.fixture(scope="module", autouse=True)
def _build():
    from imagent_amd import build
    build.build_runtime()


def plan(M, ntiles, BR, target, splits, row_bytes=0, ohw=1, img_bytes=0):
    out = (C.c_int32 * 2)()
    assert _lib.runtime().imr_wgrad_plan(M, ntiles, BR, target, splits, row_bytes, ohw, img_bytes, out) == 0
    return out[0], out[1]


# ---- the launchers' formulas before the shared planner, line by line
def old_staged(M, ntiles, BR, target, splits):
    if splits <= 0:
        want = (target + ntiles - 1) // ntiles
        maxs = (M + 4 * BR - 1) // (4 * BR)
        splits = max(1, min(want, maxs))
    mps = (M + splits - 1) // splits
    mps = (mps + BR - 1) // BR * BR
    return (M + mps - 1) // mps, mps


def old_v3(M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci):
    """launch_wgrad_v3 (bf16 operands; target 512, or the wide tile's 256); also returns how often it halved"""
    if splits <= 0:
        want = (target + ntiles - 1) // ntiles
        maxs = (M + 4 * BR - 1) // (4 * BR)
        splits = max(1, min(want, maxs))
    mps = (M + splits - 1) // splits
    mps = (mps + BR - 1) // BR * BR
    ohw, img = OH * OW, H * W * Ci * 2
    halved = 0
    while mps > BR and (mps * Co * 2 >= LIM or (mps // ohw + 2) * img >= LIM):
        mps = (mps // 2 + BR - 1) // BR * BR
        halved += 1
    splits = (M + mps - 1) // mps
    return splits, mps, halved


def old_fp8(M, ntiles, BR, splits, Co, OH, OW, H, W, Ci):
    """launch_wgrad_fp8 (1-byte operands, 512 blocks); also returns how often it halved"""
    if splits <= 0:
        want = (512 + ntiles - 1) // ntiles
        maxs = (M + 4 * BR - 1) // (4 * BR)
        splits = max(1, min(want, maxs))
    mps = (M + splits - 1) // splits
    mps = (mps + BR - 1) // BR * BR
    ohw, img = OH * OW, H * W * Ci
    halved = 0
    while mps > BR and (mps * Co >= LIM or (mps // ohw + 2) * img >= LIM):
        mps = (mps // 2 + BR - 1) // BR * BR
        halved += 1
    splits = (M + mps - 1) // mps
    return splits, mps, halved


def old_lds_dma(M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci, eb):
    if eb == 2:
        return old_v3(M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci)
    assert target == 512
    return old_fp8(M, ntiles, BR, splits, Co, OH, OW, H, W, Ci)


# (Ci, H, Co, k, stride, pad): every ResNet-50 conv (the stem as its padded 4-channel form, K = 7 x 32)
R50 = [(4, 224, 64, 7, 2, 3),
       (64, 56, 64, 1, 1, 0), (64, 56, 64, 3, 1, 1), (64, 56, 256, 1, 1, 0), (256, 56, 64, 1, 1, 0),
       (256, 56, 128, 1, 1, 0), (128, 56, 128, 3, 2, 1), (128, 28, 512, 1, 1, 0), (256, 56, 512, 1, 2, 0),
       (512, 28, 128, 1, 1, 0), (128, 28, 128, 3, 1, 1),
       (512, 28, 256, 1, 1, 0), (256, 28, 256, 3, 2, 1), (256, 14, 1024, 1, 1, 0), (512, 28, 1024, 1, 2, 0),
       (1024, 14, 256, 1, 1, 0), (256, 14, 256, 3, 1, 1),
       (1024, 14, 512, 1, 1, 0), (512, 14, 512, 3, 2, 1), (512, 7, 2048, 1, 1, 0), (1024, 14, 2048, 1, 2, 0),
       (2048, 7, 512, 1, 1, 0), (512, 7, 512, 3, 1, 1)]
# (N, Ci, H, Co, k, stride, pad): the shapes of tests/test_wgrad_exact_gpu.py, and test_wgrad_past_2gb's 1x1
SMALL = [(37, 72, 11, 200, 3, 2, 1), (29, 64, 13, 64, 3, 1, 1), (23, 96, 13, 136, 1, 1, 0), (9, 64, 10, 128, 3, 1, 1),
         (9, 128, 10, 256, 1, 1, 0), (70, 128, 9, 128, 3, 2, 1), (41, 256, 7, 128, 3, 1, 1), (33, 64, 11, 256, 1, 1, 0),
         (33, 256, 9, 64, 1, 1, 0), (19, 128, 10, 256, 1, 2, 0), (70, 256, 9, 256, 3, 2, 1), (50, 256, 11, 512, 1, 1, 0),
         (40, 512, 7, 256, 3, 1, 1), (2048, 256, 6, 256, 3, 2, 1), (2047, 256, 6, 256, 3, 2, 1),
         (300, 128, 9, 128, 3, 2, 1), (120, 256, 12, 128, 3, 1, 1), (3, 4, 224, 64, 7, 2, 3), (5, 4, 32, 64, 7, 2, 3)]
PAST_2GB = (44000, 256, 14, 256, 1, 1, 0)


def _shapes():
    for n in (256, 2048, 4096):
        for s in R50:
            yield (n,) + s
    yield from SMALL
    yield PAST_2GB


def _cases():
    """(M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci) over tiles 128 x 128 and 256 x 256 and the launchers'
    block targets"""
    for (N, Ci, H, Co, k, s, p), splits, BR in itertools.product(_shapes(), (0, 1, 5), (32, 64, 128)):
        OH = (H + 2 * p - k) // s + 1
        K = k * 32 if Ci == 4 else k * k * Ci
        for tile, targets in ((128, (512, 768, 1024, 1280)), (256, (256,))):
            ntiles = -(-Co // tile) * -(-K // tile)
            for target in targets:
                yield N * OH * OH, ntiles, BR, target, splits, Co, OH, OH, H, H, Ci


def _invariants(M, BR, splits, mps):
    assert mps % BR == 0
    assert (splits - 1) * mps < M <= splits * mps


def test_plan_without_limits_matches_register_staged_formula():
    n = 0
    for M, ntiles, BR, target, splits, *_ in _cases():
        got = plan(M, ntiles, BR, target, splits)
        assert got == old_staged(M, ntiles, BR, target, splits), (M, ntiles, BR, target, splits)
        _invariants(M, BR, *got)
        n += 1
    assert n > 3000


@pytest.mark.parametrize("eb", [1, 2])
def test_plan_with_limits_matches_lds_dma_formulas(eb):
    halved_cases = 0
    for M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci in _cases():
        if eb == 1 and target != 512:
            continue  # (launch_wgrad_fp8's one target)
        row, ohw, img = Co * eb, OH * OW, H * W * Ci * eb
        got = plan(M, ntiles, BR, target, splits, row, ohw, img)
        *want, halved = old_lds_dma(M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci, eb)
        assert got == tuple(want), (M, ntiles, BR, target, splits, Co, OH, OW, H, W, Ci)
        sp, mps = got
        _invariants(M, BR, sp, mps)
        assert mps == BR or (mps * row < LIM and (mps // ohw + 2) * img < LIM)
        halved_cases += halved > 0
    assert halved_cases > 0  # the grid reaches the halving loop


def test_plan_halves_one_split_past_2gb():
    """test_wgrad_past_2gb's 1x1: 44,000 images of 14 x 14 x 256 bf16 (4.4 GB per operand) in one requested split."""
    N, Ci, H, Co, _, _, _ = PAST_2GB
    M = N * H * H
    for BR in (32, 64, 128):
        assert old_lds_dma(M, 4, BR, 512, 1, Co, H, H, H, H, Ci, 2)[2] >= 1
        sp, mps = plan(M, 4, BR, 512, 1, Co * 2, H * H, H * H * Ci * 2)
        assert sp > 1 and mps * Co * 2 < LIM and (mps // (H * H) + 2) * H * H * Ci * 2 < LIM
        assert plan(M, 4, BR, 512, 1) == (1, -(-M // BR) * BR)  # no limits given: the one split stays


def test_plan_rejects_bad_arguments():
    out = (C.c_int32 * 2)()
    f = _lib.runtime().imr_wgrad_plan
    assert f(0, 1, 64, 512, 0, 0, 1, 0, out) == -1
    assert f(100, 0, 64, 512, 0, 0, 1, 0, out) == -1
    assert f(100, 1, 0, 512, 0, 0, 1, 0, out) == -1
    assert f(100, 1, 64, 512, 0, 512, 0, 1024, out) == -1
