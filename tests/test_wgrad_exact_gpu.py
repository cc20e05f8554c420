"""Bit-exact weight gradients: every wgrad kernel on integer operands must EQUAL the fp64 reference.

Operands are uniform integers in [-3, 3] (exact in bf16, products exact in fp32), and each case first checks on the
reference alone that the weight gradient of |dY| and |X| stays below 2^22: then every partial sum -- MFMA
accumulation, wave reductions, split-K atomics, in any order -- is an exact fp32 integer, and one missing, doubled or
misplaced pixel row is an inequality (tests/exact_ref.py; tests/test_exact_ref.py shows that a relative L2 check does
not see it). Every case runs with dW zero and with dW pre-filled with random integers (+=), and with splits 0, 1
and 5 where the entry takes a split count. Shapes are (N, Ci, H, Co, k, stride, pad).

Measured results and the kernels the default dispatch launched: profiles/exact_tests.md.
"""

import functools

import pytest
import torch

from exact_ref import assert_wgrad_exact, ints, kernel_names, out_size, short_names, stem_form, wgrad_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLITS = (0, 1, 5)


def _id(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=4)
def _case(shape, H2=None):
    """(dy, x, fp64 reference) of a shape, shared by the tests of one shape and never modified; the exactness
    precondition is checked here, on the reference."""
    N, Ci, H, Co, k, s, p = shape
    W = H if H2 is None else H2
    dy = ints((N, out_size(H, k, s, p), out_size(W, k, s, p), Co), -3, 3, 1, DEV)
    x = ints((N, H, W, Ci), -3, 3, 2, DEV)
    assert_wgrad_exact(dy, x, k, s, p, extra=8)
    return dy, x, wgrad_ref(dy, x, k, s, p)


def _bases(shape, seed=3):
    """dW before the launch: zero, and random integers in [-8, 8]."""
    return [torch.zeros(shape, device=DEV), ints(shape, -8, 8, seed, DEV, torch.float32)]


def _run(dy, x, ref, shape, splits_set=SPLITS, **kw):
    from imagent_amd.ops.conv import igemm_wgrad
    _, _, _, _, k, s, p = shape
    for splits in splits_set:
        for base in _bases(ref.shape):
            dw = base.clone()
            igemm_wgrad(dy, x, dw, s, p, k, k, splits=splits, **kw)
            torch.cuda.synchronize()
            want = base.double() + ref
            bad = (dw.double() != want).sum().item()
            assert bad == 0, f"splits {splits}, dW {'pre-filled' if base.any() else 'zero'}: {bad} of " \
                             f"{want.numel()} elements differ, max |diff| {(dw.double() - want).abs().max().item()}"


# ---- register-staged kernel: ragged Co and K with M = 1332; the 64-wide tile with 32-row stages; a 1x1
@pytest.mark.parametrize("shape", [(37, 72, 11, 200, 3, 2, 1), (29, 64, 13, 64, 3, 1, 1), (23, 96, 13, 136, 1, 1, 0)],
                         ids=_id)
def test_wgrad_register_staged(shape):
    dy, x, ref = _case(shape)
    _run(dy, x, ref, shape, variant=-1)


# ---- BN apply + ReLU on the X staging path (XB), default dispatch: padding taps must stay 0 (a positive shift makes a
# transformed padding tap visible)
@pytest.mark.parametrize("shape", [(9, 64, 10, 128, 3, 1, 1), (9, 128, 10, 256, 1, 1, 0)], ids=_id)
def test_wgrad_xbn_operand(shape):
    N, Ci, H, Co, k, s, p = shape
    dy = ints((N, out_size(H, k, s, p), out_size(H, k, s, p), Co), -3, 3, 1, DEV)
    x = ints((N, H, H, Ci), -3, 3, 2, DEV)
    ss = torch.stack([ints((Ci,), 1, 2, 4, DEV, torch.float32), ints((Ci,), -2, 2, 5, DEV, torch.float32)]).contiguous()
    assert (ss[1] > 0).any() and (ss[1] < 0).any()
    h = torch.relu(x.float() * ss[0] + ss[1]).to(torch.bfloat16)  # integers <= 8; the reference pads AFTER this
    assert_wgrad_exact(dy, h, k, s, p, extra=8)
    _run(dy, x, wgrad_ref(dy, h, k, s, p), shape, xbn=ss)


# ---- LDS-DMA loop (conv_wgrad_v3.h): (70, 128, 9, ...) has 25 pixels per image and M = 1750, so 256-row splits start
# mid-image (the per-split image-based descriptor base); Ci / Co = 64 half-used tiles; a strided 1x1
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(70, 128, 9, 128, 3, 2, 1), (41, 256, 7, 128, 3, 1, 1), (33, 64, 11, 256, 1, 1, 0),
                                   (33, 256, 9, 64, 1, 1, 0), (19, 128, 10, 256, 1, 2, 0)], ids=_id)
def test_wgrad_lds_dma(shape, variant):
    dy, x, ref = _case(shape)
    _run(dy, x, ref, shape, variant=variant)


# ---- the 256 x 256 tile on 16 waves
@pytest.mark.parametrize("shape", [(70, 256, 9, 256, 3, 2, 1), (50, 256, 11, 512, 1, 1, 0), (40, 512, 7, 256, 3, 1, 1)],
                         ids=_id)
def test_wgrad_wide_tile(shape):
    dy, x, ref = _case(shape)
    _run(dy, x, ref, shape, variant=6)


# ---- the default dispatch at step size: it keys on N (the wide tile from 2048 images per GPU)
@pytest.mark.parametrize("shape", [(2048, 256, 6, 256, 3, 2, 1), (2048, 256, 4, 512, 1, 1, 0),
                                   (2048, 512, 4, 256, 1, 2, 0), (2048, 512, 7, 512, 3, 1, 1),
                                   (2047, 256, 6, 256, 3, 2, 1)], ids=_id)
def test_wgrad_default_dispatch_at_step_size(shape):
    from imagent_amd.ops.conv import igemm_wgrad
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    dy = ints((N, OH, OH, Co), -3, 3, 1, DEV)
    x = ints((N, H, H, Ci), -3, 3, 2, DEV)
    assert_wgrad_exact(dy, x, k, s, p, extra=8)
    ref = wgrad_ref(dy, x, k, s, p)
    for base in _bases(ref.shape):
        dw = base.clone()
        _, names = kernel_names(lambda: igemm_wgrad(dy, x, dw, s, p, k, k))
        names = short_names(names)
        print(f"wgrad {shape}: {names}")
        tile = "wgrad_v3_kernel<64, 2, 4, 4" if N >= 2048 else "wgrad_v3_kernel<64, 2, 2, 2"
        assert len(names) == 1 and tile in names[0], names
        want = base.double() + ref
        bad = (dw.double() != want).sum().item()
        assert bad == 0, f"{bad} of {want.numel()} elements differ"


# ---- halo-tiled 3x3 (conv_wgrad_halo.h): variant 9 and the default dispatch (which keeps W = 7 off it);
# (N, Ci, H, W, Co)
@pytest.mark.parametrize("shape,variant", [(s, v) for s in [(5, 64, 8, 56, 64), (3, 128, 28, 28, 128),
                                                             (2, 256, 14, 14, 256)] for v in (9, 0)] +
                         [((3, 512, 7, 7, 512), 9)], ids=lambda v: _id(v) if isinstance(v, tuple) else f"v{v}")
def test_wgrad_halo(shape, variant):
    N, Ci, H, W, Co = shape
    full = (N, Ci, H, Co, 3, 1, 1)
    dy, x, ref = _case(full, W)
    _run(dy, x, ref, full, splits_set=(0,), variant=variant)


# ---- the stem: [Co][KH][32] gradient rows (KW taps x 4 channels, zero padded), x with 4 channels, channel 3 zero
def _stem(N, H, seed=1):
    OH = out_size(H, 7, 2, 3)
    dy = ints((N, OH, OH, 64), -3, 3, seed, DEV)
    x = stem_form(ints((N, H, H, 4), -3, 3, seed + 1, DEV))
    return dy, x


def _stem_rows(ref):
    """[Co][7][7][4] -> the [Co][7][32] row layout."""
    rows = torch.zeros(ref.shape[0], 7, 32, dtype=torch.float64, device=ref.device)
    rows[:, :, :28] = ref.reshape(ref.shape[0], 7, 28)
    return rows


@pytest.mark.parametrize("N,H,variant", [(3, 224, 0), (3, 224, -2), (5, 32, 0)],
                         ids=["band224", "register224", "default32"])
def test_wgrad_stem(N, H, variant):
    dy, x = _stem(N, H)
    assert_wgrad_exact(dy, x, 7, 2, 3, extra=8)
    ref = _stem_rows(wgrad_ref(dy, x, 7, 2, 3))
    _run(dy, x, ref, (N, 4, H, 64, 7, 2, 3), splits_set=SPLITS if variant == -2 or H == 32 else (0,),
         stem=True, variant=variant)


def test_stem_wgrad_bnx():
    """The stem BatchNorm's backward apply on the dY staging: bf16(A g + B bnx + c) stays an integer for A in {1, 2},
    B in {-1, 0, 1}, integer c and ternary-range g / bnx."""
    from imagent_amd.ops.conv import stem_wgrad_bnx
    N, H = 3, 224
    OH = out_size(H, 7, 2, 3)
    g = ints((N, OH, OH, 64), -1, 1, 1, DEV)
    bnx = ints((N, OH, OH, 64), -1, 1, 2, DEV)
    x = stem_form(ints((N, H, H, 4), -3, 3, 3, DEV))
    coef = torch.stack([ints((64,), 1, 2, 4, DEV, torch.float32), ints((64,), -1, 1, 5, DEV, torch.float32),
                        ints((64,), -1, 1, 6, DEV, torch.float32)]).contiguous()
    dy = (coef[0] * g.float() + coef[1] * bnx.float() + coef[2]).to(torch.bfloat16)  # |.| <= 4
    assert_wgrad_exact(dy, x, 7, 2, 3, extra=8)
    ref = _stem_rows(wgrad_ref(dy, x, 7, 2, 3))
    for base in _bases(ref.shape):
        gp = base.clone()
        assert stem_wgrad_bnx(g, x, gp, bnx, coef, 2, 3, 7, 7)
        torch.cuda.synchronize()
        assert torch.equal(gp.double(), base.double() + ref)


# ---- G += h2^T h2 (ops/bn_gram.py): one staged operand (p = 128), pixel pairs (p = 64), the plain weight gradient
# otherwise and for an odd M
@pytest.mark.parametrize("p", [64, 128, 256])
@pytest.mark.parametrize("M", [12290, 999])
def test_gram_G(p, M):
    from imagent_amd.ops.bn_gram import gram_G
    h2 = ints((M, 1, 1, p), -2, 2, 1, DEV)
    h = h2.view(M, p).double()
    ref = h.t() @ h
    assert (h.abs().t() @ h.abs()).max().item() + 8 < 2 ** 22
    base = ints((p, p), -8, 8, 2, DEV, torch.float32)
    G = base.clone()
    gram_G(h2, G)
    torch.cuda.synchronize()
    assert torch.equal(G.double(), base.double() + ref)


# ---- fp8 weight gradient: integer-valued e5m2 / e4m3 bytes; the power-of-two scale 2^(e_dy + e_x) is exact
@pytest.mark.parametrize("exps", [(0, 0), (-14, -3)], ids=["e0_0", "e-14_-3"])
@pytest.mark.parametrize("shape", [(300, 128, 9, 128, 3, 2, 1), (120, 256, 12, 128, 3, 1, 1)], ids=_id)
def test_wgrad_fp8(shape, exps):
    from imagent_amd.ops.conv import igemm_wgrad_fp8
    _, _, _, _, k, s, p = shape
    dy, x, ref = _case(shape)
    dy8 = dy.to(torch.float8_e5m2)
    x8 = x.to(torch.float8_e4m3fn)
    assert torch.equal(dy8.double(), dy.double()) and torch.equal(x8.double(), x.double())
    e_dy = torch.tensor([exps[0]], dtype=torch.int32, device=DEV)
    e_x = torch.tensor([exps[1]], dtype=torch.int32, device=DEV)
    scaled = ref * 2.0 ** (exps[0] + exps[1])  # (integer dW + multiples of 2^-17 below 2^6: 23 bits, exact in fp32)
    for splits in SPLITS:
        for base in _bases(ref.shape):
            dw = base.clone()
            assert igemm_wgrad_fp8(dy8.view(torch.uint8), x8.view(torch.uint8), dw, e_dy, e_x, s, p, k, k,
                                   splits=splits)
            torch.cuda.synchronize()
            bad = (dw.double() != base.double() + scaled).sum().item()
            assert bad == 0, f"splits {splits}: {bad} of {dw.numel()} elements differ"


def test_negative_control_one_lost_pixel_is_seen():
    """The kernel gets dY with its last pixel zeroed; the reference is of the full operands: NOT equal."""
    from imagent_amd.ops.conv import igemm_wgrad
    shape = (70, 128, 9, 128, 3, 2, 1)
    dy, x, ref = _case(shape)
    lost = dy.clone()
    assert lost[-1, -1, -1].any()
    lost[-1, -1, -1] = 0
    dw = torch.zeros(ref.shape, device=DEV)
    igemm_wgrad(lost, x, dw, 2, 1, 3, 3, variant=1)
    torch.cuda.synchronize()
    assert not torch.equal(dw.double(), ref)
    assert torch.equal(dw.double(), wgrad_ref(lost, x, 3, 2, 1))
