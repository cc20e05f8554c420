"""Bit-exact fused epilogues: the fused-output epilogue of the streaming 1x1 kernel (affine, residual (+ scale), ReLU,
mask bits, e4m3 copy), every IG_BNBWD dgrad epilogue (streaming, tiled direct / LDS-staged, v3, halo, fp8, the
Gram-form two-segment dgrad), the ``xbn`` operand path of the forwards and the fp8 forward / dgrad must EQUAL a plain
fp64 reference -- no tolerance anywhere.

Operands are integers (exact_ref.ternary / ints) and the BatchNorm constants dyadic (exact_ref.bn_consts: means and
shifts multiples of 0.5, rstd / gamma / scales in {+-0.5, +-1, +-2}), so (x - mean) * rstd, fma(x, sc, sh), the ReLU
decision and every partial sum are exact in fp32 in any order; the kernels round the conv product to bf16 at different
points and must still all give the reference's bits. Every exactness condition (the output equals its bf16 rounding;
each channel's sum |term| below 2^23 quanta) and every boundary element a case is meant to contain (exact-zero
pre-activations, both mask values, a ragged last group, three passes of the persistent loop) is asserted on the
REFERENCE or on the launch geometry, never on a kernel's output.

Sizes: the streaming kernel's cases run at a ragged small size (M % 16 != 0; one with M = 9) and at a large one where
every wave makes at least three passes of its persistent loop (launch_stream1: npb = min(resident / nsl,
ceil(ngroups / (NW * D))) with two resident blocks per CU and NW = 4, so ngroups >= 3 * 3 * 4 * (2 * CUs / nsl)):
the refill of the prefetch ring, the epilogue operands issued a pass ahead and the counted waits between passes then
run on data checked to equality. The large cases use integer means / shifts, rstd = 1 and lower ternary densities so
the sum conditions hold, and compute the reference in image chunks. Shapes are (N, Ci, H, Co, k, stride, pad) of the
convolution (a dgrad's output has Ci channels). Measured results: profiles/exact_tests.md.
"""

import re
import types

import pytest
import torch

from exact_ref import (DYADIC, abs_sums, assert_bf16_exact, assert_out_exact, assert_sums_exact, bn_consts, bnb_ref,
                       bnb_terms, dgrad_ref, dyadic, e4m3_ref, fused_out_ref, fwd_ref, halves, ints, kernel_names,
                       mask_bytes, out_size, shifted_stats_ref, short_names, stem_form, ternary, ternary_density)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NW = 4  # waves per block of the streaming kernel (conv_stream.hip stream_nw)


def _id(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _launch(fn):
    """fn(), with an existing -10x / -12x return (a combination the entry does not take) as a skip."""
    try:
        return fn()
    except RuntimeError as e:
        m = re.search(r"failed with code (-1[02]\d)$", str(e))
        if m is None:
            raise
        pytest.skip(f"unsupported combination ({m.group(1)})")


def _eq(what, got, want):
    ne = got != want
    bad = ne.sum().item()
    assert bad == 0, f"{what}: {bad} of {want.numel()} elements differ, first at {ne.nonzero()[0].tolist()}"


@pytest.fixture
def stream_toggle():
    from imagent_amd.ops import conv
    yield conv.set_stream
    conv.set_stream(True)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _chunks(N, hw, px=1 << 15):
    """Image ranges of at most ~px pixels: the fp64 reference is formed chunk by chunk."""
    step = max(1, px // hw)
    for i in range(0, N, step):
        yield slice(i, min(N, i + step))


def _big(nsl, H=14):
    """(N, H) of a large case: ngroups >= 3 * 3 * 4 * (2 * CUs / nsl) 16-pixel groups, the last one ragged."""
    groups = 3 * 3 * NW * (2 * _cus() // nsl)
    N = -(-groups * 16 // (H * H)) + 1
    while (N * H * H) % 16 == 0:
        N += 1
    return N, H


def _size(size, nsl):
    return {"tiny": (1, 3), "ragged": (5, 13)}[size] if size != "big" else _big(nsl)


def _stream_args(names):
    """(K, BN, D, MODE) of the conv_stream_kernel instances among the launched kernels."""
    out = [tuple(map(int, m.groups())) for m in
           (re.search(r"conv_stream_kernel<(\d+), (\d+), (\d+), (\d+)", n) for n in names) if m]
    return sorted(set(out))


def _check_geometry(M, Nout, names, size, mode=None):
    """The launch is one streaming kernel (of the given MODE); ragged last group; at the large size every wave
    makes >= 3 passes of the persistent loop (two resident blocks per CU)."""
    st = _stream_args(names)
    assert len(st) == 1, names
    K, BN, D, MODE = st[0]
    assert mode is None or MODE == mode, (st, mode)
    assert M % 16 != 0
    if size == "big":
        nsl, ngroups = Nout // BN, (M + 15) // 16
        npb = max(1, min(2 * _cus() // nsl, (ngroups + NW * D - 1) // (NW * D)))
        assert ngroups // (npb * NW * D) >= 3, (ngroups, npb, D)
    return st[0]


# ===================================================================== fused output (conv_stream_kernel MODE 4)

def _fwd_operands(N, H, K, C, d=None):
    d = ternary_density(K) if d is None else d
    return ternary((N, H, H, K), d, 1, DEV), ternary((C, 1, 1, K), d, 2, DEV)


FUSED = [((64, 256), "tiny"), ((64, 256), "ragged"), ((64, 256), "big"), ((128, 512), "ragged"), ((128, 512), "big")]


@pytest.mark.parametrize("q8", [False, True], ids=["noq8", "q8out"])
@pytest.mark.parametrize("res_scale", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("kc,size", FUSED, ids=[f"{_id(k)}-{s}" for k, s in FUSED])
def test_fused_output(kc, size, res_scale, q8):
    """affine + res (+ res_scale) + relu + maskout (+ q8out at exponent -1): out, the mask bytes, the e4m3 bytes
    and the amax row."""
    from imagent_amd.ops.conv import igemm_fwd
    K, C = kc
    N, H = _size(size, 1 if K == 64 else 4)
    x, w = _fwd_operands(N, H, K, C)
    aff = torch.stack([dyadic(C, 10, DYADIC, DEV), halves(C, -2, 2, 11, DEV)]).contiguous()
    res = ints((N, H, H, C), -3, 3, 12, DEV)
    rsc = dyadic(C, 13, DYADIC, DEV) if res_scale else None
    out = torch.full_like(res, float("nan"))
    ym = torch.zeros(out.numel() // 8, device=DEV, dtype=torch.uint8)
    y8 = e8 = a8 = None
    if q8:
        y8 = torch.zeros(out.shape, device=DEV, dtype=torch.uint8)
        e8 = torch.tensor([-1], device=DEV, dtype=torch.int32)
        a8 = torch.zeros(32, device=DEV)
    _, names = kernel_names(lambda: igemm_fwd(x, w, 1, 0, 1, 1, out=out, affine=aff, relu=True, res=res, maskout=ym,
                                              res_scale=rsc, q8out=(y8, e8, a8) if q8 else None))
    print(f"fused output {kc} {size}: {short_names(names)}")
    if size != "tiny":
        _check_geometry(N * H * H, C, names, size, mode=4)
    else:
        assert N * H * H < 16 and _stream_args(names)[0][3] == 4
    ymv = ym.view(N, -1)
    zeros = neg = pos = rounded = 0
    amax = 0.0
    for sl in _chunks(N, H * H):
        ref, pre = fused_out_ref(fwd_ref(x[sl], w, 1, 0), aff, res[sl], rsc, relu=True, pre=True)
        assert_bf16_exact(ref)
        zeros, neg, pos = zeros + (pre == 0).sum().item(), neg + (pre < 0).sum().item(), pos + (pre > 0).sum().item()
        _eq("out", out[sl].double(), ref)
        _eq("mask bytes", ymv[sl].reshape(-1), mask_bytes(ref > 0))
        if q8:
            q, am = e4m3_ref(ref, -1)
            rounded += (q.view(torch.float8_e4m3fn).float().double() / 2 != ref).sum().item()
            amax = max(amax, am)
            _eq("e4m3 bytes", y8[sl].reshape(-1), q.reshape(-1))
    assert zeros > 0 and neg > 0 and pos > 0, (zeros, neg, pos)  # the reference has the boundary elements
    if q8:
        assert rounded > 0 and amax > 0
        assert a8.max().item() == amax, (a8.max().item(), amax)


HALO112 = (1, 64, 112, 64, 3, 1, 1)  # halo3x3_kernel<112, 2, EPI>: layer 1 of a 448-pixel input
STEM = (2, 4, 224, 64, 7, 2, 3)      # the 224-px 7x7 / 2 stem in stem_form
EVAL = [("conv_stream", (5, 64, 13, 256, 1, 1, 0), 0, 0), ("conv_stream", (5, 128, 13, 512, 1, 1, 0), 0, 0),
        ("conv_stream", (5, 256, 13, 512, 1, 1, 0), 0, 0), ("conv_stream", "big", 0, 0),
        ("halo3x3", (3, 64, 56, 64, 3, 1, 1), 0, 0)] + \
       [("igemm", (7, 64, 14, 128, 3, 1, 1), t, e) for t in (2, 4, 8) for e in (0, 1, 2)] + \
       [("igemm", (7, 64, 14, 128, 3, 1, 1), 18, e) for e in (0, 2)] + \
       [("halo3x3_kernel<112, 2, 0>", HALO112, 0, 0), ("stem_band_kernel<4>", STEM, 0, 0),
        ("conv_stream", STEM, 23, 0)]  # (tile 18: the v3 loop has the staged epilogue only)
EVAL_IDS = [f"{f.split('<')[0]}-{_id(s)}-t{t}-e{e}" for f, s, t, e in EVAL]
# Nonzero density of the added cases (the others: ternary_density(K)). The output relu(y * sc + sh) with |sc| <= 2 and
# half-integer sh is a multiple of 0.5, exact in bf16 below 128, so |y| <= 62 is needed. Halo K = 576 at d = 0.35:
# y has variance 71, 62 = 7.4 sigma (at 0.5: 5.2 sigma of 8e5 elements). Stem K = 147 at d = 0.5: variance 37, 10 sigma
EVAL_DENSITY = {HALO112: 0.35, STEM: 0.5}


@pytest.mark.parametrize("family,shape,tile,epi", EVAL, ids=EVAL_IDS)
def test_eval_affine_relu(family, shape, tile, epi):
    """affine + relu alone (the eval epilogue) on the streaming, tiled (direct / staged), halo and stem kernels."""
    from imagent_amd.ops.conv import igemm_fwd
    big = shape == "big"
    if big:
        shape = (_big(1)[0], 64, 14, 256, 1, 1, 0)
    N, Ci, H, Co, k, s, p = shape
    stem = shape == STEM
    d = EVAL_DENSITY.get(shape, ternary_density(k * k * Ci))
    x, w = ternary((N, H, H, Ci), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    wk = w
    if stem:  # channel 3 zero, [Co][KH][32] weight rows
        x, w = stem_form(x), stem_form(w)
        wk = torch.zeros(Co, k, 32, dtype=torch.bfloat16, device=DEV)
        wk[:, :, :k * Ci] = w.reshape(Co, k, k * Ci)
    aff = torch.stack([dyadic(Co, 10, DYADIC, DEV), halves(Co, -2, 2, 11, DEV)]).contiguous()
    y, names = _launch(lambda: kernel_names(lambda: igemm_fwd(x, wk, s, p, k, k, affine=aff, relu=True, tile=tile,
                                                              epi=epi, stem=stem)))
    print(f"eval {shape} tile {tile} epi {epi}: {short_names(names)}")
    assert names and all(family in n for n in names), names
    if stem and family == "conv_stream":
        assert _stream_args(names) == [(224, 64, 2, 0)], names
    elif family == "conv_stream":
        _check_geometry(N * H * H, Co, names, "big" if big else "ragged", mode=0)
    zeros = 0
    for sl in _chunks(N, H * H):
        ref, pre = fused_out_ref(fwd_ref(x[sl], w, s, p), aff, relu=True, pre=True)
        assert_bf16_exact(ref)
        zeros += (pre == 0).sum().item()
        _eq("out", y[sl].double(), ref)
    assert zeros > 0


# ===================================================================== IG_BNBWD dgrads

def _bn(C, seed, integer=False):
    """What BNBwdFuse reads of a BatchNorm: weight, bias, work.save (mean, rstd), work.scratch (the slab)."""
    from imagent_amd.ops import _lib
    save, gamma, beta = bn_consts(C, seed, DEV, integer)
    nbw = _lib.kernels().imk_bn_bwd_scratch_floats(1)
    work = types.SimpleNamespace(save=save, scratch=torch.zeros(nbw * C, device=DEV))
    return types.SimpleNamespace(weight=gamma, bias=beta, work=work)


VARIANTS = ["y_mask", "x_mask", "x2", "accum"]


def _bnb_operands(shape, variant, big=False):
    """dy, w [Co][k][k][Ci], x, mask bits, x2, old, bn, bn2 of a dgrad with the fused BN backward."""
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    K = k * k * Co
    d = min(0.5, (16.0 / K) ** 0.5) if big else ternary_density(K)
    o = types.SimpleNamespace()
    o.dy, o.w = ternary((N, OH, OH, Co), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    o.wt = o.w.permute(3, 1, 2, 0).contiguous()
    o.x = ints((N, H, H, Ci), -3, 3, 3, DEV)
    o.bits = mask_bytes(ints((N, H, H, Ci), 0, 1, 4, DEV, torch.bool)) if variant != "x_mask" else None
    o.x2 = ints((N, H, H, Ci), -3, 3, 5, DEV) if variant == "x2" else None
    o.old = ints((N, H, H, Ci), -8, 8, 6, DEV) if variant == "accum" else None
    o.bn, o.bn2 = _bn(Ci, 20, big), (_bn(Ci, 30, big) if variant == "x2" else None)
    o.quantum = 1.0 if big else 0.25
    return o


def _bnb_check(o, shape, got, bias=None, raw=None):
    """The stored gradient and the slab rows against bnb_ref, in image chunks; preconditions on the reference."""
    N, Ci, H, Co, k, s, p = shape
    bn, bn2 = o.bn, o.bn2
    save2 = bn2.work.save if bn2 is not None else None
    bits = o.bits.view(N, -1) if o.bits is not None else None
    slab = torch.zeros(3, Ci, dtype=torch.float64, device=DEV)
    sums = torch.zeros(3 if o.x2 is not None else 2, Ci, dtype=torch.float64, device=DEV)
    kept = dropped = edge = 0
    for sl in _chunks(N, H * H):
        g = dgrad_ref(o.dy[sl], o.w, (H, H), s, p) if raw is None else raw(sl)
        xs = o.x[sl] if o.x is not None else None
        gm, sb = bnb_ref(g, old=o.old[sl] if o.old is not None else None, x=xs, save=bn.work.save,
                         gamma=bn.weight, beta=bn.bias, ymask=bits[sl].reshape(-1) if bits is not None else None,
                         x2=o.x2[sl] if o.x2 is not None else None, save2=save2, bias=bias)
        assert_bf16_exact(gm)
        sums += abs_sums(bnb_terms(gm, xs, bn.work.save, o.x2[sl] if o.x2 is not None else None, save2), o.quantum)
        slab += sb
        kept, dropped = kept + (gm != 0).sum().item(), dropped + ((gm == 0) & (g != 0)).sum().item()
        if bits is None:
            sc = bn.weight.double() * bn.work.save[1].double()
            edge += (xs.double() * sc + (bn.bias.double() - bn.work.save[0].double() * sc) == 0).sum().item()
        _eq("stored gradient", got[sl].double(), gm)
    assert_sums_exact(None, o.quantum, sums=sums)
    assert kept > 0 and dropped > 0, (kept, dropped)  # both mask values decide an element
    assert bits is not None or edge > 0               # from-x mask: fma(x, sc, sh) == 0 occurs (> versus >=)
    have = bn.work.scratch[:32 * 3 * Ci].view(32, 3, Ci).double().sum(0)
    for q, name in enumerate(("sum(g xhat)", "sum(g)", "sum(g xhat2)")):
        assert torch.equal(have[q], slab[q]), \
            f"slab row {q} {name}: {(have[q] != slab[q]).sum().item()} of {Ci} channels differ, " \
            f"max |diff| {(have[q] - slab[q]).abs().max().item()}"
    assert slab[0].any() and slab[1].any() and (o.x2 is None or slab[2].any())


def _bnb_run(o, shape, tile=0, epi=0, **kw):
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    N, Ci, H, Co, k, s, p = shape
    f = BNBwdFuse(o.x, o.bn, y=o.bits, x2=o.x2, bn2=o.bn2)
    out = o.old.clone() if o.old is not None else None
    return _launch(lambda: kernel_names(lambda: igemm_dgrad(o.dy, o.wt, (H, H), s, p, k, k, out=out,
                                                            accumulate=o.old is not None, bnb=f, tile=tile, epi=epi,
                                                            **kw)))


# dgrad GEMM K = Co into Nout = Ci channels: (Ci, Co) pairs. K = 64 / 128 / 256 into 64 / 128 / 256 / 512 reach the
# from-bits (1), from-x (2) and second-branch (3) modes on 128- and 64-channel slices; the second-branch form of K = 256
# into > 128 channels stays on 64-channel slices, into <= 128 channels it is the tiled kernels'
STREAM_BNB = [(256, 64), (512, 128), (64, 64), (128, 128), (128, 64), (64, 256), (128, 256), (512, 256)]
STREAM_BNB_BIG = [(256, 64), (512, 128), (64, 256), (512, 256)]
MODE = {"y_mask": 1, "x_mask": 2, "x2": 3, "accum": 1}


def _stream_bnb(cc, variant, size, tile=0):
    Ci, Co = cc
    on_stream = not (variant == "x2" and Co == 256 and Ci <= 128)
    # slice width: 128 where it divides Nout; K = 256 into <= 128 channels and K = 256 with the second branch on 64
    bn_w = 64 if (tile == 22 or Ci % 128 or (Co == 256 and (Ci <= 128 or variant == "x2"))) else 128
    N, H = _size(size, Ci // bn_w)
    shape = (N, Ci, H, Co, 1, 1, 0)
    o = _bnb_operands(shape, variant, big=size == "big")
    got, names = _bnb_run(o, shape, tile=tile)
    print(f"bnb dgrad {shape} {variant} tile {tile}: {short_names(names)}")
    if on_stream:
        K, BN, D, _ = _check_geometry(N * H * H, Ci, names, size, mode=MODE[variant])
        assert (K, BN) == (Co, bn_w), (K, BN, names)
    else:
        assert names and all("igemm" in n for n in names), names
    _bnb_check(o, shape, got)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", STREAM_BNB, ids=_id)
def test_stream_dgrad_bnb(cc, variant):
    _stream_bnb(cc, variant, "ragged")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", STREAM_BNB_BIG, ids=_id)
def test_stream_dgrad_bnb_three_passes(cc, variant):
    _stream_bnb(cc, variant, "big")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cc", [(256, 64), (512, 128), (512, 256)], ids=_id)
def test_stream_dgrad_bnb_64_channel_slices(cc, variant):
    _stream_bnb(cc, variant, "ragged", tile=22)


def test_stream_dgrad_bnb_less_than_one_group():
    _stream_bnb((256, 64), "y_mask", "tiny")
    _stream_bnb((256, 64), "x_mask", "tiny")


TILED = [(t, e) for t in (2, 4, 8) for e in (1, 2)] + [(t, 0) for t in (17, 18, 19)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tile,epi", TILED, ids=[f"t{t}-e{e}" for t, e in TILED])
def test_tiled_dgrad_bnb(tile, epi, variant, stream_toggle):
    """The tiled kernels' own IG_BNBWD epilogue, direct (epi 1) and LDS-staged (epi 2), and the v3 loop's."""
    stream_toggle(False)
    shape = (7, 128, 14, 128, 3, 1, 1)
    o = _bnb_operands(shape, variant)
    got, names = _bnb_run(o, shape, tile=tile, epi=epi)
    print(f"bnb dgrad {shape} {variant} tile {tile} epi {epi}: {short_names(names)}")
    assert names and all("igemm" in n for n in names), names
    assert (tile >= 17) == all("igemm_v3" in n for n in names), names
    _bnb_check(o, shape, got)


@pytest.mark.parametrize("variant", VARIANTS)
def test_stride2_dgrad_bnb(variant):
    """3x3 stride 2 on an odd image: four parity launches of different sizes into one slab, the non-dense epilogue
    (no operand prefetch)."""
    shape = (5, 128, 13, 256, 3, 2, 1)
    o = _bnb_operands(shape, variant)
    got, names = _bnb_run(o, shape)
    print(f"bnb dgrad {shape} {variant}: {len(names)} launches {short_names(names)}")
    assert len(names) == 4 and all("igemm" in n for n in names), names
    _bnb_check(o, shape, got)


HALO_BNB = [((3, 64, 56, 64, 3, 1, 1), v) for v in VARIANTS] + [(HALO112, v) for v in VARIANTS]


@pytest.mark.parametrize("shape,variant", HALO_BNB, ids=[v if s[2] == 56 else f"{v}-w{s[2]}" for s, v in HALO_BNB])
def test_halo_dgrad_bnb(shape, variant):
    """halo3x3_kernel<56, 4, EPI> and <112, 2, EPI> (EPI 1, with x2: 2)."""
    o = _bnb_operands(shape, variant)
    got, names = _bnb_run(o, shape)
    print(f"bnb dgrad {shape} {variant}: {short_names(names)}")
    assert names and all(f"halo3x3_kernel<{shape[2]}, " in n for n in names), names
    _bnb_check(o, shape, got)


@pytest.mark.parametrize("stream", [True, False], ids=["stream", "tiled"])
@pytest.mark.parametrize("variant", ["y_mask", "x_mask"])
def test_sparse_then_accumulate_sub2_bnb(variant, stream, stream_toggle):
    """A bottleneck's downsample backward: the stride-2 1x1 dgrad writes only the even pixels (``sparse``; the others
    hold NaN here), conv1's dgrad accumulates with ``old_sub2`` and the fused BN backward."""
    from imagent_amd.ops.conv import igemm_dgrad
    stream_toggle(stream)
    N, H, cmid, cin = 3, 14, 64, 256
    shape = (N, cin, H, cmid, 1, 1, 0)
    o = _bnb_operands(shape, variant)
    dds = 0.25
    g_ds, w_ds = ternary((N, H // 2, H // 2, 2 * cin), dds, 7, DEV), ternary((2 * cin, 1, 1, cin), dds, 8, DEV)
    old = dgrad_ref(g_ds, w_ds, (H, H), 2, 0)
    assert_out_exact(old)
    assert old[:, ::2, ::2].any() and not old[:, 1::2].any() and not old[:, :, 1::2].any()
    out = torch.full((N, H, H, cin), float("nan"), device=DEV, dtype=torch.bfloat16)
    igemm_dgrad(g_ds, w_ds.permute(3, 1, 2, 0).contiguous(), (H, H), 2, 0, 1, 1, out=out, sparse=True)
    _eq("sparse dgrad", out[:, ::2, ::2].double(), old[:, ::2, ::2])
    assert torch.isnan(out[:, 1::2].float()).all() and torch.isnan(out[:, :, 1::2].float()).all()
    o.old = out
    got, names = _bnb_run(o, shape, old_sub2=True)
    print(f"bnb dgrad {shape} {variant} accumulate old_sub2: {short_names(names)}")
    assert names and all(("conv_stream" in n) == stream for n in names), names
    o.old = old
    _bnb_check(o, shape, got)


# ===================================================================== Gram-form two-segment dgrad (bn_gram.gram_dgrad)

GRAM = [("stream", 64, 0, "ragged"), ("stream", 64, 0, "big"), ("v3", 64, 18, "ragged"), ("v3", 128, 0, "ragged")]


@pytest.mark.parametrize("variant", ["y_mask", "x_mask", "no_x"])
@pytest.mark.parametrize("form,p,tile,size", GRAM, ids=[f"{f}-p{p}-{s}" for f, p, _, s in GRAM])
def test_gram_two_segment_dgrad(form, p, tile, size, variant):
    """K = [g (4p) | h2 (p)] into p channels with bn2's fused backward and the bias before its mask, filled as
    ops.bn_gram.gram_dgrad fills it: the streaming form (256 + 64 -> 64) and the v3 loop's."""
    import ctypes as C
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import BNBwdFuse, _base_args, _igemm_call
    big = size == "big"
    N, H = _size(size, 1)
    C4 = 4 * p
    shape = (N, p, H, C4, 1, 1, 0)
    o = _bnb_operands(shape, "y_mask" if variant == "no_x" else variant, big=big)
    d = min(0.5, (16.0 / (C4 + p)) ** 0.5) if big else ternary_density(C4 + p)
    g = ternary((N, H, H, C4), d, 1, DEV)
    h2 = ternary((N, H, H, p), d, 7, DEV)
    wcat = ternary((p, C4 + p), d, 8, DEV)
    bias = halves(p, -2, 2, 9, DEV, 1.0 if big else 0.5)
    if variant == "no_x":
        o.x = None
    if not big:
        o.quantum = 0.125  # (g + bias: multiples of 0.5) x (xhat: multiples of 0.25)
    out = torch.full((N, H, H, p), float("nan"), device=DEV, dtype=torch.bfloat16)
    a = _base_args(g.data_ptr(), wcat.data_ptr(), out.data_ptr(), N, H, H, C4, H, H, p, C4 + p, 1)
    a.nth, a.ntw, a.dh0, a.dhs, a.dw0, a.dws = 1, 1, 0, 1, 0, 1
    a.kh0, a.khs, a.kw0, a.kws, a.KW = 0, 1, 0, 1, 1
    a.YH, a.YW, a.sY, a.oy, a.ox, a.ldy = H, H, 1, 0, 0, p
    a.flags = 0
    a.X2, a.C2 = h2.data_ptr(), p
    a.bias = bias.data_ptr()
    BNBwdFuse(o.x, o.bn, y=o.bits).fill(a)
    _, names = _launch(lambda: kernel_names(lambda: _igemm_call(a, tile, _lib.stream_ptr(), "conv dgrad (bn3 gram)")))
    print(f"gram dgrad {shape} {variant} tile {tile}: {short_names(names)}")
    if form == "stream":
        K, BN, D, _ = _check_geometry(N * H * H, p, names, size, mode=2 if variant == "x_mask" else 1)
        assert (K, BN) == (256, 64) and all("64>" in n.split("(")[0] for n in short_names(names)), names
    else:
        assert names and all("igemm_v3" in n for n in names), names
    w1, w2 = wcat[:, :C4].double().t(), wcat[:, C4:].double().t()

    def raw(sl):
        return (g[sl].double().reshape(-1, C4) @ w1 + h2[sl].double().reshape(-1, p) @ w2).view(-1, H, H, p)
    _bnb_check(o, shape, out, bias=bias, raw=raw)


# ===================================================================== xbn forwards

class _Work:
    """A BatchNorm workspace as igemm_fwd(stats=) reads it: the slab and the shift (``save[0]``)."""

    def __init__(self, c, shift):
        from imagent_amd.ops import _lib
        self.slab = torch.zeros(_lib.STAT_SLOTS, 2, c, device=DEV)
        self.save = torch.zeros(2, c, device=DEV)
        self.save[0] = shift


def _check_stats(slab, st_ref):
    have = slab.double().sum(0)
    assert torch.equal(have, st_ref), f"statistics: max |sum diff| {(have[0] - st_ref[0]).abs().max().item()}, " \
                                      f"max |sumsq diff| {(have[1] - st_ref[1]).abs().max().item()}"


def _xbn_consts(K, big=False):
    """(scale, shift) [2][K]: scales in {+-1, +-2} and integer shifts in [-2, 2] (the operand is an integer <= 8); the
    large size: scales +-1 and shifts in [-1, 1] (an integer <= 4, so a channel's sum(y * y) stays below 2^23)."""
    sc = dyadic(K, 4, (-1.0, 1.0) if big else (-2.0, -1.0, 1.0, 2.0), DEV)
    sh = halves(K, -1, 1, 5, DEV, 1.0) if big else halves(K, -2, 2, 5, DEV, 1.0)
    assert (sc < 0).any() and (sc > 0).any() and (sh > 0).any() and (sh < 0).any()
    return torch.stack([sc, sh]).contiguous()


# (K, Nout): <64, 256>, <64, 128> and <128, 128> channel slices; the large size on wider outputs (4 - 5 slices of the
# same instantiations), where three passes need fewer pixels and the sum conditions leave room for a few weights per row
XBN = [((64, 256), "ragged"), ((64, 1024), "big"), ((64, 128), "ragged"), ((64, 640), "big"), ((128, 128), "ragged"),
       ((128, 512), "big"), ((64, 256), "tiny")]


@pytest.mark.parametrize("kc,size", XBN, ids=[f"{_id(k)}-{s}" for k, s in XBN])
def test_stream_fwd_xbn(kc, size):
    """relu(x * scale + shift) on the streaming 1x1's operand load, with statistics: integers x in [-3, 3]."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import igemm_fwd
    K, C = kc
    bn_w = 256 if (K == 64 and C % 256 == 0) else 128
    N, H = _size(size, C // bn_w)
    M = N * H * H
    x = ints((N, H, H, K), -3, 3, 1, DEV)
    ss = _xbn_consts(K, size == "big")
    h = torch.relu(x.float() * ss[0] + ss[1]).to(torch.bfloat16)
    assert h.max().item() <= 8 and torch.equal(h, h.round()) and (h == 0).any()
    # y has variance K d E[h^2] with E[h^2] <= 4.3 (large) / about 12: |y| <= 256 and sum(y * y) < 2^23 with room for
    # the channel with the most weights; both are asserted on the reference below
    dw = min(0.25, 0.1 * 2 ** 23 / (M * K * 4.3))
    w = ternary((C, 1, 1, K), dw, 2, DEV)
    slab = torch.zeros(_lib.STAT_SLOTS, 2, C, device=DEV)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 0, 1, 1, stats=slab, xbn=ss))
    print(f"xbn fwd {kc} {size}: {short_names(names)}")
    if size != "tiny":
        assert _check_geometry(M, C, names, size, mode=0)[:2] == (K, bn_w), names
    assert all("true" in n for n in short_names(names)), names  # the XBN instantiation
    st = torch.zeros(2, C, dtype=torch.float64, device=DEV)
    for sl in _chunks(N, H * H):
        ref = fwd_ref(h[sl], w, 1, 0)
        assert_out_exact(ref)
        st += shifted_stats_ref(ref)
        _eq("y", y[sl].double(), ref)
    assert st[1].max().item() < 2 ** 23 and (st[1] > 0).sum().item() > 0.8 * C
    _check_stats(slab, st)


def test_halo_fwd_xbn():
    """The halo 64 -> 64 3x3 with xbn: a positive shift must not leak into the padding taps (the reference pads
    AFTER the transform)."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import igemm_fwd
    N, H, C = 3, 56, 64
    x = ints((N, H, H, C), -3, 3, 1, DEV)
    ss = _xbn_consts(C)
    h = torch.relu(x.float() * ss[0] + ss[1]).to(torch.bfloat16)
    w = ternary((C, 3, 3, C), 0.025, 2, DEV)  # K = 576, M = 9,408: a channel's sum(y * y) ~ 2^22
    ref = fwd_ref(h, w, 1, 1)
    assert_out_exact(ref)
    st = shifted_stats_ref(ref)
    assert st[1].max().item() < 2 ** 23 and ref.any()
    slab = torch.zeros(_lib.STAT_SLOTS, 2, C, device=DEV)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 1, 3, 3, stats=slab, xbn=ss))
    print(f"xbn fwd halo: {short_names(names)}")
    assert names and all("halo3x3_kernel" in n for n in names), names
    _eq("y", y.double(), ref)
    _check_stats(slab, st)


@pytest.mark.parametrize("xbn", [False, True], ids=["plain", "xbn"])
def test_fwd_shifted_statistics(xbn):
    """A BatchNorm workspace as ``stats`` with a non-zero half-integer ``save``: the slab holds the SHIFTED sums
    sum(y - shift), sum((y - shift)^2)."""
    from imagent_amd.ops.conv import igemm_fwd
    N, H, K, C = 5, 13, 64, 256
    x = ints((N, H, H, K), -3, 3, 1, DEV) if xbn else ternary((N, H, H, K), 0.5, 1, DEV)
    ss = _xbn_consts(K) if xbn else None
    h = torch.relu(x.float() * ss[0] + ss[1]).to(torch.bfloat16) if xbn else x
    w = ternary((C, 1, 1, K), 0.25 if xbn else 0.5, 2, DEV)
    shift = halves(C, -3, 3, 6, DEV)
    assert (shift != shift.round()).any() and (shift != 0).any()
    ref = fwd_ref(h, w, 1, 0)
    assert_out_exact(ref)
    dd = ref - shift.double()
    assert_sums_exact([dd], 0.5)
    assert_sums_exact([dd * dd], 0.25)
    wk = _Work(C, shift)
    y, names = kernel_names(lambda: igemm_fwd(x, w, 1, 0, 1, 1, stats=wk, xbn=ss))
    print(f"shifted statistics {'xbn' if xbn else 'plain'}: {short_names(names)}")
    assert names and all("conv_stream_kernel" in n for n in names), names
    _eq("y", y.double(), ref)
    _check_stats(wk.slab, shifted_stats_ref(ref, shift))
    assert not torch.equal(shifted_stats_ref(ref, shift), shifted_stats_ref(ref))


# ===================================================================== fp8 forward and dgrad

FP8_SHAPES = [(7, 64, 14, 192, 3, 1, 1), (5, 128, 13, 256, 3, 1, 1)]  # the round-1 ring; C % 128 == 0: the v3 loop
FP8_EXPS = [(0, 0), (2, -3)]


def _fp8_family(names, C):
    assert names and all("igemm" in n for n in names), names
    assert (C % 128 == 0) == all("igemm_v3" in n for n in names), names


def _e(*v):
    e = torch.tensor(v, dtype=torch.int32, device=DEV)
    return [e[i:i + 1] for i in range(len(v))]


@pytest.mark.parametrize("exps", FP8_EXPS, ids=_id)
@pytest.mark.parametrize("shape", FP8_SHAPES, ids=_id)
def test_fp8_forward(shape, exps):
    """Ternary bytes are exact in e4m3: the result is the integer reference times 2^(ex + ew), statistics included."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import igemm_fwd
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    d = ternary_density(k * k * Ci, N * OH * OH)
    x, w = ternary((N, H, H, Ci), d, 1, DEV), ternary((Co, k, k, Ci), d, 2, DEV)
    x8, w8 = x.float().to(torch.float8_e4m3fn), w.float().to(torch.float8_e4m3fn)
    assert torch.equal(x8.float(), x.float()) and torch.equal(w8.float(), w.float())
    iref = fwd_ref(x, w, s, p)
    assert_out_exact(iref)
    q = 2.0 ** sum(exps)
    ref = iref * q
    assert_bf16_exact(ref)
    assert_sums_exact([ref], q)
    assert_sums_exact([ref * ref], q * q)
    slab = torch.zeros(_lib.STAT_SLOTS, 2, Co, device=DEV)
    ex, ew = _e(*exps)
    y, names = kernel_names(lambda: igemm_fwd(x8.view(torch.uint8), w8.view(torch.uint8), s, p, k, k, stats=slab,
                                              fp8=(ex, ew)))
    print(f"fp8 fwd {shape} {exps}: {short_names(names)}")
    _fp8_family(names, Ci)
    _eq("y", y.double(), ref)
    _check_stats(slab, shifted_stats_ref(ref))


@pytest.mark.parametrize("variant", ["plain", "accum", "y_mask", "x_mask", "x2"])
@pytest.mark.parametrize("exps", FP8_EXPS, ids=_id)
@pytest.mark.parametrize("shape", FP8_SHAPES, ids=_id)
def test_fp8_dgrad(shape, exps, variant):
    """e5m2 gradient x e4m3 transposed weights: plain, accumulating, and with the fused BN backward."""
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    N, Ci, H, Co, k, s, p = shape
    bnb = variant in ("y_mask", "x_mask", "x2")
    o = _bnb_operands(shape, variant if bnb else "y_mask")
    dy8, wt8 = o.dy.float().to(torch.float8_e5m2), o.wt.float().to(torch.float8_e4m3fn)
    assert torch.equal(dy8.float(), o.dy.float()) and torch.equal(wt8.float(), o.wt.float())
    q = 2.0 ** sum(exps)
    iref = dgrad_ref(o.dy, o.w, (H, H), s, p)
    assert_out_exact(iref)
    old = ints((N, H, H, Ci), -8, 8, 6, DEV) if variant == "accum" else None
    eg, ew = _e(*exps)
    f = BNBwdFuse(o.x, o.bn, y=o.bits, x2=o.x2, bn2=o.bn2) if bnb else None
    out = old.clone() if old is not None else None
    got, names = _launch(lambda: kernel_names(lambda: igemm_dgrad(
        o.dy, wt8.view(torch.uint8), (H, H), s, p, k, k, out=out, accumulate=old is not None, bnb=f,
        fp8=(dy8.view(torch.uint8), eg, wt8.view(torch.uint8), ew))))
    print(f"fp8 dgrad {shape} {exps} {variant}: {short_names(names)}")
    _fp8_family(names, Co)
    if bnb:
        o.quantum = 0.25 * min(q, 1.0)
        _bnb_check(o, shape, got, raw=lambda sl: dgrad_ref(o.dy[sl], o.w, (H, H), s, p) * q)
    else:
        want = iref * q + (old.double() if old is not None else 0)
        assert_bf16_exact(want)
        assert want.any()
        _eq("dx", got.double(), want)
