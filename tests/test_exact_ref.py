"""The fp64 per-tap references of tests/exact_ref.py against PyTorch's own fp64 convolutions (CPU), the measurement
that motivates the bit-exact GPU tests (a relative L2 check does not see one lost pixel), and the dyadic-constant
references of the fused epilogues against fp64 autograd."""

import pytest
import torch
import torch.nn.functional as F

from exact_ref import (DYADIC, assert_bf16_exact, assert_sums_exact, bn_consts, bnb_ref, bnb_terms, dgrad_ref, dyadic,
                       e4m3_ref, fused_out_ref, fwd_ref, halves, ints, mask_bytes, mask_from_bytes, out_size,
                       shifted_stats_ref, stem_form, ternary, ternary_density, wgrad_ref)

# N, Ci, H, Co, k, s, p: ragged channels, odd images, strides that leave rows of the padded image unused
SHAPES = [
    (3, 72, 11, 200, 3, 2, 1),
    (2, 8, 9, 24, 3, 1, 1),
    (2, 16, 10, 8, 1, 2, 0),
    (2, 24, 7, 16, 1, 1, 0),
    (2, 4, 18, 16, 7, 2, 3),
    (1, 8, 8, 8, 3, 2, 1),
]


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_references_match_torch_fp64(shape):
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    x = ints((N, H, H, Ci), -3, 3, 1)
    dy = ints((N, OH, OH, Co), -3, 3, 2)
    w = ints((Co, k, k, Ci), -3, 3, 3)
    wn = _nchw(w)
    assert torch.equal(wgrad_ref(dy, x, k, s, p),
                       torch.nn.grad.conv2d_weight(_nchw(x), (Co, Ci, k, k), _nchw(dy), s, p).permute(0, 2, 3, 1))
    assert torch.equal(fwd_ref(x, w, s, p), F.conv2d(_nchw(x), wn, None, s, p).permute(0, 2, 3, 1))
    assert torch.equal(dgrad_ref(dy, w, (H, H), s, p),
                       torch.nn.grad.conv2d_input((N, Ci, H, H), wn, _nchw(dy), s, p).permute(0, 2, 3, 1))


def test_references_non_square_image():
    N, Ci, H, W, Co = 2, 8, 4, 9, 16
    x = ints((N, H, W, Ci), -3, 3, 4)
    dy = ints((N, H, W, Co), -3, 3, 5)
    assert torch.equal(wgrad_ref(dy, x, 3, 1, 1),
                       torch.nn.grad.conv2d_weight(_nchw(x), (Co, Ci, 3, 3), _nchw(dy), 1, 1).permute(0, 2, 3, 1))


def test_generators():
    a = ints((4, 5, 5, 8), -3, 3, 7)
    assert a.dtype == torch.bfloat16 and torch.equal(a, ints((4, 5, 5, 8), -3, 3, 7))
    assert a.min() == -3 and a.max() == 3 and torch.equal(a, a.round())
    t = ternary((64, 3, 3, 64), 0.25, 8)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.2 < (t != 0).float().mean().item() < 0.3
    s = stem_form(ints((2, 6, 6, 4), -3, 3, 9))
    assert not s[..., 3].any() and s[..., :3].any()
    # the densities the GPU tests derive: 6 sigma of y below 256, a channel's sum(y * y) over M pixels below 2^23
    for K, M in [(4608, 1), (1152, 69580), (147, 37632)]:
        d = ternary_density(K, M)
        assert d <= 0.5 and 36 * K * d * d <= 256 ** 2 and M * K * d * d <= 0.6 * 2 ** 23 + 1e-6


def test_relative_l2_misses_one_lost_pixel():
    """3x3 stride-2 weight gradient, N = 2048, Ci = Co = 256, H = 6 (M = 18,432 output pixels), integer operands in
    [-3, 3]: zeroing ONE dY pixel changes most of the 589,824 output elements, and the relative L2 error of that
    result still passes the suite's `< 1e-2`. (All sums are of integers, exact in fp64: the gradient without the
    pixel is the full one minus that pixel's own contribution, computed from its image alone.)"""
    N, Ci, H, Co, k, s, p = 2048, 256, 6, 256, 3, 2, 1
    OH = out_size(H, k, s, p)
    x = ints((N, H, H, Ci), -3, 3, 0)
    dy = ints((N, OH, OH, Co), -3, 3, 1)
    ref = wgrad_ref(dy, x, k, s, p)
    n, oh, ow = 1000, 1, 1
    only = torch.zeros_like(dy[n:n + 1])
    only[0, oh, ow] = dy[n, oh, ow]
    lost = ref - wgrad_ref(only, x[n:n + 1], k, s, p)
    differ = (lost != ref).sum().item()
    rel = ((lost - ref).norm() / ref.norm()).item()
    print(f"one dY pixel of {N * OH * OH} zeroed: {differ} of {ref.numel()} elements differ, relative L2 {rel:.4f}")
    assert differ > 100_000
    assert rel < 1e-2


# ---- the dyadic-constant references of the fused epilogues (tests/test_epilogue_exact_gpu.py)

def _design_case(K=64, C=256, N=5, H=13):
    x = ternary((N, H, H, K), ternary_density(K), 1)
    w = ternary((C, 1, 1, K), ternary_density(K), 2)
    return x, w, fwd_ref(x, w, 1, 0)


def test_dyadic_pickers():
    c = dyadic(256, 3)
    assert c.dtype == torch.float32 and set(c.tolist()) == set(DYADIC) and torch.equal(c, dyadic(256, 3))
    h = halves(256, -2, 2, 4)
    assert torch.equal(h * 2, (h * 2).round()) and h.min() == -2 and h.max() == 2 and (h != h.round()).any()
    save, gamma, beta = bn_consts(64, 5)
    assert save.shape == (2, 64) and (save[1] > 0).all() and (gamma < 0).any() and (gamma > 0).any()
    save, gamma, beta = bn_consts(64, 5, integer=True)
    assert torch.equal(save[0], save[0].round()) and torch.equal(save[1], torch.ones(64))
    assert set(gamma.tolist()) == {-1.0, 1.0} and torch.equal(beta, beta.round())


@pytest.mark.parametrize("res_scale", [False, True], ids=["identity", "downsample"])
def test_fused_out_ref_matches_torch(res_scale):
    """fused_out_ref against the same expression with F.relu and broadcasting; the seeds give exact-zero
    pre-activations, both mask values, a bf16-representable output and e4m3 values that need rounding."""
    x, w, y = _design_case()
    C = y.shape[-1]
    aff = torch.stack([dyadic(C, 10), halves(C, -2, 2, 11)])
    res = ints(y.shape, -3, 3, 12)
    rsc = dyadic(C, 13) if res_scale else None
    out, pre = fused_out_ref(y, aff, res, rsc, relu=True, pre=True)
    r = res.double() * (rsc.double().view(1, 1, 1, C) if res_scale else 1.0)
    want = F.relu(y * aff[0].double().view(1, 1, 1, C) + aff[1].double().view(1, 1, 1, C) + r)
    assert out.dtype == torch.float64 and torch.equal(out, want)
    assert torch.equal(fused_out_ref(y, aff, relu=True), F.relu(y * aff[0].double() + aff[1].double()))
    assert torch.equal(fused_out_ref(y), y)
    assert_bf16_exact(out)
    zero = (pre == 0).double().mean().item()
    print(f"max |out| {out.max().item()}, exact-zero pre-activations {100 * zero:.1f} %")
    assert zero > 0.005 and (out > 0).any() and (pre < 0).any()
    # mask bytes and the e4m3 copy
    from imagent_amd.ops.bn import relu_mask_bits
    bits = mask_bytes(out > 0)
    assert bits.dtype == torch.uint8 and torch.equal(bits, relu_mask_bits(out.to(torch.bfloat16)))
    assert torch.equal(mask_from_bytes(bits, out.shape), out > 0)
    q, amax = e4m3_ref(out, -1)
    assert amax == out.max().item()
    assert torch.equal(q, (out.float() * 2).to(torch.float8_e4m3fn).view(torch.uint8))
    back = q.view(torch.float8_e4m3fn).double() / 2
    rounded = (back != out).double().mean().item()
    print(f"e4m3 at exponent -1: {100 * rounded:.1f} % of the values rounded")
    assert rounded > 0.01


@pytest.mark.parametrize("variant", ["y_mask", "x_mask", "x2", "accum", "bias_nox"])
def test_bnb_ref_matches_autograd(variant):
    """bnb_ref against fp64 autograd of relu(bn(x) [+ bn2(x2)]): gamma.grad / beta.grad / gamma2.grad are the three
    slab rows, the gradient at the pre-activation is the stored (masked) gradient."""
    N, H, K, C = 3, 7, 64, 128
    dy = ternary((N, H, H, K), 0.5, 1)
    wt = ternary((C, 1, 1, K), 0.5, 2)
    g = dgrad_ref(dy, wt.permute(3, 1, 2, 0).contiguous(), (H, H), 1, 0)  # [N, H, H, C]
    x = ints((N, H, H, C), -3, 3, 3)
    save, gamma, beta = bn_consts(C, 20)
    save2, gamma2, beta2 = bn_consts(C, 30)
    x2 = ints((N, H, H, C), -3, 3, 4) if variant == "x2" else None
    old = ints((N, H, H, C), -8, 8, 5) if variant == "accum" else None
    bias = halves(C, -2, 2, 6) if variant == "bias_nox" else None

    gam = gamma.double().requires_grad_(True)
    bet = beta.double().requires_grad_(True)
    gam2 = gamma2.double().requires_grad_(True)
    z = torch.zeros(N, H, H, C, dtype=torch.float64, requires_grad=True)
    xin = x.double() if variant != "bias_nox" else torch.zeros(N, H, H, C, dtype=torch.float64)
    pre = (xin - save[0].double()) * save[1].double() * gam + bet + z
    if x2 is not None:
        pre = pre + (x2.double() - save2[0].double()) * save2[1].double() * gam2 + beta2.double()
    yout = F.relu(pre)
    up = g + (old.double() if old is not None else 0) + (bias.double() if bias is not None else 0)
    (yout * up).sum().backward()

    ymask = mask_bytes(yout.detach() > 0) if variant != "x_mask" else None
    got, slab = bnb_ref(g, old=old, x=x if variant != "bias_nox" else None, save=save, gamma=gamma, beta=beta,
                        ymask=ymask, x2=x2, save2=save2 if x2 is not None else None, bias=bias)
    assert torch.equal(got, z.grad)
    assert torch.equal(slab[0], gam.grad) and torch.equal(slab[1], bet.grad)
    if x2 is not None:
        assert torch.equal(slab[2], gam2.grad) and slab[2].any()
    else:
        assert not slab[2].any()
    keep = got != 0
    assert keep.any() and (~keep & (up != 0)).any()  # both mask values decide something
    if variant == "x_mask":  # the boundary the from-x mask must get right: fma(x, sc, sh) == 0 is masked
        sc = gamma.double() * save[1].double()
        zero = ((x.double() * sc + (beta.double() - save[0].double() * sc)) == 0)
        print(f"from-x mask: {100 * zero.double().mean().item():.1f} % of fma(x, sc, sh) exactly 0")
        assert zero.double().mean().item() > 0.01 and not got[zero].any() and up[zero].any()
    assert_bf16_exact(got)
    assert_sums_exact(bnb_terms(got, x if variant != "bias_nox" else None, save, x2, save2), 0.125)


def test_shifted_stats_ref():
    x, w, y = _design_case()
    shift = halves(y.shape[-1], -2, 2, 7)
    st = shifted_stats_ref(y, shift)
    y2 = y.reshape(-1, y.shape[-1])
    assert torch.equal(st[0], y2.sum(0) - y2.shape[0] * shift.double())
    assert torch.equal(st[1], (y2 * y2).sum(0) - 2 * shift.double() * y2.sum(0) + y2.shape[0] * shift.double() ** 2)
    assert torch.equal(shifted_stats_ref(y), torch.stack([y2.sum(0), (y2 * y2).sum(0)]))
    d = y - shift.double()
    assert_sums_exact([d], 0.5)
    assert_sums_exact([d * d], 0.25)
    with pytest.raises(AssertionError):
        assert_sums_exact([d], 1.0)  # off the integer grid
    with pytest.raises(AssertionError):
        assert_sums_exact([d * 2.0 ** 16], 0.5)  # past 2^23 quanta
    with pytest.raises(AssertionError):
        assert_bf16_exact(y + 2.0 ** -10)
