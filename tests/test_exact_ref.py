"""The fp64 per-tap references of tests/exact_ref.py against PyTorch's own fp64 convolutions (CPU), the measurement
that motivates the bit-exact GPU tests (a relative L2 check does not see one lost pixel), and the dyadic-constant
references of the fused epilogues against fp64 autograd."""

import pytest
import torch
import torch.nn.functional as F

from exact_ref import (BN_CS, BN_GRID_R, BN_ULPS, DYADIC, assert_bf16_exact, assert_rounded, assert_sums_exact,
                       bf16_spacing, bn_bwd_case_ref, bn_bwd_operands, bn_bwd_ref, bn_consts, bn_fwd_case_ref,
                       bn_fwd_operands, bn_fwd_ref, bn_rows, bnb_ref, bnb_terms, dgrad_ref, dyadic, e4m3_ref,
                       fused_out_ref, fwd_ref, halves, ints, mask_bytes, mask_from_bytes, out_size, shifted_stats_ref,
                       split_slots, stem_form, ternary, ternary_density, wgrad_ref)

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


# ---- the references and margins of the stand-alone BatchNorm passes (tests/test_bn_exact_gpu.py)

BN_VARIANTS = [(0, None), (0, "y"), (0, "x"), (1, None), (1, "y"), (2, None), (2, "y")]  # (mode, ReLU mask)


@pytest.mark.parametrize("mode,mask", BN_VARIANTS, ids=lambda v: str(v))
def test_bn_refs_match_autograd(mode, mask):
    """bn_fwd_ref / bn_bwd_ref against fp64 autograd of F.batch_norm (+ residual | + second batch_norm) (+ relu) on
    the batch's own statistics."""
    R, C, eps = 37, 24, 1e-5
    g = torch.Generator().manual_seed(3)
    x, x2, dy = (torch.randn(R, C, generator=g, dtype=torch.float64) * s + b for s, b in ((2, 0.5), (1, -0.2), (1, 0)))
    gamma, beta, gamma2, beta2 = (torch.randn(C, generator=g, dtype=torch.float64) for _ in range(4))
    leaves = [t.requires_grad_(True) for t in (x, x2, gamma, beta, gamma2, beta2)]
    pre = F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
    if mode == 1:
        pre = pre + x2
    if mode == 2:
        pre = pre + F.batch_norm(x2, None, None, gamma2, beta2, True, 0.1, eps)
    y = F.relu(pre) if mask else pre
    (y * dy).sum().backward()
    xd, x2d = x.detach(), x2.detach()
    mean, var, mean2, var2 = xd.mean(0), xd.var(0, unbiased=False), x2d.mean(0), x2d.var(0, unbiased=False)
    out, pre_ref, rstd, *r2 = bn_fwd_ref(xd, mean, var, gamma.detach(), beta.detach(), eps, mode, bool(mask), x2=x2d,
                                         mean2=mean2, var2=var2, gamma2=gamma2.detach(), beta2=beta2.detach())
    assert (out - y.detach()).abs().max() < 1e-12 and (pre_ref - pre.detach()).abs().max() < 1e-12
    save = torch.stack([mean, rstd])
    save2 = torch.stack([mean2, r2[0]]) if mode == 2 else None
    ref = bn_bwd_ref(dy, xd, save, gamma.detach(), beta.detach(), mode, mask, y=y.detach(), x2=x2d, save2=save2,
                     gamma2=gamma2.detach())
    if mask:
        assert (ref["gm"] == 0).any() and (ref["gm"] != 0).any()
    want = dict(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=x2.grad if mode == 1 else None,
                dx2=x2.grad if mode == 2 else None, dgamma2=gamma2.grad if mode == 2 else None,
                dbeta2=beta2.grad if mode == 2 else None)
    for k, w in want.items():
        if w is None:
            assert ref[k] is None, k
        else:
            assert (ref[k] - w).abs().max() < 1e-12 * max(1.0, w.abs().max().item()), k
    assert torch.equal(ref["Sgx"], ref["dgamma"]) and torch.equal(ref["Sg"], ref["dbeta"])


def test_bf16_spacing_and_assert_rounded():
    ref = torch.tensor([1.0, 1.99, 2.0, -3.5, 0.0, 2.0 ** -126, 2.0 ** -130, 300.0], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0]
    assert bf16_spacing(ref).tolist() == want
    # the spacing is the distance to the next bf16 value
    b = torch.tensor([1.0, 2.0, -3.5, 300.0]).to(torch.bfloat16)
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - b.double()).abs(), bf16_spacing(b.double()))
    # a correctly rounded value passes with no margin; both neighbours pass exactly at a tie
    v = torch.linspace(-5, 5, 4001, dtype=torch.float64)
    assert_rounded(v.to(torch.bfloat16), v, 0.0)
    tie = torch.tensor([1.0 + 2.0 ** -8, -(2.5 + 2.0 ** -7)], dtype=torch.float64)
    lo, hi = torch.tensor([1.0, -2.5]), torch.tensor([1.0 + 2.0 ** -7, -(2.5 + 2.0 ** -6)])
    assert torch.equal(lo.to(torch.bfloat16).double(), lo.double())
    assert torch.equal(hi.to(torch.bfloat16).double(), hi.double())
    assert_rounded(lo.to(torch.bfloat16), tie, 0.0)
    assert_rounded(hi.to(torch.bfloat16), tie, 0.0)
    # one bf16 spacing off is rejected, with the count and the first index in the message
    got = v.to(torch.bfloat16)
    off = got.clone()
    off[1234] = (off[1234:1235].view(torch.int16) + 1).view(torch.bfloat16)[0]
    with pytest.raises(AssertionError, match=r"1 of 4001 .* first at \[1234\]"):
        assert_rounded(off, got.double(), 0.0)
    # the wrong neighbour (the far side of a value just off the tie) is rejected without a margin, accepted with one
    near = tie + torch.tensor([-2.0 ** -20, 2.0 ** -20], dtype=torch.float64)
    with pytest.raises(AssertionError):
        assert_rounded(hi.to(torch.bfloat16), near, 0.0)
    assert_rounded(hi.to(torch.bfloat16), near, 2.0 ** -19)
    with pytest.raises(AssertionError):
        assert_rounded(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64), 1.0)
    with pytest.raises(AssertionError):  # a ReLU output that must be 0
        assert_rounded(torch.tensor([2.0 ** -20]), torch.zeros(1, dtype=torch.float64), 2.0 ** -21)


def test_bn_shapes_and_slab_pieces():
    assert [bn_rows(C) for C in BN_CS] == [(3, 1024, 1025, 2817), (3, 340, 341, 936), (3, 128, 129, 353),
                                           (3, 8, 9, 23), (1, 4, 5, 12)]
    assert BN_GRID_R == 12291
    total = ints((3, 24), -5000, 5000, 1, dtype=torch.float64) * 0.25
    p = split_slots(total, 32, 0.25, 2)
    assert p.shape == (32, 3, 24) and p.dtype == torch.float32 and torch.equal(p.double().sum(0), total)
    assert (p[:-1] != 0).any() and torch.equal(p * 4, (p * 4).round())


def _fwd_f32(o, mode):
    """The forward pass in fp32 in bn_fwd_kernel's operation order."""
    def consts(mean, var, gamma, beta):
        k = torch.rsqrt(var + o.eps) * gamma
        return k, beta - mean * k
    k, sh = consts(o.mean, o.var, o.gamma, o.beta)
    v = torch.addcmul(sh, o.x.float(), k)
    if mode == 1:
        v = v + o.x2.float()
    if mode == 2:
        k2, sh2 = consts(o.mean2, o.var2, o.gamma2, o.beta2)
        v = v + torch.addcmul(sh2, o.x2.float(), k2)
    assert v.dtype == torch.float32
    return v


def _bwd_f32(gm, x, save, gamma, Sgx, Sg):
    """dx in fp32 in bn_bwd_apply_kernel's operation order (the sums are exact in fp32 on these operands)."""
    R = x.numel() // x.shape[-1]
    inv = torch.tensor(1.0) / torch.tensor(float(R))
    mean, rstd = save[0], save[1]
    gr = gamma * rstd
    assert torch.equal(Sgx.float().double(), Sgx) and torch.equal(Sg.float().double(), Sg)
    kx = -gr * inv * Sgx.float() * rstd
    k0 = -gr * inv * Sg.float() - kx * mean
    v = torch.addcmul(torch.addcmul(k0, kx, x.float()), gr, gm.float())
    assert v.dtype == torch.float32
    return v


def _ratio(v, ref, delta):
    err = (v.double() - ref).abs()
    assert not err[delta == 0].any()
    return (err / delta.clamp_min(1e-300)).max().item()


def _bn_sets():
    return [(C, R) for C in BN_CS for R in bn_rows(C)] + [(2048, BN_GRID_R)]


def test_bn_margins_hold_for_fp32_evaluation():
    """The margins of the GPU tests are derived (exact_ref.bn_fwd_delta / bn_bwd_delta: BN_ULPS = 8 fp32 ulps of the
    sum of the magnitudes of the terms), not taken from the kernels: on every operand set tests/test_bn_exact_gpu.py
    uses, the kernels' formulas evaluated in fp32 in the kernels' operation order stay inside them with a factor
    >= 2 to spare. Measured worst |fp32 - fp64| / delta over all sets: forward 0.439, backward 0.327 (3.5 and 2.6
    of the 8 fp32 ulps; the constant stays at 2^-21)."""
    worst_f = worst_b = 0.0
    for C, R in _bn_sets():
        big = R == BN_GRID_R
        o = bn_fwd_operands(C, R)
        for mode in ((2,) if big else (0, 1, 2)):
            (out, pre, *_), delta = bn_fwd_case_ref(o, mode, False)
            worst_f = max(worst_f, _ratio(_fwd_f32(o, mode), pre, delta))
        o = bn_bwd_operands(C, R)
        for mode, mask in ([(2, "y")] if big else BN_VARIANTS):
            ref, d, d2 = bn_bwd_case_ref(o, mode, mask)
            worst_b = max(worst_b, _ratio(_bwd_f32(ref["gm"], o.x, o.save, o.gamma, ref["Sgx"], ref["Sg"]),
                                          ref["dx"], d))
            if mode == 2:
                worst_b = max(worst_b, _ratio(_bwd_f32(ref["gm"], o.x2, o.save2, o.gamma2, ref["Sgx2"], ref["Sg"]),
                                              ref["dx2"], d2))
    print(f"worst |fp32 - fp64| / delta: forward {worst_f:.3f}, backward {worst_b:.3f} (BN_ULPS = 2^-21)")
    assert BN_ULPS == 2.0 ** -21
    assert worst_f <= 0.5 and worst_b <= 0.5


def test_bn_operand_sets_hit_the_edges():
    """The backward's operand sets contain what the cases are about: exact-zero pre-activations under the mask from x
    (the > against >= edge) that carry a gradient, both mask values, and sums that are exact in fp32."""
    o = bn_bwd_operands(64, 129)
    sc = o.gamma.double() * o.save[1].double()
    pre = o.x.double() * sc + (o.beta.double() - o.save[0].double() * sc)
    zero = pre == 0
    assert zero.double().mean().item() > 0.01 and o.g[zero].any()
    ref, d, _ = bn_bwd_case_ref(o, 0, "x")
    assert not ref["gm"][zero].any() and (ref["gm"] != 0).any()
    assert torch.equal(o.y0 > 0, pre > 0)
    assert ref["Sg"].any() and ref["Sgx"].any() and (d > 0).any()
    assert torch.equal(o.g, bn_bwd_operands(64, 129).g) and not torch.equal(o.g, bn_bwd_operands(64, 129, seed=1).g)
    f = bn_fwd_operands(24, 341)
    assert f.x.dtype == torch.bfloat16 and (f.var > 0).all() and (f.gamma < 0).any() and (f.gamma > 0).any()
