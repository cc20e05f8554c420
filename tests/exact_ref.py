"""Integer operands and plain fp64 references for the bit-exact conv tests (a helper, not a test module).

Small integers are exact in bf16, every bf16 x bf16 product is exact in fp32, and every partial sum of such products is
exact in fp32 -- in ANY order, across MFMA accumulation, wave reductions and split-K atomics -- while its magnitude
stays below 2^24. A bf16 output is exact when it is an integer with |y| <= 256. So on these operands a kernel's result
must be EQUAL to the fp64 reference: one missing, doubled or misplaced product is a failure at any M, where a
relative L2 error against Gaussian operands moves by 1e-3 or less.

The exactness conditions are preconditions of a case and are checked on the REFERENCE only (``assert_wgrad_exact``,
``assert_out_exact``), never on a kernel's output.

Layouts: activations NHWC ``[N, H, W, C]``, weights ``[Co, KH, KW, Ci]``. The references pad X, slice one filter tap
with the stride and do one fp64 matmul per tap, on whatever device the tensors are on (no unfold of the whole tensor:
at M = 100k rows that would be gigabytes).
"""

import torch
import torch.nn.functional as F


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def ints(shape, lo, hi, seed, device="cpu", dtype=torch.bfloat16):
    """Seeded uniform integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed, device), device=device, dtype=torch.int32).to(dtype)


def ternary(shape, density, seed, device="cpu", dtype=torch.bfloat16):
    """Seeded values in {-1, 0, 1}; a fraction ``density`` of them nonzero."""
    g = _gen(seed, device)
    u = torch.rand(shape, generator=g, device=device)
    sign = torch.randint(0, 2, shape, generator=g, device=device, dtype=torch.int32) * 2 - 1
    return (sign * (u < density)).to(dtype)


def stem_form(t):
    """The stem's input form: 4 channels, channel 3 zero."""
    assert t.shape[-1] == 4
    t[..., 3] = 0
    return t


def ternary_density(K, M=1, cap=0.5):
    """One nonzero density d for both ternary operands of a K-long dot product: y has variance K d^2, so
    K d^2 <= 1800 keeps 6 sigma of y below 256, and K d^2 <= 0.6 * 2^23 / M keeps a channel's sum(y * y) over M
    output pixels below 2^23 with 40 % to spare (pass M only where statistics are checked)."""
    return min(cap, (min(1800.0, 0.6 * 2 ** 23 / M) / K) ** 0.5)


def _taps(x, k, stride, pad, oh, ow):
    """(kh, kw, [M, Ci] fp64 rows of padded X under that tap)."""
    kh_, kw_ = (k, k) if isinstance(k, int) else k
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    for kh in range(kh_):
        for kw in range(kw_):
            xs = xp[:, kh:kh + (oh - 1) * stride + 1:stride, kw:kw + (ow - 1) * stride + 1:stride, :]
            yield kh, kw, xs.reshape(-1, x.shape[-1]).double()


def wgrad_ref(dy, x, k, stride, pad):
    """dW [Co][KH][KW][Ci] fp64 of dy [N, OH, OW, Co] and x [N, H, W, Ci]."""
    N, OH, OW, Co = dy.shape
    Ci = x.shape[-1]
    assert OH == out_size(x.shape[1], k, stride, pad) and OW == out_size(x.shape[2], k, stride, pad)
    d2 = dy.reshape(-1, Co).double().t().contiguous()
    out = torch.empty(Co, k, k, Ci, dtype=torch.float64, device=dy.device)
    for kh, kw, xs in _taps(x, k, stride, pad, OH, OW):
        out[:, kh, kw, :] = d2 @ xs
    return out


def fwd_ref(x, w, stride, pad):
    """y [N, OH, OW, Co] fp64 of x [N, H, W, Ci] and w [Co, KH, KW, Ci]."""
    N, H, W, _ = x.shape
    Co, k = w.shape[0], w.shape[1]
    OH, OW = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    y = torch.zeros(N * OH * OW, Co, dtype=torch.float64, device=x.device)
    for kh, kw, xs in _taps(x, k, stride, pad, OH, OW):
        y += xs @ w[:, kh, kw, :].double().t()
    return y.view(N, OH, OW, Co)


def dgrad_ref(dy, w, in_hw, stride, pad):
    """dx [N, H, W, Ci] fp64 of dy [N, OH, OW, Co] and w [Co, KH, KW, Ci]."""
    N, OH, OW, Co = dy.shape
    k, Ci = w.shape[1], w.shape[3]
    H, W = in_hw
    assert OH == out_size(H, k, stride, pad) and OW == out_size(W, k, stride, pad)
    d2 = dy.reshape(-1, Co).double()
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, Ci, dtype=torch.float64, device=dy.device)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride, :] += \
                (d2 @ w[:, kh, kw, :].double()).view(N, OH, OW, Ci)
    return dxp[:, pad:pad + H, pad:pad + W, :].contiguous()


def assert_wgrad_exact(dy, x, k, stride, pad, extra=0.0):
    """Precondition of a weight-gradient case: the same gradient of |dY| and |X| (plus the largest pre-filled
    |dW|) bounds every partial sum, in any order; below 2^22 there is a factor 4 to the 2^24 limit."""
    S = wgrad_ref(dy.abs(), x.abs(), k, stride, pad)
    assert S.max().item() + extra < 2 ** 22, S.max().item()


def assert_out_exact(ref, base=None):
    """Precondition of a forward / dgrad case: the bf16 output (and, accumulating, the old value and the sum) is an
    integer of magnitude <= 256."""
    tot = ref.abs() if base is None else ref.abs() + base.double().abs()
    assert tot.max().item() <= 256, tot.max().item()


# ---- dyadic BatchNorm constants: the fused epilogues on integer operands
#
# With integer x, means and shifts that are multiples of 0.5 and rstd / gamma / scales in {+-0.5, +-1, +-2},
# (x - mean) * rstd, fma(x, sc, sh), fma(v, sc, sh) + res * rsc, the ReLU decision and every partial sum are exact in
# fp32 in any order while the sums stay below 2^24 quanta. The kernels round the conv product to bf16 at different
# points (the direct epilogue after the accumulate, the staged and streaming ones before it); on such operands all of
# them must give the bits of the fp64 reference.

DYADIC = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
DYADIC_POS = (0.5, 1.0, 2.0)
UNIT = (-1.0, 1.0)


def dyadic(n, seed, values=DYADIC, device="cpu"):
    """Seeded per-channel fp32 constants drawn from a short list of dyadic values."""
    idx = torch.randint(0, len(values), (n,), generator=_gen(seed, device), device=device)
    return torch.tensor(values, dtype=torch.float32, device=device)[idx]


def halves(n, lo, hi, seed, device="cpu", step=0.5):
    """Seeded per-channel fp32 multiples of ``step`` in [lo, hi]."""
    k = torch.randint(round(lo / step), round(hi / step) + 1, (n,), generator=_gen(seed, device), device=device)
    return k.float() * step


def bn_consts(C, seed, device="cpu", integer=False):
    """(save [2][C] = (mean, rstd), gamma [C], beta [C]) fp32. ``integer``: integer means and shifts, rstd = 1 and
    gamma = +-1 (every term of every sum an integer: the large cases)."""
    if integer:
        mean, rstd = halves(C, -2, 2, seed, device, 1.0), torch.ones(C, device=device)
        gamma, beta = dyadic(C, seed + 2, UNIT, device), halves(C, -2, 2, seed + 3, device, 1.0)
    else:
        mean, rstd = halves(C, -2, 2, seed, device), dyadic(C, seed + 1, DYADIC_POS, device)
        gamma, beta = dyadic(C, seed + 2, DYADIC, device), halves(C, -2, 2, seed + 3, device)
    return torch.stack([mean, rstd]).contiguous(), gamma, beta


def fused_out_ref(y, affine=None, res=None, res_scale=None, relu=False, pre=False):
    """The fused-output epilogue in fp64: act(y * affine[0] + affine[1] + res * res_scale) of a conv result y
    [..., C]; ``pre``: (output, pre-activation)."""
    v = y.double()
    if affine is not None:
        v = v * affine[0].double() + affine[1].double()
    if res is not None:
        v = v + (res.double() if res_scale is None else res.double() * res_scale.double())
    out = v.clamp_min(0) if relu else v
    return (out, v) if pre else out


def mask_bytes(keep):
    """A boolean tensor as the ReLU mask bits (``ops.bn.relu_mask_bits`` layout): byte e // 8 of the flat element
    index e, bit e % 8."""
    b = keep.reshape(-1, 8).to(torch.int64)
    return (b << torch.arange(8, device=keep.device)).sum(1).to(torch.uint8)


def mask_from_bytes(bits, shape):
    """The inverse of :func:`mask_bytes`: a boolean tensor of ``shape``."""
    b = (bits.to(torch.int64).reshape(-1, 1) >> torch.arange(8, device=bits.device)) & 1
    return b.reshape(shape).bool()


def e4m3_ref(out, exponent):
    """(e4m3 bytes of out * 2^-exponent, max |out|) of an fp64 output, quantised as
    test_kernels_gpu.py::test_fp8_quant_matches_torch_e4m3 does."""
    q = (out * 2.0 ** -exponent).float().clamp(-448, 448).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), out.abs().max().item()


def bnb_ref(g, old=None, x=None, save=None, gamma=None, beta=None, ymask=None, x2=None, save2=None, bias=None):
    """The IG_BNBWD epilogue in fp64 on a raw dgrad product g [..., C]: (stored gradient, slab [3][C]).
    ``old`` (an accumulating dgrad's previous output) and ``bias`` [C] are added before the mask; the mask is the
    given bits (``ymask``, :func:`mask_bytes` layout) or fma(x, gamma * rstd, beta - mean * gamma * rstd) > 0. Slab
    rows, in the order the kernels write them: sum(g_m * xhat), sum(g_m), sum(g_m * xhat2) (zeros without ``x2``),
    xhat = (x - mean) * rstd. ``x`` None (mask bits given): the kernels read x as zeros."""
    C = g.shape[-1]
    v = g.double()
    if old is not None:
        v = v + old.double()
    if bias is not None:
        v = v + bias.double()
    mean, rstd = save[0].double(), save[1].double()
    xd = x.double() if x is not None else torch.zeros_like(v)
    if ymask is not None:
        keep = mask_from_bytes(ymask, v.shape)
    else:
        sc = gamma.double() * rstd
        keep = xd * sc + (beta.double() - mean * sc) > 0
    gm = v * keep
    xhat = (xd - mean) * rstd
    rows = [(gm * xhat).reshape(-1, C).sum(0), gm.reshape(-1, C).sum(0)]
    if x2 is not None:
        rows.append((gm * ((x2.double() - save2[0].double()) * save2[1].double())).reshape(-1, C).sum(0))
    else:
        rows.append(torch.zeros_like(rows[0]))
    return gm, torch.stack(rows)


def bnb_terms(gm, x, save, x2=None, save2=None):
    """The per-element terms of :func:`bnb_ref`'s slab rows, for :func:`assert_sums_exact`."""
    xd = x.double() if x is not None else torch.zeros_like(gm)
    t = [gm * ((xd - save[0].double()) * save[1].double()), gm]
    if x2 is not None:
        t.append(gm * ((x2.double() - save2[0].double()) * save2[1].double()))
    return t


def assert_bf16_exact(ref):
    """Precondition on a reference: it equals its own bf16 rounding (what a kernel stores is then the value)."""
    assert torch.equal(ref.to(torch.bfloat16).double(), ref), (ref.to(torch.bfloat16).double() != ref).sum().item()


def abs_sums(terms, quantum):
    """Per-channel sum |term| of each [..., C] term, after checking that every term is a multiple of ``quantum``."""
    out = []
    for t in terms:
        assert torch.equal((t / quantum).round() * quantum, t), "a term off the quantum grid"
        out.append(t.abs().reshape(-1, t.shape[-1]).sum(0))
    return torch.stack(out)


def assert_sums_exact(terms, quantum, sums=None):
    """Precondition of a reduction checked to equality: every term is a multiple of ``quantum`` and each channel's
    sum |term| stays below 2^23 quanta (2^21 at quantum 0.25, 2^23 for integers), so every partial sum, in any
    order, is exact in fp32 with a factor 2 to spare. ``sums``: :func:`abs_sums` accumulated over chunks."""
    s = abs_sums(terms, quantum) if sums is None else sums
    assert s.max().item() < 2 ** 23 * quantum, (s.max().item(), quantum)


def shifted_stats_ref(ref, shift=None):
    """Forward statistics [2][C] fp64 as the conv epilogues accumulate them: sum(y - shift), sum((y - shift)^2)."""
    d = ref.reshape(-1, ref.shape[-1])
    if shift is not None:
        d = d - shift.double()
    return torch.stack([d.sum(0), (d * d).sum(0)])


def kernel_names(fn):
    """Run fn under torch.profiler: (its result, the conv kernel names it launched)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    return out, [n for n in names if any(s in n for s in ("igemm", "conv_stream", "wgrad_", "halo3x3", "stem_band"))]


def short_names(names):
    return sorted({n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for n in names})


# ---- the stand-alone BatchNorm passes (csrc/kernels/bn.hip; tests/test_bn_exact_gpu.py)
#
# A pass's per-element work is a handful of fp32 operations on bf16 inputs and per-channel fp32 constants, then one
# rounding to bf16. The references below are the definitions in fp64; `assert_rounded` allows that one rounding of a
# value within `delta` of the reference, with `delta` a few fp32 ulps of the sum of the magnitudes of the terms
# (`bn_fwd_delta`, `bn_bwd_delta`; validated against an fp32 evaluation in the kernels' operation order on every
# operand set the GPU tests use: tests/test_exact_ref.py). The backward runs on the dyadic operands above, so its
# masks and sums are exact; the forward has a real rsqrt and runs on Gaussian x.

BN_U = 4  # rows per thread per loop iteration (bn.hip U)
BN_CS = (8, 24, 64, 1000, 2048)  # cpr = C / 8 chunks per row, rpb = 256 // cpr rows per block iteration
BN_GRID_R = 3 * 4096 + 3  # C = 2048 (rpb = 1): above 2048 * U (forward grid), 1024 * U (reduce), 4 * CUs * U (apply)
# the margins' constant: 8 fp32 ulps of the sum of magnitudes. Measured worst |fp32 evaluation - fp64| / margin over
# every operand set of the GPU tests (test_exact_ref.py::test_bn_margins_hold_for_fp32_evaluation): forward 0.439,
# backward 0.327 -- inside with the required factor 2, so the constant is not raised
BN_ULPS = 2.0 ** -21


def bn_rpb(C):
    return 256 // (C // 8)


def bn_rows(C):
    """The row counts of one C: fewer rows than one block holds, exactly one full block iteration, one more row (a
    second block whose loads all clamp to R - 1), and a tail in the middle of the u loop."""
    rpb = bn_rpb(C)
    return (1 if C == 2048 else 3, BN_U * rpb, BN_U * rpb + 1, 3 * BN_U * rpb - rpb + 1)


def bf16_spacing(ref):
    """The distance between neighbouring bf16 values at |ref| (fp64): 2^(floor(log2 |ref|) - 7), and the smallest
    subnormal 2^-133 below the smallest normal (and at 0)."""
    _, e = torch.frexp(ref.double().abs())  # |ref| = m 2^e, m in [0.5, 1): floor(log2 |ref|) = e - 1
    e = torch.where(ref == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), (e - 8).clamp_min(-133))


def assert_rounded(out, ref, delta, what="output"):
    """Every element of ``out`` is within half a bf16 spacing (at the reference) plus ``delta`` of the fp64 ``ref``:
    one correct rounding to bf16 of a value within ``delta`` of the reference, and nothing more."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = (out.double() - ref).abs()
    bad = ~(err <= bf16_spacing(ref) / 2 + delta)  # (a NaN is bad)
    n = bad.sum().item()
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {ref.numel()} elements off by more than one bf16 rounding, first at "
                             f"{list(i)}: got {out[i].item()!r}, reference {ref[i].item()!r}, |error| "
                             f"{err[i].item():.3e}")


def _affine(x, mean, rstd, gamma, beta):
    return (x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()


def bn_fwd_ref(x, mean, var, gamma, beta, eps, mode, relu, x2=None, mean2=None, var2=None, gamma2=None, beta2=None):
    """act((x - mean) / sqrt(var + eps) * gamma + beta [+ x2 | + the same of branch 2]) in fp64:
    (output, pre-activation, rstd[, rstd2])."""
    rstd = 1.0 / torch.sqrt(var.double() + eps)
    pre = _affine(x, mean, rstd, gamma, beta)
    out = [rstd]
    if mode == 1:
        pre = pre + x2.double()
    elif mode == 2:
        rstd2 = 1.0 / torch.sqrt(var2.double() + eps)
        pre = pre + _affine(x2, mean2, rstd2, gamma2, beta2)
        out.append(rstd2)
    return (pre.clamp_min(0) if relu else pre, pre, *out)


def bn_fwd_delta(x, mean, var, gamma, beta, eps, mode, x2=None, mean2=None, var2=None, gamma2=None, beta2=None):
    """The forward's margin: BN_ULPS * (|x sc| + |mean sc| + |beta| [+ |res|] [+ the same of branch 2]), sc = gamma *
    rstd in fp64 -- var + eps and the rsqrt (2 ulps), rstd * gamma (1), beta - mean * k (2), the FMA (1), the branch
    add (1 or 2)."""
    sc = gamma.double() / torch.sqrt(var.double() + eps)
    d = (x.double() * sc).abs() + (mean.double() * sc).abs() + beta.double().abs()
    if mode == 1:
        d = d + x2.double().abs()
    elif mode == 2:
        sc2 = gamma2.double() / torch.sqrt(var2.double() + eps)
        d = d + (x2.double() * sc2).abs() + (mean2.double() * sc2).abs() + beta2.double().abs()
    return BN_ULPS * d


def bn_bwd_ref(dy, x, save, gamma, beta, mode, mask, y=None, x2=None, save2=None, gamma2=None):
    """The BatchNorm backward in fp64, the formulas of the kernel comments: the gradient masked by ``mask`` (None,
    "y": y > 0, "x": x sc + sh > 0 with sc = gamma rstd, sh = beta - mean sc), Sg = sum gm, Sgx = sum gm xhat with
    xhat = (x - mean) rstd, dx = gamma rstd (gm - Sg / R - xhat Sgx / R); mode 1: dres = gm; mode 2: Sgx2 and dx2
    over branch 2 (x2, save2, gamma2), dbeta2 = Sg. Keys that a mode does not produce are None."""
    C = x.shape[-1]
    R = x.numel() // C
    mean, rstd, gam = save[0].double(), save[1].double(), gamma.double()
    xd, gm = x.double(), dy.double()
    if mask == "y":
        gm = gm * (y.double() > 0)
    elif mask == "x":
        sc = gam * rstd
        gm = gm * (xd * sc + (beta.double() - mean * sc) > 0)
    else:
        assert mask is None, mask
    xhat = (xd - mean) * rstd
    Sgx, Sg = (gm * xhat).reshape(-1, C).sum(0), gm.reshape(-1, C).sum(0)
    out = dict(gm=gm, Sgx=Sgx, Sg=Sg, Sgx2=torch.zeros_like(Sg), dx=gam * rstd * (gm - Sg / R - xhat * Sgx / R),
               dres=gm if mode == 1 else None, dx2=None, dgamma=Sgx, dbeta=Sg, dgamma2=None, dbeta2=None)
    if mode == 2:
        mean2, rstd2 = save2[0].double(), save2[1].double()
        xhat2 = (x2.double() - mean2) * rstd2
        Sgx2 = (gm * xhat2).reshape(-1, C).sum(0)
        out.update(Sgx2=Sgx2, dgamma2=Sgx2, dbeta2=Sg, dx2=gamma2.double() * rstd2 * (gm - Sg / R - xhat2 * Sgx2 / R))
    return out


def bn_bwd_delta(gm, x, save, gamma, Sgx, Sg):
    """The backward's margin for dx = k1 g + kx x + k0 (k1 = gamma rstd, kx = -k1 rstd Sgx / R, k0 = -k1 Sg / R - kx
    mean): BN_ULPS * (|k1 g| + |kx x| + |kx mean| + |k1 Sg / R|), in fp64. dx2: the same with branch 2's x2, save2,
    gamma2 and Sgx2."""
    R = x.numel() // x.shape[-1]
    mean, rstd = save[0].double(), save[1].double()
    k1 = gamma.double() * rstd
    kx = -k1 * rstd * Sgx / R
    return BN_ULPS * ((k1 * gm).abs() + (kx * x.double()).abs() + (kx * mean).abs() + (k1 * Sg / R).abs())


class Operands(dict):
    """A dict with attribute access; ``to(device)`` moves every tensor."""
    __getattr__ = dict.__getitem__

    def to(self, device):
        return Operands({k: v.to(device) if torch.is_tensor(v) else v for k, v in self.items()})


def bn_bwd_operands(C, R, seed=0):
    """The backward's dyadic operand set [R][C] (CPU; the same values wherever it is used): g integers in [-3, 3], x
    and x2 integers in [-4, 4], `bn_consts` for both branches, and the bf16 forward outputs y0 / y1 / y2 of modes
    0 / 1 / 2 (with ReLU) that the mask-from-y cases read."""
    s = 1000 * seed
    o = Operands(C=C, R=R, g=ints((R, C), -3, 3, s + 1), x=ints((R, C), -4, 4, s + 2), x2=ints((R, C), -4, 4, s + 3))
    o["save"], o["gamma"], o["beta"] = bn_consts(C, s + 10)
    o["save2"], o["gamma2"], o["beta2"] = bn_consts(C, s + 20)
    a = _affine(o.x, o.save[0], o.save[1], o.gamma, o.beta)
    o["y0"] = a.clamp_min(0).to(torch.bfloat16)
    o["y1"] = (a + o.x2.double()).clamp_min(0).to(torch.bfloat16)
    o["y2"] = (a + _affine(o.x2, o.save2[0], o.save2[1], o.gamma2, o.beta2)).clamp_min(0).to(torch.bfloat16)
    return o


def bn_bwd_case_ref(o, mode, mask):
    """(`bn_bwd_ref` of the operand set ``o`` for one mode and mask, after its exactness preconditions; delta of dx;
    delta of dx2 or None)."""
    ref = bn_bwd_ref(o.g, o.x, o.save, o.gamma, o.beta, mode, mask, y=o["y%d" % mode] if mask == "y" else None,
                     x2=o.x2 if mode == 2 else None, save2=o.save2, gamma2=o.gamma2)
    assert_sums_exact(bnb_terms(ref["gm"], o.x, o.save, o.x2 if mode == 2 else None, o.save2), 0.25)
    d = bn_bwd_delta(ref["gm"], o.x, o.save, o.gamma, ref["Sgx"], ref["Sg"])
    d2 = bn_bwd_delta(ref["gm"], o.x2, o.save2, o.gamma2, ref["Sgx2"], ref["Sg"]) if mode == 2 else None
    return ref, d, d2


def bn_fwd_operands(C, R, seed=0):
    """The forward's operand set [R][C] (CPU): Gaussian x (scale 2, offset 0.5), integer x2 in [-4, 4] (the residual
    or branch 2's input), random means, positive variances in [0.05, 4], gammas of both signs in +-[0.5, 1.5] and
    betas for both branches."""
    g = _gen(2000 * seed + 7, "cpu")

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    o = Operands(C=C, R=R, eps=1e-5, x=(rn(R, C) * 2 + 0.5).to(torch.bfloat16), x2=ints((R, C), -4, 4, 2000 * seed + 8))
    for k in ("", "2"):
        o["mean" + k] = rn(C) * 0.5 + (0.5 if k == "" else 0.0)
        o["var" + k] = torch.rand(C, generator=g) * 3.95 + 0.05
        sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
        o["gamma" + k] = sign * (torch.rand(C, generator=g) + 0.5)
        o["beta" + k] = rn(C) * 0.5
    return o


def bn_fwd_case_ref(o, mode, relu):
    """(`bn_fwd_ref` of the operand set ``o``, `bn_fwd_delta`)."""
    kw = dict(x2=o.x2, mean2=o.mean2, var2=o.var2, gamma2=o.gamma2, beta2=o.beta2) if mode else {}
    return (bn_fwd_ref(o.x, o.mean, o.var, o.gamma, o.beta, o.eps, mode, relu, **kw),
            bn_fwd_delta(o.x, o.mean, o.var, o.gamma, o.beta, o.eps, mode, **kw))


def split_slots(total, slots, quantum, seed, spread=64):
    """[slots][...] fp32 pieces, each a multiple of ``quantum`` of magnitude <= spread * quantum except the last,
    that add up to ``total`` (fp64, on the quantum grid) exactly: a slab whose fold is known."""
    g = _gen(seed, "cpu")
    k = torch.randint(-spread, spread + 1, (slots - 1, *total.shape), generator=g).double().to(total.device) * quantum
    last = total.double() - k.sum(0)
    out = torch.cat([k, last[None]]).float()
    assert torch.equal(out.double().sum(0), total.double()), "pieces do not add up exactly in fp32"
    return out
