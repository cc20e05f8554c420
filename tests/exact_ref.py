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
