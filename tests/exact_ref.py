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
