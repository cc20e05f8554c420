"""The 1-byte weight-gradient loop (csrc/kernels/conv_wgrad_fp8.h): e5m2 dY x e4m3 X -> fp32 dW.

Reference for every numeric check: the exact bytes given to the kernel, decoded (``view(float8)``, ``.double() *
2**e``) and put through ``torch.nn.grad.conv2d_weight`` in fp64 -- quantisation error cancels, only the kernel's
summation is judged. Every e5m2 x e4m3 product is exact in fp32, so the only error is fp32 accumulation: per element
``|dW - ref| <= n * 2^-23 * S`` with n the number of pixels summed (in-image taps only) and S the same weight gradient
of |dY| and |X| (twice the round-to-nearest worst case, for the MFMA's internal summation order). Each case prints its
largest observed ratio ``|err| / (n * 2^-23 * S)``.

Measured on an MI355X: the dispatched kernel (fragments converted to bf16, ``v_mfma_f32_16x16x32_bf16``) stays below
0.08 on every case. ``v_mfma_f32_16x16x32_bf8_fp8`` on the same bytes (entry-point variants 11-13, A/B only) does NOT
hold this bound on full-range data -- ratios 2.7 to 85 (up to 3.2e-4 of S from ONE MFMA of 32 products), exact on
bytes within a factor 4 of each other: its internal sum aligns the products to the largest and drops the low bits of
the small ones, so it is not an fp32 sum. That is why those variants are not the default and have no case here."""

import ctypes as C
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_DY, E_X = -14, -3


def _bytes(shape, fmt, seed):
    """Random finite fp8 bytes over the whole range: e5m2 subnormals .. +-57344, e4m3 subnormals .. +-448 (no NaN /
    inf encodings: the project's quantisers saturate)."""
    g = torch.Generator().manual_seed(seed)
    top = 0x7C if fmt == "e5m2" else 0x7F  # first non-finite magnitude code
    mag = torch.randint(0, top, shape, generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 7
    b = (mag | sign).to(torch.uint8)
    flat = b.view(-1)
    flat[0], flat[1], flat[2], flat[3] = top - 1, (top - 1) | 0x80, 1, 0x81  # the extremes are present
    return b


def _decode(b, fmt, e):
    dt = torch.float8_e5m2 if fmt == "e5m2" else torch.float8_e4m3fn
    return b.view(dt).double() * 2.0 ** e


def _ref(dy8, x8, e_dy, e_x, k, stride, pad):
    """(fp64 reference [Co][KH][KW][Ci], S, n) on the CPU from the bytes."""
    dy = _decode(dy8.cpu(), "e5m2", e_dy).permute(0, 3, 1, 2)  # NCHW views
    x = _decode(x8.cpu(), "e4m3", e_x).permute(0, 3, 1, 2)

    def f(a, b):
        ws = (b.shape[1], a.shape[1], k, k)
        return torch.nn.grad.conv2d_weight(a, ws, b, stride=stride, padding=pad).permute(0, 2, 3, 1)
    ref = f(x, dy)
    S = f(x.abs(), dy.abs())
    n = f(torch.ones_like(x[:, :1]), torch.ones_like(dy[:, :1]))  # [1][KH][KW][1]: pixels per tap
    return ref, S, n


def _exps(e_dy=E_DY, e_x=E_X):
    return (torch.tensor([e_dy], dtype=torch.int32, device=DEV), torch.tensor([e_x], dtype=torch.int32, device=DEV))


def _operands(N, Ci, H, Co, k, stride, pad, seed):
    OH = (H + 2 * pad - k) // stride + 1
    dy8 = _bytes((N, OH, OH, Co), "e5m2", seed).to(DEV)
    x8 = _bytes((N, H, H, Ci), "e4m3", seed + 1).to(DEV)
    return dy8, x8


def _check(dw, base, ref, S, n, what):
    err = (dw.double().cpu() - (base.double().cpu() + ref)).abs()
    bound = n * 2.0 ** -23 * S
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max |err| / (n 2^-23 S) = {ratio:.4f}")
    assert (err <= bound).all(), (what, ratio)


CASES = [
    (2, 128, 9, 128, 1, 1, 0, 0),     # M = 162: the tail rows of the last stage read zeros; one tile
    (3, 256, 12, 128, 3, 1, 1, 0),    # nine taps, padding on all four sides, two ci tiles per tap
    (2, 128, 13, 256, 3, 2, 1, 0),    # stride 2 on an odd image, two co tiles
    (2, 512, 7, 512, 1, 2, 0, 0),     # the strided 1x1 downsample form
    (4, 128, 14, 128, 3, 1, 1, 1),    # M = 784, splits 1 and 3: not whole stages per split; dW pre-filled (+=, split-K)
    (4, 128, 14, 128, 3, 1, 1, 3),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_fp8_matches_fp64_of_the_bytes(case):
    from imagent_amd.ops.conv import igemm_wgrad_fp8
    N, Ci, H, Co, k, stride, pad, splits = case
    dy8, x8 = _operands(N, Ci, H, Co, k, stride, pad, seed=H + Ci + splits)
    ref, S, n = _ref(dy8, x8, E_DY, E_X, k, stride, pad)
    e_dy, e_x = _exps()
    torch.manual_seed(3)
    base = torch.randn(Co, k, k, Ci, device=DEV) * 10 if splits else torch.zeros(Co, k, k, Ci, device=DEV)
    dw = base.clone()
    assert igemm_wgrad_fp8(dy8, x8, dw, e_dy, e_x, stride, pad, k, k, splits=splits)
    torch.cuda.synchronize()
    _check(dw, base, ref, S, n, f"wgrad fp8 {case}")


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_wgrad_fp8_stage_shapes(variant):
    """The other stage shapes of the entry point (A/B variants) on the nine-tap case."""
    from imagent_amd.ops.conv import igemm_wgrad_fp8
    N, Ci, H, Co, k, stride, pad = 3, 256, 12, 128, 3, 1, 1
    dy8, x8 = _operands(N, Ci, H, Co, k, stride, pad, seed=77)
    ref, S, n = _ref(dy8, x8, E_DY, E_X, k, stride, pad)
    e_dy, e_x = _exps()
    dw = torch.zeros(Co, k, k, Ci, device=DEV)
    assert igemm_wgrad_fp8(dy8, x8, dw, e_dy, e_x, stride, pad, k, k, variant=variant)
    torch.cuda.synchronize()
    _check(dw, torch.zeros_like(dw), ref, S, n, f"wgrad fp8 variant {variant}")


def test_wgrad_fp8_scale_is_exact():
    """One block per element (splits = 1): exponents (e_dy + 1, e_x + 2) give 8 x the result, bit for bit."""
    from imagent_amd.ops.conv import igemm_wgrad_fp8
    N, Ci, H, Co, k, stride, pad = 3, 256, 12, 128, 3, 1, 1
    dy8, x8 = _operands(N, Ci, H, Co, k, stride, pad, seed=5)
    a = torch.zeros(Co, k, k, Ci, device=DEV)
    b = torch.zeros_like(a)
    assert igemm_wgrad_fp8(dy8, x8, a, *_exps(), stride, pad, k, k, splits=1)
    assert igemm_wgrad_fp8(dy8, x8, b, *_exps(E_DY + 1, E_X + 2), stride, pad, k, k, splits=1)
    torch.cuda.synchronize()
    assert a.abs().max() > 0
    assert torch.equal(b, a * 8)


@pytest.mark.parametrize("ci,co", [(64, 128), (128, 192)])
def test_wgrad_fp8_unsupported_shapes(ci, co):
    """Ci = 64 / Co = 192: -106 from the C entry; through conv_wgrad(fp8=) the bf16 path's result."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import _wgrad_args, conv_wgrad, igemm_wgrad, igemm_wgrad_fp8
    N, H, k = 2, 8, 3
    dy8, x8 = _operands(N, ci, H, co, k, 1, 1, seed=9)
    e_dy, e_x = _exps()
    dw = torch.zeros(co, k, k, ci, device=DEV)
    args = _wgrad_args(dy8, x8, dw, 1, 1, k, k, False, None)
    r = _lib.kernels().imk_conv_wgrad_fp8(C.byref(args), e_dy.data_ptr(), e_x.data_ptr(), 0, 0, _lib.stream_ptr())
    assert r == -106
    assert not igemm_wgrad_fp8(dy8, x8, dw, e_dy, e_x, 1, 1, k, k)
    torch.cuda.synchronize()
    assert not dw.any()
    # through the module-level seam: the bf16 tensors decide the result
    torch.manual_seed(1)
    dy = torch.randn(N, H, H, co, device=DEV).to(torch.bfloat16)
    x = torch.randn(N, H, H, ci, device=DEV).to(torch.bfloat16)
    want = torch.zeros(co, k, k, ci, device=DEV)
    igemm_wgrad(dy, x, want, 1, 1, k, k)
    w = torch.nn.Parameter(torch.zeros(co, ci, k, k, device=DEV).contiguous(memory_format=torch.channels_last))
    w.grad = torch.zeros_like(w)
    mod = types.SimpleNamespace(weight=w, stride=1, padding=1, kh=k, kw=k, grad_pad=None)
    conv_wgrad(mod, dy, x, fp8=(dy8, e_dy, x8, e_x))
    torch.cuda.synchronize()
    # (the bf16 kernels' split-K fp32 atomics: equal up to summation order)
    assert torch.allclose(w.grad.permute(0, 2, 3, 1), want, rtol=1e-5, atol=1e-4)


def test_ds_read_tr8_lane_map():
    """ds_read_b64_tr_b8, one wave: a 16-lane group reads a block of 8 rows x 16 byte columns; lane 2q + p of the
    group supplies the address of row q, columns 8p .. 8p + 7; lane i receives column i of the 8 rows, row q in byte
    q of its 64-bit result. Four groups read four blocks of a [32][16] byte image whose bytes are all distinct in
    (row, column) -- once with the low and once with the high byte of 16 * row + column + 1 as the pattern."""
    from imagent_amd.ops import _lib
    rows, cols, pitch = 32, 16, 48  # 48-B rows (a multiple of 8): the map may not depend on dense rows
    addr = (C.c_int * 64)()
    for lane in range(64):
        g, l = divmod(lane, 16)
        q, p = divmod(l, 2)
        addr[lane] = (8 * g + q) * pitch + 8 * p
    for shift in (0, 8):
        img = bytearray(rows * pitch)
        for r in range(rows):
            for c in range(cols):
                img[r * pitch + c] = ((16 * r + c + 1) >> shift) & 0xFF
        src = (C.c_uint8 * len(img)).from_buffer(img)
        out = (C.c_uint32 * 128)()
        _lib.check(_lib.kernels().imk_probe_ds_read_tr8(C.addressof(src), len(img), C.addressof(addr),
                                                        C.addressof(out)), "tr8 probe")
        for lane in range(64):
            g, i = divmod(lane, 16)
            got = out[2 * lane] | (out[2 * lane + 1] << 32)
            want = 0
            for q in range(8):
                want |= (((16 * (8 * g + q) + i + 1) >> shift) & 0xFF) << (8 * q)
            assert got == want, (shift, lane, hex(got), hex(want))


def test_wgrad_fp8_past_2gb():
    """dY8 and X8 as cat([t, t]), each over 2^31 bytes, 1x1 128 -> 128: the result is 2 x the half-size launch within
    the bound (n and S of the large launch)."""
    from imagent_amd.ops.conv import igemm_wgrad_fp8
    N, H, Cc = 11000, 28, 128
    g = torch.Generator(device=DEV).manual_seed(11)
    dy = (torch.randint(0, 0x7C, (N, H, H, Cc), generator=g, device=DEV, dtype=torch.int16)
          | (torch.randint(0, 2, (N, H, H, Cc), generator=g, device=DEV, dtype=torch.int16) << 7)).to(torch.uint8)
    x = (torch.randint(0, 0x7F, (N, H, H, Cc), generator=g, device=DEV, dtype=torch.int16)
         | (torch.randint(0, 2, (N, H, H, Cc), generator=g, device=DEV, dtype=torch.int16) << 7)).to(torch.uint8)
    dy2, x2 = torch.cat([dy, dy]), torch.cat([x, x])
    assert dy2.numel() > 2 ** 31 and x2.numel() > 2 ** 31
    e_dy, e_x = _exps()
    dw = torch.zeros(Cc, Cc, device=DEV)
    dw2 = torch.zeros_like(dw)
    assert igemm_wgrad_fp8(dy, x, dw, e_dy, e_x, 1, 0, 1, 1)
    assert igemm_wgrad_fp8(dy2, x2, dw2, e_dy, e_x, 1, 0, 1, 1)
    torch.cuda.synchronize()
    # S of the large launch = 2 x the half's, in fp64 by row chunks
    S = torch.zeros(Cc, Cc, device=DEV, dtype=torch.float64)
    dyf, xf = dy.view(-1, Cc), x.view(-1, Cc)
    step = 1 << 20
    for r in range(0, dyf.shape[0], step):
        a = _decode(dyf[r:r + step], "e5m2", E_DY).abs()
        b = _decode(xf[r:r + step], "e4m3", E_X).abs()
        S += a.t() @ b
    S *= 2
    n = 2 * dyf.shape[0]
    err = (dw2.double() - 2 * dw.double()).abs()
    ratio = (err / (n * 2.0 ** -23 * S)).max().item()
    print(f"wgrad fp8 past 2 GB: max |err| / (n 2^-23 S) = {ratio:.3e}")
    assert dw.abs().max() > 0 and (err <= n * 2.0 ** -23 * S).all(), ratio
