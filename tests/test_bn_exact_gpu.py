"""The stand-alone BatchNorm passes of csrc/kernels/bn.hip, element for element against fp64 references.

Every output that training reads is checked: y, save / save2, the ReLU mask bits, the e4m3 copy and its amax, the
column sums, the in-pass slab fold and eval mode of ``imk_bn_fwd``; the folded sums, dgamma / dbeta (accumulated into
pre-filled slots), dx, dres and dx2 of ``imk_bn_bwd`` (atomic and deterministic reduce) and of ``imk_bn_bwd_apply``
(fold inside the pass and as a launch of its own, ``sgx_row=2`` on another BN's slab, the e5m2 copies and their amax);
the per-channel kernels (statistics finalize, finalize + affine, running update, eval affine); the deterministic
mode's forward statistics pass; the host's refusals. Outputs the test allocates sit between sentinel rows that must
stay untouched. Measured results and the mutations the file was tried against: profiles/exact_tests.md.

The backward runs on dyadic operands (exact_ref.bn_bwd_operands): every mask decision and every term of the sums is
exact in fp32 in any order, so the sums, dgamma / dbeta and dres must EQUAL the reference, and fma(x, sc, sh) is exactly
0 on many elements (the > against >= edge of the mask from x). dx / dx2 and the forward's y (Gaussian x, a real
rsqrt) are held to ``assert_rounded``: one bf16 rounding of a value within a derived margin of a few fp32 ulps of the
reference (exact_ref.bn_fwd_delta / bn_bwd_delta, validated on the CPU in test_exact_ref.py). Exactness conditions
are asserted on the references only.

Shapes: C sets the lane geometry (cpr = C / 8 chunks per row, rpb = 256 // cpr rows per block iteration; C = 24 and
1000 leave idle lanes and ragged channel loops), R the row path (exact_ref.bn_rows: fewer rows than a block, one full
block iteration, one row more, a tail inside the u loop), and one case per pass at C = 2048 has more rows than any
grid cap covers in one iteration (BN_GRID_R).
"""

import ctypes
import functools
import types

import pytest
import torch

from exact_ref import (BN_CS, BN_GRID_R, BN_U, assert_rounded, bn_bwd_case_ref, bn_bwd_operands, bn_fwd_case_ref,
                       bn_fwd_delta, bn_fwd_operands, bn_fwd_ref, bn_rows, bn_rpb, e4m3_ref, halves, split_slots)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS = 32
U22 = 2.0 ** -22  # 4 fp32 ulps (unit roundoff 2^-24), relative

GRID = [(C, R) for C in BN_CS for R in bn_rows(C)]
BIG = (2048, BN_GRID_R)
Q_CS = (8, 64, 2048)  # the fp8 copies and the column sums need every lane active (C / 8 divides 256)


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _eq(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = got.double() != want.double()
    bad = ne.sum().item()
    if bad:
        i = tuple(ne.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {bad} of {want.numel()} elements differ, first at {list(i)}: got "
                             f"{got[i].item()!r}, reference {want[i].item()!r}")


def _close(what, got, want, tol):
    """|got - want| <= tol per element (fp64)."""
    err = (got.double() - want.double()).abs()
    bad = ~(err <= tol)
    n = bad.sum().item()
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} of {want.numel()} elements off, first at {list(i)}: got {got[i].item()!r}, "
                             f"reference {want[i].item()!r}, |error| {err[i].item():.3e}, allowed "
                             f"{(tol[i] if torch.is_tensor(tol) and tol.dim() else tol):.3e}")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_grid_stride(C, R):
    """R rows are more than one grid iteration of any pass covers (bn.hip: grid_for caps the forward at 2048 blocks
    of U * rpb rows, imk_bn_bwd the reduce at 1024, imk_bn_bwd_apply the apply at 4 blocks per CU), and no multiple
    of a block's rows: some blocks run a second, partly empty iteration."""
    rows = BN_U * bn_rpb(C)
    for cap in (2048, 1024, 4 * _cus()):
        assert R > cap * rows, (R, cap, rows)
    assert R % rows


def _work(C):
    from imagent_amd.models.resnet import BNWork
    from imagent_amd.ops import _lib
    assert _lib.STAT_SLOTS == SLOTS
    return BNWork(torch.zeros(SLOTS, 2, C, device=DEV), torch.zeros(2, C, device=DEV), torch.zeros(2, C, device=DEV),
                  torch.zeros(_lib.kernels().imk_bn_bwd_scratch_floats(C), device=DEV))


def _prefill(C, k):
    """Nonzero integers of magnitude <= 64 that differ from channel to channel (and from k to k)."""
    v = (torch.arange(C, device=DEV) * 37 + 11 * k) % 129 - 64
    return torch.where(v == 0, torch.full_like(v, 7 + k), v).float()


def _bn(C, gamma, beta, save=None, k=0):
    """What the ops read of a BatchNorm2d: work, weight / bias and their (pre-filled) gradient slots."""
    bn = types.SimpleNamespace(work=_work(C), weight=gamma.clone(), bias=beta.clone(), eps=1e-5)
    if save is not None:
        bn.work.save.copy_(save)
    bn.weight.grad, bn.bias.grad = _prefill(C, k), _prefill(C, k + 1)
    return bn


class _Guarded:
    """An output buffer of R rows of `width` elements between two sentinel rows that the kernel must leave alone."""

    def __init__(self, R, width, dtype, fill):
        self.buf = torch.full((R + 2, width), fill, device=DEV, dtype=dtype)
        self.fill = self.buf[0].clone()
        self.t = self.buf[1:R + 1]

    def check(self, what):
        for row, name in ((self.buf[0], "before"), (self.buf[-1], "after")):
            assert torch.equal(row.view(torch.uint8), self.fill.view(torch.uint8)), f"{what}: the row {name} it was written"


def _guarded_bf16(R, C):
    return _Guarded(R, C, torch.bfloat16, float("nan"))


@functools.lru_cache(maxsize=None)
def _fwd_ops(C, R):
    return bn_fwd_operands(C, R).to(DEV)


@functools.lru_cache(maxsize=None)
def _bwd_ops(C, R):
    return bn_bwd_operands(C, R).to(DEV)


@functools.lru_cache(maxsize=None)
def _bwd_case(C, R, mode, mask):
    """(operands, reference dict, delta of dx, delta of dx2) on the GPU, computed once and left unchanged."""
    o = _bwd_ops(C, R)
    return (o,) + bn_bwd_case_ref(o, mode, mask)


# ===================================================================== imk_bn_fwd

def _fwd_kw(o, mode):
    if mode == 0:
        return {}
    kw = dict(x2=o.x2)
    if mode == 2:
        kw.update(stats2=torch.stack([o.mean2, o.var2]), gamma2=o.gamma2, beta2=o.beta2)
    return kw


def _check_y(y, out, pre, delta, relu):
    assert_rounded(y, out, delta, "y")
    if relu:  # the decision itself: certainly negative -> 0, certainly positive -> positive
        neg, pos = pre < -delta, pre > delta
        assert neg.any() and pos.any()
        assert not y[neg].any(), f"{(y[neg] != 0).sum().item()} outputs nonzero under a negative pre-activation"
        assert (y[pos] > 0).all(), f"{(~(y[pos] > 0)).sum().item()} outputs not positive over a positive one"


def _check_save(save, mean, rstd64, what="save"):
    _eq(what + "[0] (mean)", save[0], mean)
    _close(what + "[1] (rstd)", save[1], rstd64, U22 * rstd64)


def _run_fwd(C, R, mode, relu):
    from imagent_amd.ops.bn import bn_fwd_launch, relu_mask_bits
    o = _fwd_ops(C, R)
    (out, pre, rstd, *r2), delta = bn_fwd_case_ref(o, mode, relu)
    yg, mg = _guarded_bf16(R, C), _Guarded(R, C // 8, torch.uint8, 0xA5)
    y, ym = yg.t, (mg.t.view(-1) if mode and relu else None)
    save, save2 = torch.full((2, C), -7.0, device=DEV), torch.full((2, C), -7.0, device=DEV)
    bn_fwd_launch(o.x, torch.stack([o.mean, o.var]), o.gamma, o.beta, y, save, save2=save2 if mode == 2 else None,
                  mode=mode, relu=relu, eps=o.eps, ym=ym, **_fwd_kw(o, mode))
    torch.cuda.synchronize()
    _check_y(y, out, pre, delta, relu)
    yg.check("y")
    mg.check("ReLU mask bits")
    _check_save(save, o.mean, rstd)
    if mode == 2:
        _check_save(save2, o.mean2, r2[0], "save2")
    else:
        assert (save2 == -7.0).all()
    if ym is not None:
        _eq("ReLU mask bits", ym, relu_mask_bits(y))


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", GRID, ids=_id)
def test_bn_fwd(shape, mode, relu):
    _run_fwd(*shape, mode, relu)


def test_bn_fwd_grid_stride():
    _assert_grid_stride(*BIG)
    _run_fwd(*BIG, 2, True)


@pytest.mark.parametrize("C", Q_CS)
def test_bn_fwd_colsum(C):
    """colsum += the column sums of the stored bf16 y (mode 0), over a pre-filled accumulator. Each channel is an fp32
    sum of the pre-fill and n_rows values in some order: the standard bound n_rows * 2^-24 * (sum of the magnitudes
    of the terms) against the fp64 sum. (The pre-fill is one of the terms: at R = 3 the rounding of `pre-fill + sum`
    alone exceeds 3 * 2^-24 * sum |y|.)"""
    from imagent_amd.ops.bn import bn_fwd_launch
    for R in bn_rows(C):
        o = _fwd_ops(C, R)
        (out, pre, *_), delta = bn_fwd_case_ref(o, 0, True)
        y = torch.empty_like(o.x)
        fill = _prefill(C, 3)
        colsum = fill.clone()
        bn_fwd_launch(o.x, torch.stack([o.mean, o.var]), o.gamma, o.beta, y, None, mode=0, relu=True, eps=o.eps,
                      colsum=colsum)
        torch.cuda.synchronize()
        _check_y(y, out, pre, delta, True)
        yd = y.double()
        _close(f"colsum at R = {R}", colsum, fill.double() + yd.sum(0),
               R * 2.0 ** -24 * (fill.double().abs() + yd.abs().sum(0)))


@pytest.mark.parametrize("C,exp", [(8, -3), (64, 0), (2048, 2), (64, -8)])
def test_bn_fwd_q8(C, exp):
    """The e4m3 copy is the quantised STORED y, its amax max |stored y| (exponent -8: the clamp at 448)."""
    from imagent_amd.ops.bn import bn_fwd_launch
    for R, mode in zip(bn_rows(C), (0, 1, 2, 0)):
        o = _fwd_ops(C, R)
        (out, pre, *_), delta = bn_fwd_case_ref(o, mode, True)
        y = torch.empty_like(o.x)
        qg = _Guarded(R, C, torch.uint8, 0x55)
        y8 = qg.t.view(-1)
        amax = torch.zeros(SLOTS, device=DEV)
        bn_fwd_launch(o.x, torch.stack([o.mean, o.var]), o.gamma, o.beta, y, None, mode=mode, relu=True, eps=o.eps,
                      q8=(y8, torch.tensor([exp], device=DEV, dtype=torch.int32), amax), **_fwd_kw(o, mode))
        torch.cuda.synchronize()
        _check_y(y, out, pre, delta, True)
        q, top = e4m3_ref(y.double(), exp)
        if exp == -8:
            assert top * 2.0 ** -exp > 448
        _eq(f"e4m3 bytes at R = {R}", y8, q.reshape(-1))
        qg.check("e4m3 copy")
        assert amax.max().item() == top and (amax >= 0).all(), (amax.max().item(), top)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape", [(C, bn_rows(C)[k]) for C in BN_CS for k in (0, 3)], ids=_id)
def test_bn_eval(shape, mode):
    """Eval mode (ops.bn.bn_eval): the running statistics as `sums`, no save."""
    from imagent_amd.ops.bn import bn_eval
    C, R = shape
    o = _fwd_ops(C, R)
    (out, pre, *_), delta = bn_fwd_case_ref(o, mode, True)
    bn = types.SimpleNamespace(running_mean=o.mean, running_var=o.var, weight=o.gamma, bias=o.beta, eps=o.eps)
    bn2 = types.SimpleNamespace(running_mean=o.mean2, running_var=o.var2, weight=o.gamma2, bias=o.beta2, eps=o.eps)
    y = bn_eval(o.x, bn, True, x2=o.x2 if mode else None, bn2=bn2 if mode else None, mode=mode)
    torch.cuda.synchronize()
    _check_y(y, out, pre, delta, True)


def _slab_case(C, R, seed=5):
    """An integer x [R][C], an integer shift and the [32][2][C] slab of exact pieces of sum(x - shift) and
    sum((x - shift)^2): (x, shift, slab, mean fp64, biased variance fp64, their tolerances). The fold's fp32 result
    is within 4 fp32 ulps of the sum of the magnitudes of the terms: mean = shift + E[d] (the 1 / R constant, one
    product, one sum), var = E[d^2] - E[d]^2 (each term: 1 / R, one or two products; one difference)."""
    o = _fwd_ops(C, R)
    x = o.x2
    shift = halves(C, -2, 2, seed, step=1.0).to(DEV)
    d = x.double() - shift.double()
    sums = torch.stack([d.sum(0), (d * d).sum(0)])
    slab = split_slots(sums, SLOTS, 1.0, seed + 1)
    m1, m2 = sums[0] / R, sums[1] / R
    return x, shift, slab, shift.double() + m1, m2 - m1 * m1, U22 * (shift.double().abs() + m1.abs()), \
        U22 * (m2 + m1 * m1)


@pytest.mark.parametrize("shape", GRID, ids=_id)
def test_bn_fwd_fold_inside_the_pass(shape):
    """fold=work (mode 0): the pass folds the slab into `stats` itself; the statistics against fp64, y and save
    against the reference built from the statistics the pass stored."""
    from imagent_amd.ops.bn import bn_fwd_launch
    from imagent_amd.ops.conv import _SHIFT
    assert _SHIFT
    C, R = shape
    o = _fwd_ops(C, R)
    x, shift, slab, mean, var, tol_m, tol_v = _slab_case(C, R)
    w = _work(C)
    w.slab.copy_(slab)
    w.save[0].copy_(shift)
    w.scratch.zero_()  # the publish counter
    y = torch.full_like(x, float("nan"))
    bn_fwd_launch(x, w.stats, o.gamma, o.beta, y, w.save, mode=0, relu=True, eps=o.eps, fold=w)
    torch.cuda.synchronize()
    _close("folded mean", w.stats[0], mean, tol_m)
    _close("folded variance", w.stats[1], var, tol_v)
    out, pre, rstd = bn_fwd_ref(x, w.stats[0], w.stats[1], o.gamma, o.beta, o.eps, 0, True)
    assert_rounded(y, out, bn_fwd_delta(x, w.stats[0], w.stats[1], o.gamma, o.beta, o.eps, 0), "y")
    _check_save(w.save, w.stats[0], rstd)


def _raises(code, fn):
    with pytest.raises(RuntimeError, match=rf"failed with code {code}$"):
        fn()


def test_bn_fwd_refusals():
    from imagent_amd.ops.bn import bn_fwd_launch

    def launch(C, **kw):
        o = _fwd_ops(C, 3) if C in BN_CS else None
        x = o.x if o is not None else torch.zeros(3, C, device=DEV, dtype=torch.bfloat16)
        f = (lambda n: torch.ones(n, device=DEV))
        gamma, beta, stats = (o.gamma, o.beta, torch.stack([o.mean, o.var])) if o is not None else (f(C), f(C), f(2 * C))
        if kw.get("mode"):
            kw["x2"] = x
        return lambda: bn_fwd_launch(x, stats, gamma, beta, torch.empty_like(x), None, **kw)

    q8 = (torch.zeros(72, device=DEV, dtype=torch.uint8), torch.zeros(1, device=DEV, dtype=torch.int32),
          torch.zeros(SLOTS, device=DEV))
    _raises(-102, launch(24, q8=q8))
    _raises(-103, launch(24, colsum=torch.zeros(24, device=DEV)))
    _raises(-104, launch(64, mode=1, fold=_work(64)))
    _raises(-100, launch(12))
    _raises(-100, launch(2056))
    torch.cuda.synchronize()


# ===================================================================== imk_bn_bwd

BWD = [(0, None), (0, "y"), (0, "x"), (1, None), (1, "y"), (2, None), (2, "y")]  # (mode, ReLU mask)


def _bwd_launch(o, bn, bn2, mode, mask):
    """(dx, dres | dx2) through ops.bn.bn_act_backward; mode 0 with the mask from y (a combination the op never
    asks for) through the exported function."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import bn_act_backward
    if (mode, mask) != (0, "y"):
        return bn_act_backward(o.g, o.x, o.x2 if mode == 2 else None, o["y%d" % mode] if mask == "y" else None, bn,
                               bn2 if mode == 2 else None, mode, mask is not None)
    dx = torch.empty_like(o.x)
    _lib.check(_lib.kernels().imk_bn_bwd(
        o.g.data_ptr(), o.y0.data_ptr(), o.x.data_ptr(), bn.work.save.data_ptr(), bn.weight.data_ptr(),
        bn.bias.data_ptr(), None, None, None, bn.work.scratch.data_ptr(), dx.data_ptr(), None, None,
        bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), None, None, o.R, o.C, 0, 1, _lib.stream_ptr()), "bn bwd")
    return dx, None


def _check_bwd(o, ref, d, d2, mode, bn, bn2, dx, second, scratch, sgx_row=0, decoy=None):
    C = o.C
    rows = [ref["Sgx"], ref["Sg"], ref["Sgx2"]]
    if sgx_row == 2:
        rows = [decoy, ref["Sg"], ref["Sgx"]]
    _eq("folded sums", scratch[SLOTS * 3 * C:SLOTS * 3 * C + 3 * C].view(3, C), torch.stack(rows))
    _eq("dgamma", bn.weight.grad, _prefill(C, 0).double() + ref["dgamma"])
    _eq("dbeta", bn.bias.grad, _prefill(C, 1).double() + ref["dbeta"])
    assert_rounded(dx, ref["dx"], d, "dx")
    if mode == 2:
        _eq("dgamma2", bn2.weight.grad, _prefill(C, 2).double() + ref["dgamma2"])
        _eq("dbeta2", bn2.bias.grad, _prefill(C, 3).double() + ref["dbeta2"])
        assert_rounded(second, ref["dx2"], d2, "dx2")
    else:  # the other BN's slots are not this launch's
        _eq("dgamma2", bn2.weight.grad, _prefill(C, 2))
        _eq("dbeta2", bn2.bias.grad, _prefill(C, 3))


def _run_bwd(C, R, mode, mask):
    o, ref, d, d2 = _bwd_case(C, R, mode, mask)
    bn, bn2 = _bn(C, o.gamma, o.beta, o.save, 0), _bn(C, o.gamma2, o.beta2, o.save2, 2)
    dx, second = _bwd_launch(o, bn, bn2, mode, mask)
    torch.cuda.synchronize()
    _check_bwd(o, ref, d, d2, mode, bn, bn2, dx, second, bn.work.scratch)
    if mode == 1:
        _eq("dres", second, ref["dres"])
    if mask is not None:
        assert (ref["gm"] == 0).any() and (ref["gm"] != 0).any()


@pytest.mark.parametrize("mode,mask", BWD, ids=_id)
@pytest.mark.parametrize("shape", GRID, ids=_id)
def test_bn_bwd(shape, mode, mask):
    _run_bwd(*shape, mode, mask)


def test_bn_bwd_grid_stride():
    _assert_grid_stride(*BIG)
    _run_bwd(*BIG, 2, "y")


@pytest.mark.parametrize("shape", [(64, R) for R in bn_rows(64)] + [BIG], ids=_id)
def test_bn_bwd_deterministic(shape):
    """set_deterministic(True): the reduce writes each block's sums into its own `partial` row and det_fold_kernel
    adds the rows in block order; the same checks."""
    from imagent_amd.ops import conv as cv
    prev = cv.deterministic()
    cv.set_deterministic(True)
    try:
        for mode, mask in ([(2, "y")] if shape == BIG else BWD):
            _run_bwd(*shape, mode, mask)
    finally:
        cv.set_deterministic(prev)


# ===================================================================== imk_bn_bwd_apply

APPLY = [(0, "x", 0), (1, "y", 0), (1, "y", 2), (2, "y", 0)]  # (mode, the mask the pre-masked g was made with, sgx_row)


def _g8(n, exp):
    return (torch.full((n,), 0x55, device=DEV, dtype=torch.uint8), torch.tensor([exp], device=DEV, dtype=torch.int32),
            torch.zeros(SLOTS, device=DEV))


def _check_g8(what, g8, stored, ref, exp, saturates):
    q, _, amax = g8
    top = ref.abs().max().item() * 2.0 ** -exp  # (the case's precondition, on the reference)
    assert top > 1.01 * 57344 if saturates else top < 0.99 * 57344, (what, top)
    scaled = stored.float() * 2.0 ** -exp
    _eq(what + " e5m2 bytes", q, scaled.clamp(-57344, 57344).to(torch.float8_e5m2).view(torch.uint8).reshape(-1))
    assert amax.max().item() == stored.abs().max().item() and (amax >= 0).all(), what


def _run_apply(C, R, mode, mask, sgx_row, fold_in, g8=None):
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import _g8desc, bn_apply_backward
    o, ref, d, d2 = _bwd_case(C, R, mode, mask)
    g = ref["gm"].to(torch.bfloat16)  # pre-masked by the producing dgrad
    bn, bn2 = _bn(C, o.gamma, o.beta, o.save, 0), _bn(C, o.gamma2, o.beta2, o.save2, 2)
    other = _bn(C, o.gamma2, o.beta2, o.save2, 4) if sgx_row else None  # the BN whose slab holds the sums
    decoy = _prefill(C, 5).double() * 0.25
    rows = [ref["Sgx"], ref["Sg"], ref["Sgx2"]] if not sgx_row else [decoy, ref["Sg"], ref["Sgx"]]
    scratch = (other or bn).work.scratch
    scratch.zero_()
    scratch[:SLOTS * 3 * C].view(SLOTS, 3, C).copy_(split_slots(torch.stack(rows), SLOTS, 0.25, 9))
    x2 = o.x2 if mode == 2 else None
    if fold_in:
        dx, dx2 = bn_apply_backward(g, o.x, x2, bn, bn2 if mode == 2 else None, mode, g8=g8, slab_of=other,
                                    sgx_row=sgx_row)
    else:
        m2 = mode == 2
        guards = [_guarded_bf16(R, C), _guarded_bf16(R, C)]
        dx, dx2 = guards[0].t, (guards[1].t if m2 else None)
        _lib.check(_lib.kernels().imk_bn_bwd_apply(
            g.data_ptr(), o.x.data_ptr(), bn.work.save.data_ptr(), bn.weight.data_ptr(), _lib.ptr(x2),
            bn2.work.save.data_ptr() if m2 else None, bn2.weight.data_ptr() if m2 else None, scratch.data_ptr(),
            dx.data_ptr(), _lib.ptr(dx2), bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(),
            bn2.weight.grad.data_ptr() if m2 else None, bn2.bias.grad.data_ptr() if m2 else None, R, C, mode,
            _g8desc(g8), sgx_row, 0, _lib.stream_ptr()), "bn bwd apply")
        torch.cuda.synchronize()
        guards[0].check("dx")
        guards[1].check("dx2")
    torch.cuda.synchronize()
    _check_bwd(o, ref, d, d2, mode, bn, bn2, dx, dx2, scratch, sgx_row, decoy)
    if other is not None:
        _eq("the slab owner's dgamma", other.weight.grad, _prefill(C, 4))
        _eq("the slab owner's dbeta", other.bias.grad, _prefill(C, 5))
    return dx, dx2


@pytest.mark.parametrize("fold_in", [1, 0], ids=["fold_in", "fold_launch"])
@pytest.mark.parametrize("mode,mask,sgx_row", APPLY, ids=_id)
@pytest.mark.parametrize("shape", GRID, ids=_id)
def test_bn_bwd_apply(shape, mode, mask, sgx_row, fold_in):
    _run_apply(*shape, mode, mask, sgx_row, fold_in)


@pytest.mark.parametrize("fold_in", [1, 0], ids=["fold_in", "fold_launch"])
def test_bn_bwd_apply_grid_stride(fold_in):
    """Mode 2 (UB = 2 rows per thread per iteration on a grid sized for U = 4)."""
    _assert_grid_stride(*BIG)
    _run_apply(*BIG, 2, "y", 0, fold_in)


# (mode, mask, sgx_row, exponents of dx / dx2 (None: no copy), which of them saturate e5m2)
G8 = [(0, "x", 0, (0, None), (False, False)), (1, "y", 2, (-15, None), (True, False)),
      (2, "y", 0, (3, -15), (False, True)), (2, "y", 0, (-2, None), (False, False))]


@pytest.mark.parametrize("mode,mask,sgx_row,exps,sat", G8, ids=_id)
@pytest.mark.parametrize("C", Q_CS)
def test_bn_bwd_apply_g8(C, mode, mask, sgx_row, exps, sat):
    """The e5m2 copies of dx / dx2 are the quantised STORED bf16 values, each amax row's maximum max |stored|."""
    R = bn_rows(C)[3]
    g8 = tuple(_g8(R * C, e) if e is not None else None for e in exps)
    dx, dx2 = _run_apply(C, R, mode, mask, sgx_row, 1, g8=g8)
    ref = _bwd_case(C, R, mode, mask)[1]
    _check_g8("dx", g8[0], dx, ref["dx"], exps[0], sat[0])
    if g8[1] is not None:
        _check_g8("dx2", g8[1], dx2, ref["dx2"], exps[1], sat[1])


def test_bn_bwd_apply_refusals():
    _raises(-102, lambda: _run_apply(24, 3, 0, "x", 0, 1, g8=(_g8(72, 0), None)))
    _raises(-100, lambda: _run_apply(24, 3, 2, "y", 2, 1))
    torch.cuda.synchronize()


# ===================================================================== per-channel kernels

PC_CS = (8, 24, 1000, 2048)


@pytest.mark.parametrize("use_shift", [0, 1])
@pytest.mark.parametrize("C", PC_CS)
def test_bn_stats_finalize(C, use_shift):
    """imk_bn_stats_finalize and imk_bn_finalize_affine: (mean, biased variance) of a known slab within 4 fp32 ulps
    of the sum of the magnitudes of the terms; save = (that mean, bit for bit; rsqrt(var + eps)), ss = (gamma rstd,
    beta - mean gamma rstd) against fp64 of the stored statistics."""
    from imagent_amd.ops import _lib
    k = _lib.kernels()
    R = bn_rows(C)[3]
    o = _fwd_ops(C, R)
    x, shift, slab, mean, var, tol_m, tol_v = _slab_case(C, R)
    if not use_shift:
        mean, tol_m = mean - shift.double(), U22 * (mean - shift.double()).abs()
    slab = slab.contiguous()
    out = torch.full((2, C), float("nan"), device=DEV)
    _lib.check(k.imk_bn_stats_finalize(slab.data_ptr(), shift.data_ptr() if use_shift else None, out.data_ptr(),
                                       SLOTS, C, R, _lib.stream_ptr()), "finalize")
    torch.cuda.synchronize()
    _close("mean", out[0], mean, tol_m)
    _close("variance", out[1], var, tol_v)
    out2 = torch.full((2, C), float("nan"), device=DEV)
    save = torch.stack([shift, torch.full_like(shift, -7.0)])
    ss = torch.full((2, C), float("nan"), device=DEV)
    _lib.check(k.imk_bn_finalize_affine(slab.data_ptr(), save.data_ptr(), out2.data_ptr(), o.gamma.data_ptr(),
                                        o.beta.data_ptr(), ss.data_ptr(), SLOTS, C, R, o.eps, use_shift,
                                        _lib.stream_ptr()), "finalize + affine")
    torch.cuda.synchronize()
    _close("mean (finalize + affine)", out2[0], mean, tol_m)
    _close("variance (finalize + affine)", out2[1], var, tol_v)
    rstd = 1.0 / torch.sqrt(out2[1].double() + o.eps)
    _check_save(save, out2[0], rstd)
    sc = o.gamma.double() * rstd
    _close("scale", ss[0], sc, U22 * sc.abs())
    _close("shift", ss[1], o.beta.double() - out2[0].double() * sc,
           U22 * (o.beta.double().abs() + (out2[0].double() * sc).abs()))


@pytest.mark.parametrize("use_shift", [0, 1])
@pytest.mark.parametrize("shape", GRID + [BIG], ids=_id)
def test_bn_stats_det(shape, use_shift):
    """imk_bn_stats_det (the deterministic mode's forward statistics): slot 0 of the slab += (sum d, sum d^2) of an
    integer y around an integer shift, equal to the fp64 sums; the other slots and the words past the partial rows
    stay as they were."""
    from imagent_amd.ops import _lib
    k = _lib.kernels()
    C, R = shape
    y, shift, _, _, _, _, _ = _slab_case(C, R)
    d = y.double() - (shift.double() if use_shift else 0.0)
    sums = torch.stack([d.sum(0), (d * d).sum(0)])
    assert sums.abs().max().item() + 64 < 2 ** 23
    slab = torch.stack([_prefill(C, s) for s in range(2 * SLOTS)]).view(SLOTS, 2, C).contiguous()
    want = slab.double()
    want[0] += sums
    n = k.imk_bn_stats_det_floats(R, C)
    part = torch.full((n + 64,), -7.0, device=DEV)
    _lib.check(k.imk_bn_stats_det(y.data_ptr(), shift.data_ptr() if use_shift else None, slab.data_ptr(),
                                  part.data_ptr(), R, C, _lib.stream_ptr()), "bn stats (deterministic)")
    torch.cuda.synchronize()
    _eq("slab", slab, want)
    assert (part[n:] == -7.0).all()


def _table(descs):
    return torch.frombuffer(bytearray(bytes(memoryview(descs))), dtype=torch.uint8).to(DEV)


@pytest.mark.parametrize("Cs", [(8, 1000), (2048, 24)], ids=_id)
def test_bn_running_update(Cs):
    """One launch over a table of two BNs of different C and R (built as models/native.py builds it): momentum 0.1,
    the unbiased variance (R / (R - 1)), num_batches_tracked + 1."""
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import running_update
    descs = (_lib.RunDesc * 2)()
    keep, want = [], []
    for d, C, R, nbt0 in zip(descs, Cs, (37, 5001), (0, 41)):
        o = _fwd_ops(C, bn_rows(C)[0])
        stats = torch.stack([o.mean, o.var])
        rmean, rvar = o.mean2.clone(), o.var2.clone()
        nbt = torch.tensor(nbt0, device=DEV, dtype=torch.long)
        d.sums, d.rmean, d.rvar, d.nbt = stats.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), nbt.data_ptr()
        d.C, d.momentum, d.inv_cnt, d.unbias = C, 0.1, 1.0 / R, R / max(1, R - 1)
        m, ub = float(ctypes.c_float(0.1).value), float(ctypes.c_float(R / (R - 1)).value)
        keep.append((stats, rmean, rvar, nbt))
        want.append(((1 - m) * o.mean2.double(), m * o.mean.double(), (1 - m) * o.var2.double(),
                     m * o.var.double() * ub, nbt0 + 1))
    running_update(_table(descs), 2)
    torch.cuda.synchronize()
    for (stats, rmean, rvar, nbt), (a, b, c, e, n) in zip(keep, want):
        _close("running_mean", rmean, a + b, U22 * (a.abs() + b.abs()))
        _close("running_var", rvar, c + e, U22 * (c.abs() + e.abs()))
        assert nbt.item() == n


@pytest.mark.parametrize("Cs", [(8, 1000), (2048, 24)], ids=_id)
def test_bn_eval_affine(Cs):
    """imk_bn_eval_affine over a table of two BNs: out = [gamma rstd; beta - running_mean gamma rstd]."""
    from imagent_amd.ops import _lib
    descs = (_lib.AffDesc * 2)()
    keep = []
    for d, C in zip(descs, Cs):
        o = _fwd_ops(C, bn_rows(C)[0])
        out = torch.full((2, C), float("nan"), device=DEV)
        d.gamma, d.beta, d.rmean, d.rvar = o.gamma.data_ptr(), o.beta.data_ptr(), o.mean.data_ptr(), o.var.data_ptr()
        d.out, d.C, d.eps = out.data_ptr(), C, o.eps
        keep.append((o, out))
    _lib.check(_lib.kernels().imk_bn_eval_affine(_table(descs).data_ptr(), 2, _lib.stream_ptr()), "bn eval affine")
    torch.cuda.synchronize()
    for o, out in keep:
        sc = o.gamma.double() / torch.sqrt(o.var.double() + float(ctypes.c_float(o.eps).value))
        _close("scale", out[0], sc, U22 * sc.abs())
        _close("shift", out[1], o.beta.double() - o.mean.double() * sc,
               U22 * (o.beta.double().abs() + (o.mean.double() * sc).abs()))
