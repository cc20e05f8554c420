"""A Gram-form block's T = g^T h2 formed by the kernel that writes g: the next block's conv1 dgrad with the fused
BN-backward epilogue (conv_stream.hip modes 6 / 7, ``BNBwdFuse(gramt=)``, ``IMAGENT_GRAM_T``).

Exact: integer operands (|dX| <= 8 after the accumulate, h2 in {0..3}, random mask bits), so every fp32 partial sum
is exact in any order: T must EQUAL an int64 (stored dX)^T h2, dX and the slab rows sum(g), sum(g xhat2) must equal
the same call without T and the exact integer sums. Random bf16 operands: dX bit-identical to the unfused call, T
against fp64 of the stored bits within twice the stand-alone ``gram_T``'s error on the same inputs (another summation
order, the same fp32 accumulate). Uncovered combinations raise -125 and launch nothing. Model: ResNet-50 against the
fp32 model with the switch on and off, the gram_T calls that disappear, the hand-over absent, and two steps.

Shapes (N, H, W): M = 9 (one partial group, seven of a block's eight waves idle), 147 (a 3-row tail group), 6,272
(one or two groups per wave), 75,264 (more groups than resident waves x prefetch depth); K = 128 with ``old_sub2``
on even-sized grids.
"""

import types

import pytest
import torch

from exact_ref import bn_consts, ints, kernel_names, mask_bytes, mask_from_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 64

SHAPES = [(1, 3, 3), (3, 7, 7), (2, 56, 56), (24, 56, 56)]
SUB2_SHAPES = [(2, 8, 8), (6, 56, 56)]
# (id, K of the dgrad, second BN branch, old_sub2, shapes)
FORMS = [("k64-mode6", 64, False, False, SHAPES), ("k64-mode7-x2", 64, True, False, SHAPES),
         ("k128-sub2", 128, False, True, SUB2_SHAPES)]
CASES = [pytest.param(k, x2, sub2, s, id=f"{name}-{s[0]}x{s[1]}x{s[2]}") for name, k, x2, sub2, shapes in FORMS
         for s in shapes]
KERNEL = {(64, False): "conv_stream_kernel<64, 128, 3, 6", (64, True): "conv_stream_kernel<64, 128, 3, 7",
          (128, False): "conv_stream_kernel<128, 128, 2, 6"}


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _bn(C, seed):
    """What BNBwdFuse reads of a BatchNorm (integer means, rstd = 1): weight, bias, work.save, work.scratch."""
    from imagent_amd.ops import _lib
    save, gamma, beta = bn_consts(C, seed, DEV, integer=True)
    nbw = _lib.kernels().imk_bn_bwd_scratch_floats(1)
    return types.SimpleNamespace(weight=gamma, bias=beta,
                                 work=types.SimpleNamespace(save=save, scratch=torch.zeros(nbw * C, device=DEV)))


def _slab(bn, C):
    return bn.work.scratch[:32 * 3 * C].view(32, 3, C).double().sum(0)


def _operands(K, N, H, W, x2, sub2, exact):
    """dy [N,H,W,K], wt [256,1,1,K], old dX, mask bits, h2 [N,H,W,64], second-branch x2 -- integers (``exact``: every
    wt row has four +-1 entries and dy is in {-1, 0, 1}, so |dy wt^T| <= 4, old in [-4, 4]) or random bf16."""
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + H + K)
    C4 = 4 * P
    if exact:
        dy = ints((N, H, W, K), -1, 1, 1, DEV)
        wt = torch.zeros(C4, K, device=DEV)
        cols = torch.rand(C4, K, generator=g, device=DEV).argsort(1)[:, :4]
        wt.scatter_(1, cols, torch.randint(0, 2, (C4, 4), generator=g, device=DEV).float() * 2 - 1)
        wt = wt.to(torch.bfloat16).view(C4, 1, 1, K)
        old = ints((N, H, W, C4), -4, 4, 2, DEV)
        h2 = ints((N, H, W, P), 0, 3, 3, DEV)
        xb = ints((N, H, W, C4), -2, 2, 4, DEV) if x2 else None
    else:
        dy = torch.randn(N, H, W, K, generator=g, device=DEV).to(torch.bfloat16)
        wt = (torch.randn(C4, 1, 1, K, generator=g, device=DEV) * (2.0 / K) ** 0.5).to(torch.bfloat16)
        old = torch.randn(N, H, W, C4, generator=g, device=DEV).to(torch.bfloat16)
        h2 = torch.relu(torch.randn(N, H, W, P, generator=g, device=DEV)).to(torch.bfloat16)
        xb = torch.randn(N, H, W, C4, generator=g, device=DEV).to(torch.bfloat16) if x2 else None
    keep = torch.rand(N, H, W, C4, generator=g, device=DEV) < 0.6
    even = torch.zeros(N, H, W, 1, dtype=torch.bool, device=DEV)
    even[:, ::2, ::2] = True
    if sub2:  # only the even pixels hold a value (a sparse stride-2 dgrad wrote them): NaN elsewhere
        old = torch.where(even, old, torch.full_like(old, float("nan")))
    return types.SimpleNamespace(dy=dy, wt=wt, old=old, bits=mask_bytes(keep), keep=keep, h2=h2, x2=xb, even=even,
                                 sub2=sub2)


def _run(o, H, W, with_t, seed=7):
    """The accumulating conv1 dgrad with the fused BN backward (no x), with or without T: (dX, slab [3][256], T,
    kernel names)."""
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    C4 = 4 * P
    bn, bn2 = _bn(C4, seed), (_bn(C4, seed + 10) if o.x2 is not None else None)
    T = torch.zeros(C4, P, device=DEV) if with_t else None
    f = BNBwdFuse(None, bn, y=o.bits, x2=o.x2, bn2=bn2, gramt=(o.h2, T) if with_t else None)
    out = o.old.clone()
    _, names = kernel_names(lambda: igemm_dgrad(o.dy, o.wt, (H, W), 1, 0, 1, 1, out=out, accumulate=True, bnb=f,
                                                old_sub2=o.sub2))
    return out, _slab(bn, C4), T, names, bn2


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("K,x2,sub2,shape", CASES)
def test_gram_t_exact(K, x2, sub2, shape):
    N, H, W = shape
    o = _operands(K, N, H, W, x2, sub2, exact=True)
    C4 = 4 * P
    # the reference, all integers: v = dy wt^T + old (old_sub2: zero off the even pixels), masked
    raw = (o.dy.reshape(-1, K).double() @ o.wt.view(C4, K).double().t()).view(N, H, W, C4)
    oldv = torch.where(o.even, o.old.double(), torch.zeros((), device=DEV, dtype=torch.double)) if sub2 \
        else o.old.double()
    gm = (raw + oldv) * o.keep
    assert gm.abs().max().item() <= 8 and gm.abs().max().item() >= 4  # the precondition on |dX|; not trivially small
    assert N * H * W * 8 * 3 < 2 ** 24
    # (integers below 2^24 in an fp64 GEMM are exact: the device has no int64 GEMM)
    t_ref = (gm.reshape(-1, C4).t() @ o.h2.reshape(-1, P).double()).long()
    out1, slab1, T, names, bn2 = _run(o, H, W, True)
    out0, slab0, _, names0, _ = _run(o, H, W, False)
    torch.cuda.synchronize()
    print(f"K={K} x2={x2} sub2={sub2} M={N * H * W}: {sorted(set(n.split('(')[0] for n in names))} "
          f"max|T| {t_ref.abs().max().item()}")
    assert len(names) == 1 and KERNEL[(K, x2)] in names[0], names
    assert len(names0) == 1 and f"conv_stream_kernel<{K}, 128, {3 if K == 64 else 2}, {3 if x2 else 1}" in names0[0]
    assert torch.equal(out1.double(), gm), (out1.double() != gm).sum().item()
    assert torch.equal(_bits(out1), _bits(out0))
    assert torch.equal(T.double(), t_ref.double()), \
        f"{(T.double() != t_ref.double()).sum().item()} of {T.numel()} T entries differ"
    assert t_ref.any()
    # slab rows: sum(g) and, with the second branch, sum(g xhat2) -- integers, exact, and as the unfused call's
    # (row 0, sum(g xhat) with x absent, is what T replaces: the T modes leave it alone)
    rows = [1] + ([2] if x2 else [])
    want = {1: gm.reshape(-1, C4).sum(0)}
    if x2:
        want[2] = (gm * ((o.x2.double() - bn2.work.save[0].double()) * bn2.work.save[1].double())).reshape(-1, C4).sum(0)
        assert (gm * (o.x2.double() - bn2.work.save[0].double())).abs().reshape(-1, C4).sum(0).max().item() < 2 ** 23
    for r in rows:
        assert torch.equal(slab1[r], want[r]), (r, (slab1[r] != want[r]).sum().item())
        assert torch.equal(slab1[r], slab0[r]), r
    assert not slab1[0].any()


@pytest.mark.parametrize("K,x2,sub2,shape", CASES)
def test_gram_t_random_bf16(K, x2, sub2, shape):
    """dX bit-identical to the unfused call; T within 2 x the stand-alone gram_T's error against fp64 of the stored
    bits (the fused arm sums the same fp32 products in another order)."""
    from imagent_amd.ops.bn_gram import gram_T
    N, H, W = shape
    o = _operands(K, N, H, W, x2, sub2, exact=False)
    C4 = 4 * P
    out1, slab1, T, names, _ = _run(o, H, W, True)
    out0, slab0, _, _, _ = _run(o, H, W, False)
    t_alone = gram_T(out0, o.h2)
    torch.cuda.synchronize()
    assert KERNEL[(K, x2)] in names[0], names
    assert not torch.isnan(out0.float()).any()
    assert torch.equal(_bits(out1), _bits(out0))
    t64 = out0.reshape(-1, C4).double().t() @ o.h2.reshape(-1, P).double()
    e_fused, e_alone = rel(T, t64), rel(t_alone, t64)
    m_fused = (T.double() - t64).abs().max().item()
    m_alone = (t_alone.double() - t64).abs().max().item()
    print(f"K={K} x2={x2} sub2={sub2} M={N * H * W}: T rel err fused {e_fused:.3e} stand-alone {e_alone:.3e}; "
          f"max abs fused {m_fused:.3e} stand-alone {m_alone:.3e}")
    assert e_fused <= 2.0 * e_alone, (e_fused, e_alone)
    # the slab rows the consumers read: the same values summed in another order (fp32 atomics)
    for r in [1] + ([2] if x2 else []):
        assert rel(slab1[r], slab0[r]) < 1e-4, (r, rel(slab1[r], slab0[r]))


def test_gram_t_uncovered_is_an_error():
    """gramt with x given, without the accumulate, or with p = 256: the call raises -125 and nothing is launched (the
    output and T stay as they were)."""
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    N, H, W = 2, 8, 8
    o = _operands(64, N, H, W, False, False, exact=True)
    C4 = 4 * P
    T = torch.zeros(C4, P, device=DEV)

    def refused(fn, out):
        before = out.clone()
        launched = []
        with pytest.raises(RuntimeError, match="failed with code -125$"):
            _, names = kernel_names(fn)
            launched += names
        torch.cuda.synchronize()
        assert not launched and torch.equal(_bits(out), _bits(before)) and not T.any()

    x = ints((N, H, W, C4), -2, 2, 5, DEV)
    out = o.old.clone()
    refused(lambda: igemm_dgrad(o.dy, o.wt, (H, W), 1, 0, 1, 1, out=out, accumulate=True,
                                bnb=BNBwdFuse(x, _bn(C4, 1), y=o.bits, gramt=(o.h2, T))), out)
    refused(lambda: igemm_dgrad(o.dy, o.wt, (H, W), 1, 0, 1, 1, out=out, accumulate=False,
                                bnb=BNBwdFuse(None, _bn(C4, 1), y=o.bits, gramt=(o.h2, T))), out)
    # p = 256: K = 256 into 1024 channels
    dy = ints((N, H, W, 256), -1, 1, 1, DEV)
    wt = ints((1024, 1, 1, 256), -1, 1, 2, DEV)
    out = ints((N, H, W, 1024), -4, 4, 3, DEV)
    h2 = ints((N, H, W, 256), 0, 3, 4, DEV)
    bits = mask_bytes(torch.rand(N, H, W, 1024, device=DEV) < 0.5)
    T = torch.zeros(1024, 256, device=DEV)
    refused(lambda: igemm_dgrad(dy, wt, (H, W), 1, 0, 1, 1, out=out, accumulate=True,
                                bnb=BNBwdFuse(None, _bn(1024, 1), y=bits, gramt=(h2, T))), out)
    assert mask_from_bytes(bits, out.shape).any()


_TMODES = ("conv_stream_kernel<64, 128, 3, 6", "conv_stream_kernel<64, 128, 3, 7", "conv_stream_kernel<128, 128, 2, 6")


def _count_gram_t(monkeypatch, block):
    """Counts the gram_T calls that make their pass over g (``formed=True`` takes the T the producing dgrad left and
    launches nothing: tests/test_model_gpu.py counts every call, 15 either way)."""
    calls = []
    real = block.gram_T
    monkeypatch.setattr(block, "gram_T",
                        lambda *a, **k: (None if k.get("formed") else calls.append(1)) or real(*a, **k))
    return calls


def test_gram_t_model_matches_torch(monkeypatch):
    """ResNet-50 forward + backward against the fp32 PyTorch model (test_hip_vs_torch_forward_backward and its
    bounds) with IMAGENT_GRAM_T off, then on. On: the three layer-1 blocks' T comes from their successors' conv1
    dgrads -- three gram_T passes over g fewer, three mode-6 / 7 launches."""
    from test_model_gpu import test_hip_vs_torch_forward_backward
    from imagent_amd.ops import block
    monkeypatch.setattr(block, "_GRAM", True)
    monkeypatch.setattr(block, "_GRAM_NOX", True)
    monkeypatch.setattr(block, "_GRAM_FWD", True)
    monkeypatch.setattr(block, "_GRAM_MIN_ROWS", 0)  # every block, at this test's 16 x 64 x 64 input
    calls = _count_gram_t(monkeypatch, block)
    seen = {}
    for on in (False, True):
        monkeypatch.setattr(block, "_GRAM_T", on)
        del calls[:]
        _, names = kernel_names(lambda: test_hip_vs_torch_forward_backward("resnet50", True))
        seen[on] = (len(calls), sum(any(m in n for m in _TMODES) for n in names))
        print(f"switch {on}: (gram_T calls, mode-6/7 launches) = {seen[on]}")
    covered = 3
    assert seen[False][1] == 0 and seen[True][1] == covered, seen
    assert seen[False][0] - seen[True][0] == covered, seen


def test_gram_t_hand_over(monkeypatch):
    """Two layer-1 blocks, backward through both. Taken: the successor's dgrad forms T and the first block makes no
    gram_T pass over g. Absent (the successor's dgrad ran WITHOUT T): the first block falls back to gram_T. In both, the T the
    first block's backward used must match what the switch-off path computes from the same gradient -- gram_T on the
    very g and h2 of that step -- to 1e-2 (a stale T is zeros, rel = 1; one counted twice, rel = 1), and conv3's
    weight gradient must be finite and nonzero. Then two whole steps: T holds one step's sum, not two.

    (The arms are compared on one step's own g, not across steps: two block-level steps of this chain differ by
    1e-2 .. 4e-2 in g BEFORE the conv1 dgrad runs, with the switch off in both -- measured, profiles/ab/gram_t.txt --
    so a cross-step comparison at 1e-2 tests that variation and not the hand-over.)"""
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops import _lib, block
    from imagent_amd.ops.bn_gram import gram_T
    monkeypatch.setattr(block, "_GRAM_MIN_ROWS", 0)
    calls = _count_gram_t(monkeypatch, block)
    target = block._gram_t_target
    torch.manual_seed(0)
    model = resnet.build("resnet50", num_classes=10).to(DEV)
    st = bind_native(model, DEV)
    model.train()
    b0, b1 = model.layer1[0], model.layer1[1]
    x = torch.relu(torch.randn(4, 16, 16, 64, device=DEV)).to(torch.bfloat16)
    up = torch.randn(4, 16, 16, 256, device=DEV).to(torch.bfloat16)
    seen = {}
    real_coef = block.gram_coef
    monkeypatch.setattr(block, "gram_coef", lambda bn, g, T=None, **k: seen.update(g=g, T=T) or real_coef(bn, g, T=T, **k))

    def step(on, absent=False):
        # b1 ends the chain here: its backward gets an unmasked gradient, so its forward must keep conv3's output
        # (the form of a block without a successor)
        monkeypatch.setattr(b1, "_has_next", False)
        monkeypatch.setattr(block, "_GRAM_T", on)
        monkeypatch.setattr(block, "_gram_t_target", (lambda *a: None) if absent else target)
        _lib.zero_(st.zero_ws)
        st.arena.zero_grad()
        del calls[:]
        xi = x.clone().requires_grad_(True)
        o0 = block.BlockFn.apply(xi, b0)
        h2 = b0._gram_t[0]
        o1 = block.BlockFn.apply(o0, b1)
        _, names = kernel_names(lambda: o1.backward(up))
        torch.cuda.synchronize()
        assert not b0._T_done and b0._gram_t is None
        g, T = seen["g"], seen["T"]  # the last gram_coef call is b0's
        assert T is not None and T.data_ptr() == b0._gram_ws[0].data_ptr()
        t_off = gram_T(g, h2)  # the switch-off computation on the same gradient
        w3 = b0.convs_bns()[-1][0].weight.grad
        assert torch.isfinite(w3).all() and w3.any() and torch.isfinite(xi.grad.float()).all()
        return rel(T, t_off), len(calls), sum(any(m in n for m in _TMODES) for n in names)

    e0, n0, k0 = step(False)
    e1, n1, k1 = step(True)
    e2, n2, k2 = step(True, absent=True)
    print(f"T against gram_T of the same g: switch off {e0:.2e} (gram_T calls {n0}), hand-over taken {e1:.2e} "
          f"(calls {n1}, T launches {k1}), absent {e2:.2e} (calls {n2}, T launches {k2})")
    assert (n0, k0) == (1, 0) and (n1, k1) == (0, 1) and (n2, k2) == (1, 0)
    assert e0 < 1e-2 and e1 < 1e-2 and e2 < 1e-2, (e0, e1, e2)
    # two whole training steps of the model on the same batch (the weights do not move: no optimizer step): the
    # workspace T after the second is that step's sum alone (a T carried over would give rel = 1)
    from imagent_amd.ops.misc import normalize_u8
    monkeypatch.setattr(block, "_GRAM_T", True)
    monkeypatch.setattr(block, "_gram_t_target", target)
    monkeypatch.setattr(b1, "_has_next", True)
    img = torch.randint(0, 256, (4, 64, 64, 3), device=DEV, dtype=torch.uint8)
    xm = normalize_u8(img, (64, 64), 4, (0.5,) * 3, (0.5,) * 3)
    lab = torch.randint(0, 10, (4,), device=DEV)
    es = []
    for _ in range(2):
        st.arena.zero_grad()
        del calls[:]
        loss = torch.nn.functional.cross_entropy(model(xm), lab)
        h2 = b0._gram_t[0]
        loss.backward()
        torch.cuda.synchronize()
        # (the last gram_coef call of a whole backward is the first block's)
        assert seen["T"].data_ptr() == b0._gram_ws[0].data_ptr()
        es.append(rel(b0._gram_ws[0], gram_T(seen["g"], h2)))
    # bound: a T that also held the first step's sum differs from this step's g^T h2 by that whole sum, rel ~ 1
    print(f"two steps: T against gram_T of the step's own g {es[0]:.2e} {es[1]:.2e}")
    assert es[0] < 1e-2 and es[1] < 1e-2, es
