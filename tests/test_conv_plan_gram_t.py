"""The dispatch plan of the conv1 dgrads that also form T = g^T h2 (csrc/kernels/conv_plan.h gramt_plan; IGemmArgs
gt_h2 / gt_T / gt_p), without a GPU: the covered argument sets map to conv_stream.hip's modes 6 / 7, every other set
with gt_T given is the error -125 (never a kernel that would ignore T), and the same arguments without gt_T plan
exactly as before (tests/test_conv_plan.py holds the whole recorded grid to the parent's table)."""

import ctypes as C
import os
import sys

import pytest

from imagent_amd.ops import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import conv_dispatch_grid as G  # noqa: E402

CUS = 256


@pytest.fixture(scope="module", autouse=True)
def _build():
    from imagent_amd import build
    build.build_runtime()


def plan(a, tile=0, gt=None):
    """(return code, [kernel names], listed) of the argument dict ``a``; gt = (h2 given, T given, p)"""
    s = _lib.IGemmArgs()
    for f in G.INTS:
        setattr(s, f, a[f])
    for f in G.PTRS:
        setattr(s, f, 4096 if a[f] else None)
    if gt is not None:
        s.gt_h2, s.gt_T, s.gt_p = (4096 if gt[0] else None), (8192 if gt[1] else None), gt[2]
    rt = _lib.runtime()
    out = (C.c_int32 * rt.imr_conv_plan_out_ints())()
    assert rt.imr_conv_plan(C.byref(s), tile, CUS, 0, out) == 0
    per = (len(out) - 2) // 2
    names = [C.string_at(C.addressof(out) + 4 * (2 + i * per + 3)).decode() for i in range(out[1])]
    listed = all(out[2 + i * per + 2] == 1 for i in range(out[1]))
    return out[0], names, listed


def conv1_dgrad(N, H, K, x2=False, sub2=False, **kw):
    """the accumulating dgrad of a bottleneck's conv1 (256 -> K, 1x1) with the fused BN backward from the mask bits,
    without x"""
    (a,) = G.dgrad(N, 256, H, K, 1, 1, 0, accumulate=True, **G.bnb("nox", x2))
    if sub2:
        a = G._with(a, flags=G.ACCUM_SUB2)
    return G._with(a, **kw)


COVERED = [
    (dict(K=64), "conv_stream_kernel<64, 128, 3, 6, false, false, 0>", "conv_stream_kernel<64, 128, 3, 1, false, false, 0>"),
    (dict(K=64, x2=True), "conv_stream_kernel<64, 128, 3, 7, false, false, 0>",
     "conv_stream_kernel<64, 128, 3, 3, false, false, 0>"),
    (dict(K=128, sub2=True), "conv_stream_kernel<128, 128, 2, 6, false, false, 0>",
     "conv_stream_kernel<128, 128, 2, 1, false, false, 0>"),
    (dict(K=128), "conv_stream_kernel<128, 128, 2, 6, false, false, 0>",
     "conv_stream_kernel<128, 128, 2, 1, false, false, 0>"),
]


@pytest.mark.parametrize("N", [2, 256, 4096])
@pytest.mark.parametrize("kw,fused,plain", COVERED, ids=["k64", "k64-x2", "k128-sub2", "k128"])
def test_covered_sets_take_the_t_kernels(kw, fused, plain, N):
    a = conv1_dgrad(N, 56, **kw)
    assert plan(a, gt=(1, 1, 64)) == (0, [fused], True)
    # without gt_T: the parent's kernel, whatever the other two fields hold
    assert plan(a) == (0, [plain], True)
    assert plan(a, gt=(1, 0, 64)) == (0, [plain], True)


def test_uncovered_sets_are_errors():
    ok = conv1_dgrad(256, 56, 64)
    assert plan(ok, gt=(1, 1, 64))[0] == 0
    bad = {
        "x given": G._with(ok, bnx=1),
        "no accumulate": dict(ok, flags=ok["flags"] & ~G.ACCUM),
        "no BN backward": dict(G.dgrad(256, 256, 56, 64, 1, 1, 0, accumulate=True)[0]),
        "mask from x": G._with(G.dgrad(256, 256, 56, 64, 1, 1, 0, accumulate=True, **G.bnb("x"))[0]),
        "streaming kernel off": G._with(ok, flags=G.NOSTREAM),
        "register-staged": G._with(ok, flags=G.REGSTAGE),
        "K = 128 with a second branch": conv1_dgrad(256, 56, 128, x2=True),
        "K = 256 (p = 64)": conv1_dgrad(256, 56, 256),
        "3x3": G._with(G.dgrad(256, 256, 56, 64, 3, 1, 1, accumulate=True, **G.bnb("nox"))[0]),
        "forward fused output": G.fwd(256, 64, 56, 256, 1, 1, 0, **G.MASK_KW),
    }
    for what, a in bad.items():
        rc, names, _ = plan(a, gt=(1, 1, 64))
        assert (rc, names) == (-125, []), (what, rc, names)
    # p: 128 (K = 128 into 512) and 256 (K = 256 into 1024) are not built; p must be Nout / 4; h2 must be given
    (a512,) = G.dgrad(256, 512, 28, 128, 1, 1, 0, accumulate=True, **G.bnb("nox"))
    (a1024,) = G.dgrad(256, 1024, 14, 256, 1, 1, 0, accumulate=True, **G.bnb("nox"))
    for what, a, gt in (("p = 128", a512, (1, 1, 128)), ("p = 256", a1024, (1, 1, 256)), ("p != Nout / 4", ok, (1, 1, 128)),
                        ("no h2", ok, (0, 1, 64)), ("p = 0", ok, (1, 1, 0))):
        rc, names, _ = plan(a, gt=gt)
        assert (rc, names) == (-125, []), (what, rc, names)
    # an explicit tile is a request for another kernel: refused too
    for tile in (2, 18, 21, 22):
        assert plan(ok, tile=tile, gt=(1, 1, 64))[:2] == (-125, []), tile
    # the BN-backward operand check still comes first (no x needs the staged epilogue)
    assert plan(dict(ok, bnsave=0), gt=(1, 1, 64))[0] == -104
    assert plan(G._with(ok, flags=G.EPI_DIRECT), gt=(1, 1, 64))[:2] == (-104, [])


def test_error_is_explained():
    rt = _lib.runtime()
    why = rt.imr_conv_error_reason(-125).decode()
    assert "g^T h2" in why and "-125" not in why
    with pytest.raises(RuntimeError, match=r"conv dgrad \(.*gt_T.*\) failed with code -125$"):
        _lib.check_conv(-125, "conv dgrad")


def test_args_struct_matches():
    rt = _lib.runtime()
    assert rt.imr_conv_args_size() == C.sizeof(_lib.IGemmArgs)
    assert [f for f, _ in _lib.IGemmArgs._fields_][-3:] == ["gt_h2", "gt_T", "gt_p"]
