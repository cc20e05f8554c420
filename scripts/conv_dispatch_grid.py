"""The case grid of the forward / dgrad conv dispatch table (tests/data/conv_dispatch_parent.jsonl).

Deterministic, no randomness: `cases()` lists every case, each a dict of IGemmArgs fields (pointers as 0 / 1: the
dispatch only tests them for null), `tile` and `deep` (IMAGENT_V3_DEEP). tests/test_conv_plan.py imports this module
and checks csrc/kernels/conv_plan.h against the table recorded from the commit before the plan existed; how that
table was recorded: profiles/conv_plan_refactor.md.

    python scripts/conv_dispatch_grid.py                              # case count by group
    python scripts/conv_dispatch_grid.py --record LIB.so OUT.jsonl   # record the table from a recorder build
"""

from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# IG_* (csrc/kernels/conv_args.h)
OUT_F32, RELU, STEM, ACCUM, REGSTAGE, BNBWD, EPI_LDS, EPI_DIRECT = 1, 2, 4, 8, 16, 32, 64, 128
FP8, BF8X, AFFINE, NOSTREAM, ACCUM_SUB2, RES, MASKOUT, Q8OUT, NEXT1 = 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536

INTS = ("N", "H", "W", "C", "OH", "OW", "M", "Nout", "ldb", "sA", "nth", "ntw", "dh0", "dhs", "dw0", "dws", "kh0",
        "khs", "kw0", "kws", "KW", "YH", "YW", "sY", "oy", "ox", "ldy", "flags", "C2", "Co2", "ldb2")
PTRS = ("X", "Wk", "Y", "bias", "stats", "bnx", "bnym", "bnsave", "bngamma", "bnbeta", "bnx2", "bnsave2", "xexp",
        "wexp", "shift", "xbn", "X2", "Y8", "y8exp", "y8amax", "W2", "Y2", "stats2", "shift2")
# a 1x1 stride-1 forward's constants, everything else 0: what fwd() / dgrad() fill in
_BLANK = dict({f: 0 for f in INTS + PTRS}, X=1, Wk=1, Y=1, sA=1, nth=1, ntw=1, dhs=1, dws=1, khs=1, kws=1, KW=1, sY=1)

BATCHES = (2, 32, 256, 1024, 2048, 4096)
TILES = tuple(range(0, 10)) + tuple(range(17, 24)) + tuple(range(27, 33))


def out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def fwd(N, Ci, H, Co, k, s, p, stem=False, **kw):
    """ops/conv.py igemm_fwd's arguments"""
    OH = out_size(H, k, s, p)
    a = dict(_BLANK, N=N, H=H, W=H, C=Ci, OH=OH, OW=OH, M=N * OH * OH, Nout=Co, ldb=k * 32 if stem else k * k * Ci, sA=s,
             nth=k, ntw=k, dh0=-p, dw0=-p, KW=k, YH=OH, YW=OH, ldy=Co, flags=STEM if stem else 0)
    return _with(a, **kw)


def dgrad(N, Ci, H, Co, k, s, p, accumulate=False, **kw):
    """ops/conv.py igemm_dgrad's arguments, one per computed parity class, for the conv Ci -> Co on H x H"""
    OH = out_size(H, k, s, p)
    skip_empty = accumulate or (s > 1 and k < s)
    out = []
    for ph in range(s):
        for pw in range(s):
            gh, gw = (H - ph + s - 1) // s, (H - pw + s - 1) // s
            if gh <= 0 or gw <= 0:
                continue
            kh0, kw0 = (ph + p) % s, (pw + p) % s
            nth, ntw = max(0, (k - kh0 + s - 1) // s), max(0, (k - kw0 + s - 1) // s)
            if skip_empty and (nth == 0 or ntw == 0):
                continue
            a = dict(_BLANK, N=N, H=OH, W=OH, C=Co, OH=gh, OW=gw, M=N * gh * gw, Nout=Ci, ldb=k * k * Co, sA=1, nth=nth,
                     ntw=ntw, dh0=(ph + p - kh0) // s, dhs=-1, dw0=(pw + p - kw0) // s, dws=-1, kh0=kh0, khs=s, kw0=kw0,
                     kws=s, KW=k, YH=H, YW=H, sY=s, oy=ph, ox=pw, ldy=Ci, flags=ACCUM if accumulate else 0)
            out.append(_with(a, **kw))
    return out


def _with(a, flags=0, **kw):
    a = dict(a, **kw)
    a["flags"] |= flags
    return a


def model_convs():
    """Every distinct conv (Ci, H, Co, k, stride, pad) ResNet-18 and ResNet-50 issue at 224 input, in model order; the
    stem as its padded 4-channel form. Then the fc layers (in_features, out_features)."""
    from imagent_amd.models import resnet
    convs, fcs = [], []

    def add(c, h):
        s = (c.in_channels, h, c.out_channels, c.kh, c.stride, c.padding)
        if s not in convs:
            convs.append(s)
        return out_size(h, c.kh, c.stride, c.padding)

    for arch in ("resnet18", "resnet50"):
        m = resnet.build(arch)
        h = out_size(224, m.conv1.kh, m.conv1.stride, m.conv1.padding)
        stem = (m.STEM_CPAD, 224, m.conv1.out_channels, m.conv1.kh, m.conv1.stride, m.conv1.padding)
        if stem not in convs:
            convs.append(stem)
        h = out_size(h, 3, 2, 1)  # max pool
        for b in m.blocks():
            hin = h
            for c, _, _ in b.convs_bns():
                h = add(c, h)
            if b.downsample is not None:
                add(b.downsample[0], hin)
        if (m.fc.in_features, m.fc.out_features) not in fcs:
            fcs.append((m.fc.in_features, m.fc.out_features))
    return convs, fcs


# ---- the forms a conv occurs in
STATS = dict(stats=1, shift=1)
EVAL = dict(flags=AFFINE, bias=1)
FUSED = dict(flags=AFFINE | RELU, bias=1)  # a training block's fused output rides on the folded BatchNorm
# the base case the table's lines are written against (a line holds the fields that differ from it): the 256 -> 256 1x1
# forward at 14 x 14 on 256 images, with statistics
BASE = fwd(256, 256, 14, 256, 1, 1, 0, **STATS)


def bnb(mask, x2=False):
    """IG_BNBWD with the ReLU mask from the mask bits ('bits'), recomputed from x ('x'), or the bits without x ('nox')"""
    kw = dict(flags=BNBWD, stats=1, bnsave=1, bngamma=1, bnbeta=1, bnx=int(mask != "nox"), bnym=int(mask != "x"))
    if x2:
        kw.update(bnx2=1, bnsave2=1)
    return kw


BNB_FORMS = [bnb(m, x2) for m in ("bits", "x", "nox") for x2 in (False, True)]
RES_KW = dict(FUSED, flags=AFFINE | RELU | RES, bnx=1)
MASK_KW = dict(FUSED, flags=AFFINE | RELU | MASKOUT, bnym=1)
Q8_KW = dict(FUSED, flags=AFFINE | RELU | Q8OUT, Y8=1, y8exp=1, y8amax=1)
ALL_OUT = dict(FUSED, flags=AFFINE | RELU | RES | MASKOUT | Q8OUT, bnx=1, bnym=1, Y8=1, y8exp=1, y8amax=1)
NEXT1_KW = dict(FUSED, flags=AFFINE | RELU | RES | MASKOUT | NEXT1, bnx=1, bnym=1, W2=1, Y2=1, stats2=1, shift2=1, Co2=64,
                ldb2=256)
FP8_F = dict(flags=FP8, xexp=1, wexp=1)
FP8_D = dict(flags=FP8 | BF8X, xexp=1, wexp=1)
SWITCHES = (NOSTREAM, REGSTAGE, EPI_LDS, EPI_DIRECT)


def gram(N, C, C2, Nout, H, mask="bits", **kw):
    """the two-segment Gram-form conv3 dgrad (bn_gram.hip): K = [g (C) | h2 (C2)] into Nout channels, 1x1"""
    a = fwd(N, C, H, Nout, 1, 1, 0, X2=1, C2=C2, ldb=C + C2, bias=1, **bnb(mask))
    return _with(a, **kw)


def cases():
    """[(group, args, tile, deep)] -- every case, in a fixed order"""
    convs, fcs = model_convs()
    body = [c for c in convs if c[0] != 4]
    stem = [c for c in convs if c[0] == 4][0]
    out, seen = [], set()

    def add(group, a, tile=0, deep=0):
        for x in (a if isinstance(a, list) else [a]):
            key = (tuple(x[f] for f in INTS + PTRS), tile, deep)
            if key not in seen:  # (the two models share shapes, and some forms coincide)
                seen.add(key)
                out.append((group, x, tile, deep))

    # 1. every model conv, forward at three batch sizes and dgrad (all parity classes) at two, stem, fc; the convs whose
    # choice turns on the batch size (enough 256x256 tiles, whole rounds of them) at every batch size
    sweep = [c for c in body if c in ((256, 14, 256, 3, 1, 1), (1024, 14, 256, 1, 1, 0), (512, 7, 512, 3, 1, 1))]
    assert len(sweep) == 3
    for c in body:
        for N in (BATCHES if c in sweep else (32, 256, 2048)):
            add("fwd", fwd(N, *c, **STATS))
        for N in (256, 2048):
            add("dgrad", dgrad(N, *c))
    for N in (2, 256):
        add("stem", fwd(N, *stem, stem=True, **STATS))
    for fin, fout in fcs:
        add("fc", fwd(256, fin, 1, fout, 1, 1, 0, flags=OUT_F32, bias=1))
        add("fc", dgrad(256, fin, 1, fout, 1, 1, 0))
    # 2. the forms a conv occurs in, on the convs of each routing (halo, streaming K = 64 / 128 / 256, strided, tiled)
    N = 256
    for f in ({}, EVAL, FUSED):
        add("stem", fwd(N, *stem, stem=True, **f))
    formed = [c for c in body if c in ((64, 56, 64, 3, 1, 1), (64, 56, 256, 1, 1, 0), (256, 56, 64, 1, 1, 0),
                                       (128, 56, 128, 3, 2, 1), (256, 14, 256, 3, 1, 1), (256, 14, 1024, 1, 1, 0),
                                       (128, 28, 128, 3, 1, 1), (128, 28, 512, 1, 1, 0), (512, 28, 128, 1, 1, 0),
                                       (512, 28, 1024, 1, 2, 0), (512, 7, 512, 3, 1, 1), (512, 7, 2048, 1, 1, 0))]
    assert len(formed) == 12
    for c in formed:
        k, s = c[3], c[4]
        add("plain", fwd(N, *c))
        add("eval", fwd(N, *c, **EVAL))
        add("eval", fwd(N, *c, **FUSED))
        add("accum", dgrad(N, *c, accumulate=True))
        add("fp8", fwd(N, *c, **dict(FP8_F, **STATS)))
        add("fp8", dgrad(N, *c, **FP8_D)[:1])
        if k >= s:  # (the fused BN backward needs every parity class computed)
            for f in (BNB_FORMS if s == 1 else (BNB_FORMS[0], BNB_FORMS[3])):
                add("bnbwd", dgrad(N, *c, **f))
        if s == 1:
            add("fp8", dgrad(N, *c, accumulate=True, **FP8_D))
            add("fp8", dgrad(N, *c, **dict(bnb("bits"), flags=BNBWD | FP8 | BF8X, xexp=1, wexp=1)))
        if k == 1:
            add("accum", dgrad(N, *c, accumulate=True, flags=ACCUM_SUB2))  # (the consumer of a sparse stride-2 dgrad)
            for f in (RES_KW, MASK_KW, Q8_KW, ALL_OUT):
                add("fused", fwd(N, *c, **f))
        if c[0] in (64, 128) and s == 1:
            add("xbn", fwd(N, *c, xbn=1, **STATS))
        if c[0] == 64 and c[2] == 256:
            add("next1", fwd(N, *c, **NEXT1_KW))
    # the 112-wide halo kernel (no model conv: a 448-pixel input's first stage)
    add("halo112", fwd(32, 64, 112, 64, 3, 1, 1, **STATS))
    add("halo112", dgrad(32, 64, 112, 64, 3, 1, 1, **bnb("bits")))
    add("halo112", dgrad(32, 64, 112, 64, 3, 1, 1, **bnb("bits", True)))
    # the register-staged kernel's fused (direct) BN-backward epilogue, both gather modes; its 128x128 tile off C % 64
    for ci in (128, 72):
        add("rs", dgrad(32, 64, 28, ci, 3, 1, 1, **dict(bnb("bits"), flags=BNBWD | EPI_DIRECT)))
        add("rs", dgrad(32, 128, 28, ci, 3, 1, 1, **dict(bnb("x"), flags=BNBWD | EPI_DIRECT | REGSTAGE)))
    for f in (0, EPI_DIRECT):
        add("rs", fwd(32, 72, 28, 128, 3, 1, 1, flags=REGSTAGE | f, **STATS))
        add("rs", fwd(32, 128, 28, 128, 3, 1, 1, flags=REGSTAGE | f, **STATS))
    add("x2", gram(32, 256, 64, 64, 56))                    # the 256 + 64 -> 64 Gram form
    add("x2", gram(32, 256, 64, 64, 56, mask="x"))
    add("x2", gram(32, 256, 64, 64, 56), tile=18)
    add("x2", gram(256, 512, 128, 128, 28))                 # shapes only the v3 loop takes, both tile sizes
    add("x2", gram(32, 1024, 256, 256, 14))
    add("x2", gram(2048, 1024, 256, 256, 14))
    for N in (256, 1024, 2048):
        # the LDS-DMA ring's two-launch split (C % 64 != 0 keeps the conv off the v3 loop) and its unsplit neighbour
        add("dma-split", fwd(N, 96, 14, 256, 3, 1, 1, **STATS))
    # 3. the A/B switches and IMAGENT_V3_DEEP
    ab = [c for c in body if c in ((64, 56, 64, 3, 1, 1), (64, 56, 256, 1, 1, 0), (256, 14, 256, 3, 1, 1),
                                   (1024, 14, 256, 1, 1, 0), (128, 56, 128, 3, 2, 1), (512, 7, 512, 3, 1, 1))]
    assert len(ab) == 6
    for c in ab:
        for sw in SWITCHES:
            add("switch", fwd(2048, *c, flags=sw, **STATS))
            add("switch", dgrad(2048, *c, **dict(bnb("bits"), flags=BNBWD | sw))[:1])
        add("switch", fwd(2048, *c, **dict(EVAL, flags=AFFINE | EPI_DIRECT)))
        add("deep", fwd(32, *c, **STATS), deep=1)
        add("deep", fwd(2048, *c, **STATS), deep=1)
        if c[3] == 3 and c[4] == 1:
            add("deep", fwd(2048, *c), deep=1)
            add("deep", fwd(2048, *c, **FUSED), deep=1)
        add("deep", dgrad(2048, *c, **bnb("x"))[:1], deep=1)
    # 4. every explicit tile on a dozen shapes
    for a in (fwd(256, 256, 14, 256, 3, 1, 1, **STATS), fwd(256, 256, 14, 1024, 1, 1, 0, **STATS),
              fwd(32, 64, 56, 256, 1, 1, 0, **STATS),
              fwd(32, 128, 28, 256, 1, 1, 0, **STATS),                           # short K: direct epilogue, C % 64 == 0
              fwd(37, 24, 11, 200, 3, 2, 1, **STATS),                            # short K: direct epilogue, C % 64 != 0
              fwd(37, 72, 11, 200, 3, 2, 1, **STATS),                            # long K, C % 64 != 0
              fwd(32, 128, 28, 64, 3, 1, 1, **STATS),                            # Nout <= 64
              fwd(64, 512, 1, 100, 1, 1, 0, flags=OUT_F32, bias=1),              # Nout % 8 != 0
              fwd(32, 128, 28, 128, 3, 1, 1, ldy=132),                           # ldy % 8 != 0
              dgrad(32, 256, 56, 64, 1, 1, 0, **bnb("bits"))[0], dgrad(256, 512, 7, 512, 3, 1, 1, **bnb("bits"))[0],
              fwd(256, 256, 14, 256, 3, 1, 1, **dict(FP8_F, **STATS))):
        for t in TILES:
            add("tile", a, tile=t)
    for t in (2, 4, 8, 17, 20, 22):
        add("tile", fwd(32, 256, 56, 64, 1, 1, 0), tile=t)
    for t in (2, 23):
        add("tile", fwd(32, *stem, stem=True, **STATS), tile=t)
    # 5. rejections: one case at least for each code argument checking returns
    c33, c11 = (64, 56, 64, 3, 1, 1), (64, 56, 256, 1, 1, 0)
    add("reject", fwd(32, *c33, flags=ACCUM | OUT_F32))                                      # -103
    add("reject", dgrad(32, *c33, **dict(bnb("bits"), bnsave=0)))                           # -104
    add("reject", dgrad(32, *c33, **dict(bnb("nox"), flags=BNBWD | EPI_DIRECT)))            # -104
    add("reject", fwd(32, *c11, **NEXT1_KW), tile=2)                                         # -122
    add("reject", fwd(32, 128, 28, 512, 1, 1, 0, **NEXT1_KW))                                # -122
    add("reject", fwd(32, 8, 224, 64, 7, 2, 3, flags=STEM))                                  # -102
    add("reject", fwd(32, *c11, xbn=1, flags=RELU))                                          # -120
    add("reject", fwd(32, 128, 28, 128, 3, 1, 1, xbn=1))                                     # -120 (no halo shape)
    add("reject", fwd(32, 256, 14, 1024, 1, 1, 0, xbn=1))                                    # -120 (K = 256)
    add("reject", fwd(32, *c11, xbn=1, flags=NOSTREAM))                                      # 1: not an error code
    add("reject", gram(32, 256, 64, 96, 56))                                                 # -106
    add("reject", gram(32, 256, 48, 64, 56), tile=17)                                        # -106
    add("reject", fwd(32, 24, 56, 64, 3, 1, 1, **FP8_F))                                     # -105
    add("reject", fwd(32, 128, 28, 128, 3, 1, 1, **dict(FP8_F, flags=FP8 | ACCUM)))          # -105
    add("reject", dgrad(32, 64, 56, 64, 3, 1, 1, **dict(bnb("bits"), flags=BNBWD | FP8 | BF8X | EPI_DIRECT,
                                                        xexp=1, wexp=1)))                     # -104 (fp8)
    add("reject", fwd(32, 64, 56, 64, 1, 1, 0, **FP8_F), tile=5)                             # -101 (fp8)
    add("reject", fwd(32, 12, 56, 64, 3, 1, 1))                                              # -100
    add("reject", fwd(32, 72, 28, 128, 3, 1, 1), tile=17)                                    # -105
    add("reject", fwd(32, 128, 28, 128, 3, 1, 1, **RES_KW))                                  # -121
    add("reject", fwd(32, *c11, flags=RES | AFFINE, bias=1))                                 # -121 (no residual)
    add("reject", fwd(32, 128, 28, 256, 1, 1, 0), tile=10)                                   # -101 (short K, direct)
    add("reject", fwd(32, 128, 28, 256, 1, 1, 0, flags=REGSTAGE), tile=5)                    # -101 (register-staged)
    add("reject", fwd(32, 128, 28, 128, 3, 1, 1), tile=10)                # 0: a staged epilogue ignores an unknown tile
    add("reject", fwd(32, 128, 28, 128, 3, 1, 1, flags=REGSTAGE), tile=5)                    # 0: likewise
    add("reject", fwd(0, *c33))                                                              # nothing to do: 0, no launch
    return out


def compact(a):
    """the fields that differ from BASE"""
    return {f: a[f] for f in INTS + PTRS if a[f] != BASE[f]}


def expand(d):
    return dict(BASE, **d)


# ---- recording the table from a kernels library built with the dry-run recorder (profiles/conv_plan_refactor.md)
_KERNEL = {"v3": "igemm_v3_kernel", "dma": "igemm_dma_kernel", "rs": "igemm_rs_kernel", "stream1": "conv_stream_kernel",
           "stem_band": "stem_band_kernel", "halo": "halo3x3_kernel"}


def _kernel_name(pretty):
    """a launcher's __PRETTY_FUNCTION__ -> the kernel name a profiler shows"""
    import re
    fam = re.search(r"launch_(\w+)\(", pretty).group(1)
    b = re.search(r"\[(.*)\]", pretty)
    params = [p.split(" = ")[1] for p in b.group(1).split(", ")] if b else ["4"]  # (launch_stem_band had R = 4 inside)
    return f"{_KERNEL[fam]}<{', '.join(params)}>"


def _record_one(lib, deep):
    """{case index: (return code, [[kernel, N, M]])} of the cases with this IMAGENT_V3_DEEP (read once per process)"""
    import ctypes as C
    from imagent_amd.ops._lib import IGemmArgs
    l = C.CDLL(lib)
    l.imk_dry_log.restype = C.c_char_p
    l.imk_conv_igemm.argtypes = [C.POINTER(IGemmArgs), C.c_int, C.c_void_p]
    assert l.imk_igemm_args_size() == C.sizeof(IGemmArgs)
    res = {}
    for i, (_, a, tile, d) in enumerate(cases()):
        if d != deep:
            continue
        s = IGemmArgs()
        for f in INTS:
            setattr(s, f, a[f])
        for f in PTRS:
            setattr(s, f, 4096 if a[f] else None)
        l.imk_dry_begin()
        rc = l.imk_conv_igemm(C.byref(s), tile, None)
        ks = [line.split("\t") for line in l.imk_dry_log().decode().splitlines()]
        res[i] = (rc, [[_kernel_name(k), int(n), int(m)] for k, n, m in ks])
    return res


def record(lib, out):
    import json
    import subprocess
    res = {}
    for deep in (0, 1):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--record-deep", lib, str(deep)], check=True,
                           env=dict(os.environ, IMAGENT_V3_DEEP=str(deep)), stdout=subprocess.PIPE)
        res.update({int(k): v for k, v in json.loads(r.stdout).items()})
    cs = cases()
    assert sorted(res) == list(range(len(cs)))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for i, (_, a, tile, deep) in enumerate(cs):
            f.write(json.dumps({"a": compact(a), "t": tile, "d": deep, "rc": res[i][0], "k": res[i][1]},
                               separators=(",", ":")) + "\n")
    print(len(cs), "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    import collections
    if len(sys.argv) == 4 and sys.argv[1] == "--record-deep":
        import json
        print(json.dumps(_record_one(sys.argv[2], int(sys.argv[3]))))
        sys.exit(0)
    if len(sys.argv) == 4 and sys.argv[1] == "--record":
        record(sys.argv[2], sys.argv[3])
        sys.exit(0)
    cs = cases()
    n = collections.Counter(g for g, *_ in cs)
    print(len(cs), dict(n))
