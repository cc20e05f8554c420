"""The forward / dgrad conv dispatch plan (csrc/kernels/conv_plan.h, exported from the host runtime as imr_conv_plan)
against the decisions of the dispatch chain it replaced, without a GPU.

tests/data/conv_dispatch_parent.jsonl holds, for every case of scripts/conv_dispatch_grid.py, what the commit before
the plan decided: the return code and each launch's kernel, N and M (recorded by a dry-run of that commit's
imk_conv_igemm, profiles/conv_plan_refactor.md). A wrong branch in the plan would not fail on the GPU -- it would run
another kernel -- so every row is compared here.
"""

import ctypes as C
import json
import os
import re
import sys

import pytest

from imagent_amd.ops import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import conv_dispatch_grid as G  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "data", "conv_dispatch_parent.jsonl")
CUS = 256  # what the recording saw: no device, the MI355X's count


@pytest.fixture(scope="module", autouse=True)
def _build():
    from imagent_amd import build
    build.build_runtime()


def struct(a):
    s = _lib.IGemmArgs()
    for f in G.INTS:
        setattr(s, f, a[f])
    for f in G.PTRS:
        setattr(s, f, 4096 if a[f] else None)
    return s


def plan(a, tile=0, deep=0, cus=CUS):
    """(return code, [(kernel name, N, M)], every kernel in its family's list)"""
    rt = _lib.runtime()
    out = (C.c_int32 * rt.imr_conv_plan_out_ints())()
    assert rt.imr_conv_plan(C.byref(struct(a)), tile, cus, deep, out) == 0
    per = (len(out) - 2) // 2
    launches, listed = [], True
    for i in range(out[1]):
        o = 2 + i * per
        name = C.string_at(C.addressof(out) + 4 * (o + 3)).decode()
        launches.append([name, out[o + 1], out[o + 1] * a["OH"] * a["OW"]])
        listed = listed and out[o + 2] == 1
    if out[1] == 2:  # the two parts are the images [0, i1) and [i1, N)
        assert (out[2], out[2 + per], out[3] + out[3 + per]) == (0, out[3], a["N"])
    return out[0], launches, listed


@pytest.fixture(scope="module")
def rows():
    with open(TABLE) as f:
        return [json.loads(line) for line in f]


@pytest.fixture(scope="module")
def cases():
    return G.cases()


def test_table_holds_the_grid(rows, cases):
    """every case the generator produces and no other, in its order"""
    assert len(rows) == len(cases)
    for r, (_, a, tile, deep) in zip(rows, cases):
        assert (r["a"], r["t"], r["d"]) == (G.compact(a), tile, deep)
        assert G.expand(r["a"]) == a


def test_plan_matches_parent(rows):
    bad = []
    for i, r in enumerate(rows):
        rc, launches, listed = plan(G.expand(r["a"]), r["t"], r["d"])
        if (rc, launches) != (r["rc"], r["k"]) or not listed:
            bad.append((i, r, rc, launches, listed))
    assert not bad, f"{len(bad)} of {len(rows)} differ, first: {bad[0]}"


def test_planned_kernels_are_listed(rows):
    """the not-in-its-list error is unreachable over the grid (imk_conv_igemm would return -124)"""
    n = 0
    for r in rows:
        rc, launches, listed = plan(G.expand(r["a"]), r["t"], r["d"])
        assert listed and rc != -124, r
        n += len(launches)
    assert n > len(rows) // 2


def _family(name, case):
    k, args = name.split("<")[0], [x.strip() for x in name.split("<")[1].rstrip(">").split(",")]
    if k == "igemm_rs_kernel":
        return "rs"
    if k == "igemm_dma_kernel":
        return "dma-fp8" if args[7] == "1" else "dma"
    if k == "igemm_v3_kernel":
        return "v3-fp8" if args[6] == "1" else "v3"
    if k == "conv_stream_kernel":
        return "stream-stem" if args[4] == "true" else f"stream-mode{args[3]}"
    if k == "stem_band_kernel":
        return "stem-band"
    assert k == "halo3x3_kernel", name
    return f"halo-epi{args[2]}"


def test_table_coverage(rows):
    """the conditions the grid was built to meet, counted from the file"""
    fams = {_family(k[0], r) for r in rows for k in r["k"]}
    want = {"rs", "dma", "v3", "v3-fp8", "dma-fp8", "stream-stem", "stem-band"} | \
        {f"stream-mode{m}" for m in range(6)} | {f"halo-epi{e}" for e in range(3)}
    assert fams == want
    codes = {r["rc"] for r in rows}
    assert {-100, -101, -102, -103, -104, -105, -106, -120, -121, -122} <= codes and 0 in codes
    assert -123 not in codes and -124 not in codes
    # both two-launch splits, each next to the same conv at another batch size that is not split
    for kern in ("igemm_v3_kernel", "igemm_dma_kernel"):
        split = [r for r in rows if len(r["k"]) == 2 and r["k"][0][0].startswith(kern)]
        assert split, kern
        shape = lambda r: {f: v for f, v in r["a"].items() if f not in ("N", "M")}  # noqa: E731
        whole = [r for r in rows if len(r["k"]) == 1 and r["t"] == 0 and
                 any(shape(r) == shape(s) and r["d"] == s["d"] for s in split)]
        assert whole and all(r["k"][0][0].startswith(kern) for r in whole), kern
    for r in rows:  # a split is the big tile on the first images, the small one on the rest
        if len(r["k"]) == 2:
            (k0, n0, m0), (k1, n1, m1) = r["k"]
            a = G.expand(r["a"])
            assert "<256, 256," in k0 and "<128, 128," in k1
            assert n0 + n1 == a["N"] and m0 + m1 == a["M"] and m0 == n0 * a["OH"] * a["OW"]
    # the tiled kernels' corners: both bf16 -101 returns (ring and register-staged), every direct-epilogue ring tile in
    # both gather modes, the register-staged kernel's fused (EPI 1) epilogue, the 112-wide halo kernel
    bf16_101 = [r for r in rows if r["rc"] == -101 and not G.expand(r["a"])["flags"] & G.FP8]
    assert any(G.expand(r["a"])["flags"] & G.REGSTAGE for r in bf16_101)
    assert any(not G.expand(r["a"])["flags"] & G.REGSTAGE and r["t"] == 10 for r in bf16_101)
    names = {k[0] for r in rows for k in r["k"]}
    direct = {n for n in names if n.startswith("igemm_dma_kernel") and n.endswith(", 0, 2, 0, 128>")}
    assert len(direct) == 18, sorted(direct)
    assert {"igemm_rs_kernel<128, 64, 1, 0, 1>", "igemm_rs_kernel<128, 64, 1, 1, 1>", "igemm_rs_kernel<128, 128, 2, 1, 2>"} <= names
    assert {f"halo3x3_kernel<112, 2, {e}>" for e in range(3)} <= names
    assert len(names) >= 94  # of the 124 listed instantiations
    # the explicit tiles and the switches all occur
    assert {r["t"] for r in rows} >= set(G.TILES)
    assert {0, 1} == {r["d"] for r in rows}
    for sw in G.SWITCHES:
        assert any(r["a"].get("flags", 0) & sw for r in rows), sw


def _tail_split_ref(a, S):
    """conv_igemm.hip's tail_split_images before the plan, line by line"""
    if a["N"] < 2 or (a["flags"] & (G.BNBWD | G.ACCUM)):
        return 0
    ohw = a["OH"] * a["OW"]
    nbn = (a["Nout"] + 255) // 256
    tiles = ((a["M"] + 255) // 256) * nbn
    full = tiles // S
    rem = tiles - full * S
    if full < 1 or rem == 0 or rem > C.c_float(C.c_float(0.3).value * S).value:
        return 0
    mt = full * S // nbn
    i1 = mt * 256 // ohw
    return i1 if 1 <= i1 < a["N"] else 0


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_tail_split_images(cus):
    """every model conv at every batch size of the grid (forward, its dgrads, and an accumulating dgrad: never split)"""
    rt = _lib.runtime()
    convs, _ = G.model_convs()
    n = split = 0
    for c in convs:
        for N in G.BATCHES:
            todo = [G.fwd(N, *c)] if c[0] == 4 else [G.fwd(N, *c)] + G.dgrad(N, *c) + G.dgrad(N, *c, accumulate=True)[:1]
            for a in todo:
                want = _tail_split_ref(a, cus)
                assert rt.imr_conv_tail_split_images(C.byref(struct(a)), cus) == want, (c, N, cus)
                n, split = n + 1, split + (want > 0)
    assert split > 5 and n > 400
    # the plan uses it: 256 -> 256 3x3 at 14 x 14 splits where the last round is a small remainder
    for N in (256, 1024, 2048, 4096):
        a = G.fwd(N, 256, 14, 256, 3, 1, 1, **G.STATS)
        i1 = _tail_split_ref(a, cus)
        rc, launches, _ = plan(a, cus=cus)
        assert rc == 0 and [l[1] for l in launches] == ([i1, N - i1] if i1 else [N])


def test_flag_names_match_the_header():
    rt = _lib.runtime()
    buf = C.create_string_buffer(32)
    got, i = {}, 0
    while True:
        v = rt.imr_conv_flag(i, buf)
        if v == 0:
            break
        got[buf.value.decode()] = v
        i += 1
    mine = {k: v for k, v in vars(_lib).items() if k.startswith("IG_")}
    assert got == mine and len(got) == 17
    header = open(os.path.join(ROOT, "imagent_amd", "csrc", "kernels", "conv_args.h")).read()
    assert dict((n, int(v)) for n, v in re.findall(r"#define (IG_\w+) (\d+)", header)) == mine
    assert sorted(mine.values()) == [1 << b for b in range(17)]
    for name in ("OUT_F32", "RELU", "STEM", "ACCUM", "REGSTAGE", "BNBWD", "EPI_LDS", "EPI_DIRECT", "FP8", "BF8X", "AFFINE",
                 "NOSTREAM", "ACCUM_SUB2", "RES", "MASKOUT", "Q8OUT", "NEXT1"):
        assert getattr(G, name) == mine["IG_" + name]


def test_conv_errors_are_explained():
    rt = _lib.runtime()
    for rc in (1, -100, -101, -102, -103, -104, -105, -106, -120, -121, -122, -123, -124):
        assert rt.imr_conv_error_reason(rc), rc
    assert rt.imr_conv_error_reason(-7) == b""
    with pytest.raises(RuntimeError, match=r"conv fwd \(.*streaming.*\) failed with code -121$"):
        _lib.check_conv(-121, "conv fwd")
    _lib.check_conv(0, "conv fwd")
