"""Stand-alone timing of the grouped 3x3 convs (ops.conv.gconv_fwd / gconv_dgrad / gconv_wgrad, csrc/kernels/
conv_group.hip) on ResNeXt-50 32x4d's conv2 shapes at --batch images: the four stride-1 shapes and the three stride-2
ones, forward, dgrad and wgrad each against

(a) the dense kernels (igemm_fwd / igemm_dgrad / igemm_wgrad) on the block-diagonal expansion of the same weights and
    the same activation tensors -- the only way to compute the op without the grouped kernels -- and
(b) the bytes the op must move (both activation tensors once, bf16) over the copy roof of profiles/hbm_roof.md.

One event pair per launch, 3 warm-up rounds, the median (and minimum) of --reps rounds, the grouped and the dense arm
of every case interleaved round by round in one process. The forward outputs of both arms are compared first.

python scripts/gconv_bench.py [--batch 256] [--reps 20] [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

COPY_ROOF_TBS = 5.8  # profiles/hbm_roof.md: copy-like streams
SHAPES = [(128, 4, 56, 1), (256, 8, 28, 1), (512, 16, 14, 1), (1024, 32, 7, 1),  # (C, cg, H, stride)
          (256, 8, 56, 2), (512, 16, 28, 2), (1024, 32, 14, 2)]


def cases_for(N, Cc, cg, H, s, dev, g):
    from imagent_amd.ops.conv import gconv_dgrad, gconv_fwd, gconv_wgrad, igemm_dgrad, igemm_fwd, igemm_wgrad
    G, OH = Cc // cg, (H - 1) // s + 1
    x = torch.randn((N, H, H, Cc), device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn((N, OH, OH, Cc), device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn((Cc, 3, 3, cg), device=dev, generator=g) * (2.0 / (9 * cg)) ** 0.5).to(torch.bfloat16)
    wt = w.view(G, cg, 3, 3, cg).permute(0, 4, 2, 3, 1).reshape(Cc, 3, 3, cg).contiguous()
    wd = torch.zeros((Cc, 3, 3, Cc), device=dev, dtype=torch.bfloat16)  # block-diagonal dense expansion
    for gi in range(G):
        wd[gi * cg:(gi + 1) * cg, :, :, gi * cg:(gi + 1) * cg] = w[gi * cg:(gi + 1) * cg]
    wdt = wd.permute(3, 1, 2, 0).contiguous()
    dw = torch.zeros((Cc, 3, 3, cg), device=dev)
    dwd = torch.zeros((Cc, 9 * Cc), device=dev)
    yg, yd = gconv_fwd(x, w, s, G), igemm_fwd(x, wd, s, 1, 3, 3)
    torch.cuda.synchronize()
    err = (yg.float() - yd.float()).abs().max().item()
    assert err <= 2.0 ** -7 * yd.float().abs().max().item(), ("grouped vs dense forward", err)
    nb = (x.numel() + dy.numel()) * 2
    tag = f"{Cc}@{H} cg {cg} s{s}"
    return [(tag, "fwd", nb, lambda: gconv_fwd(x, w, s, G), lambda: igemm_fwd(x, wd, s, 1, 3, 3)),
            (tag, "dgrad", nb, lambda: gconv_dgrad(dy, wt, (H, H), s, G),
             lambda: igemm_dgrad(dy, wdt, (H, H), s, 1, 3, 3)),
            (tag, "wgrad", nb, lambda: gconv_wgrad(dy, x, dw, s, G), lambda: igemm_wgrad(dy, x, dwd, s, 1, 3, 3))]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"| shape ({args.batch} images) | op | MB moved | grouped us (median / min) | dense block-diagonal us "
             "(median / min) | dense / grouped | grouped TB/s | share of the copy roof |",
             "|---|---|---:|---:|---:|---:|---:|---:|"]
    for shape in SHAPES:
        cases = cases_for(args.batch, *shape, dev, g)
        tg, td = [[] for _ in cases], [[] for _ in cases]
        for _ in range(3):
            for c in cases:
                c[3](), c[4]()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for i, c in enumerate(cases):
                tg[i].append(timed(c[3]))
                td[i].append(timed(c[4]))
        for (tag, op, nb, _, _), a, b in zip(cases, tg, td):
            ma, mb = statistics.median(a), statistics.median(b)
            tbs = nb / ma / 1e6
            lines.append(f"| {tag} | {op} | {nb / 1e6:.1f} | {ma:.1f} / {min(a):.1f} | {mb:.1f} / {min(b):.1f} | "
                         f"{mb / ma:.2f} | {tbs:.2f} | {100 * tbs / COPY_ROOF_TBS:.0f} % |")
        del cases
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
