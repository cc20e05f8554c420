"""Isolated timing of the Mixup / CutMix kernel (ops.misc.mix_pairs) at the production shape: 4096 x 224 x 224 x 4
bf16 (1.64 GB in, 1.64 GB out), in one process on the same tensors:

  mixup    every sample blended (data.mix.mix_params, Mixup alpha 0.2 only): two reads + one write per sample
  cutmix   every sample a box of its partner (CutMix alpha 1.0 only): about one read + one write
  mixed    both kinds, switch probability 0.5
  copy     no sample mixed (lam 1, empty boxes): the kernel as a plain copy

One event pair per launch, 3 warm-up launches, the median (and the minimum) of --reps launches, the cases and the
grid variants interleaved round by round. Bytes are what the kernel must move: per sample its output once, its own
pixels once unless it is a copy of its partner, and the partner's once where 0 < lam < 1 blends them (a Beta(0.2, 0.2)
draw rounds to exactly 0 or 1 in fp32 for a few samples in a hundred: those are copies); a box sample counts one read
(the 16-byte vectors that straddle a box edge read both sources: two per box row, not counted). The roof is the least
time profiles/hbm_roof.md allows for those bytes: the blended samples' at the 2-in 1-out rate (6.32 TB/s), the others'
at the copy rate (5.77 TB/s). --bpc: blocks per CU of the grid-stride launch (IMAGENT_MIX_BPC; first = the default).

python scripts/mix_bench.py [--batch 4096] [--reps 20] [--bpc 2 4 8 16] [--dtype bf16] [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

COPY_ROOF_TBS, R2W1_ROOF_TBS = 5.77, 6.32  # profiles/hbm_roof.md
STEP_MS = 231.0  # the 4096-image training step the mix joins (profiles/rrc_normalize.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bpc", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs a GPU: a timing taken elsewhere says nothing")
    from imagent_amd.data.mix import mix_params
    from imagent_amd.ops.misc import mix_pairs
    dev = torch.device("cuda")
    B, S = args.batch, args.size
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty((B, S, S, 4), device=dev, dtype=dtype)
    for i in range(0, B, 256):  # normalised-image-like values, drawn in slices (no 6.6 GB fp32 temporary)
        x[i:i + 256] = torch.randn((min(256, B - i), S, S, 4), device=dev, generator=g)
    out = torch.empty_like(x)
    sample = S * S * 4 * x.element_size()
    draws = {"mixup": mix_params(B, S, S, 0.2, 0.0, generator=g, device=dev),
             "cutmix": mix_params(B, S, S, 0.0, 1.0, generator=g, device=dev),
             "mixed": mix_params(B, S, S, 0.2, 1.0, generator=g, device=dev),
             "copy": mix_params(B, S, S, 0.2, 1.0, prob=0.0, generator=g, device=dev)}
    cases = []
    for name, (pair, lam, boxes) in draws.items():
        boxed = (boxes[:, 2] > 0) & (boxes[:, 3] > 0)
        blend = ~boxed & (lam > 0) & (lam < 1)
        nb, n = int(blend.sum().item()), B
        b_r2w1, b_copy = nb * 3 * sample, (n - nb) * 2 * sample
        roof_us = (b_r2w1 / R2W1_ROOF_TBS + b_copy / COPY_ROOF_TBS) / 1e6
        for bpc in args.bpc:
            def f(p=(pair, lam, boxes), bpc=bpc):
                os.environ["IMAGENT_MIX_BPC"] = str(bpc)
                mix_pairs(x, *p, out=out)
            cases.append((name, bpc, f, b_r2w1 + b_copy, roof_us, int(boxed.sum().item()), nb))
    times = [[] for _ in cases]
    for _ in range(3):
        for c in cases:
            c[2]()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for i, c in enumerate(cases):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            c[2]()
            e.record()
            e.synchronize()
            times[i].append(s.elapsed_time(e) * 1e3)
    os.environ.pop("IMAGENT_MIX_BPC", None)
    lines = [f"| case ({B} x {S} x {S} x 4 {args.dtype}) | box / blend / copy samples | blocks per CU | median us | min us "
             "| GB moved | TB/s (median) | roof us | of roof | of the 231 ms step |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for (name, bpc, _, nbytes, roof_us, nbox, nblend), t in zip(cases, times):
        med, mn = statistics.median(t), min(t)
        lines.append(f"| {name} | {nbox} / {nblend} / {B - nbox - nblend} | {bpc} | {med:.1f} | {mn:.1f} | "
                     f"{nbytes / 1e9:.3f} | {nbytes / med / 1e6:.2f} | {roof_us:.1f} | {100 * roof_us / med:.0f} % | "
                     f"{100 * med / 1e3 / STEP_MS:.2f} % |")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
